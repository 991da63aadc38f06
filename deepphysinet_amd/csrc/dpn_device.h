// Shared by every unit of the dpn_* family (dpn_point.hip, dpn_wgrad.hip, dpn_residual.hip, dpn_gemm.hip, dpn_optim.hip): vector types, bf16
// pair packing, the bf16 matrix instruction, the C ABI's error cast.  A helper that only one unit uses lives in that unit, not here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/dpn_hip.h"
#include "dpn_layout.h"

using namespace dpn;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned short u16;

#define DEV __device__ __forceinline__

typedef unsigned int u32;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) u32 u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

DEV u32 pack2(float a, float b) {             // one v_cvt_pk_bf16_f32
    const f32x2 v = {a, b};
    return __builtin_bit_cast(u32, __builtin_convertvector(v, bf16x2));
}
DEV float bf_lo(u32 w) { return __uint_as_float(w << 16); }
DEV float bf_hi(u32 w) { return __uint_as_float(w & 0xFFFF0000u); }

DEV bf16x8 as_bf(u32x4 w) { return __builtin_bit_cast(bf16x8, w); }
DEV f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

static inline int ck(hipError_t e) { return (int)e; }

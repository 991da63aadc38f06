// The PDE criterion (DpnPhysics.criterion, beta), stated once for the units that evaluate it per residual (dpn_residual.hip, dpn_causal.hip): its
// value rho(r) and slope rho'(r) in fp32, rho(r) in fp64 as the block sums take it, and the range check of the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/dpn_hip.h"

#define DEV __device__ __forceinline__

// every criterion the reference's builder offers is a function of input - target alone, so `loss(lhs, 0)` (interface_physics.py:104) and the gas
// law's `loss(p, rho R T)` (:179) are both mean(rho(r))
DEV float crit_value(const float r, const int kind, const float beta) {
    const float ar = fabsf(r);
    if (kind == DPN_CRIT_L1) return ar;
    return ar < beta ? 0.5f * r * r / beta : ar - 0.5f * beta;             // nn.SmoothL1Loss
}
DEV float crit_slope(const float r, const int kind, const float beta) {
    if (kind == DPN_CRIT_MSE) return 2.0f * r;
    const float sg = r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f);
    if (kind == DPN_CRIT_L1) return sg;
    return fabsf(r) < beta ? r / beta : sg;
}
// rho(r) in fp64: MSE squares in fp64 (exact: two 24-bit significands), the others cast the fp32 value up -- what dpn_residual_kernel sums
DEV double rho64(const float r, const int kind, const float beta) {
#pragma clang fp contract(off)
    return kind == DPN_CRIT_MSE ? (double)r * (double)r : (double)crit_value(r, kind, beta);
}

static inline bool criterion_ok(const DpnPhysics* ph) {
    return ph->criterion >= DPN_CRIT_MSE && ph->criterion <= DPN_CRIT_SMOOTH_L1 && !(ph->criterion == DPN_CRIT_SMOOTH_L1 && !(ph->beta > 0.f));
}

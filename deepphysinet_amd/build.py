"""Builds libdpn_hip.so (the C-ABI HIP library) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the build container; the
.so travels to the GPU box with the snapshot (it is git-ignored, not gpurun-ignored).
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, 'libdpn_hip.so')


# (source, extra flags, object name).  One unit per kernel family.  Only the point forward / backward kernels are compiled with MFMA results
# in VGPRs (no v_accvgpr_read per epilogue element: forward kernel -10 %); the weight-gradient kernel, the GEMMs and the optimiser measure
# better with hipcc's default AGPR accumulators.  tools/variant_build.py --unit=I and EXP_UNITS address units by index: units 0 .. 11 keep theirs.
# dpn_causal.hip stays the LAST entry (tests/test_causal_cpu.py holds it there), and the list is closed: a new unit goes into MORE_UNITS below.
def _src(name):
    return os.path.join(HERE, 'csrc', name)


# The point unit is also compiled without SLP vectorisation: hipcc packs adjacent fp32 adds / multiplies / fmas of the feature and epilogue code into
# v_pk_*_f32, which issue slower than the two instructions they replace beside MFMAs (profiles/valu_diet_ab.txt; the results are the same bits).
UNITS = [(_src('dpn_point.hip'), ['-mllvm', '-amdgpu-mfma-vgpr-form', '-fno-slp-vectorize'], 'dpn_point.o'),
         (_src('dpn_wgrad.hip'), [], 'dpn_wgrad.o'),      # weight packing, weight-gradient and finish kernels, sizes, self-test
         (_src('dpn_encoder.hip'), [], 'dpn_encoder.o'),
         (_src('dpn_sampler.hip'), [], 'dpn_sampler.o'),
         (_src('dpn_fp8.hip'), [], 'dpn_fp8.o'),
         (_src('dpn_encoder_chain.hip'), ['-mllvm', '-amdgpu-mfma-vgpr-form'], 'dpn_encoder_chain.o'),
         (_src('dpn_eval.hip'), [], 'dpn_eval.o'),        # the validation pass's label statistics
         (_src('dpn_adaptive.hip'), [], 'dpn_adaptive.o'),  # residual-weighted collocation points (scores, prefix sum, draw)
         (_src('dpn_residual.hip'), [], 'dpn_residual.o'),  # residual and SmoothL1 losses
         (_src('dpn_gemm.hip'), [], 'dpn_gemm.o'),        # the exact-fp32 GEMM family
         (_src('dpn_optim.hip'), [], 'dpn_optim.o'),      # fused clip + Adam
         (_src('dpn_balance.hip'), [], 'dpn_balance.o'),  # loss balancing by gradient norms
         (_src('dpn_diag.hip'), [], 'dpn_diag.o'),        # derived diagnostics from the Jacobian (inference)
         (_src('dpn_causal.hip'), [], 'dpn_causal.o')]    # per-point weights and causal time weighting of the PDE losses
# UNITS is closed at these fourteen: tests hold dpn_diag.hip at index 12, dpn_causal.hip last and the count at 14.  A unit added since goes here
# (same tuples); it is compiled and linked with the others wherever a library is built (ALL_UNITS), and nothing addresses it by index.
MORE_UNITS = [(_src('dpn_traj.hip'), [], 'dpn_traj.o')]   # parcel trajectories: one Runge-Kutta stage per launch (inference)
ALL_UNITS = UNITS + MORE_UNITS
SRCS = [u[0] for u in ALL_UNITS]
COMMON = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC']


def _listed(folder, suffixes):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(suffixes))


# every source, header and include file, taken from the directories (csrc/_obj is not looked into): a file forgotten in a hand-kept list would
# leave a stale libdpn_hip.so in place, and the tests would run it
DEPS = _listed(os.path.join(HERE, 'csrc'), ('.hip', '.h', '.inc')) + _listed(os.path.join(os.path.dirname(HERE), 'include'), ('.h',))


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build_library(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        raise RuntimeError('hipcc not found: libdpn_hip.so cannot be built (no CPU fallback exists)')
    obj_dir = os.path.join(HERE, 'csrc', '_obj')
    os.makedirs(obj_dir, exist_ok=True)
    procs = []
    for src, flags, obj in ALL_UNITS:                               # the units compile side by side
        cmd = [hipcc, *COMMON, *flags, '-I' + os.path.join(os.path.dirname(HERE), 'include'), '-c', src, '-o', os.path.join(obj_dir, obj)]
        if verbose:
            print(' '.join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            if '-mllvm' in cmd:                                     # a toolchain without that (internal) LLVM option: the unit is
                i = cmd.index('-mllvm')                             # correct without it, only ~2 % slower
                retry = cmd[:i] + cmd[i + 2:]
                print('[build] retrying without %s' % ' '.join(cmd[i:i + 2]))
                subprocess.run(retry, check=True)
                continue
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', *[os.path.join(obj_dir, u[2]) for u in ALL_UNITS], '-o', LIB + '.tmp']
    if verbose:
        print(' '.join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(LIB + '.tmp', LIB)
    return LIB


EXP_LIB = os.path.join(HERE, 'libdpn_hip_exp.so')
EXP_UNITS = (4,)              # dpn_fp8.hip (the non-scaled fp8 GEMM): include/dpn_hip_experiments.h


def build_experiments(force: bool = False) -> str:
    """libdpn_hip_exp.so: the product objects with the unit that holds shelved kernels recompiled -DDPN_EXPERIMENTS (their entry points are
    compiled out of the product library).  Tests of those kernels and the tools under tools/ that measure them load it."""
    build_library()
    if not force and os.path.exists(EXP_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(EXP_LIB) for d in DEPS):
        return EXP_LIB
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    obj_dir = os.path.join(HERE, 'csrc', '_obj')
    objs, procs = [], []
    for i, (src, flags, obj) in enumerate(ALL_UNITS):             # (EXP_UNITS: indices into UNITS, the head of ALL_UNITS)
        if i in EXP_UNITS:
            o = os.path.join(obj_dir, 'exp_' + obj)
            procs.append(subprocess.Popen([hipcc, *COMMON, *flags, '-DDPN_EXPERIMENTS', '-I' + os.path.join(os.path.dirname(HERE), 'include'), '-c', src, '-o', o]))
            objs.append(o)
        else:
            objs.append(os.path.join(obj_dir, obj))
    for pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, 'hipcc -DDPN_EXPERIMENTS')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', *objs, '-o', EXP_LIB + '.tmp'], check=True)
    os.replace(EXP_LIB + '.tmp', EXP_LIB)
    return EXP_LIB


if __name__ == '__main__':
    import sys
    print(build_library(force=True, verbose=True))
    if '--experiments' in sys.argv:
        print(build_experiments(force=True))

"""ctypes binding of libdpn_hip.so (include/dpn_hip.h).  There is no CPU fallback: if the
library is missing or no MI355X is visible, every point-path call raises."""
import ctypes
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p

from .verification import DpnVerifyOut, DpnVerifyState          # (the structs of the verification calls live with their restatement)
from .prob_verification import DpnPVerifyOut, DpnPVerifyState    # (and those of the probabilistic verification with theirs)
from .neighbourhood import DpnNbhdOut, DpnNbhdState              # (and those of the neighbourhood verification with theirs)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DPN_LIB', os.path.join(_HERE, 'libdpn_hip.so'))    # DPN_LIB: experiment builds only

NETS = 6
PREC_BF16 = 1       # bf16 MFMA operands, fp32 accumulate
PREC_BF16X2 = 2     # bf16 hi+lo split operands (3 MFMAs per product), fp32-class accuracy
PREC_NAMES = {'bf16': PREC_BF16, 'bf16x2': PREC_BF16X2, 1: PREC_BF16, 2: PREC_BF16X2}

_NET_FIELDS = ('w1b1', 'w2b2', 'evec', 'Wd', 'bd', 'W1', 'bf1', 'W2', 'bf2', 'wo', 'bo')


class DpnNetPtrs(Structure):
    _fields_ = [(n, c_void_p) for n in _NET_FIELDS] + [('ld_w1b1', c_int64), ('ld_w2b2', c_int64)]


class DpnNetGradPtrs(Structure):
    _fields_ = [(n, c_void_p) for n in _NET_FIELDS] + [('ld_w1b1', c_int64), ('ld_w2b2', c_int64)]


class DpnGeometry(Structure):
    _fields_ = [('dx', c_float), ('dy', c_float), ('lon_m1', c_float), ('lat_m1', c_float), ('pred_t_span', c_float)]


class DpnPhysics(Structure):
    _fields_ = [('mean', c_float * NETS), ('std', c_float * NETS), ('clip_lo', c_float * NETS), ('clip_hi', c_float * NETS),
                ('clip_on', c_int * NETS), ('factor', c_float * NETS), ('criterion', c_int), ('beta', c_float), ('sq_on', c_int * NETS),
                ('sq_add', c_float * NETS), ('reduce_sum', c_int)]


EVAL_STATS = 25        # DPN_EVAL_STATS: one segment's row of dpn_label_errors (include/dpn_hip.h)
CRIT_MSE, CRIT_L1, CRIT_SMOOTH_L1 = 0, 1, 2          # DpnPhysics.criterion (include/dpn_hip.h)


class DpnGemmProblem(Structure):
    _fields_ = [('A', c_void_p * 12), ('B', c_void_p * 12), ('lda', c_int32 * 12), ('ldb', c_int32 * 12), ('k_term', c_int32 * 12),
                ('bias', c_void_p), ('C', c_void_p),
                ('asum', c_void_p), ('M', c_int32), ('N', c_int32), ('K', c_int32), ('ldc', c_int32), ('ta', c_int32), ('tb', c_int32),
                ('nterms', c_int32), ('aux', c_void_p), ('aux_out', c_void_p), ('epi', c_int32)]


EPI_NONE, EPI_GELU, EPI_MUL_GELU_GRAD, EPI_ADD = 0, 1, 2, 3


class DpnLnGemm(Structure):
    _fields_ = [(n, c_int32) for n in ('mode', 'M', 'N', 'tb', 'ldb', 'ldc', 'epi')] + \
               [(n, c_void_p) for n in ('x', 'r', 'gamma', 'beta', 'rstd_in', 'y_out', 'xhat_out', 'rstd_out', 'partial', 'B', 'bias', 'C', 'aux', 'aux_out')]


class DpnColsumJob(Structure):
    _fields_ = [('partial', c_void_p), ('out_a', c_void_p), ('out_b', c_void_p), ('n_blocks', c_int32)]


class DpnEncFwd(Structure):
    """include/dpn_hip.h DpnEncFwd: one row-local forward launch of the encoder (csrc/dpn_encoder_chain.hip)."""
    _fields_ = [('wpack', c_void_p)] + [(n, c_int32) for n in ('n_mats', 'rows', 'row_tiles', 'tail', 'next', 'm_o', 'm_c1', 'm_c2', 'm_n0', 'm_n1', 'm_n2')] + \
               [(n, c_void_p) for n in ('o', 'x', 'xin', 'bo', 'g1', 'be1', 'bc1', 'bc2', 'g2', 'be2', 'gf', 'bef', 'bn0', 'bn1', 'bn2',
                                        'x1', 'xhat1', 'rstd1', 'pre', 'act', 'x2', 'xhat2', 'rstd2', 'xf', 'xhatf', 'rstdf', 'y0', 'y1', 'y2',
                                        'emb_parts', 'emb_bias', 'emb_pos', 'emb_te', 'emb_token', 'emb_out')] + \
               [('emb_part_stride', c_int64), ('emb_n_parts', c_int32), ('emb_n_tok', c_int32)]


class DpnEncBwd(Structure):
    _fields_ = [('wpack', c_void_p)] + [(n, c_int32) for n in ('n_mats', 'rows', 'row_tiles', 'head', 'body', 'm_h0', 'm_h1', 'm_h2', 'm_c2', 'm_c1', 'm_o')] + \
               [(n, c_void_p) for n in ('res', 'dq', 'dk', 'dv', 'dmeta', 'xhatf', 'rstdf', 'gin', 'xhat2', 'rstd2', 'pre', 'xhat1', 'rstd1', 'g2', 'g1', 'gf',
                                        'gs2', 'dpre', 'gs1', 'dout', 'gx', 'partial_f', 'partial2', 'partial1', 'gx_head')] + [('gx_head_rows', c_int32)]


class DpnGemm16Problem(Structure):
    """include/dpn_hip_experiments.h: the strided-GEMM description of dpn_wgrad16's core (layout mirror only: no entry point takes it)."""
    _fields_ = [(n, c_void_p) for n in ('A', 'B', 'C', 'asum', 'bias')] + [(n, c_int32) for n in ('M', 'N', 'K', 'ldc')] + \
               [(n, c_int64) for n in ('a_sm', 'a_sk', 'b_sn', 'b_sk')]


class DpnEncPrep(Structure):
    _fields_ = [('n_mats', c_int32), ('weights', c_void_p), ('packed', c_void_p), ('status_dev', c_void_p),
                ('x', c_void_p), ('T', c_int32), ('C', c_int32), ('batch', c_int32), ('xu', c_void_p),
                ('h', c_void_p), ('freqs_a', c_void_p), ('n_a', c_int32), ('out_a', c_void_p), ('freqs_b', c_void_p), ('n_b', c_int32), ('out_b', c_void_p)]


class DpnWgradProblem(Structure):
    _fields_ = [('G', c_void_p), ('X', c_void_p), ('dW', c_void_p), ('db', c_void_p)] + [(n, c_int32) for n in ('M', 'N', 'rows', 'ldg', 'ldx', 'ldw')]


ENC_MAX_MATS = 32
WGRAD_MAX_PROBLEMS = 32
GEMM_MAX_PROBLEMS, GEMM_MAX_JOBS = 26, 10


class DpnSampler(Structure):
    _fields_ = [('lon', c_int32), ('lat', c_int32), ('lon_in', c_int32), ('lat_in', c_int32), ('t_in', c_int32), ('t_hours', c_int32),
                ('cells_x', c_double), ('cells_y', c_double), ('t_step_hours', c_double), ('begin_lat', c_double), ('dlat', c_double),
                ('dx', c_float), ('dy', c_float)]


SAMPLE_INTERIOR, SAMPLE_MARGIN, SAMPLE_EXPLICIT = 0, 1, 2


class DpnLattice(Structure):
    _fields_ = [(n, c_double) for n in ('x0', 'xstep', 'y0', 'ystep', 't0', 'tstep')] + [(n, c_int32) for n in ('nx', 'ny', 'nt')]


class DpnTrajStage(Structure):
    """include/dpn_hip.h DpnTrajStage: the host scalars of one Runge-Kutta stage of dpn_traj_stage."""
    _fields_ = [(n, c_double) for n in ('t0', 'h', 'w', 'a_next', 'c_next', 'inv_wsum')] + [('step', c_int64)] + \
               [(n, c_int32) for n in ('first', 'last', 'record_only', 'with_clip')]


class DpnEnsembleOut(Structure):
    """include/dpn_hip.h DpnEnsembleOut: the six destinations of dpn_ensemble_finish, in row form or in map form."""
    _fields_ = [(n, c_void_p) for n in ('mean', 'spread', 'min', 'max', 'count', 'prob')]


class DpnExtremeState(Structure):
    """include/dpn_hip.h DpnExtremeState: the seven [C][n] arrays of a window-extremes request."""
    _fields_ = [(n, c_void_p) for n in ('best_v', 'best_t', 'best_k', 'acc', 'status', 'lo', 'hi')]


class DpnSpellState(Structure):
    """include/dpn_hip.h DpnSpellState: the thirteen [C][n] arrays of a threshold-spells request."""
    _fields_ = [(n, c_void_p) for n in ('prev_x', 'hours', 'excess', 'crossings', 'k_first', 'k_last', 'status', 'part_first', 'part_last', 'f_lo', 'f_hi',
                                        'l_lo', 'l_hi')]


class DpnRegionPlan(Structure):
    """include/dpn_hip.h DpnRegionPlan: the region-sorted list of a regional-statistics request (device arrays) and its sizes."""
    _fields_ = [(n, c_void_p) for n in ('seg', 'wgt', 'offs')] + [('n_sel', c_int64), ('n_regions', c_int32), ('nt', c_int32)]


class DpnRegionState(Structure):
    """include/dpn_hip.h DpnRegionState: the eight slot-major partial arrays of a regional-statistics request."""
    _fields_ = [(n, c_void_p) for n in ('w', 'wx', 'count', 'vmin', 'vmax', 'imin', 'imax', 'wexc')]


class DpnRegionOut(Structure):
    """include/dpn_hip.h DpnRegionOut: the nine destinations of dpn_region_finish."""
    _fields_ = [(n, c_void_p) for n in ('mean', 'total', 'weight', 'min', 'max', 'where_min', 'where_max', 'count', 'frac')]


class DpnStepGuard(Structure):
    _fields_ = [(n, c_int32) for n in ('skipped_nonfinite', 'skipped_spike', 'verdict', 'seen', 'consecutive', 'reserved')] + \
               [('running', c_double), ('last', c_double)]


class DpnLbfgsState(Structure):
    """include/dpn_hip.h DpnLbfgsState: the ring, the counters and the scalars of the L-BFGS kernels (lbfgs.py)."""
    _fields_ = [(n, c_int32) for n in ('count', 'newest', 'iters', 'skipped', 'pending', 'reserved')] + \
               [(n, c_double) for n in ('gamma', 'gtd', 'dnorm', 'g_l1', 'g_inf', 'gg')]


class DpnSizes(Structure):
    _fields_ = [('n_pad', c_int64), ('packed', c_int64), ('saved', c_int64), ('operands', c_int64), ('partials', c_int64),
                ('k_splits', c_int32)]


EXPORTS = {
    'dpn_version': (c_int, []),
    'dpn_sizes': (c_int, [c_int64, c_int, POINTER(DpnSizes)]),
    'dpn_clock_stamp': (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
    'dpn_clock_rate_khz': (c_int, [POINTER(c_int)]),
    'dpn_pack_weights': (c_int, [POINTER(DpnNetPtrs), c_int, c_void_p, c_void_p]),
    'dpn_fwd_form': (c_int, [c_int, c_int]),
    'dpn_pack_weights_form': (c_int, [POINTER(DpnNetPtrs), c_int, c_int, c_void_p, c_void_p]),
    'dpn_pack_weights_batch': (c_int, [POINTER(DpnNetPtrs), c_int, c_int64, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p]),
    'dpn_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                        c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_fwd_ref': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                            c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_fwd_ref_nets': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                                 c_int, c_void_p, c_void_p, c_void_p]),
    'dpn_fwd_ref_derivs': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_contract_gpe': (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    'dpn_residual': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnGeometry), POINTER(DpnPhysics), c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p]),
    'dpn_residual_finish': (c_int, [c_void_p, c_int64, POINTER(DpnPhysics), c_void_p, c_void_p]),
    'dpn_residual_finish_batch': (c_int, [c_void_p, c_int64, c_int, POINTER(DpnPhysics), c_void_p, c_void_p]),
    'dpn_bwd_points': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_bwd_points_scaled': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_bwd_points_derivs': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, POINTER(DpnGeometry), c_void_p, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_wgrad':(c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_wgrad_finish': (c_int, [POINTER(DpnNetPtrs), c_void_p, c_int64, c_int, c_void_p, POINTER(DpnNetGradPtrs), c_void_p]),
    'dpn_wgrad_finish_parts': (c_int, [POINTER(DpnNetPtrs), c_void_p, c_int64, c_int, c_void_p, POINTER(DpnNetGradPtrs), c_int, c_void_p]),
    'dpn_smooth_l1': (c_int, [c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'dpn_sgemm': (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                          c_void_p, c_int64, c_void_p]),
    'dpn_sgemm_ln': (c_int, [POINTER(DpnLnGemm), c_void_p]),
    'dpn_sgemm_batch_jobs': (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'dpn_sgemm_batch': (c_int, [c_int, POINTER(DpnGemmProblem), c_void_p]),
    'dpn_attn_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'dpn_attn16_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'dpn_attn_bwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_enc_pack_bytes': (c_int64, [c_int]),
    'dpn_enc_pack': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_wgrad16_partial_floats': (c_int64, [c_int, c_void_p, c_int]),
    'dpn_wgrad16': (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'dpn_enc_prep': (c_int, [POINTER(DpnEncPrep), c_void_p]),
    'dpn_enc_fwd': (c_int, [POINTER(DpnEncFwd), c_void_p]),
    'dpn_enc_bwd': (c_int, [POINTER(DpnEncBwd), c_void_p]),
    'dpn_add_ln_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_add_ln_bwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_clip_adam_scratch_doubles': (c_int64, [c_int, c_void_p]),
    'dpn_clip_adam': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                              c_float, c_float, c_void_p, c_void_p]),
    'dpn_sum_parts': (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p]),
    'dpn_lead_pe': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'dpn_im2col_circ3': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'dpn_embed_assemble': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_sample_points': (c_int, [POINTER(DpnSampler), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_uint64, c_uint64,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_sample_points_replay': (c_int, [POINTER(DpnSampler), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_uint64, c_uint64,
                                         c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_grid_maps': (c_int, [c_void_p, c_int, c_int, POINTER(DpnPhysics), c_int, c_void_p, c_void_p]),
    'dpn_sample_at': (c_int, [POINTER(DpnSampler), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(DpnLattice), c_int64, c_int64,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_fields_out': (c_int, [c_void_p, c_int64, POINTER(DpnPhysics), c_int, c_void_p, c_void_p, POINTER(DpnLattice), c_int64, c_void_p]),
    'dpn_residual_points': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnGeometry), POINTER(DpnPhysics), c_void_p, c_void_p]),
    'dpn_diagnostics_out': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnPhysics), c_int, POINTER(c_int32), c_int, c_void_p, c_void_p,
                                    POINTER(DpnLattice), c_int64, c_void_p]),
    'dpn_ensemble_accumulate': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnPhysics), c_int, POINTER(c_int32), c_int, POINTER(c_int32),
                                        POINTER(c_float), c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_ensemble_finish': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, POINTER(c_int32), c_int, c_int64, c_int64,
                                    POINTER(DpnEnsembleOut), POINTER(DpnEnsembleOut), POINTER(DpnLattice), c_void_p]),
    'dpn_region_accumulate': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnPhysics), c_int, POINTER(c_int32), c_int, POINTER(c_int32),
                                      POINTER(c_float), c_int, c_int64, POINTER(DpnRegionPlan), POINTER(DpnRegionState), c_void_p]),
    'dpn_region_finish': (c_int, [POINTER(DpnRegionPlan), POINTER(DpnRegionState), c_int, POINTER(c_int32), c_int, POINTER(DpnRegionOut), c_void_p]),
    'dpn_verify_accumulate': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnPhysics), c_int, POINTER(c_int32), c_int, POINTER(c_int32),
                                      POINTER(c_float), POINTER(c_int32), c_int, c_int64, c_int64, POINTER(DpnVerifyState), c_void_p]),
    'dpn_verify_pool': (c_int, [POINTER(DpnVerifyState), c_int64, c_void_p, c_void_p, POINTER(c_int64), c_int64, c_int, POINTER(c_int32), c_int,
                                POINTER(DpnVerifyState), c_void_p]),
    'dpn_verify_finish': (c_int, [POINTER(DpnVerifyState), c_int64, c_int, POINTER(c_int32), c_int, c_int64, c_int64, POINTER(DpnVerifyOut), c_void_p]),
    'dpn_pverify_stage': (c_int, [c_void_p, c_void_p, c_int64, POINTER(DpnPhysics), c_int, POINTER(c_int32), c_int, c_int, c_int, c_int64, c_int64,
                                  c_void_p, c_void_p, c_void_p]),
    'dpn_pverify_case': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, POINTER(c_int32), POINTER(c_float), POINTER(c_int32), c_int, c_int,
                                 c_int64, c_int64, POINTER(DpnPVerifyState), c_void_p]),
    'dpn_pverify_pool': (c_int, [POINTER(DpnPVerifyState), c_int64, c_void_p, c_void_p, POINTER(c_int64), c_int64, c_int, POINTER(c_int32), c_int,
                                 c_int, POINTER(DpnPVerifyState), c_void_p]),
    'dpn_pverify_finish': (c_int, [POINTER(DpnPVerifyState), c_int64, c_int, POINTER(c_int32), c_int, c_int, c_int64, c_int64,
                                   POINTER(DpnPVerifyOut), c_void_p]),
    'dpn_nbhd_stage': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnPhysics), c_int, POINTER(c_int32), c_int, POINTER(c_int32),
                               POINTER(c_float), POINTER(c_int32), c_int, POINTER(DpnLattice), c_int64, c_void_p, c_void_p]),
    'dpn_nbhd_fold': (c_int, [c_void_p, POINTER(DpnLattice), c_int, POINTER(c_int32), c_int, c_int64, c_int64, c_void_p, POINTER(DpnNbhdState),
                              c_void_p]),
    'dpn_nbhd_finish': (c_int, [POINTER(DpnNbhdState), c_int, c_int, c_int, POINTER(DpnNbhdOut), POINTER(DpnNbhdOut), c_void_p]),
    'dpn_traj_stage': (c_int, [POINTER(DpnSampler), c_void_p, POINTER(DpnPhysics), c_void_p, c_int64, POINTER(DpnTrajStage), c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_extreme_scan': (c_int, [POINTER(DpnSampler), c_void_p, POINTER(DpnPhysics), c_int, c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32), c_int,
                                 c_int, c_int, c_double, c_double, c_void_p, c_void_p, POINTER(DpnExtremeState), c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    'dpn_extreme_begin': (c_int, [POINTER(DpnSampler), c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32), c_int, c_int, c_double, c_double, c_void_p,
                                  c_void_p, POINTER(DpnExtremeState), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_extreme_refine': (c_int, [POINTER(DpnSampler), c_void_p, POINTER(DpnPhysics), c_int, c_void_p, c_void_p, c_int64, POINTER(c_int32),
                                   POINTER(c_int32), c_int, c_int, c_int, c_double, c_double, c_void_p, c_void_p, POINTER(DpnExtremeState), c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_spell_scan': (c_int, [POINTER(DpnSampler), c_void_p, POINTER(DpnPhysics), c_int, c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32),
                               POINTER(c_float), c_int, c_int, c_int, c_double, c_double, c_void_p, c_void_p, POINTER(DpnSpellState), c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_spell_begin': (c_int, [POINTER(DpnSampler), c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_float), c_int, c_int, c_double,
                                c_double, c_void_p, c_void_p, POINTER(DpnSpellState), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_spell_refine': (c_int, [POINTER(DpnSampler), c_void_p, POINTER(DpnPhysics), c_int, c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32),
                                 POINTER(c_float), c_int, c_int, c_int, c_double, c_double, c_void_p, c_void_p, POINTER(DpnSpellState), c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_spell_finish': (c_int, [c_int64, c_int, c_int, c_double, c_double, POINTER(DpnSpellState), c_void_p]),
    'dpn_label_errors_blocks': (c_int64, [c_int64]),
    'dpn_label_errors': (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(DpnPhysics), c_float, c_int, c_void_p, c_void_p]),
    'dpn_label_errors_finish': (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    'dpn_clip_adam_flat_floats': (c_int64, [c_int, c_void_p]),
    'dpn_clip_adam_flat': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                   c_float, c_float, c_void_p, c_void_p]),
    'dpn_clip_adam_flat_dev': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_clip_adam_flat_ema': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_void_p]),
    'dpn_clip_adam_flat_groups': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'dpn_clip_adam_flat_guard': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_double, c_double, c_int, c_int, c_void_p]),
    'dpn_ema_swap': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_lbfgs_scratch_doubles': (c_int64, [c_int, c_void_p, c_int]),
    'dpn_lbfgs_save': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_lbfgs_move': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p]),
    'dpn_lbfgs_push': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'dpn_lbfgs_gram': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_lbfgs_gtd': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_lbfgs_direction': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_gemm_fp8_mx': (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'dpn_selftest': (c_int, [c_void_p, c_void_p]),
    'dpn_adaptive_scratch_doubles': (c_int64, [c_int64]),
    'dpn_adaptive_scores': (c_int, [c_void_p, c_int64, POINTER(c_double), c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_adaptive_select': (c_int, [c_void_p, c_int64, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_uint64, c_uint64,
                                    c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_causal_rows_doubles': (c_int64, [c_int64, c_int]),
    'dpn_causal_bins': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnGeometry), POINTER(DpnPhysics), POINTER(c_double), c_double,
                                c_double, c_int, c_void_p, c_void_p, c_void_p]),
    'dpn_causal_weights': (c_int, [c_void_p, c_int64, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p]),
    'dpn_residual_weighted': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DpnGeometry), POINTER(DpnPhysics), c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_balance_scratch_doubles': (c_int64, [c_int, c_void_p]),
    'dpn_balance_sumsq': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_balance_update': (c_int, [c_void_p, c_int, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    'dpn_balance_combine': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_step_rows_doubles': (c_int64, [c_int64, c_int64]),
    'dpn_step_residual': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, POINTER(DpnGeometry), POINTER(DpnPhysics), c_float, c_float,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'dpn_step_finish_batch': (c_int, [c_void_p, c_int64, c_int64, c_int, POINTER(DpnPhysics), c_float, c_void_p, c_void_p]),
}

STEP_LOSSES = 16              # one field's row of dpn_step_finish_batch (include/dpn_hip.h)

DIAG_PRODUCTS = 28            # DPN_DIAG_PRODUCTS (include/dpn_hip.h)
ENS_PRODUCTS, ENS_MAX_THRESHOLDS = 34, 16          # DPN_ENS_PRODUCTS, DPN_ENS_MAX_THRESHOLDS (include/dpn_hip.h)
REG_GROUP, REG_MAX_COLUMNS, REG_MAX_THRESHOLDS = 64, 16, 16          # DPN_REG_GROUP, DPN_REG_MAX_COLUMNS, DPN_REG_MAX_THRESHOLDS (include/dpn_hip.h)
VERIFY_MAX_COLUMNS, VERIFY_MAX_THRESHOLDS = 16, 16                   # DPN_VERIFY_MAX_COLUMNS, DPN_VERIFY_MAX_THRESHOLDS (include/dpn_hip.h)
VERIFY_ABOVE, VERIFY_BELOW = 0, 1                                    # DPN_VERIFY_ABOVE, _BELOW: a threshold's side
PV_MAX_MEMBERS = 64                                                  # DPN_PV_MAX_MEMBERS: members per case of dpn_pverify_*
NBHD_MAX_SCALES = 8                                                  # DPN_NBHD_MAX_SCALES: window half-widths of dpn_nbhd_*
EXT_MAX_COLUMNS = 32          # DPN_EXT_MAX_COLUMNS (include/dpn_hip.h)
EXT_MAX, EXT_MIN, EXT_MEAN = 0, 1, 2                                                 # DPN_EXT_MAX, _MIN, _MEAN: a column's sense
EXT_OK, EXT_BAD_SCAN, EXT_STOPPED, EXT_AT_START, EXT_AT_END = 0, 1, 2, 3, 4         # DPN_EXT_*: a column's status
SPELL_MAX_COLUMNS = 16        # DPN_SPELL_MAX_COLUMNS (include/dpn_hip.h)
SPELL_ABOVE, SPELL_BELOW = 0, 1                                                      # DPN_SPELL_ABOVE, _BELOW: a column's side
SPELL_BAD_SCAN, SPELL_STOPPED, SPELL_NEVER, SPELL_HOLDS_AT_START, SPELL_HOLDS_AT_END = 1, 2, 4, 8, 16       # DPN_SPELL_*: the bits of a column's status
CAUSAL_MAX_BINS = 64          # DPN_CAUSAL_MAX_BINS (include/dpn_hip.h)
BALANCE_MAX_TERMS, BALANCE_STEP_TERMS = 16, 13          # DPN_BALANCE_MAX_TERMS, DPN_BALANCE_STEP_TERMS (include/dpn_hip.h)

# Shelved experiments (include/dpn_hip_experiments.h): compiled only into libdpn_hip_exp.so (`python -m deepphysinet_amd.build --experiments`), which also
# holds every product symbol; reached through load_experiments() by the code paths behind the matching frozen switches (config.py)
EXPERIMENT_EXPORTS = {
    'dpn_gemm_fp8': (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
}
EXP_LIB_PATH = os.path.join(_HERE, 'libdpn_hip_exp.so')

_lib = None
_exp = None

# The per-FIELD math (encoder GEMMs, attention, LayerNorm, hyper-network heads, SmoothL1) has plain-torch expressions for host tensors.
# They exist for the CPU-side tests of the module tree / state_dict contract / encoder math against the reference's golden vectors
# (the build container has no GPU); the product never takes them: a host tensor reaching one of these ops raises unless reference math
# has been switched on explicitly (tests do, DPN_CPU_REFERENCE_MATH=1 does).  The per-POINT path has no host form at all.
_cpu_reference_math = [os.environ.get('DPN_CPU_REFERENCE_MATH') == '1']


def enable_cpu_reference_math(on=True):
    _cpu_reference_math[0] = bool(on)


def host_math_or_raise(t, what):
    """Called where an op is about to evaluate its torch expression instead of a HIP kernel: allowed for device tensors of a shape the
    kernels do not cover, and for host tensors only in reference-math mode."""
    if not t.is_cuda and not _cpu_reference_math[0]:
        raise RuntimeError('deepphysinet_amd: %s got a tensor on %s; the HIP kernels are the only product path (no CPU fallback). '
                           'deepphysinet_amd._lib.enable_cpu_reference_math() switches the torch expressions on for CPU-side tests.' % (what, t.device))


def load_experiments():
    """dlopen the experiment library (product symbols + the shelved kernels' entry points); raises if it has not been built."""
    global _exp
    if _exp is not None:
        return _exp
    if not os.path.exists(EXP_LIB_PATH):
        raise RuntimeError('deepphysinet_amd: a shelved experiment was switched on (deepphysinet_amd/config.py) but %s is missing; build it with '
                           '`python -m deepphysinet_amd.build --experiments`' % EXP_LIB_PATH)
    lib = ctypes.CDLL(EXP_LIB_PATH)
    for name, (res, args) in list(EXPORTS.items()) + list(EXPERIMENT_EXPORTS.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _exp = lib
    return lib


def load():
    """dlopen libdpn_hip.so and declare every prototype; raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('deepphysinet_amd: %s is missing. Build it with `python -m deepphysinet_amd.build` '
                           '(hipcc --offload-arch=gfx950). There is no CPU fallback for the point path.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        raise RuntimeError('libdpn_hip: %s failed with code %d' % (what, code))

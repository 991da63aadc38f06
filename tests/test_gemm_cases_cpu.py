"""CPU: the case table of tests/test_gpu_gemm.py (tests/gemm_cases.py) is what it claims to be, before it is trusted on the GPU.

1. the whole table through the numpy model of the ABI: every case inside the ABI limits, the host's form choice as intended, kind-A partial
   sums below 2^24, the NaN guards not in the reference;
2. the kind-C bound separates an fp32 evaluation from one with bfloat16 operands;
3. the restated split-count arithmetic of dpn_sgemm on the shapes used;
4. the fp64 GELU reference against math.erf.
"""
import math

import numpy as np
import pytest

import gemm_cases as G


@pytest.mark.parametrize('launch', G.BATCH, ids=lambda l_: l_.name)
def test_batch_table_respects_the_abi_and_stays_exact(launch):
    assert 1 <= len(launch.probs) <= G.MAX_PROBLEMS and len(launch.jobs) <= G.MAX_JOBS
    assert sum(len(p.ks) for p in launch.probs) <= G.TERM_POOL
    assert G.host_form(launch.probs) == launch.form
    for p in launch.probs:
        assert 1 <= len(p.ks) <= G.MAX_TERMS and all(k > 0 for k in p.ks) and sum(p.ks) <= 7215
        assert not (p.asum and len(p.ks) != 1) and not (p.aux_out and p.epi != G.EPI_GELU)
    for kind in launch.kinds:
        if kind == 'C':
            assert all(sum(p.ks) <= 320 and p.epi == G.EPI_NONE for p in launch.probs)
        for tt in G.TT:
            for pad in (True, False):
                probs, jobs = G.build_batch(launch, kind, tt, pad)
                for q in probs:
                    ref = G.reference_problem(q)
                    assert np.isfinite(ref['C']).all() and np.isfinite(ref['magnitude']).all()        # the guards are not in the reference
                    assert q.A[0].ld == q.A[0].cols + (G.PAD if pad else 0) and np.isnan(q.A[0].full[0]).all()
                    if pad:
                        assert np.isnan(q.A[0].full[:, q.A[0].cols:]).all() and (q.C.full.view(np.uint32) == G.SENTINEL_BITS).all()
                    assert q.k_term[q.spec.zero_k] == 0 and q.K == q.spec.ks[q.spec.zero_k]
                    if kind == 'A':
                        assert ref['magnitude'].max() < 2 ** 24 and (ref['C'] == np.rint(ref['C'])).all()
                        assert (ref['C'].astype(np.float32) == ref['C']).all()
                    if kind == 'G':
                        assert np.abs(ref['v']).max() <= 6 and (ref['v'] == np.rint(ref['v'])).all()
                    if kind in ('B1', 'B2'):
                        assert (ref['C'].astype(np.float32) == ref['C']).all()                         # one exact product per output
                        sel = q.B[0] if kind == 'B1' else q.A[0]
                        assert set(np.abs(sel.win[sel.win != 0])) <= {2.0 ** e for e in range(-3, 4)}
                for job in jobs:
                    a, b = G.reference_job(job)
                    assert np.abs(a).max() <= 4 * job[3] and np.abs(b).max() <= 4 * job[3]


def test_mixed_launch_is_at_every_limit_at_once():
    m = G.batch_by_name('mixed_26_problems_32_terms_10_jobs')
    assert len(m.probs) == 26 and sum(len(p.ks) for p in m.probs) == 32 and len(m.jobs) == 10
    assert (m.probs[0].M, m.probs[0].N) == (1, 1) and (m.probs[1].M, m.probs[1].N) == (65, 70)
    assert {(p.ta, p.tb) for p in m.probs} == set(G.TT) and m.probs[25].asum
    assert {nb for l_ in G.BATCH for nb in l_.jobs} >= {1, 7, 8, 9, 72}


def test_table_covers_the_ragged_values_and_both_forms():
    single = [l_ for l_ in G.BATCH if l_.name.startswith('mn_')]
    assert {p.M for l_ in single for p in l_.probs} >= {1, 31, 32, 33, 65} and {p.N for l_ in single for p in l_.probs} >= {1, 32, 33, 70}
    tiles64 = {sum((k + 63) // 64 for k in p.ks) for l_ in G.BATCH if l_.form == '64x2' for p in l_.probs}
    assert tiles64 >= {1, 2, 3}                                                                         # the three prologue branches
    assert G.host_form(G.batch_by_name('dispatch_512_tiles').probs) == '256x1' and G.host_form(G.batch_by_name('dispatch_513_tiles').probs) == '64x2'
    t12 = G.batch_by_name('terms12').probs[0]
    assert len(t12.ks) == 12 and any(a % 64 == 0 and b % 64 != 0 for a, b in zip(t12.ks, t12.ks[1:]))
    for kind in ('B1', 'B2'):
        assert {l_.form for l_ in G.BATCH if kind in l_.kinds} == {'256x1', '64x2'}


@pytest.mark.parametrize('s', G.SGEMM, ids=lambda s: s.name)
def test_sgemm_table_stays_exact_and_split_counts_are_as_restated(s):
    has_ws, ws_bytes, splits, kps = G.sgemm_workspace(s)
    tiles = ((s.M + 31) // 32) * ((s.N + 31) // 32)
    assert splits == -(-s.K // kps) and kps % 32 == 0 and (splits - 1) * kps < s.K
    if not has_ws or s.K < 1024 or tiles >= 256 or s.ws == 'zero':
        assert splits == 1
    else:
        wanted, _ = G.sgemm_plan(s.M, s.N, s.K, True, 1 << 62)
        assert 1 < wanted <= min(32, s.K // 256)
        assert splits == wanted if s.ws == 'exact' else splits < wanted                                 # one byte less: fewer splits
        assert G.sgemm_ws_bytes(s.M, s.N, splits) <= ws_bytes
    for tt in G.TT:
        d = G.build_sgemm(s, 'A', tt, True)
        ref = G.reference_sgemm(s, tt, d)
        assert np.isfinite(ref['C']).all() and ref['magnitude'].max() < 2 ** 24 and ref['asum_abs'].max() < 2 ** 24
        assert (ref['C'].astype(np.float32) == ref['C']).all()


def test_split_counts_of_the_production_shapes():
    # token convolution: 287 x 256 over K = 7215 with the workspace linear._sgemm_splitk allocates (32 splits' worth)
    # 72 output tiles -> ceil(512 / 72) = 8 splits of ceil(7215 / 8) = 902 -> 928 (a multiple of 32) k-values, and 8 * 928 >= 7215 > 7 * 928
    assert G.sgemm_plan(287, 256, 7215, True, 32 * (287 * 256 + 287) * 4) == (8, 928)
    assert G.sgemm_plan(159, 256, 7215, True, 1 << 40) == (13, 576) and G.sgemm_plan(1, 1, 1024, True, 1 << 40) == (4, 256)
    assert G.sgemm_plan(33, 17, 1030, True, 1 << 40) == (4, 288) and G.sgemm_plan(33, 17, 1023, True, 1 << 40) == (1, 1024)


def _kind_c_problems():
    for launch in G.BATCH:
        if 'C' in launch.kinds:
            for tt in ((0, 0), (1, 1)):
                for q in G.build_batch(launch, 'C', tt, True)[0]:
                    yield launch.name, q


def test_kind_c_bound_separates_fp32_from_bfloat16_operands():
    """A sequential fp32 evaluation of every kind-C case stays inside (K + 16) 2^-24 |A||B| + 2^-24 |C64|; the same evaluation with the operands
    rounded to bfloat16 leaves it in every case, at K = 256 .. 320 by about an order of magnitude."""
    n = 0
    for name, q in _kind_c_problems():
        p, ref = q.spec, G.reference_problem(q)
        a = np.concatenate([G.op_read(q.A[t], p.M, k, q.ta) for t, k in enumerate(p.ks)], 1)
        b = np.concatenate([G.op_read(q.B[t], k, p.N, q.tb) for t, k in enumerate(p.ks)], 0)
        bias = G.op_read(q.bias, 1, p.N, 0) if q.bias is not None else None
        assert np.allclose(ref['absprod'], np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)), rtol=1e-12, atol=0)   # |A||B| alone: no bias in it
        bound = G.kind_c_bound(sum(p.ks), ref['absprod'], ref['C'])
        err32 = np.abs(G.fma_chain_fp32(a, b, bias).astype(np.float64) - ref['C'])
        err16 = np.abs(G.fma_chain_fp32(G.round_bf16(a), G.round_bf16(b), bias).astype(np.float64) - ref['C'])
        assert (err32 <= bound).all(), (name, float((err32 / bound).max()))
        worst = float((err16 / bound).max())
        assert worst > 1.0, (name, worst)
        if sum(p.ks) >= 256 and p.M * p.N >= 1024:
            assert worst > 8.0, (name, worst)
        n += 1
    assert n >= 20


@pytest.mark.parametrize('s', G.SGEMM_KIND_C, ids=lambda s: s.name)
def test_kind_c_bound_separates_fp32_from_bfloat16_operands_in_the_sgemm_cases(s):
    """The same for dpn_sgemm's kind-C cases, in the kernel's own order: the fp32 chain, then + bias, then + the pre-filled C, one rounding each.
    The bound takes |A||B| alone: the roundings of the two final additions are inside 2^-24 |C64| and the 16."""
    for tt in G.TT:
        d = G.build_sgemm(s, 'C', tt, True)
        ref = G.reference_sgemm(s, tt, d)
        a, b = G.op_read(d['A'], s.M, s.K, tt[0]), G.op_read(d['B'], s.K, s.N, tt[1])
        assert np.allclose(ref['absprod'], np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)), rtol=1e-12, atol=0)
        bound = G.kind_c_bound(s.K, ref['absprod'], ref['C'])
        worst = []
        for rnd in (lambda x: x, G.round_bf16):
            v = G.fma_chain_fp32(rnd(a), rnd(b), G.op_read(d['bias'], 1, s.N, 0))
            if s.accumulate:
                v = (d['c0'] + v).astype(np.float32)
            worst.append(float((np.abs(v.astype(np.float64) - ref['C']) / bound).max()))
        assert worst[0] <= 1.0 < worst[1], (s.name, tt, worst)


def test_round_bf16_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 3 * 2.0 ** -8, -3.14159274, 0.0], np.float32)
    assert G.round_bf16(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -3.140625, 0.0]


def test_gelu_reference_against_math_erf():
    for x in [v * 0.5 for v in range(-14, 15)]:
        cdf = 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
        assert abs(float(G.gelu64(x)) - x * cdf) <= 1e-15 * max(1.0, abs(x))
        grad = cdf + x * math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        assert abs(float(G.gelu_grad64(x)) - grad) <= 1e-15
        h = 1e-6                                                      # and the derivative is the derivative of the function
        assert abs((float(G.gelu64(x + h)) - float(G.gelu64(x - h))) / (2 * h) - grad) <= 1e-8
    assert float(G.gelu64(0.0)) == 0.0 and float(G.gelu_grad64(0.0)) == 0.5


@pytest.mark.parametrize('mode', [1, 2])
def test_ln_reference_is_free_of_the_guards_and_sums_only_existing_rows(mode):
    for M in G.LN_M:
        d = G.build_ln(mode, M, 33, 1, True)
        ref = G.reference_ln(mode, M, 33, 1, d)
        assert all(np.isfinite(v).all() for v in ref.values())
        if mode == 2 and M == 33:
            g, xh = d['x'].win.astype(np.float64), d['r'].win.astype(np.float64)
            assert np.array_equal(ref['partial'][1, 256:], g[32]) and np.array_equal(ref['partial'][1, :256], g[32] * xh[32])


def test_outside_is_sentinel_notices_one_touched_guard_element():
    b = G.output_buf(3, 4, True)
    after = b.full.copy()
    after[G.GUARD_ROWS:G.GUARD_ROWS + 3, :4] = 1.0
    assert G.outside_is_sentinel(after, b)
    for r, c in ((G.GUARD_ROWS - 1, 0), (G.GUARD_ROWS, 4), (G.GUARD_ROWS + 3, 0), (0, 0), (after.shape[0] - 1, after.shape[1] - 1)):
        bad = after.copy()
        bad[r, c] = 0.0
        assert not G.outside_is_sentinel(bad, b)

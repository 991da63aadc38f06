"""GPU (MI355X): what the two verification states share through point_path._ScoreState -- `finish` of a point range, `pool` over a plan and
`clear` -- on both classes at the size where the second chunk is one point behind the 64-lane tile of dpn_pverify_case.  The yardsticks are the
states' own bits and the numpy restatements of the two pool kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import _dev

N, M, CASES = 65, 2, 2                                                    # chunks of 64 + 1
IDS, THR = [31, 25], ([0], [280.0], [0])                                  # T and speed; T above 280 K


def _data():
    """Seeded normalised fields and coarse values [CASES, M, N, 6] and reports [CASES, N, 2] with a few NaN."""
    g = torch.Generator().manual_seed(11)
    out_n, cd = (0.5 * torch.randn((CASES, M, N, 6), generator=g) for _ in range(2))
    obs = torch.stack([283.6 + 15.6 * torch.randn((CASES, N), generator=g), (3.0 * torch.randn((CASES, N), generator=g)).abs()], dim=-1)
    obs[0, 3, 0] = obs[1, 64, 1] = obs[1, 17, 0] = obs[0, 64, 0] = float('nan')
    return out_n.to(_dev()), cd.to(_dev()), obs.contiguous().to(_dev())


def _fold(kind, st, ph, out_n, cd, obs):
    for c in range(CASES):
        for first, n in ((0, 64), (64, 1)):
            sl = slice(first, first + n)
            if kind == 'verify':
                st.accumulate(out_n[c, 0, sl], cd[c, 0, sl], obs[c, sl], ph, first)
                continue
            for m in range(M):
                st.stage(out_n[c, m, sl], cd[c, m, sl], ph, m, first)
        if kind != 'verify':
            for first, n in ((0, 64), (64, 1)):
                st.case(obs[c, first:first + n], first)


def _host(state):
    return {k: v.cpu().numpy() for k, v in state.arrays().items()}


def _bits(a, b):
    return list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize('kind', ['verify', 'verify_ensemble'])
def test_finish_range_pool_and_clear_through_the_base(kind):
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd import verification as VF
    from deepphysinet_amd.point_path import PointConfig, ProbVerifyState, VerifyState
    ph = PointConfig().physics()
    data = _data()
    st = VerifyState(N, IDS, *THR, _dev()) if kind == 'verify' else ProbVerifyState(N, IDS, *THR, M, _dev())
    _fold(kind, st, ph, *data)
    first = _host(st)
    assert 0 < int(first['n'].sum()) < CASES * N * len(IDS) and int(first['n'][:, 64].sum()) > 0        # some pairs count, the NaN reports do not
    rows, last = st.finish(), st.finish(first=64, n=1)
    assert _bits({k: v.cpu().numpy() for k, v in last.items()}, {k: v[64:65].cpu().numpy() for k, v in rows.items()})
    plan = VF.pool_plan(np.where(np.arange(N) < 64, 2, 1), n_groups=3)   # groups of 0, 1 and 64 points
    assert np.diff(plan[1]).tolist() == [0, 1, 64]
    reference = VF.verify_pool_reference if kind == 'verify' else PV.pverify_pool_reference
    want = reference(first, *plan, THR[0])
    got = _host(st.pool(*plan))
    assert _bits(got, {k: want[k] for k in got})
    st.clear()
    assert not bool(st.buffer.any())
    _fold(kind, st, ph, *data)
    assert _bits(_host(st), first)

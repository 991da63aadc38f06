"""GPU (MI355X): the row-local encoder forward launches write what they wrote before their q / k / v tail was split over three workgroups
per row block (csrc/dpn_encoder_chain.hip, dpn_enc_fwd_kernel<.., REP = 3>), and so does the first layer's q / k / v backward, whose two
workgroups per row block take one of every wave's two channel tiles each (dpn_enc_bwd_qkv2_kernel).

tools/enc_digest.py drives dpn_enc_pack, dpn_enc_fwd and dpn_enc_bwd (head 1 without body) through the C ABI with CPU-seeded inputs, every output buffer zero-filled before the
launch (a store that every replica skips, or a projection that none writes, leaves zeros), and takes the SHA-256 of every output tensor.
tests/golden/enc_replicas_parent.json holds these digests as the commit BEFORE the replicas computes them (written by the same tool with that
commit's library selected through DPN_LIB).  Every replica runs the same instruction sequence on the same inputs as the single workgroup
did, so every digest has to be EQUAL -- no tolerance -- in all five forward launch kinds and the backward one at
    1 row (one block, 15 padding rows), 16 (one exact block), 17 (a second block of one row), 287 (one field: 18 blocks, the last ragged),
    574 (B = 2) and 2 296 rows (B = 8: 32-row workgroups, which do not replicate)."""
import ctypes
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('enc_digest', os.path.join(ROOT, 'tools', 'enc_digest.py'))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

_cache = {}
N_OUT = {'first': 3, 'first_emb': 4, 'tail_next0': 8, 'tail_next1': 11, 'tail_next2': 12, 'bwd_qkv': 2}


def _fixture():
    if 'fx' not in _cache:
        with open(D.FIXTURE) as f:
            _cache['fx'] = json.load(f)
    return _cache['fx']


def test_the_fixture_covers_every_case():
    fx = _fixture()['cases']
    assert sorted(fx) == sorted(D.case_key(r, k) for r, k in D.all_cases())
    for r, k in D.all_cases():
        assert len(fx[D.case_key(r, k)]) == N_OUT[k], (r, k)


@pytest.mark.parametrize('kind', D.KINDS)
@pytest.mark.parametrize('rows', D.ROWS)
def test_launch_writes_the_parent_commits_bits(rows, kind):
    got = D.digest(D.run_case(rows, kind))
    ref = _fixture()['cases'][D.case_key(rows, kind)]
    diff = [k for k in ref if got.get(k) != ref[k]]
    assert len(got) == N_OUT[kind] and not diff, diff


def test_the_workload_launches_do_replicate():
    """What the equality above is about: at one field and at B = 2 the q / k / v launches run three workgroups per row block, the others one."""
    from deepphysinet_amd import _lib as L
    fn = L.load().dpn_enc_fwd_replicas
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    for rows in (1, 16, 17, 287, 574):
        assert fn(rows, 1, 0, 1) == 3 and fn(rows, 1, 1, 1) == 3
        assert fn(rows, 1, 1, 0) == 1 and fn(rows, 1, 1, 2) == 1
    assert fn(2296, 2, 1, 1) == 1
    fb = L.load().dpn_enc_bwd_replicas
    fb.restype, fb.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    for rows in (1, 16, 17, 287, 574):
        assert fb(rows, 1, 1, 0) == 2 and fb(rows, 1, 1, 1) == 1
    assert fb(2296, 2, 1, 0) == 1

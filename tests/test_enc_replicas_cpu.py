"""CPU: dpn_enc_fwd_replicas, the host rule that decides how many workgroups run one 16-row block of a row-local encoder forward launch
(csrc/dpn_encoder_chain.hip).  Three -- one per q / k / v projection -- only for launches that have that tail (next == 1) on 16-row workgroups
(row_tiles == 1), and only while every workgroup of the launch is resident in one round of the chip's 256 CUs:
    3 x row blocks + the L2 warm-up helpers (64 while there are at most 64 row blocks, none above) <= 256.
dpn_enc_bwd_replicas is the same rule with TWO workgroups per row block for the q / k / v backward without a body (head == 1, body == 0)."""
import ctypes

CUS, HELPERS, HELPER_MAX_BLOCKS = 256, 64, 64


def _fn():
    from deepphysinet_amd import _lib
    fn = _lib.load().dpn_enc_fwd_replicas
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    return fn


def _grid(rows, reps):
    blocks = (rows + 15) // 16
    return blocks * reps + (HELPERS if blocks <= HELPER_MAX_BLOCKS else 0)


def test_one_field_replicates_in_both_launch_kinds():
    fn = _fn()
    assert fn(287, 1, 0, 1) == 3 and fn(287, 1, 1, 1) == 3
    assert _grid(287, 3) == 18 * 3 + 64


def test_only_the_qkv_tail_on_16_row_workgroups_replicates():
    fn = _fn()
    for rows in (1, 16, 17, 287, 574, 2296, 17707):
        for tail in (0, 1):
            assert fn(rows, 2, tail, 1) == 1
            assert fn(rows, 1, tail, 0) == 1 and fn(rows, 1, tail, 2) == 1
    assert fn(0, 1, 1, 1) == 1 and fn(-5, 1, 1, 1) == 1 and fn(287, 3, 1, 1) == 1


def test_the_bound():
    fn = _fn()
    # with helpers: 64 row blocks x 3 + 64 = 256 workgroups, exactly one round
    assert fn(64 * 16, 1, 1, 1) == 3 and _grid(64 * 16, 3) == 256
    # without helpers (65 row blocks and up): 85 x 3 = 255 fits, 86 x 3 = 258 does not
    assert fn(64 * 16 + 1, 1, 1, 1) == 3 and _grid(64 * 16 + 1, 3) == 195
    assert fn(85 * 16, 1, 1, 1) == 3 and _grid(85 * 16, 3) == 255
    assert fn(85 * 16 + 1, 1, 1, 1) == 1
    assert fn(2048, 1, 1, 1) == 1


def test_a_replicated_launch_never_exceeds_one_round():
    fn = _fn()
    seen = set()
    for rows in range(1, 2049):
        for tail in (0, 1):
            r = fn(rows, 1, tail, 1)
            assert r in (1, 3)
            seen.add(r)
            if r == 3:
                assert _grid(rows, 3) <= CUS, rows
            else:
                assert _grid(rows, 3) > CUS, rows          # the rule is the bound and nothing else
    assert seen == {1, 3}


def _fb():
    from deepphysinet_amd import _lib
    fn = _lib.load().dpn_enc_bwd_replicas
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    return fn


def test_backward_only_the_qkv_launch_without_a_body_replicates():
    fb = _fb()
    assert fb(287, 1, 1, 0) == 2 and _grid(287, 2) == 18 * 2 + 64
    for rows in (1, 16, 17, 287, 574, 2296):
        assert fb(rows, 2, 1, 0) == 1
        for head, body in ((0, 1), (1, 1), (2, 1), (2, 0), (0, 0)):
            assert fb(rows, 1, head, body) == 1
    assert fb(0, 1, 1, 0) == 1 and fb(287, 3, 1, 0) == 1


def test_backward_bound():
    fb = _fb()
    assert fb(64 * 16, 1, 1, 0) == 2 and _grid(64 * 16, 2) == 192
    assert fb(128 * 16, 1, 1, 0) == 2 and _grid(128 * 16, 2) == 256          # 2 048 rows: the largest 16-row launch, exactly one round
    assert fb(128 * 16 + 1, 1, 1, 0) == 1
    for rows in range(1, 2200):
        r = fb(rows, 1, 1, 0)
        assert (r == 2 and _grid(rows, 2) <= CUS) or (r == 1 and _grid(rows, 2) > CUS), rows

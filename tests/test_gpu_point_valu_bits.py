"""GPU (MI355X): the point kernels after their instruction-count work (profiles/valu_diet_ab.txt) write the bits they wrote before it.

Each case drives the C ABI as tests/test_gpu_z0_table.py does (tools/point_bits_digest.py holds the launch sequence): dpn_fwd -> dpn_residual ->
dpn_bwd_points at n = 1, 70, 129 and 1 037 points in both precision modes, and dpn_fwd_ref_derivs -> dpn_residual -> dpn_bwd_points_derivs at n = 70.
What is compared is the SHA-256 of the fields, the Jacobian (and the second and third derivatives), the whole saved state and the whole operand buffer,
both zeroed before the launches.  EXPECTED was printed by that tool on an MI355X for the library of the commit in front of the work, selected through
DPN_LIB, before any kernel was edited: equal, not close."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('point_bits_digest', os.path.join(ROOT, 'tools', 'point_bits_digest.py'))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

EXPECTED = {
    'plain/1/bf16x2': {
        'fields': '7f9646c9349714d819e11e780add8a76fdfd8907f3660e58064d410c29b288c7',
        'jacobian': 'efc6e507922ea42c6439f6a6218dd764f6af29e9086240b44424457438f0c17b',
        'operands': '0d1881183ac44ac5524881bce7f50af652e3b262466d1317909f124139179057',
        'saved': '481467ae8399917594f7662c685cce7a59e23766458dcfef219246099cdf0dd0',
    },
    'plain/1/bf16': {
        'fields': 'f99dbebd21d79617185fb6aedd12045ea4b7967f10942c07b2d3314507118d96',
        'jacobian': 'b53256ea1308c94b21b2baee1bef8aa50da5a83f6f03374c471e7c017f0b6795',
        'operands': '048a99fe3067266473951269f844b49a8bb47ac66b11a8d14b9ea8cc9a254c0e',
        'saved': '959608f13931e52ec1439e371cdfb7e4e2581f561142bad3d2228f8e32f5a0bb',
    },
    'plain/70/bf16x2': {
        'fields': 'bd06efc4d173ec1fd01b9ceab4eb0fa411cc9081bb7d63b1a31473187b45d3fe',
        'jacobian': 'c5115c7a119e7dcd9bd1648eeb1a1c530d6af4a719f2cff5fc8b793a29eb701d',
        'operands': '9ffd137c0c275435956fe98ebaef05c63a749ca9dd4c6b4dcbf1eacf6e1992bc',
        'saved': 'd8c2d20e279566a0f4d899ecd4e32f056febde073caf1feab62aa82aece7c9ec',
    },
    'plain/70/bf16': {
        'fields': '84f3bb21708a03b59a3be93f02dee6f98911cfe184ee6dcb533c91e9e6417d32',
        'jacobian': 'd59f051cdc76d622348793f94d499eb2a2bf7f30938e1bc5354605e713ae28b1',
        'operands': '46fca59fb8d8d9cd9a721a5f805422449f0d09a662e3c072972e392fe501fb65',
        'saved': '21fee0c9ac17917b0fdfde071d3180a54bccb4010ee45e396ef4da7fb78c8cb2',
    },
    'plain/129/bf16x2': {
        'fields': '714bc9f8ed01647b404e146772401cfb8098b8a4214f1c1e8803c4e8f8d88297',
        'jacobian': 'a78bdcac10fa866dda7744980b85d5a1626e7f61aa62dd2770eeda9b4275f66c',
        'operands': '038f64e6d6e30a66ae0d28dfad1904077011b9e855757b21ecbb01c43913694f',
        'saved': '40effdb5b1b5295dc7b88063c62ccf6a472877d83e5823398c931288aba72cf9',
    },
    'plain/129/bf16': {
        'fields': '05cb66218ea8c6c1c0c741891878d4b144e410b0533d4435e89a3c7bda7b1ef9',
        'jacobian': '155976c833e686379cd917f167a93b237ba8fa5bff955875535be6409d4c2b82',
        'operands': 'e1013ec2b6a63c0eee64ea5ff508d4f1438439d002fd2e563d51c5bb6a47edfd',
        'saved': '8b4b06f591d350b06703d8ca5df73d6ee6533d76a14237d0180b3feb33ac401a',
    },
    'plain/1037/bf16x2': {
        'fields': 'ad746cfbcfed504c60715f952503328c16d41b6fa725d274d142f96d9215a3a6',
        'jacobian': '164622b2318a70740b9f4013646c81927cd2498b4ce553f70f07864beda93655',
        'operands': 'c2769dfcecc37242f26f073c0479f0be061b528cc74b8401598bb01d9e8631d2',
        'saved': 'f7c6cb0ea5918afbc051b0626d71f95520808ea444c41b6f2b44df75e1056ffc',
    },
    'plain/1037/bf16': {
        'fields': 'eaeb9d2ddcdec4051a6af0d345c4bd1b1a12ac4129b388a2f572f490b006fad6',
        'jacobian': '2b0c52ca80850ab6692fcbe9ad7c0ea6edeb69c2668c7a55fe5c08fc93f85f42',
        'operands': '09e9b2c17dbcd4c8c99570ca976161ff017b59ef080247b650f3800866161c0c',
        'saved': '667112d999c8fd3437b00ad96712801a69889f87e1373f7d9d65d0fbb969a8d2',
    },
    'deriv/70/bf16x2': {
        'fields': 'bd06efc4d173ec1fd01b9ceab4eb0fa411cc9081bb7d63b1a31473187b45d3fe',
        'hessian': 'aeb50f1cf7a8581aea049ab1204bf71e5cdfd4e1041f99a5f13b61db41b47792',
        'jacobian': 'c5115c7a119e7dcd9bd1648eeb1a1c530d6af4a719f2cff5fc8b793a29eb701d',
        'operands': '46e6f141ee55f1a4c3e8e2381fe0bcdd1053d7a84ed06b9136ff47bc79330031',
        'saved': 'd8c2d20e279566a0f4d899ecd4e32f056febde073caf1feab62aa82aece7c9ec',
        'third': '384ee7caa77b79623461bdcb1545e79fd471452f3524da7b143d6253c349cd05',
    },
    'deriv/70/bf16': {
        'fields': '84f3bb21708a03b59a3be93f02dee6f98911cfe184ee6dcb533c91e9e6417d32',
        'hessian': 'da066e34dc2a77ebd55ca09c9c4d7952891ef282c90ac0ce94db3d4702d8e0c2',
        'jacobian': 'd59f051cdc76d622348793f94d499eb2a2bf7f30938e1bc5354605e713ae28b1',
        'operands': '2a9d5d53493012c79d6b9eaabcd30b69fed0919054f120d5a69423fa9dfd2e93',
        'saved': '21fee0c9ac17917b0fdfde071d3180a54bccb4010ee45e396ef4da7fb78c8cb2',
        'third': '9c5359a54f957d2ce428e8031edf5f8f7cb6dce212e44b9cb8976cef514c8dfe',
    },
}


def test_the_table_covers_the_cases():
    assert sorted(EXPECTED) == sorted(B.case_key(*c) for c in B.all_cases())
    assert B.SIZES == (1, 70, 129, 1037) and B.PRECS == ('bf16x2', 'bf16') and B.DERIV_N == 70


@pytest.mark.parametrize('route,n,prec', B.all_cases(), ids=[B.case_key(*c) for c in B.all_cases()])
def test_point_kernels_write_the_parent_commits_bits(route, n, prec):
    res = B.run_case(route, n, prec)
    got, ref = B.digest(res), EXPECTED[B.case_key(route, n, prec)]
    assert sorted(got) == sorted(ref)
    diff = [k for k in sorted(got) if got[k] != ref[k]]
    assert not diff, (B.case_key(route, n, prec), diff)
    assert all(int(v.count_nonzero()) > 0 for v in res.values())

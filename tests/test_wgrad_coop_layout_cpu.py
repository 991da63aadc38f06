"""No GPU: the deal of a product-2 tile's 1-KB pieces over the eight waves of dpn_wgrad_kernel (csrc/dpn_layout.h: wgrad_coop_piece).  A wave forms
G6 = g pe6 in LDS from the table pieces it fetched itself, behind nothing but its own counted wait -- so the deal has to hand every piece of the slot
image to exactly one wave, both planes of a column pair to the SAME wave, and the kernel's "this slot is a table piece" predicate has to say so.
tests/test_capi_cpu.py::test_layout_algebra is the model."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEAL_TEST = r'''
#include <cstdio>
#include <map>
#include <set>
#include "dpn_layout.h"
using namespace dpn;
// (ns, DMA instructions per wave and tile): hi+lo 16 + 24 pieces = 8 x 5; plain bf16 16 + 12 = 28 pieces in 8 x 4 slots, four pads
int check(int ns, int issue) {
    std::set<int> seen;
    std::map<int, int> pair_wave;
    int pads = 0;
    for (int wave = 0; wave < 8; ++wave) {
        int pairs = 0;
        for (int j = 0; j < issue; ++j) {
            const int q = wgrad_coop_piece(ns, issue, wave, j);
            if (q < -1 || q >= 16 + 12 * ns) return 1;
            if (wgrad_coop_is_y(ns, wave, j) != (q >= 16)) return 2;        // table pieces: no non-temporal hint, and the ones form() rewrites
            if (q < 0) { ++pads; continue; }
            if (!seen.insert(q).second) return 3;                            // fetched twice
            if (q >= 16) {
                const int s = (q - 16) / 12, p = (q - 16) % 12;
                if (p % 8 != wave || p / 8 > (wave < 4 ? 1 : 0)) return 4;   // form(): pair p = wave + 8 q, the second one on waves 0 .. 3 only
                if (pair_wave.count(p) && pair_wave[p] != wave) return 5;    // hi and lo plane of a pair on one wave
                pair_wave[p] = wave;
                if (s == 0) ++pairs;
                if (j != s + ns * (p / 8)) return 6;                         // slot order: pair `wave` first, plane by plane
            }
        }
        if (pairs != (wave < 4 ? 2 : 1)) return 7;
    }
    if ((int)seen.size() != 16 + 12 * ns) return 8;                          // ... and every piece fetched
    if (pads != 8 * issue - 16 - 12 * ns) return 9;
    return 0;
}
int main() {
    if (int r = check(2, 5)) return r;
    if (int r = check(1, 4)) return 10 + r;
    std::puts("deal ok");
    return 0;
}
'''


def test_product_2_piece_deal_is_a_bijection_and_pairs_stay_on_one_wave(tmp_path):
    src = tmp_path / 'deal_test.cpp'
    src.write_text(DEAL_TEST)
    exe = tmp_path / 'deal_test'
    subprocess.run(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'deepphysinet_amd', 'csrc'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, 'deal check %d failed' % out.returncode
    assert 'deal ok' in out.stdout


def test_the_kernel_uses_the_deal_it_is_tested_on():
    with open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_wgrad.hip')) as f:
        src = f.read()
    assert 'wgrad_coop_piece(NS, S::kIssue, wave, j)' in src and 'wgrad_coop_is_y(NS, wave, j)' in src

"""No GPU: product 3 of dpn_wgrad_kernel with Z0 in the table form (csrc/dpn_point_common.h, OperandView; csrc/dpn_layout.h: wgrad_z0_piece).  A wave
forms Z0 = g pe3 + gJ_c d pe3 / d xi_c in LDS from the fp32 table pieces it fetched itself, behind nothing but its own counted wait: the deal has to hand
each of the 56 pieces of the slot image to exactly one wave, both halves of a column pair to the SAME wave, all pairs of a wave have to share one column
tile (one gJ_c and one frequency per lane), and the partner-lane and column -> frequency maps of form_z0() have to agree with the slot algebra the
stage-1 kernels build Z0 with.  tests/test_wgrad_coop_layout_cpu.py is the model."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEAL_TEST = r'''
#include <cstdio>
#include <map>
#include <set>
#include "dpn_layout.h"
using namespace dpn;
int deal() {
    std::set<int> seen;
    std::map<int, int> pair_wave;
    for (int wave = 0; wave < 8; ++wave) {
        std::map<int, int> halves;                                           // pair -> bit mask of the halves this wave fetches
        for (int j = 0; j < 7; ++j) {
            const int q = wgrad_z0_piece(wave, j);
            if (q < 0 || q >= 56) return 1;                                  // 32 X + 24 Y pieces, no pad
            if (wgrad_z0_is_y(wave, j) != (q >= 32)) return 2;               // table pieces: no non-temporal hint, and the ones form_z0() rewrites
            if (!seen.insert(q).second) return 3;                            // fetched twice
            if (q >= 32) {
                const int s = (q - 32) / 12, p = (q - 32) % 12, kk = p / 6, ct = p % 6;
                if (ct != wgrad_z0_ct(wave)) return 4;                       // one column tile per wave: one coordinate, one frequency per lane
                if (pair_wave.count(p) && pair_wave[p] != wave) return 5;    // both halves of a pair on one wave
                pair_wave[p] = wave;
                halves[p] |= 1 << s;
                if (kk != wgrad_z0_kk(wave, j >> 1) || s != (j & 1)) return 6;   // slot order: table pieces first, pair by pair, half 0 then half 1
            }
        }
        if ((int)halves.size() != wgrad_z0_pairs(wave) || wgrad_z0_pairs(wave) != (wave < 4 ? 2 : 1)) return 7;
        for (auto& kv : halves)
            if (kv.second != 3) return 8;                                    // a wave's Y pieces are exactly both halves of its pairs
        for (int q2 = 0; q2 < wgrad_z0_pairs(wave); ++q2)
            if (!halves.count(6 * wgrad_z0_kk(wave, q2) + wgrad_z0_ct(wave))) return 9;   // ... and they are the pairs form_z0() forms
    }
    if ((int)seen.size() != 56 || (int)pair_wave.size() != 12) return 10;   // a bijection
    return 0;
}
// column jj of column tile ct is PE slot (ks = 2 ct + (jj >> 4), h = (jj >> 3) & 1, e = jj & 7) (dpn_point_common.h, K-layout); ts::z0_frag builds slot
// (ks, h, e = 2 q + fn) from the angle xi_c freqs[8 (ks & 3) + 4 h + q], c = ks >> 2, fn = 0 sine | 1 cosine
int maps() {
    for (int ct = 0; ct < 6; ++ct)
        for (int jj = 0; jj < 32; ++jj) {
            const int ks = 2 * ct + (jj >> 4), h = (jj >> 3) & 1, e = jj & 7;
            if (z0_freq_index(ct, jj) != 8 * (ks & 3) + 4 * h + (e >> 1)) return 1;
            if ((ks >> 2) != (ct >> 1)) return 2;                            // the coordinate of a column tile
            if (pe3_angle(ks, h, e) != 32 * (ct >> 1) + z0_freq_index(ct, jj)) return 3;        // ... and of the layout's own angle numbering
            // the partner: column jj ^ 1 = the same k-step, half and angle, the other function
            const int pj = jj ^ 1, pks = 2 * ct + (pj >> 4), ph = (pj >> 3) & 1, pe = pj & 7;
            if (pks != ks || ph != h || (pe >> 1) != (e >> 1) || (pe & 1) == (e & 1)) return 4;
            if (pe3_angle(pks, ph, pe) != pe3_angle(ks, h, e)) return 5;
            if (z0_freq_index(ct, pj) != z0_freq_index(ct, jj)) return 6;
            if (pe3_ch(ks, h, e) + ((e & 1) ? -3 : 3) != pe3_ch(pks, ph, pe)) return 7;         // reference channels f*6 + fn*3 + c: sine <-> cosine
        }
    // K-layout: lane = column + 32 (point half), 16 bytes per lane inside a 1-KB piece: the partner's bytes are lane ^ 1's, same piece, same point half
    for (int lane = 0; lane < 64; ++lane) {
        const int pl = lane ^ 1;
        if ((pl & 31) != ((lane & 31) ^ 1) || (pl >> 5) != (lane >> 5) || pl * 16 / 1024 != lane * 16 / 1024) return 8;
    }
    // a lane's eight points of k-step kk: drow32(8 kk + e, h) = 16 kk + 4 h + (e & 3) + 8 (e >> 2): half s = e >> 2 reads g / gJ at float 16 kk + 4 h + 8 s
    for (int kk = 0; kk < 2; ++kk)
        for (int h = 0; h < 2; ++h)
            for (int e = 0; e < 8; ++e)
                if (drow32(8 * kk + e, h) != 16 * kk + 4 * h + 8 * (e >> 2) + (e & 3)) return 9;
    return 0;
}
int main() {
    if (int r = deal()) return r;
    if (int r = maps()) return 20 + r;
    std::puts("z0 table layout ok");
    return 0;
}
'''


def test_product_3_table_deal_and_the_forming_maps(tmp_path):
    src = tmp_path / 'z0_deal_test.cpp'
    src.write_text(DEAL_TEST)
    exe = tmp_path / 'z0_deal_test'
    subprocess.run(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'deepphysinet_amd', 'csrc'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, 'layout check %d failed' % out.returncode
    assert 'z0 table layout ok' in out.stdout


def test_the_kernels_use_the_maps_they_are_tested_on():
    csrc = os.path.join(ROOT, 'deepphysinet_amd', 'csrc')
    with open(os.path.join(csrc, 'dpn_wgrad.hip')) as f:
        src = f.read()
    for needle in ('wgrad_z0_piece(wave, j)', 'wgrad_z0_is_y(wave, j)', 'wgrad_z0_ct(wave)', 'wgrad_z0_kk(wave, 0)', 'wgrad_z0_kk(wave, 1)',
                   'z0_freq_index(ct, lane & 31)', '(lane ^ 1) * 16'):
        assert needle in src, needle
    # the slot keeps its size and the ring its depth: no new LDS area beside the per-wave g copies
    assert 'static constexpr int kGOff = kX + kY;' in src and 'static constexpr int kPadOff = kGOff + 8 * 256;' in src


def test_the_table_form_fits_the_space_of_the_stored_z0():
    """OperandView: table (768 B per point, net 0's two planes) + gJ (72 B per point, in net 1's space) inside the 4 608 B per point of the stored Z0,
    the header in the 1 024-byte slack behind gnet past the 128 bytes the last tile's 64-lane g copy reads."""
    for n_pad in (128, 1152, 37376):
        z0 = 6 * 2 * n_pad * 384
        table, gj_off, gj = 2 * n_pad * 384, 2 * n_pad * 384, 6 * 3 * n_pad * 4
        assert table == 768 * n_pad and gj_off + gj <= z0
        hdr_off, hdr = 256, 4 * (4 + 32)
        assert 128 <= hdr_off and hdr_off + hdr <= 1024 and hdr_off % 16 == 0

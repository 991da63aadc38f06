#!/usr/bin/env python
"""Static instruction census of a unit's kernels (no GPU needed): what the vector ALU has to issue beside the MFMAs.

    python tools/valu_census.py [--unit=I] [--all] [--opcodes] [-DFLAG | -fflag ...] [kernel-name substring ...]

The unit (default 0, the point kernels; an index into deepphysinet_amd.build.ALL_UNITS) is compiled to gfx950 assembly (-S --cuda-device-only) with that
unit's flags from build.py (minus -fPIC, as tools/kernel_isa_digest.py does) plus the extra flags given.  Per kernel -- by default the tile-split point
kernels, --all or name substrings select others -- it prints
  the instruction counts by category: every instruction of the body is counted once per OCCURRENCE in the text, loops are not weighted (the tile-split
  kernels are fully unrolled: the count is what a wave on the longest path issues, give or take the branches around saved-state stores), and
  .amdhsa_next_free_vgpr, .amdhsa_accum_offset, scratch bytes and LDS bytes of the kernel descriptor, with the workgroups per CU they allow.
--opcodes adds the line-level view: every opcode with its count, most frequent first.
Categories (a vector instruction is in exactly one of the rows between 'vector, not MFMA' and 'other vector'):
  sincos sites     v_rndne_f32: one per sincos_precise evaluation
  fp32 divisions   v_div_fixup_f32: one per IEEE division
  packed fp32      v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 (SLP vectorisation: an anti-lever beside MFMAs)
"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter, OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepphysinet_amd.build import ALL_UNITS, COMMON

DEFAULT_KERNELS = ('dpn_fwd_tiles_kernel', 'dpn_bwd_tiles_kernel', 'dpn_fwd_tiles_deriv_kernel', 'dpn_bwd_tiles_deriv_kernel')
INT_CMP = re.compile(r'v_(cmp|cmpx)_|v_(and|or|xor|not|lshl|lshr|ashr|lshlrev|lshrrev|ashrrev|bfe|bfi|bfm|add_u|add_i|add_co|addc|sub_u|sub_i|sub_co|subrev|mul_lo|mul_hi|mul_u|mul_i|mad_u|mad_i|lshl_add|lshl_or|and_or|or3|xor3|add3|add_lshl|alignbit|perm|min_u|min_i|max_u|max_i|mbcnt)')
FP32 = re.compile(r'v_(fma|fmac|fmaak|fmamk|mul|add|sub|subrev|mac|mad|max|min|med3|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|rndne|trunc|floor|fract|ldexp|sin|cos|exp|log|frexp)\w*_f32')


def demangle_key(name):
    m = re.match(r'_Z\d+(\w+?)ILi(\d)E', name)
    return '%s<%s>' % (m.group(1), m.group(2)) if m else name


def kernel_bodies(asm):
    out = OrderedDict()
    for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel', asm, re.M | re.S):
        name = m.group(1)
        start = asm.index('\n%s:' % name) + 1
        body = asm[start:asm.index('.Lfunc_end', start)]
        out[name] = (body, m.group(2))
    return out


def census(body):
    c = Counter()
    for ln in body.splitlines():
        ln = re.sub(r';.*', '', ln).strip()
        if not ln or ln.endswith(':') or ln.startswith('.'):
            continue
        op = ln.split()[0]
        c['instructions'] += 1
        c['op:' + re.sub(r'_e(32|64)$|_dpp$|_sdwa$', '', op)] += 1
        if op.startswith('v_mfma') or op.startswith('v_smfma'):
            c['MFMA'] += 1
        elif op.startswith('v_'):
            c['vector, not MFMA'] += 1
            if op in ('v_pk_add_f32', 'v_pk_mul_f32', 'v_pk_fma_f32'):
                c[op] += 1
                c['  packed fp32'] += 1
            elif op == 'v_cndmask_b32' or op.startswith('v_cndmask_b32'):
                c['  v_cndmask_b32'] += 1
            elif op.startswith('v_cvt_pk_bf16_f32'):
                c['  v_cvt_pk_bf16_f32'] += 1
            elif op.startswith('v_cvt_'):
                c['  other v_cvt'] += 1
            elif INT_CMP.match(op):
                c['  integer / compare'] += 1
            elif FP32.match(op):
                c['  fp32 arithmetic'] += 1
            elif op.startswith('v_mov') or op.startswith('v_accvgpr') or op.startswith('v_readlane') or op.startswith('v_readfirstlane') or op.startswith('v_writelane') or op.startswith('v_swap'):
                c['  moves / lane access'] += 1
            else:
                c['  other vector'] += 1
                c['other:' + op] += 1
            if op.startswith('v_rndne_f32'):
                c['sincos sites (v_rndne_f32)'] += 1
            if op.startswith('v_div_fixup_f32'):
                c['fp32 divisions (v_div_fixup_f32)'] += 1
        elif op == 's_nop':
            c['s_nop'] += 1
        elif op.startswith('s_waitcnt'):
            c['s_waitcnt'] += 1
        elif op.startswith('s_'):
            c['other scalar'] += 1
        elif op.startswith('ds_'):
            c['LDS (ds_*)'] += 1
        elif op.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
            c['vector memory'] += 1
            if op.startswith('scratch_'):
                c['  of which scratch_*'] += 1
        else:
            c['unclassified'] += 1
    return c


ROWS = ('instructions', 'vector, not MFMA', 'MFMA', 'sincos sites (v_rndne_f32)', 'fp32 divisions (v_div_fixup_f32)', '  v_cndmask_b32', '  v_cvt_pk_bf16_f32',
        '  other v_cvt', '  integer / compare', '  fp32 arithmetic', '  packed fp32', '  moves / lane access', '  other vector', 'v_pk_add_f32', 'v_pk_mul_f32',
        'v_pk_fma_f32', 's_nop', 's_waitcnt', 'other scalar', 'LDS (ds_*)', 'vector memory', '  of which scratch_*', 'unclassified')


def descriptor(desc):
    def val(key, default=0):
        m = re.search(r'\.%s\s+(\S+)' % key, desc)
        return int(m.group(1), 0) if m else default
    d = OrderedDict()
    d['.amdhsa_next_free_vgpr'] = val('amdhsa_next_free_vgpr')
    d['.amdhsa_accum_offset'] = val('amdhsa_accum_offset')
    d['.amdhsa_next_free_sgpr'] = val('amdhsa_next_free_sgpr')
    d['scratch bytes'] = val('amdhsa_private_segment_fixed_size')
    d['LDS bytes'] = val('amdhsa_group_segment_fixed_size')
    return d


def workgroups_per_cu(d, waves_per_wg=4):
    """256-thread workgroups: one wave per SIMD each.  512 unified registers per SIMD lane in allocation units of 8; 160 KB of LDS per CU."""
    regs = -(-max(d['.amdhsa_next_free_vgpr'], 1) // 8) * 8
    by_regs = 512 // regs
    by_lds = (160 * 1024) // d['LDS bytes'] if d['LDS bytes'] else 8
    return min(by_regs, by_lds, 8)


def main():
    unit, extra, names, show_all, opcodes = 0, [], [], False, False
    for a in sys.argv[1:]:
        if a.startswith('--unit='):
            unit = int(a.split('=')[1])
        elif a == '--all':
            show_all = True
        elif a == '--opcodes':
            opcodes = True
        elif a.startswith('-'):
            extra.append(a)
        else:
            names.append(a)
    src, flags, obj = ALL_UNITS[unit]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'unit.s')
        cmd = ['hipcc', *[f for f in COMMON if f != '-fPIC'], *flags, *extra, '--cuda-device-only', '-S', '-I' + os.path.join(ROOT, 'include'), src, '-o', out]
        subprocess.run(cmd, check=True)
        asm = open(out).read()
    print('# unit %d: %s   flags: %s' % (unit, os.path.basename(src), ' '.join([f for f in COMMON if f != '-fPIC'] + list(flags) + extra)))
    picked = []
    for name, (body, desc) in kernel_bodies(asm).items():
        key = demangle_key(name)
        if names:
            ok = any(n in key or n in name for n in names)
        else:
            ok = show_all or any(key.startswith(k + '<') for k in DEFAULT_KERNELS)
        if ok:
            picked.append((key, census(body), descriptor(desc)))
    picked.sort(key=lambda x: x[0])
    for key, c, d in picked:
        print('\n== %s' % key)
        for r in ROWS:
            if c[r] or not r.startswith(' '):
                print('  %-38s %6d' % (r, c[r]))
        others = sorted(((k[6:], v) for k, v in c.items() if k.startswith('other:')), key=lambda kv: -kv[1])
        if others:
            print('  other vector, by opcode: ' + ', '.join('%s %d' % kv for kv in others[:12]))
        if opcodes:
            ops = sorted(((k[3:], v) for k, v in c.items() if k.startswith('op:')), key=lambda kv: (-kv[1], kv[0]))
            for i in range(0, len(ops), 4):
                print('    ' + '  '.join('%-26s %5d' % kv for kv in ops[i:i + 4]))
        for k, v in d.items():
            print('  %-38s %6d' % (k, v))
        print('  %-38s %6d' % ('workgroups per CU (registers, LDS)', workgroups_per_cu(d)))


if __name__ == '__main__':
    main()

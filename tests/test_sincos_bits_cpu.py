"""CPU: sincos_precise of csrc/dpn_sincos.h (quadrant signs as shift-and-add on the bits) returns the bits of the form it replaced.

tests/sincos_bits.cpp holds the old form verbatim beside the header's; it is compiled for the host with -ffp-contract=off and compares s and c bit for
bit over every 61st fp32 pattern (7.04e7 values), +-0 / denormals / +-inf / NaNs, 2e6 values around the multiples of pi/2 up to |theta| = 1e4, and the
quadrant alone at the ends of the int range.  A few seconds; no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'deepphysinet_amd', 'csrc')


def _cxx():
    for c in ('g++', 'c++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    raise RuntimeError('no host C++ compiler')


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('sincos') / 'sincos_bits')
    subprocess.run([_cxx(), '-O2', '-std=c++17', '-ffp-contract=off', '-I' + CSRC, os.path.join(ROOT, 'tests', 'sincos_bits.cpp'), '-o', exe, '-lm'], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout


def test_new_quadrant_form_returns_the_old_bits(report):
    rc, out = report
    parts = dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in re.finditer(r'^([\w /]+): (\d+) values, (\d+) mismatches$', out, re.M))
    assert rc == 0, out
    assert set(parts) == {'sweep', 'special', 'multiples of pi/2', 'quadrant'}, out
    assert all(bad == 0 for _, bad in parts.values()), out
    assert parts['sweep'][0] >= (1 << 32) // 61                   # every 61st pattern, all of them
    assert parts['multiples of pi/2'][0] >= 1000000
    assert parts['special'][0] >= 18 and parts['quadrant'][0] >= 4000


def test_the_point_unit_uses_the_header():
    """one definition: dpn_point.hip includes the header and defines no sincos_precise of its own; the header's polynomial lines are the program's"""
    src = open(os.path.join(CSRC, 'dpn_point.hip')).read()
    hdr = open(os.path.join(CSRC, 'dpn_sincos.h')).read()
    prog = open(os.path.join(ROOT, 'tests', 'sincos_bits.cpp')).read()
    assert '#include "dpn_sincos.h"' in src and not re.search(r'void\s+sincos_precise\s*\(', src)
    poly = [ln.strip() for ln in prog.splitlines() if re.match(r'\s*(const float k|float r|r|const float r2|float sp|sp|float cp|cp) = ', ln)]
    assert len(poly) == 12                                          # reduction and polynomials of the old form
    for ln in poly:
        assert ln in hdr, ln

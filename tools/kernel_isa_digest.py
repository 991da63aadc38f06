"""One line per kernel of the library: mangled name, unit object, digest of its instruction stream, digest of its kernel descriptor.

    python tools/kernel_isa_digest.py > after.txt          # no GPU needed; the same on the commit to compare with, then diff the tables

Every entry of deepphysinet_amd.build.ALL_UNITS is compiled to gfx950 assembly with that unit's flags (minus -fPIC, as the hazard test does).
Body = the text from the kernel's label to its .Lfunc_end, without `;` comments, with the function index taken out of the local labels
(.LBB<i>_ -> .LBB_, .Ltmp<i> -> .Ltmp), the kernel's own mangled name written $self, and without the directive that returns to the kernel's
text section (.text, or the comdat .section .text.<name> of a template instantiation): it does not change when kernels move between units,
change their order inside one, are renamed or become template instantiations.
Descriptor = the .amdhsa_kernel ... .end_amdhsa_kernel block: register counts, LDS, scratch.  Two tables with equal digests for a kernel mean
the same code object for it; a name listed under two units is a template instantiated twice (it would link silently as a weak symbol).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepphysinet_amd.build import ALL_UNITS, COMMON


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def body_text(asm, name):
    start = asm.index('\n%s:' % name) + 1
    lines = (re.sub(r';.*', '', ln).rstrip() for ln in asm[start:asm.index('.Lfunc_end', start)].splitlines())
    text = '\n'.join(ln for ln in lines if ln and not re.match(r'\s*\.(text|section\s+\.text\.\S*)$', ln))
    return re.sub(r'\.Ltmp\d+', '.Ltmp', re.sub(r'\.LBB\d+_', '.LBB_', text.replace(name, '$self')))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for i, (src, flags, obj) in enumerate(ALL_UNITS):               # the units compile side by side
            out = os.path.join(tmp, '%d.s' % i)
            procs.append((obj, out, subprocess.Popen(['hipcc', *[f for f in COMMON if f != '-fPIC'], *flags, '--cuda-device-only', '-S',
                                                      '-I' + os.path.join(ROOT, 'include'), src, '-o', out])))
        for obj, out, pr in procs:
            if pr.wait() != 0:
                raise SystemExit('%s did not compile' % obj)
            asm = open(out).read()
            for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel', asm, re.M | re.S):
                print(m.group(1), obj, digest(body_text(asm, m.group(1))), digest(m.group(2)))


if __name__ == '__main__':
    main()

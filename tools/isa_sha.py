"""sha256 of the gfx950 disassembly of whole translation units' device code, to show that an edit left
every kernel of a unit instruction for instruction unchanged (tools/isa_digest.py does one kernel of a
-S listing with labels renumbered; this is the assembled code object, every kernel, nothing normalised).

    python tools/isa_sha.py [--tree DIR] [--defs="-DA -DB=1"] [unit ...]   (default units: simaps simaps_mixed)

Each unit csrc/<unit>.hip of the tree DIR (default: this one; another revision's checkout to compare)
is compiled with the Makefile's flags, device only, and `llvm-objdump -d` of the code object is
hashed without its first lines (the file name).  The source hash define is a host-side string and is
passed as a constant, so the same device source gives the same digest in any tree.  --defs is split on
blanks and appended to the hipcc line: the diag and prof targets' defines, to compare those builds too.
"""
import argparse
import hashlib
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')


def unit_sha(tree, unit, arch='gfx950', defs=''):
    csrc = os.path.join(tree, 'spatial-intention-maps_amd', 'csrc')
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, unit + '.co')
        subprocess.check_call([os.path.join(ROCM, 'bin', 'hipcc'), '-O3', '--offload-arch=' + arch, '-std=c++17',
                               '-ffp-contract=off', '-fPIC', '-I' + os.path.join(tree, 'include'), '-I' + csrc,
                               '-DSIMAPS_SOURCE_HASH="isa_sha"', '--cuda-device-only', '--no-gpu-bundle-output', '-c',
                               os.path.join(csrc, unit + '.hip'), '-o', co] + defs.split())
        dis = subprocess.check_output([os.path.join(ROCM, 'llvm', 'bin', 'llvm-objdump'), '-d', co]).decode()
    lines = dis.splitlines()
    body = [ln for ln in lines if 'file format' not in ln and not ln.startswith(co)]
    n_insn = sum(1 for ln in body if ln.startswith('\t'))
    return hashlib.sha256('\n'.join(body).encode()).hexdigest(), n_insn


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--defs', default='', help='extra hipcc arguments, written --defs="-DSIMAPS_PHASE_STAMPS"')
    ap.add_argument('units', nargs='*', default=['simaps', 'simaps_mixed'])
    args = ap.parse_args()
    for u in args.units:
        h, n = unit_sha(os.path.abspath(args.tree), u, defs=args.defs)
        print('%-20s %8d instructions  sha256 %s' % (u, n, h))

"""Shows that a change to csrc/resample.hip left the device code of the EXISTING resampler kernels alone.

Compiles resample.hip of a parent revision (git archive) and of the working tree to gfx950 code objects with the
library's flags, disassembles both, and diffs every kernel symbol the parent's code object holds, instruction by
instruction (addresses dropped, encodings kept).  Kernels that only the working tree has are listed, not compared.

    python tools/resample_isa_diff.py [--rev HEAD] [--out profiles/resample_indexed_isa.txt] [--src FILE.hip[=PARENT.hip] ...]
                                      [--define NAME=VALUE ...]

--define adds -DNAME=VALUE to the parent's and the tree's compile alike, so builds that only a switch selects are compared
too (profiles/wino_body_split_isa.txt: --src conv_wino.hip, once plain and once per ablation, e.g. --define WINO_ABL=64).

--src names other files of csrc/ (each with its per-file flags of csrc/build.py), e.g. the wide Winograd family
(profiles/wide_wino_shared_isa.txt: --src wino_fused.hip wino_fused_f16x3.hip wino_gemm.hip).  FILE.hip=PARENT.hip says
that the tree's FILE.hip holds kernels that the parent kept in PARENT.hip: the tree files that name one parent file are
taken together, so a kernel that moved is compared with the parent's instead of being listed as new
(profiles/splat_split_isa.txt: --src resample.hip splat.hip=resample.hip).

The kernels that exist as a plain and an indexed form are written once (csrc/resample_gather.inc, included twice by
resample.hip) and keep their names, so a change to that file is checked here like any other: every symbol of both forms
against the parent's (profiles/resample_shared_isa.txt is the report of the change that folded the two copies into one).

The report's diff section is empty when nothing changed; the exit status is 1 otherwise.  Needs hipcc, no GPU.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latentfusion_amd.csrc import build as hip_build  # noqa: E402

CSRC = os.path.join('latentfusion_amd', 'csrc')


def _objdump():
    hipcc = hip_build._hipcc()
    for cand in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), '..', 'llvm', 'bin', 'llvm-objdump'),
                 '/opt/rocm/llvm/bin/llvm-objdump'):
        if os.path.exists(cand):
            return cand
    return 'llvm-objdump'


def disassemble(tree, workdir, tag, src='resample.hip', defines=()):
    """{symbol: [instruction lines]} of the gfx950 code object of csrc/`src` in `tree`."""
    co = os.path.join(workdir, tag + '.' + src + '.co')
    cmd = [hip_build._hipcc(), '-x', 'hip', '--cuda-device-only', '--no-gpu-bundle-output', '-c', os.path.join(tree, CSRC, src), '-o', co]
    cmd += [f for f in hip_build.FLAGS if f != '-fPIC'] + hip_build.EXTRA.get(src, []) + ['-D' + d for d in defines]
    subprocess.run(cmd, check=True)
    text = subprocess.run([_objdump(), '-d', '--no-leading-addr', co], check=True, stdout=subprocess.PIPE).stdout.decode()
    syms, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]*\s*<(.+)>:$', line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip() not in ('', '...'):
            # ('...' is elided zero padding behind a symbol: it depends on what follows the kernel in its file, not on the kernel)
            # "\tinsn operands   // 000000020C10: BF88003C <sym+0x104>": the address goes, the encoding and the target stay
            cur.append(re.sub(r'//\s*[0-9A-Fa-f]+:', '//', line).rstrip())
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rev', default='HEAD')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_indexed_isa.txt'))
    ap.add_argument('--src', nargs='+', default=['resample.hip'], help='files of csrc/ to compare')
    ap.add_argument('--define', action='append', default=[], metavar='NAME=VALUE', help='-D for the parent and the tree compile')
    a = ap.parse_args()
    rev = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', a.rev], check=True, stdout=subprocess.PIPE).stdout.decode().strip()
    lines, diff, nsym = [], [], 0
    with tempfile.TemporaryDirectory() as tmp:
        parent = os.path.join(tmp, 'parent')
        os.makedirs(parent)
        ar = subprocess.run(['git', '-C', ROOT, 'archive', a.rev, 'latentfusion_amd/csrc', 'include'], check=True, stdout=subprocess.PIPE)
        subprocess.run(['tar', '-x', '-C', parent], input=ar.stdout, check=True)
        origin = {}                                       # parent file -> the tree files that hold its kernels now
        for item in a.src:
            src, _, old_src = item.partition('=')
            origin.setdefault(old_src or src, []).append(src)
        for old_src, srcs in origin.items():
            old = disassemble(parent, tmp, 'parent', old_src, a.define)
            new = {}
            for src in srcs:
                new.update(disassemble(ROOT, tmp, 'tree', src, a.define))
            lines += [f'# {os.path.join(CSRC, old_src)}: kernel symbols of revision {rev} against {", ".join(srcs)} of the working tree, gfx950, '
                      f'flags {" ".join(hip_build.FLAGS + hip_build.EXTRA.get(old_src, []) + ["-D" + d for d in a.define])}',
                      '# symbol: instructions (parent / tree)']
            for name in sorted(old):
                lines.append(f'#   {name}: {len(old[name])} / {len(new.get(name, []))}')
                diff += list(difflib.unified_diff(old[name], new.get(name, []), 'parent:' + name, 'tree:' + name, lineterm='', n=2))
            lines.append('# symbols only in the tree (not compared):')
            lines += [f'#   {name}: {len(new[name])}' for name in sorted(new) if name not in old]
            nsym += len(old)
    lines.append(f'# diff over the {nsym} parent symbols ({len(diff)} lines):')
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines + diff) + '\n')
    print(f'{nsym} symbols compared, {len(diff)} diff lines -> {a.out}')
    return 1 if diff else 0


if __name__ == '__main__':
    sys.exit(main())

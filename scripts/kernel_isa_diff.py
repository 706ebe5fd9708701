"""gfx950 device assembly of the GEMM kernels, this tree against another revision: `python scripts/kernel_isa_diff.py REV`.

Compiles gemm.hip, gemm_split.hip and gemm_nn2.hip of both trees with the library's flags (+ --cuda-device-only -S) and prints one line
per kernel: whether the instruction text is identical, and agpr/vgpr/sgpr/spill/scratch/lds/instructions of REV and of this tree.  Kernels
are matched by name; what is left over on both sides (a changed template list) is paired in file order."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qagnn_amd.build import FLAGS  # noqa: E402

FILES = ['gemm.hip', 'gemm_split.hip', 'gemm_nn2.hip']
KEYS = ['vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size']


def assemble(root, src, out):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc] + FLAGS + ['-w', '--cuda-device-only', '-S', '-o', out, os.path.join(root, 'qagnn_amd', 'csrc', src)])
    return out


def kernels(path):
    """[(demangled name, instruction text, figures)] of one .s file, in file order"""
    txt = re.sub(r'__hip_cuid_\w+', '__hip_cuid_0', open(path).read())
    res = []
    for blk in txt.split('  - .agpr_count:')[1:]:
        get = lambda k: re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)  # noqa: E731
        sym = get('name')
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(sym), txt, re.M | re.S).group(1).replace(sym, 'KERNEL')
        body = re.sub(r'\.LBB\d+_', '.LBB_', body)
        insns = len(re.findall(r'^\t[a-z]', body, re.M))
        dem = subprocess.run(['c++filt', sym], capture_output=True, text=True).stdout.strip().split('(')[0]
        res.append((dem.replace('void qagnn::', ''), body, [blk.split('\n')[0].strip()] + [get(k) for k in KEYS] + [str(insns)]))
    return res


def compare(old, new):
    """one line per kernel; returns the number of kernels that are not identical"""
    left = [k for k in old if k[0] not in {n[0] for n in new}]
    n_diff = 0
    for name, body, fig in new:
        o = next((k for k in old if k[0] == name), None) or (left.pop(0) if left else None)
        tag = 'new' if o is None else 'identical' if o[1] == body else 'differs'
        n_diff += tag != 'identical'
        print('%-72s %-9s  %s | %s' % (name[:72], tag, '/'.join(o[2]) if o else '-', '/'.join(fig)))
    for name, _, fig in left:
        print('%-72s %-9s  %s | -' % (name[:72], 'gone', '/'.join(fig)))
    return n_diff + len(left)


if __name__ == '__main__':
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, 'old')
        os.mkdir(old_root)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'qagnn_amd/csrc', 'include'], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', old_root], input=tar, check=True)
        print('%-72s %-9s  agpr/vgpr/sgpr/spill/scratch/lds/insns: %s | this tree' % ('kernel', '', rev))
        n = sum(compare(kernels(assemble(old_root, s, os.path.join(tmp, 'old.s'))), kernels(assemble(ROOT, s, os.path.join(tmp, 'new.s')))) for s in FILES)
        print('%d kernel(s) not identical' % n)

#!/usr/bin/env python3
"""Static size of the output passes of the fused F(4x4,3x3) kernel (csrc/ct_wino4f.hip): cross-compiles the file to gfx950
assembly (no GPU needed) and counts, per instantiation, the instructions of each of the four output quarters of an item -- from
the barrier that ends the previous phase to the barrier that ends the quarter -- by kind, next to the kernel's register metadata.
    python tools/w4f_isa_count.py [kernel-name-substring ...]  >  profiles/w4f_epilogue_isa.txt
A quarter's count includes both sides of its branches (the partial-row block of the lean epilogue, the per-row blocks of the old
one), so it is an upper bound of what a wave issues."""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'context-transformer_amd')
KINDS = [('v_readlane', 'v_readlane'), ('v_writelane', 'v_writelane'), ('s_nop', 's_nop'), ('v_max', 'v_max'), ('v_cndmask', 'v_cndmask'),
         ('v_cmp', 'v_cmp'), ('s_cbranch', 'cbranch'), ('ds_read', 'ds_read'), ('ds_write', 'ds_write'), ('buffer_store', 'buffer_store'),
         ('global_', 'global'), ('s_waitcnt', 's_waitcnt'), ('s_load', 's_load')]


def kind(op):
    if 'saveexec' in op:
        return 'saveexec'
    for prefix, name in KINDS:
        if op.startswith(prefix):
            return name
    return 'other_s' if op.startswith('s_') else 'other_v'


def main():
    hipcc = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'w4f.s')
        subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + os.path.join(REPO, 'include'), '-I' + os.path.join(PKG, 'csrc'),
                        '-x', 'hip', '--cuda-device-only', '-S', os.path.join(PKG, 'csrc', 'ct_wino4f.hip'), '-o', out],
                       check=True, stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    text = '\n'.join(lines)
    meta = {}
    for m in re.finditer(r'\.name:\s+(\S*wino_f4x4_3x3_x3\S*)\n(.*?)\.wavefront_size', text, re.S):
        meta[m.group(1)] = {k: int(v) for k, v in re.findall(r'\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)', m.group(2))}
    for name in sorted(meta):
        if sys.argv[1:] and not any(s in name for s in sys.argv[1:]):
            continue
        i0 = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
        i1 = next(i for i in range(i0, len(lines)) if 's_endpgm' in lines[i])
        ops = [ln.split()[0] for ln in lines[i0 + 1:i1 + 1] if ln.startswith('\t') and not ln.strip().startswith(('.', ';'))]
        tail = ops[max(k for k, op in enumerate(ops) if op.startswith('v_mfma')) + 1:]
        bars = [k for k, op in enumerate(tail) if op == 's_barrier']
        flags = re.search(r'ILb(\d)ELb(\d)ELb(\d)ELb(\d)E', name).groups()
        print('%s\n   <SEG %s, PLAIN %s, H2 %s, LEAN %s>  %s  instructions %d' % (name, *flags, ' '.join('%s %d' % kv for kv in sorted(meta[name].items())), len(ops)))
        if len(bars) not in (8, 9):
            print('   (the compiler laid this instantiation out otherwise -- not eight or nine barriers behind the last MFMA: no per-quarter split)')
            continue
        # (accumulators -> LDS, barrier, transform + epilogue, barrier) x 4; the first quarter starts at the main loop's last barrier
        edge = [bars[-9] if len(bars) > 8 else -1] + [bars[-8 + 2 * q + 1] for q in range(4)]
        for q in range(4):
            seg = tail[edge[q] + 1:edge[q + 1] + 1]
            c = collections.Counter(kind(op) for op in seg)
            print('   quarter %d: %4d instructions   %s' % (q, len(seg), ' '.join('%s %d' % kv for kv in sorted(c.items()))))


if __name__ == '__main__':
    main()

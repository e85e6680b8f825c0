"""The bench.py contract on the device: one JSON line with the fields the driver and the judge read, a roofline
fraction that IS a fraction (executed matrix-pipe work / peak), stage rooflines from the library's profile scopes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_contract():
    d = _run('--full', '--steps', '3', '--warmup', '4', '--batch', '4', '--no-cpu-baseline', '--no-other-configs')
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['scaling'] == 'weak' and d['dtype'] == 'f32' and d['vs_baseline'] is None
    assert d['launch_mode'] == 'hipGraph replay'
    assert abs(d['value'] - 4 / (d['ms_per_step'] * 1e-3)) < 0.02 * d['value']
    r = d['roofline']
    # the dominant kernel's own pipe: fp32 MFMA, or the bf16 MFMA for a bf16x3 kernel (six bf16 products per fp32 multiply-add)
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s'
    # kernels on the 16-bit matrix pipe: bf16x3 (direct, fused Winograd, the GEMM kernel of the three-kernel F(4x4) form) or the
    # f16x2 twins of the same kernels (three piece products instead of six)
    on_h2 = r['kernel'].startswith('conv_h2_f32') or '_h2' in r['kernel']
    on_bf16 = on_h2 or r['kernel'].startswith('conv_x3_f32') or '_x3' in r['kernel'] or r['kernel'].startswith('wino4s')
    assert r['peak'] == (2500.0 if on_bf16 else 157.3)
    assert 0.0 < r['frac'] <= 1.0 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    if r['kernel'].startswith('conv_x3_f32') or r['kernel'].startswith('conv_h2_f32'):
        assert abs(r['flops_per_launch'] / r['algorithmic_flops_per_launch'] - (3.0 if on_h2 else 6.0)) < 1e-6
    assert 'arith' in d and 'bf16x3' in d['arith'] and 'f16x2' in d['arith']
    assert d['config']['operand_form'] in ('f16x2', 'bf16x3') and d['config']['live_tuned_layers']['count'] == 0
    # every kernel-choice switch in force is on the line (engine.Runtime.policy_record), and the fraction that compares across operand forms
    pol = d['config']['policy']
    assert pol['operand_form'] == d['config']['operand_form'] and pol['live_tuned_layers'] == 0 and pol['tune_table'] == 'conv_tune_gfx950.json'
    assert isinstance(pol['env'], dict) and all(k.startswith('CTDET_') for k in pol['env'])
    assert abs(r['frac_bf16x3_equivalent'] - r['frac'] * (2.0 if on_h2 else 1.0)) < 1e-3
    assert len(d['per_rank_ms_per_step']) == 1 and d['dist']['rccl_ranks'] == 1
    if r['kernel'] == 'wino4s_gemm':
        # a three-kernel launch dominates: kernel-level fields = its matrix kernel, launch-level ones kept beside them
        assert r['dominant_launch']['kernel'].startswith('wino4s') and r['dominant_launch']['avg_launch_us'] > r['avg_launch_us']
        assert r['stages']['wino4s_in']['bound'] == 'hbm' and r['stages']['wino4s_out']['bound'] == 'hbm'
        assert 0 < r['stages']['wino4s_in']['frac'] < 1 and 0 < r['stages']['wino4s_out']['frac'] < 1
    elif r['kernel'].startswith('wino'):
        assert r['winograd_mult_ratio'] in (round(16 / 36, 4), 0.25)
        assert abs(r['flops_per_launch'] / r['algorithmic_flops_per_launch'] - r['winograd_mult_ratio'] * (3 if on_h2 else 6 if on_bf16 else 1)) < 1e-3
        assert r['algorithmic_frac'] > r['frac']
    st = r['stages']
    for k in ('detect_kernel', 'select_sort_kernel', 'nms_segments_kernel'):
        assert st[k]['avg_launch_us'] > 0 and 0 < st[k]['frac'] < 1 and st[k]['algorithmic_per_launch'] > 0, k
    assert st['nms_segments_kernel']['launches_per_step'] == 2.0


def test_bench_phase2_reports_the_attention_stage():
    d = _run('--full', '--steps', '2', '--warmup', '4', '--batch', '2', '--phase', '2', '--classes', '60', '--no-cpu-baseline',
             '--no-other-configs')
    st = d['roofline']['stages']
    assert st['ctx_attn_kernel']['bound'] == 'mfma' and 0 < st['ctx_attn_kernel']['frac'] < 1
    assert st['ctx_attn_kernel.hbm']['bound'] == 'hbm'
    assert st['ctx_attn_kernel']['piece_products'] == 6          # bf16x3 unless CTDET_ATTN_H2=1 (opt-in: DESIGN.md section 8 item 9)


def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """Without --full the line carries the headline fields only (no roofline, other configurations or CPU baseline);
    --dump-outputs writes what the timed path returned at its last step, and a second run with the same arguments
    writes the same arrays."""
    import numpy as np
    d = _run('--steps', '3', '--warmup', '3', '--batch', '4', '--dump-outputs', str(tmp_path / 'a'))
    _run('--steps', '3', '--warmup', '3', '--batch', '4', '--dump-outputs', str(tmp_path / 'b'))
    assert d['steps'] == 3 and d['warmup'] == 3 and d['ms_per_step'] > 0 and d['launch_mode'] == 'hipGraph replay'
    assert abs(d['value'] - 4 / (d['ms_per_step'] * 1e-3)) < 0.02 * d['value']
    assert d['roofline'] is None and d['cpu_baseline'] is None and d['other_configs'] is None
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['boxes.npy', 'detection_counts.npy', 'detections.npy', 'scores.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64e6
    out = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    assert all(v.dtype == np.float32 for v in out.values())
    dets, cnt = out['detections'], out['detection_counts']
    assert dets.shape[:2] == cnt.shape == (4, 20) and dets.shape[3] == 5
    assert int(cnt.sum()) == d['config']['detections_per_batch'] > 0
    for b in range(4):
        for c in range(20):
            k = int(cnt[b, c])
            assert not dets[b, c, k:].any() and (np.diff(dets[b, c, :k, 4]) <= 0).all()      # rows in descending score order
    for f in files:
        assert np.array_equal(out[f[:-4]], np.load(tmp_path / 'b' / f)), f

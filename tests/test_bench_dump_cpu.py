"""bench.py --dump-outputs on the host: the sample of a large output is fixed and made of its own elements, the files
stay within the 64 MB bound, and only the rows [0, count) of a class carry detections."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(REPO, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    bench = _bench()
    big = torch.randn(3_000_000, generator=torch.Generator().manual_seed(1))
    arrays = [('loss', torch.tensor([0.5], dtype=torch.float64), 1), ('small', big[:1000].view(10, 100), 1 << 20),
              ('big', big, 1 << 20)]
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    bench.dump_outputs(str(tmp_path / 'b'), arrays)
    loss, small, sample = (np.load(tmp_path / 'a' / (n + '.npy')) for n in ('loss', 'small', 'big'))
    assert loss.dtype == np.float64 and loss.tolist() == [0.5]
    assert small.dtype == np.float32 and np.array_equal(small, big[:1000].view(10, 100).numpy())
    assert sample.shape == (1 << 20,) and np.array_equal(sample, np.load(tmp_path / 'b' / 'big.npy'))
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(big.numel(), 1 << 20, replace=False))
    assert np.array_equal(sample, big.numpy()[idx])
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / 'c'), [('too_big', torch.zeros(17_000_000), 1 << 25)])


def test_inference_outputs_zero_the_rows_past_each_count(tmp_path):
    bench = _bench()
    B, T, cap, P = 2, 3, 16, 50
    g = torch.Generator().manual_seed(2)
    cnt = torch.tensor([[0, 5, 16], [3, 1, 7]], dtype=torch.int32)
    post = types.SimpleNamespace(out_dets=torch.rand(B, T, cap, 5, generator=g) + 1, out_count=cnt,
                                 overflow=torch.zeros(1, dtype=torch.int32), cap=cap)
    pipe = types.SimpleNamespace(post=post, boxes=torch.rand(B, P, 4, generator=g), scores=torch.rand(B, P, T + 1, generator=g))
    bench.dump_outputs(str(tmp_path), bench.inference_outputs(pipe))
    dets = np.load(tmp_path / 'detections.npy')
    assert np.array_equal(np.load(tmp_path / 'detection_counts.npy'), cnt.numpy().astype(np.float32))
    for b in range(B):
        for c in range(T):
            k = int(cnt[b, c])
            assert np.array_equal(dets[b, c, :k], post.out_dets[b, c, :k].numpy()) and not dets[b, c, k:].any()
    assert np.array_equal(np.load(tmp_path / 'scores.npy'), pipe.scores.numpy())
    post.overflow[0] = 1
    with pytest.raises(SystemExit):
        bench.inference_outputs(pipe)

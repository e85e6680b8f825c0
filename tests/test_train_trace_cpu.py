"""The launches of one whole training step on the shipped plans, call by call and argument by argument, against a golden recorded
before ctdet/train_engine.py was restructured (tests/train_trace.py records; tools/gen_train_trace.py wrote the golden and dumps
full traces for a diff by hand).  The golden is not regenerated for a refactor: a changed digest means the refactor changed what is
launched.  The per-entry-point counts say where to look first."""
import json
import os

import pytest

import train_trace
from ctdet import wgrad_routes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_trace.json')


def _trace(case, monkeypatch):
    _, net, env, mode = case
    return train_trace.trace(net, env, mode, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))


@pytest.mark.parametrize('case', train_trace.CASES, ids=[c[0] for c in train_trace.CASES])
def test_training_step_launches_what_the_golden_recorded(case, monkeypatch):
    log, pointers, unnamed = _trace(case, monkeypatch)
    assert not unnamed, 'pointer arguments outside every named tensor: %s' % sorted(set(unnamed))
    assert train_trace.UNNAMED not in train_trace.canonical(log)
    got = train_trace.summary(log, pointers)
    want = json.load(open(GOLDEN))[case[0]]
    assert got['calls'] == want['calls']
    assert got['pointers'] == want['pointers']
    assert got['sha256'] == want['sha256']
    if case[0] == '300p2-default':              # not the trace of an empty walk
        calls = got['calls']
        need = ['ct_conv2d_wino4s_fwd', 'ct_conv2d_wino4f_pool_fwd_v', 'ct_conv2d_x3_fwd', 'ct_maxpool2x2_bias_relu_bwd',
                'ct_bn_train_backward', 'ct_head_grad_gather', 'ct_pack_run', 'ct_conv_x3_pack_run', 'ct_conv_wino_h2_pack_run']
        need += [r.launch for r in wgrad_routes.ROUTES.values() if r.name != 'h2']      # h2 is opt-in (CTDET_WGRAD_H2)
        assert all(calls.get(n, 0) >= 1 for n in need), [n for n in need if not calls.get(n)]
    if case[3] == 'again':                      # the cached lists are replayed, not rebuilt
        assert not [n for n in got['calls'] if n.endswith(('_pack_item', '_record_begin', '_record_end'))]
        assert all(got['calls'][n] == 1 for n in ('ct_pack_run', 'ct_conv_x3_pack_run', 'ct_conv_wino_h2_pack_run'))
    if case[3] == 'retile':                     # ... and rebuilt when a layer changed kernels
        assert got['calls']['ct_pack_record_begin'] == 1 and got['calls']['ct_conv_wino_h2_pack_item'] >= 1
        assert got['calls']['ct_conv_x3_pack_item'] >= 1


def test_opt_in_weight_gradient_route_is_traced(monkeypatch):
    log, _, _ = _trace(('', '300p2', 'wgrad_h2_1', 'step'), monkeypatch)
    assert any(e[0] == wgrad_routes.ROUTES['h2'].launch for e in log)

"""The case table of tests/ctx_block_cases.py can fail for the right reason: on the float64 reference alone (no GPU, no
libctdet.so) the regimes are what their labels say, every listed edge value is in the table, and four modelled kernel faults move
the reference by far more than the 1e-4 tests/test_gpu_ctx_block.py holds the kernels to.

Margins.  (a) / (b): 1e-2 of the tensor's range, 100x the bound, wherever the unmasked padding would carry at least a quarter of a
uniform softmax row (share = n_pad / M_pad; the measurements behind the 1e-2 were taken at 26 of 96 keys and more; here 1.4e-2 to
3.9e-1).  Where the padding is ONE key of 32 ... 128 (M = 31, 63, 127) or 28 of 288 (M = 260) no draw reaches 1e-2 -- amplitudes
0.025 ... 0.25 and five seeds each gave 1.1e-4 ... 4.5e-3 for M = 31 / 63 / 127 and 2.4e-3 ... 7.6e-3 for M = 260 in the forward,
5.9e-3 ... 7.8e-3 for fault (b) at M = 127: the fault moves the row by its share and no more -- and those rows are held to 3e-4,
three times the bound (the kernels sit 1e-6 from float64 there, so a GPU run with the fault still fails).  (b) is asserted in the
diffuse and mixed regimes only: in the peaked and tie rows a zero pool row has no weight (moved: 1e-15 ... 3e-3), which is the
reason those regimes cannot test the mask.  (c) / (d): 1e-3, ten times the bound, every diffuse row.
d = 1 is exempt from (a) and (c): its output is +-scale * obj_w whatever the softmax does."""
import pytest

import ctx_block_cases as cc

MARGIN, MARGIN_LOW_SHARE, MARGIN_CD = 1e-2, 3e-4, 1e-3


def _pad_margin(case, multiple):
    M_pad = -(-case.M // multiple) * multiple
    return MARGIN if (M_pad - case.M) / M_pad >= 0.25 else MARGIN_LOW_SHARE


def _ids(cases):
    return [c.name for c in cases]


def test_case_table_covers_every_listed_edge():
    diffuse = cc.by_regime('diffuse')
    for field, values in cc.LISTED.items():
        have = {getattr(c, field) for c in diffuse}
        assert set(values) <= have, (field, sorted(set(values) - have))
    for split, (lo, hi) in cc.P_RANGES.items():
        rows = [c for c in diffuse if lo <= c.P <= hi]
        assert rows and all(c.kv_split == split for c in rows), (split, rows)
        # valid queries in the last 32-query tile of the last slice: its tail is work, not padding
        assert any(c.P > -(-c.P // cc.QB) * cc.QB - cc.KT for c in rows), split
    assert any(c.kv_split == 2 for c in diffuse)
    nt = lambda c: -(-c.P // cc.QB) * cc.QB // cc.KT
    assert any(c.kv_split > 1 and nt(c) % c.kv_split for c in diffuse), 'no uneven split of the query tiles'
    assert {c.incre for c in diffuse} == {False, True} and {1, 3} <= {c.B for c in diffuse}
    assert {c.regime for c in cc.CASES} == set(cc.AMP)
    assert max(c.B for c in cc.CASES) <= 3 and max(c.P for c in cc.CASES) <= 1024 and max(c.M for c in cc.CASES) <= 260
    assert len(set(cc.IDS)) == len(cc.CASES)
    assert any(c.fwd_only for c in diffuse)


@pytest.mark.parametrize('case', cc.by_regime('diffuse', 'peaked'), ids=_ids(cc.by_regime('diffuse', 'peaked')))
def test_regime_labels_mean_something(case):
    neff, pmax = cc.softmax_stats(case)
    if case.regime == 'peaked':
        assert neff <= 1.5, (case.name, neff, pmax)
    elif case.M >= 31:
        assert neff >= case.M / 4, (case.name, neff, pmax)


@pytest.mark.parametrize('case', cc.by_regime('tie'), ids=_ids(cc.by_regime('tie')))
def test_tie_rows_share_their_maximum_between_the_first_and_the_last_key_tile(case):
    inp = cc.inputs(case)
    theta, phi = cc._theta_phi(inp.conf, inp.pool, inp.p)
    for b, (j, j2) in enumerate(inp.tie):
        assert j < cc.KT and j2 // cc.KT == (case.M - 1) // cc.KT > 0 and (inp.pool[b, j] == inp.pool[b, j2]).all()
        s = theta[b] @ phi[b].t()
        tied = s.max(1).values == s[:, j]
        assert int(tied.sum()) >= 1, (case.name, b)
        assert (s[tied, j] == s[tied, j2]).all()


_A = [c for c in cc.by_regime('diffuse', 'mixed') if c.M % 32 and not c.fwd_only]


@pytest.mark.parametrize('case', _A, ids=_ids(_A))
def test_fault_a_unmasked_padding_keys_move_the_output(case):
    out, _ = cc.fault_pad_keys(case, 32)
    m = cc.moved(out, cc.reference(case).out)
    assert m >= _pad_margin(case, 32), (case.name, m)


_B = [c for c in cc.by_regime('diffuse', 'mixed') if c.M % 128 and not c.fwd_only]


@pytest.mark.parametrize('case', _B, ids=_ids(_B))
def test_fault_b_unmasked_backward_padding_moves_dphi_w_or_dpool(case):
    ref = cc.reference(case)
    _, g = cc.fault_pad_keys(case, 128)
    m = cc.moved(g['pool'], ref.grads['pool'])
    if case.M > 1:                          # M = 1: dphi_w is exactly zero in the reference
        m = max(m, cc.moved(g['phi_w'], ref.grads['phi_w']))
    assert m >= _pad_margin(case, 128), (case.name, m)


_CD = [c for c in cc.by_regime('diffuse') if c.M >= 2 and not c.fwd_only]


@pytest.mark.parametrize('case', _CD, ids=_ids(_CD))
def test_fault_c_last_key_masked_and_fault_d_query_tail_dropped(case):
    ref = cc.reference(case)
    out, _ = cc.fault_drop_last_key(case)
    mc = cc.moved(out, ref.out)
    md = cc.moved(cc.fault_drop_query_tail(case)['pool'], ref.grads['pool'])
    assert mc >= MARGIN_CD and md >= MARGIN_CD, (case.name, mc, md)


def test_exact_zeros_of_the_reference():
    """What the GPU test judges on an absolute scale: phi_b always (the rows of dS sum to zero), theta / phi with a single key;
    and d = 1, where the output does not depend on the softmax at all."""
    for case in cc.CASES:
        ref = cc.reference(case)
        if case.fwd_only:
            assert not ref.grads
            for fault in (cc.fault_pad_keys(case, 32)[0], cc.fault_drop_last_key(case)[0]):
                assert cc.moved(fault, ref.out) == 0.0
            continue
        scale = float(ref.grads['g_w'].abs().max())
        for k in ref.zero:
            assert float(ref.grads[k].abs().max()) <= 1e-12 * scale, (case.name, k)
        assert set(ref.e32) == {'out'} | (set(ref.grads) - set(ref.zero))

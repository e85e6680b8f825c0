"""The mining-free focal classification terms (conf_loss='focal') as far as they can be checked without a GPU: the float64
twin itself, the criterion's torch path against the twin, and the surface (header, binding, switches, C ABI refusals,
focal_prior_init).  Tolerances are the project's loss rule (tests/iou_loss_cases.py: check_loss / check_grad): each loss
within 2e-5 * max(1, |ref|), each gradient within 2e-5 * max|ref grad| + 1e-9 in max-norm, all gradients finite."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from ctdet import _lib
from layers.modules.multibox_loss_combined import MatchedTargets, MultiBoxLoss_combined, focal_prior_init

import focal_loss_ref as twin
import iou_loss_cases as cases


def _crit(ncls=21, **kw):
    return MultiBoxLoss_combined(ncls, 0.5, True, 0, True, 3, 0.5, False, **kw)


def _run_torch_path(c, pred, gamma, alpha, conf_t=None, **kw):
    pred = [p.clone().requires_grad_(True) for p in pred]
    crit = _crit(c.ncls, fused=False, conf_loss='focal', focal_gamma=gamma, focal_alpha=alpha, **kw)
    out = crit(pred, c.priors, MatchedTargets(c.loc_t, c.conf_t if conf_t is None else conf_t, c.obj_t))
    sum(out.values()).backward()
    return out, [p.grad for p in pred]


# ------------------------------------------------------------------------------------ 1: the twin
def test_twin_at_gamma_0_without_alpha_is_cross_entropy_over_every_row_that_is_not_ignored():
    c = cases.case('A_mixup_ignored')
    assert (c.conf_t[..., 0] < 0).any()
    conf, obj = c.pred[1].double(), c.pred[2].double()
    w = torch.where(c.conf_t[..., 0] >= 0, c.conf_t[..., 1], torch.zeros(())).double()
    logit = torch.cat((obj[..., :1] + torch.logsumexp(conf, -1, keepdim=True), obj[..., 1:2] + conf), -1).view(-1, c.ncls)
    cls = (F.cross_entropy(logit, c.conf_t[..., 0].long().clamp_min(0).view(-1), reduction='none') * w.view(-1)).sum()
    ob = (F.cross_entropy(obj.view(-1, 2), c.obj_t.long().view(-1), reduction='none') * w.view(-1)).sum()
    got_c, got_o = twin.focal_sums(conf, obj, c.conf_t, c.obj_t, 0.0, -1.0)
    print('cls %.12g / %.12g, obj %.12g / %.12g' % (float(got_c), float(cls), float(got_o), float(ob)))
    assert abs(float(got_c) - float(cls)) <= 1e-12 * float(cls) and abs(float(got_o) - float(ob)) <= 1e-12 * float(ob)
    assert float(cls) > 1000 and float(ob) > 1000              # tens of thousands of rows, not a mined sample


def test_twin_on_rows_worked_by_hand():
    """Two classes, uniform logits: s = (1/2, 1/2), q = (1/2, 1/2), so p = (1/2, 1/4, 1/4)."""
    conf, obj = torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64)
    conf_t = torch.tensor([[0.0, 1.0], [2.0, 0.5]])
    obj_t = torch.tensor([False, True])
    cls, ob = twin.focal_sums(conf, obj, conf_t, obj_t, 2.0, 0.25)
    want_cls = 0.75 * 0.5 ** 2 * math.log(2) + 0.5 * 0.25 * 0.75 ** 2 * math.log(4)
    want_obj = 0.75 * 0.5 ** 2 * math.log(2) + 0.5 * 0.25 * 0.5 ** 2 * math.log(2)
    assert abs(float(cls) - want_cls) < 1e-15 and abs(float(ob) - want_obj) < 1e-15
    cls, ob = twin.focal_sums(conf, obj, conf_t, obj_t, 0.5, -1.0)
    assert abs(float(cls) - (math.sqrt(0.5) * math.log(2) + 0.5 * math.sqrt(0.75) * math.log(4))) < 1e-15
    # 0^0 = 1: a saturated row at gamma = 0 keeps its cross-entropy, and is 0 for any gamma > 0
    obj = torch.tensor([[800.0, -800.0]], dtype=torch.float64)
    one = (conf[:1], obj, torch.tensor([[0.0, 1.0]]), torch.tensor([True]))
    assert float(twin.focal_sums(*one, 0.0, -1.0)[1]) == 1600.0 and float(twin.focal_sums(*one, 2.0, -1.0)[1]) == 1600.0
    one = (conf[:1], obj, torch.tensor([[0.0, 1.0]]), torch.tensor([False]))
    assert float(twin.focal_sums(*one, 0.0, -1.0)[1]) == 0.0 and float(twin.focal_sums(*one, 2.0, -1.0)[1]) == 0.0


# ------------------------------------------------------------------------------------ 2: the criterion's torch path
@pytest.mark.parametrize('gamma,alpha', twin.GAMMA_ALPHA)
@pytest.mark.parametrize('name', ['A', 'A_mixup', 'A_ignored', 'A_mixup_ignored'])
def test_torch_path_against_the_twin(name, gamma, alpha):
    c = cases.case(name)
    assert (c.conf_t[..., 0] < 0).any() == name.endswith('ignored')
    want, want_g = twin.criterion_reference(name, gamma, alpha)
    out, grads = _run_torch_path(c, c.pred, gamma, alpha)
    for k in cases.KEYS:
        cases.check_loss(k, out[k], want[k])
    for what, got, ref in zip(('loc', 'conf', 'obj'), grads, want_g):
        cases.check_grad(what, got, ref)
    # nothing is mined: the class term sees every row that is not ignored, far more than 4 * num_pos
    assert int((twin.row_weights(c.conf_t) != 0).sum()) > 30000 > 4 * c.n


def test_torch_path_with_an_iou_term_and_a_loc_weight():
    c = cases.case('A_mixup')
    want, want_g = twin.criterion_reference('A_mixup', 2.0, 0.25)
    out, grads = _run_torch_path(c, c.pred, 2.0, 0.25, loc_loss='giou', loc_weight=2.0)
    loc_want, loc_g = c.loc['giou']
    cases.check_loss('giou', out['loss_box_reg'], 2.0 * loc_want)
    cases.check_grad('loc', grads[0], 2.0 * loc_g)
    cases.check_loss('loss_cls', out['loss_cls'], want['loss_cls'])
    cases.check_loss('loss_obj', out['loss_obj'], want['loss_obj'])
    cases.check_grad('conf', grads[1], want_g[1])
    cases.check_grad('obj', grads[2], want_g[2])


@pytest.mark.parametrize('gamma,alpha', [(0.5, 0.25), (2.0, -1.0)])
def test_torch_path_never_reads_ignored_rows_or_background_conf_rows(gamma, alpha):
    c = cases.case('A_mixup_ignored')
    label = c.conf_t[..., 0]
    ignored, bg = label < 0, label == 0
    conf_t = c.conf_t.clone()
    first = (label > 0).nonzero()[0]
    conf_t[first[0], first[1], 1] = 0.0                 # and one foreground row of weight 0
    dead = ignored.clone()
    dead[first[0], first[1]] = True
    assert int(ignored.sum()) > 0 and int(bg.sum()) > 30000
    clean, clean_g = _run_torch_path(c, c.pred, gamma, alpha, conf_t=conf_t)
    pred = [p.clone() for p in c.pred]
    pred[1][dead] = float('nan')
    pred[2][dead] = float('inf')
    pred[1][bg] = float('nan')
    pred[1][:, ::2][bg[:, ::2]] = float('inf')
    out, grads = _run_torch_path(c, pred, gamma, alpha, conf_t=conf_t)
    for k in cases.KEYS:
        assert torch.equal(out[k], clean[k]), k
    assert float(grads[1][dead | bg].abs().max()) == 0.0 and float(grads[2][dead].abs().max()) == 0.0
    live = ~(dead | bg)
    assert torch.equal(grads[1][live], clean_g[1][live]) and torch.equal(grads[2][~dead], clean_g[2][~dead])
    assert torch.equal(grads[0], clean_g[0]) and float(clean_g[1][live].abs().max()) > 0


# ------------------------------------------------------------------------------------ 3: the surface
def test_default_is_cross_entropy_and_the_environment_is_honoured(monkeypatch):
    for k in ('CTDET_CONF_LOSS', 'CTDET_FOCAL_GAMMA', 'CTDET_FOCAL_ALPHA'):
        monkeypatch.delenv(k, raising=False)
    crit = _crit()
    assert (crit.conf_loss, crit.focal_gamma, crit.focal_alpha) == ('ce', 2.0, 0.25)
    monkeypatch.setenv('CTDET_CONF_LOSS', '')
    assert _crit().conf_loss == 'ce'
    monkeypatch.setenv('CTDET_CONF_LOSS', 'focal')
    monkeypatch.setenv('CTDET_FOCAL_GAMMA', '1.5')
    monkeypatch.setenv('CTDET_FOCAL_ALPHA', '-1')
    crit = _crit()
    assert (crit.conf_loss, crit.focal_gamma, crit.focal_alpha) == ('focal', 1.5, -1.0)
    crit = _crit(conf_loss='ce', focal_gamma=0, focal_alpha=0.5)         # arguments win over the environment
    assert (crit.conf_loss, crit.focal_gamma, crit.focal_alpha) == ('ce', 0.0, 0.5)
    assert _lib.CONF_LOSSES == ('ce', 'focal')


def test_bad_names_and_constants_raise_value_error(monkeypatch):
    for k in ('CTDET_CONF_LOSS', 'CTDET_FOCAL_GAMMA', 'CTDET_FOCAL_ALPHA'):
        monkeypatch.delenv(k, raising=False)
    for kw in (dict(conf_loss='Focal'), dict(conf_loss='bce'), dict(focal_gamma=-0.5), dict(focal_gamma=math.inf),
               dict(focal_gamma=math.nan), dict(focal_alpha=1.5), dict(focal_alpha=math.nan), dict(focal_alpha=math.inf)):
        with pytest.raises(ValueError):
            _crit(conf_loss=kw.pop('conf_loss', 'focal'), **kw)
    for name, text in (('CTDET_CONF_LOSS', 'FOCAL'), ('CTDET_FOCAL_GAMMA', '-1'), ('CTDET_FOCAL_GAMMA', 'two'),
                       ('CTDET_FOCAL_ALPHA', '1.01')):
        monkeypatch.setenv(name, text)
        with pytest.raises(ValueError):
            _crit()
        monkeypatch.delenv(name)
    for ok in (dict(focal_gamma=0.0, focal_alpha=0.0), dict(focal_gamma=5.0, focal_alpha=1.0), dict(focal_alpha=-3.0)):
        _crit(conf_loss='focal', **ok)
    from ctdet import ops
    with pytest.raises(ValueError, match='ce, focal'):
        ops.check_focal('varifocal', 2.0, 0.25)
    with pytest.raises(ValueError, match='focal_gamma'):
        ops.check_focal('focal', -1.0, 0.25)
    assert ops.check_focal('focal', 2, -1) == ('focal', 2.0, -1.0)


def test_header_enum_struct_and_binding():
    hdr = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    declared = set(re.findall(r'\b(ct_[a-z0-9_]+)\s*\(', hdr))
    for s in ('ct_multibox_loss_fwd_terms', 'ct_multibox_loss_bwd_terms'):
        assert s in declared and s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES['ct_multibox_loss_fwd_terms'][1]) == 17 + 1
    assert len(_lib.SIGNATURES['ct_multibox_loss_bwd_terms'][1]) == 15 + 1
    for i, name in enumerate(('CT_CONF_CE', 'CT_CONF_FOCAL')):
        assert re.search(r'\b%s = %d\b' % (name, i), hdr), name
        assert _lib.CONF_LOSSES[i] == name[len('CT_CONF_'):].lower()
    body = re.search(r'typedef struct ct_loss_terms \{(.*?)\} ct_loss_terms;', hdr, re.S).group(1)
    fields = re.findall(r'(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert fields == [f for f, _ in _lib.LossTerms._fields_], fields
    assert C.sizeof(_lib.LossTerms) == 32
    assert 'CTDET_ABI_VERSION 1' in hdr and _lib.lib().ct_abi_version() == 1
    assert 'THE SUM OF THE OTHER PROBABILITIES' in hdr


def test_c_abi_refuses_bad_terms_without_a_device():
    """The checks of the _terms entries come before any HIP call and before the other pointers are looked at."""
    lib = _lib.lib()
    buf = (C.c_float * 16)()
    host = C.cast(buf, C.c_void_p)

    def fwd(terms):
        return lib.ct_multibox_loss_fwd_terms(None, None, None, None, None, None, 2, 100, 21, 3, None, None, None, None,
                                              None, 0, None, terms)

    def bwd(terms):
        return lib.ct_multibox_loss_bwd_terms(None, None, None, None, None, None, None, None, 2, 100, 21, None, None, None,
                                              None, terms)

    def terms(priors=None, loc=0, v0=0.1, v1=0.2, conf=1, gamma=2.0, alpha=0.25):
        return C.byref(_lib.LossTerms(priors, loc, v0, v1, conf, gamma, alpha))

    for fn, name in ((fwd, b'ct_multibox_loss_fwd_terms'), (bwd, b'ct_multibox_loss_bwd_terms')):
        for arg, word in ((None, b'terms is a null pointer'), (terms(conf=2), b'conf_loss=2'), (terms(conf=-1), b'conf_loss=-1'),
                          (terms(gamma=-0.5), b'focal_gamma'), (terms(gamma=math.nan), b'focal_gamma'),
                          (terms(gamma=math.inf), b'focal_gamma'), (terms(alpha=1.5), b'focal_alpha'),
                          (terms(alpha=math.nan), b'focal_alpha'), (terms(loc=5), b'loc_loss=5'),
                          (terms(loc=2), b'priors'), (terms(host, 2, 0.0), b'variances'),
                          # valid terms: the old checks answer, for the focal form and for the cross-entropy one, whose
                          # gamma and alpha are not read
                          (terms(), b'null pointer'), (terms(alpha=-1.0, gamma=0.0), b'null pointer'),
                          (terms(host, 2), b'null pointer'), (terms(conf=0, gamma=-1.0, alpha=7.0), b'null pointer')):
            assert fn(arg) == 1, (name, word)
            msg = lib.ct_last_error_string()
            assert name in msg and word in msg, (word, msg)


def test_fused_focal_still_refuses_cpu_tensors():
    c = cases.case('A')
    crit = _crit(c.ncls, fused=True, conf_loss='focal')
    with pytest.raises(_lib.CtdetError, match='HIP device'):
        crit(c.pred, c.priors, MatchedTargets(c.loc_t, c.conf_t, c.obj_t))


# ------------------------------------------------------------------------------------ 4: the initialisation
@pytest.mark.parametrize('pi', [0.01, 0.1])
def test_focal_prior_init_sets_the_objectness_prior_and_nothing_else(pi):
    from models.RFB_Net_vgg import build_net
    torch.manual_seed(3)
    net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
    for conv in net.obj:
        torch.nn.init.normal_(conv.bias)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert focal_prior_init(net, pi) is net
    after = net.state_dict()
    touched = {'obj.%d.bias' % i for i in range(len(net.obj))}
    for k, v in before.items():
        assert torch.equal(after[k], v) != (k in touched), k
    for conv in net.obj:
        bias = conv.bias.detach().view(-1, 2)
        assert bias.shape[0] * 2 == conv.out_channels and float(bias[:, 0].abs().max()) == 0.0
        prob = torch.softmax(bias.double(), 1)[:, 1]
        assert float((prob - pi).abs().max()) < 1e-7, float((prob - pi).abs().max())
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            focal_prior_init(net, bad)

"""Shared by tests/test_ctx_block_ref_cpu.py and tests/test_gpu_ctx_block.py: ONE case table for the Context-Transformer block
(csrc/ct_attn.hip, ct_attn_bwd.hip), its seeded inputs, the float64 reference (oracle.rfbnet_ref.context_block and float64
autograd over it) and four fault models evaluated on that reference.  Importable without a GPU (nothing here loads libctdet.so).

Why regimes.  With conf / pool drawn as randn * 1.5 the softmax of the block is near-arg-max: one key carries a row (median
1 / sum p^2 = 1.00-1.07), so a padding key that is not masked, a wrong term of l_run, or a wrong contribution of any but one or
two keys to dK / dV / dQ moves nothing.  The table therefore draws the same shapes at smaller amplitudes:
    diffuse  0.25   effective keys >= M / 4: every key and every query tile carries weight
    mixed    0.5    a few to a few dozen effective keys
    peaked   1.5    the regime of tests/test_gpu_ctx_train.py, kept for a few rows
    tie      1.5    and per image pool[b, last key] = pool[b, j], j the key of the FIRST key tile that is the arg-max of most
                    queries: the row maximum of those queries is shared exactly between the first and the last 32-key tile
Edges of the kernels the rows are placed on: the 16-feature fragment groups, the 32 + 32 accumulator halves and DP = 64 (d),
T = 1 / 31 / 32, M around the forward's 32-key tiles and the backward's 128-key padding, P around the 32-query tiles and the
128-query workgroups, and the two P ranges where the backward splits the query tiles of a key block over 3 (28 tiles: uneven)
and 4 workgroups (kv_split below restates the host's rule)."""
import functools
import types
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import rfbnet_ref
from test_gpu_ctx_train import _oracle_sd, _params

AMP = {'diffuse': 0.25, 'mixed': 0.5, 'peaked': 1.5, 'tie': 1.5}
KT, QB = 32, 128                    # keys (queries) per MFMA tile, rows per workgroup / padding of the backward (ct_attn_common.h)
ZERO_KEYS_M1 = ('theta_w', 'theta_b', 'phi_w', 'phi_b')      # a single key: the softmax is the constant 1


@dataclass(frozen=True)
class Case:
    regime: str
    B: int
    P: int
    M: int
    d: int
    T: int
    incre: bool
    bump: int = 0                   # added to the seed (a row whose reference alone misses a fault margin gets another draw)

    @property
    def name(self):
        return '%s-b%d-p%d-m%d-d%d-t%d-%s' % (self.regime, self.B, self.P, self.M, self.d, self.T, self.setting)

    @property
    def setting(self):
        return 'incre' if self.incre else 'transfer'

    @property
    def amp(self):
        return AMP[self.regime]

    @property
    def seed(self):
        return zlib.crc32(repr((self.regime, self.B, self.P, self.M, self.d, self.T, self.incre)).encode()) % 10007 + self.bump

    @property
    def fwd_only(self):
        """d = 1: the L2 normalisation makes the output +-1 and every gradient but obj_w exactly zero."""
        return self.d == 1

    @property
    def kv_split(self):
        """Workgroups the backward spreads the query tiles of one key block over (ct_ctx_attention_bwd)."""
        P_pad, M_pad = -(-self.P // QB) * QB, -(-self.M // QB) * QB
        kv_blocks = M_pad // QB * self.B
        return max(1, min(P_pad // (8 * KT), (1024 + kv_blocks - 1) // kv_blocks))


def _c(regime, B, P, M, d, T, incre, bump=0):
    return Case(regime, B, P, M, d, T, bool(incre), bump)


CASES = [
    # every listed value of d, T, M and P at least once in the diffuse regime
    _c('diffuse', 1, 1, 1, 2, 1, 0),
    _c('diffuse', 3, 31, 2, 15, 20, 1),
    _c('diffuse', 1, 33, 31, 16, 31, 0),
    _c('diffuse', 3, 127, 32, 17, 32, 1),
    _c('diffuse', 1, 128, 33, 32, 20, 0),
    _c('diffuse', 3, 129, 63, 33, 1, 1),
    _c('diffuse', 1, 257, 64, 48, 31, 1),
    _c('diffuse', 1, 640, 65, 60, 20, 0),           # kv_split 2
    _c('diffuse', 3, 877, 127, 63, 32, 0),          # kv_split 3 over 28 query tiles (9 / 9 / 10), valid queries in the last one
    _c('diffuse', 1, 1001, 128, 64, 20, 1),         # kv_split 4, valid queries in the last tile
    _c('diffuse', 3, 130, 129, 64, 32, 0),          # also the batch-mate independence row
    _c('diffuse', 2, 300, 260, 60, 20, 1),
    _c('diffuse', 1, 129, 260, 17, 1, 0, bump=3),   # first draw: fault (c) at 1.0e-3, on the margin
    _c('diffuse', 3, 33, 1, 33, 32, 1),             # M = 1 at a feature-group edge
    _c('diffuse', 2, 40, 31, 1, 3, 0),              # d = 1: forward only
    _c('mixed', 2, 300, 70, 60, 20, 0),
    _c('mixed', 2, 130, 33, 64, 32, 1),
    _c('mixed', 1, 129, 65, 17, 1, 0),
    _c('mixed', 3, 257, 72, 48, 31, 1),
    _c('mixed', 1, 877, 40, 32, 20, 0),             # kv_split 3
    _c('peaked', 2, 257, 129, 60, 20, 1),
    _c('peaked', 1, 640, 33, 20, 15, 0),
    _c('peaked', 1, 129, 63, 64, 32, 0),
    _c('tie', 2, 130, 70, 60, 20, 0),
    _c('tie', 3, 257, 260, 33, 31, 1),
    _c('tie', 1, 33, 33, 16, 1, 0),                 # the last tile holds the tied key alone
]
IDS = [c.name for c in CASES]
LISTED = {
    'd': (2, 15, 16, 17, 32, 33, 48, 60, 63, 64),
    'T': (1, 20, 31, 32),
    'M': (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 260),
    'P': (1, 31, 33, 127, 128, 129, 257, 640),
}
P_RANGES = {3: (769, 896), 4: (897, 1024)}          # kv_split: the P range the table must reach it in


def by_regime(*regimes):
    return [c for c in CASES if c.regime in regimes]


def _theta_phi(conf, pool, p):
    lin = lambda t, w, b: F.linear(t, w.double(), b.double()) + t
    return lin(conf.double(), p['theta_w'], p['theta_b']), lin(pool.double(), p['phi_w'], p['phi_b'])


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> namespace(conf [B,P,d], pool [B,M,d], p {name: tensor}, R [B,P,(d)+T], tie [(j, j2)] per image or None), float32."""
    g = torch.Generator().manual_seed(case.seed)
    conf = torch.randn(case.B, case.P, case.d, generator=g) * case.amp
    pool = torch.randn(case.B, case.M, case.d, generator=g) * case.amp
    p = _params(case.d, case.T, case.incre, case.seed + 1)
    R = torch.randn(case.B, case.P, (case.d if case.incre else 0) + case.T, generator=g)
    tie = None
    if case.regime == 'tie':
        assert case.M > KT
        theta, phi = _theta_phi(conf, pool, p)
        tie = []
        for b in range(case.B):
            am = (theta[b] @ phi[b].t()).argmax(1)
            j = int(torch.bincount(am[am < KT], minlength=KT).argmax())
            pool[b, case.M - 1] = pool[b, j]
            tie.append((j, case.M - 1))
    return types.SimpleNamespace(conf=conf, pool=pool, p=p, R=R, tie=tie)


def block(case, conf, pool, p, R, dtype=torch.float64, queries=None, grad=True):
    """The oracle block and autograd over it in `dtype`.  queries: a boolean mask [P] of the query rows that enter the loss
    sum(out * R) (all by default).  -> (out, {conf, pool, parameter names: gradient}) ({} with grad=False)."""
    leaves = {k: v.to(dtype).clone().requires_grad_(grad) for k, v in p.items()}
    c, q = conf.to(dtype).clone().requires_grad_(grad), pool.to(dtype).clone().requires_grad_(grad)
    sd = _oracle_sd(leaves, case.incre)
    sd['scale'] = torch.tensor([5.0], dtype=dtype)
    out = rfbnet_ref.context_block(sd, c, q, case.setting)
    if not grad:
        return out.detach(), {}
    w = out * R.to(dtype)
    (w if queries is None else w[:, queries]).sum().backward()
    return out.detach(), dict(conf=c.grad, pool=q.grad, **{k: v.grad for k, v in leaves.items()})


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def reference(case):
    """Computed once per case and shared; nobody writes to it.  -> namespace(inp, out, grads (float64), e32 {'out' / gradient
    name: the normalised error of torch float32 autograd on the same inputs}, zero: names whose gradient is exactly zero)."""
    inp = inputs(case)
    grad = not case.fwd_only
    out, grads = block(case, inp.conf, inp.pool, inp.p, inp.R, grad=grad)
    out32, g32 = block(case, inp.conf, inp.pool, inp.p, inp.R, torch.float32, grad=grad)
    zero = ('phi_b',) + (ZERO_KEYS_M1 if case.M == 1 else ())
    e32 = {'out': _rel(out32, out)}
    e32.update({k: _rel(g32[k], grads[k]) for k in grads if k not in zero})
    return types.SimpleNamespace(inp=inp, out=out, grads=grads, e32=e32, zero=tuple(sorted(set(zero))))


def softmax_stats(case):
    """-> (median over the query rows of the effective number of keys 1 / sum p^2, median row maximum), float64."""
    inp = inputs(case)
    theta, phi = _theta_phi(inp.conf, inp.pool, inp.p)
    w = F.softmax(theta @ phi.transpose(1, 2), dim=2)
    return float((1.0 / w.pow(2).sum(2)).median()), float(w.max(2).values.median())


# ---- fault models: what a specific kernel mistake would compute, evaluated in float64 on the reference ----
def fault_pad_keys(case, multiple):
    """(a) multiple = 32, (b) multiple = 128: the padding keys up to the next multiple take part in the softmax (zero pool
    rows, as the kernels pad them).  -> (out, grads); grads['pool'] is cut back to the M real rows."""
    inp = inputs(case)
    M_pad = -(-case.M // multiple) * multiple
    pool = torch.cat([inp.pool, torch.zeros(case.B, M_pad - case.M, case.d)], 1)
    out, grads = block(case, inp.conf, pool, inp.p, inp.R, grad=not case.fwd_only)
    if grads:
        grads['pool'] = grads['pool'][:, :case.M]
    return out, grads


def fault_drop_last_key(case):
    """(c) the last valid key masked out (`> M - 1` where `>= M` is meant).  -> (out, grads), its dpool row zero."""
    assert case.M >= 2
    inp = inputs(case)
    out, grads = block(case, inp.conf, inp.pool[:, :case.M - 1], inp.p, inp.R, grad=not case.fwd_only)
    if grads:
        grads['pool'] = torch.cat([grads['pool'], torch.zeros(case.B, 1, case.d, dtype=torch.float64)], 1)
    return out, grads


def dropped_queries(case):
    """Fault (d): the query rows of the last 32-query tile that holds valid rows -- the tail of the last kv_split slice of
    ctx_attn_bwd_kv (the tiles behind it are padding and contribute nothing either way).  -> boolean mask [P] of the rows kept."""
    keep = torch.ones(case.P, dtype=torch.bool)
    keep[(case.P - 1) // KT * KT:] = False
    return keep


def fault_drop_query_tail(case):
    """(d) those rows left out of the sums over queries: dpool, dphi_*, dg_* (a query row of `out` depends on its own conf row
    only, so dropping the rows from the loss drops exactly their terms).  -> grads (pool, phi_w, phi_b, g_w, g_b)."""
    inp = inputs(case)
    _, grads = block(case, inp.conf, inp.pool, inp.p, inp.R, queries=dropped_queries(case))
    return {k: grads[k] for k in ('pool', 'phi_w', 'phi_b', 'g_w', 'g_b')}


def moved(a, b):
    """max |a - b| / max |b|: how far a fault moves a reference tensor, on conftest.rel_err's scale."""
    return _rel(a, b)

"""Which kernel a forward or data-gradient convolution runs: the switches resolved ONCE into a record, and the rules as pure
functions of that record, the committed table and a layer (the weight-gradient routes have ctdet/wgrad_routes.py).

  resolve(net, batch, env, training)             -> ConvPolicy: the only place the CTDET_* selection variables are read
  wino_tiles(policy, layer)                      -> the Winograd codes the tuner / the table may use on that layer
  choose_forward(policy, table, kernels, layer)  -> Choice of the forward launch, None where the table has no entry
  choose_dgrad(policy, layer, fwd_tile, supported) -> (Winograd code or None, bf16x3 config or None) of the data gradient

Nothing here needs a backend, a prepared step or a device: tests/test_conv_policy_cpu.py asks "what would this layer run under
that policy" on hand-made records, and pins the outcome for the shipped networks."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

from .wino_forms import FORMS, geometry_ok

WINO_NAME = {c: f.name for c, f in FORMS.items()}
WINO_CODE = {f.name: c for c, f in FORMS.items()}
WINO4S_TILES = tuple(c for c, f in FORMS.items() if f.split)
WINO4F_TILES = tuple(c for c, f in FORMS.items() if f.ok == 'wino4f_ok')
F4_TILES = tuple(c for c, f in FORMS.items() if f.f4)
# bf16x3 tile -> the same kernel on the f16x2 operand form (csrc/ct_f16x2.h: two binary16 pieces, three products)
H2_OF_TILE = {f.plain: c for c, f in FORMS.items() if f.h2}

WINO_TILES_DEFAULT = (2, 4, 44, 46)
H2_MIN_PIXELS = 8 * 300 * 300
CTX_TILES_DEFAULT = 'h2'
CTX_F4_MAX_CIN_DEFAULT = '128'
CTX_F4_TILE_DEFAULT = '4'
CTX_W4S_MIN_CIN_DEFAULT = '0'
CTX_DIL_W4S_DEFAULT = '1'


@dataclass(frozen=True)
class ConvPolicy:
    """Every switch that shapes the choice, resolved to what is in force.  The defaults are those of a backend no runtime has
    bound (kernel tests, tools/): the committed table on the bf16x3 forms."""
    # CTDET_WINO=0: no Winograd kernel anywhere
    wino: bool = True
    # bf16x3 (ct_conv2d_x3_fwd) is a candidate for every forward conv except the 3-channel image layer (K = 27: nothing to
    # gain); CTDET_X3=0 keeps the fp32 MFMA kernel everywhere (x3_allowed)
    x3: bool = True
    # CTDET_WINO_TILES as a tuple, None if unset.  Winograd variants the tuner / the table may use (st.rt['wino'] codes).
    # Default '2,4,44,46': the two fp32-MFMA kernels, the three-kernel F(4x4,3x3) / bf16x3 form with two accumulators
    # (csrc/ct_wino4s.hip) and the fused F(4x4,3x3) / bf16x3 kernel for the narrow layers on big maps (csrc/ct_wino4f.hip).  The
    # fused F(2x2) bf16x3 form (23) is faster than the fused fp32 kernels per layer ALONE (512 -> 512 @38x38: 742 -> 630 us) but
    # not in the two-stream pipeline (same-box A/B of two tables: 3 360-3 371 vs 3 228-3 398 images/s) and
    # slower than tile 44 wherever that applies, so the committed table does not hold it; CTDET_WINO_TILES=2,4,23,44 lets the
    # tuner time it.  A runtime with an accuracy policy (tile_set: networks with the Context-Transformer block) uses ITS set
    # instead (narrowed by an explicit CTDET_WINO_TILES), plus F(4x4) / fp32 on layers with at most f4_max_cin input channels
    # (and tile 44 from w4s_min_cin input channels up, see choose_forward).
    tiles_env: Optional[Tuple[int, ...]] = None
    # (h2, h2_direct): whether a runtime runs its bf16x3 Winograd table entries on the f16x2 operand form, and whether it may
    # use the f16x2 twins of the direct kernel's tiles (csrc/ct_f16x2.h: two binary16 pieces, three products; same error against
    # fp64 per layer, tests/test_gpu_wino.py::test_wino_rounding_error_vs_fp64, half the matrix instructions).  CTDET_H2: '1'
    # (default) = from batch x size^2 >= 8 x 300^2 up (H2_MIN_PIXELS), '2' = always, '0' = never.  Why a threshold: an f16x2
    # launch waits for its input's maxima when it starts and folds its own in when it ends -- a few us per launch that the
    # launch-bound small batches do not get back (same-box, images/s bf16x3 -> f16x2: RFBNet-300 bs 4 2 065 -> 1 830, bs 8
    # 2 850 -> 2 990, bs 16 3 450 -> 3 945, bs 32 4 005 -> 4 655; RFBNet-512 bs 4 1 120 -> 1 126, bs 8 1 340 -> 1 438, bs 32
    # 1 608 -> 1 805; profiles/r06_ab_batches.txt).  Networks with the Context-Transformer block (ctx_tiles): under the shipped
    # policy 'h2' the Winograd forms at EVERY batch size and never the direct twins -- the combination the parity sweeps were
    # made on; under a tile-set policy neither.  CTDET_H2_X3=0: no direct twins.
    # Training: the Winograd launches of the step (forward and data gradients) wherever the table's bf16x3 tile has that twin,
    # under the same batch rule; CTDET_TRAIN_H2=0 keeps bf16x3.  Direct layers stay on bf16x3 (h2_direct = False): their
    # inputs come from the BatchNorm kernels, which do not track maxima.
    h2: bool = False
    h2_direct: bool = False
    # CTDET_CTX_TILES for a network with the Context-Transformer block (models/RFB_Net_vgg.py:253-271), None for any other:
    # 'h2' (default, round 6), 'any', or a comma list of Winograd tile codes (the round-2 .. 5 tile-set policies; '2,23' was
    # round 5's).
    ctx_tiles: Optional[str] = None
    # Winograd tile SET of networks with the Context-Transformer block; None = no restriction (every other network, the
    # policies 'h2' / 'any', and EVERY training runtime: it runs the unconstrained table whatever CTDET_CTX_TILES says, with
    # w4f_max_cin as its accuracy rule).
    #
    # The block's un-scaled theta.phi^T softmax is near-arg-max and amplifies a perturbation of its INPUT (the conf-head
    # output) ~1000x (tools/ctx_parity.py --budget: 970x), so the reference's own fp32 CPU path sits 5..7e-5 from an fp64
    # evaluation, two correct fp32 evaluations differ by up to ~1e-4, and which side of north_star's flat 1e-4 the worst of 7e5
    # elements lands on is decided by single layers' summation orders: every policy is a MEASURED choice over the nine sweep
    # cases (bs {2, 8, 32} x seeds {1234, 7, 99}) x the reference at 8 and 128 threads, not a guarantee for other seeds.
    #
    # Round 6, shipped: 'h2' -- the unconstrained table with its F(4x4,3x3) entries on the f16x2 operand form (three-kernel form
    # with two accumulators, fused kernel) and the direct layers on bf16x3 with two accumulators (h2 / h2_direct).  All 18 pairs
    # inside 1e-4 (worst 9.76e-5), RFBNet-300 + Context-Transformer bs 32 at 3 640 images/s against 2 560 for round 5's policy;
    # on ten further cases (seeds 1..5, bs 8 / 32) 2 of 20 pairs above 1e-4 against 5 of 20 for round 5's policy
    # (profiles/r06_ctx_policy.txt, r06_ctx_policy_seeds.txt).  With the direct layers on f16x2 too: 3 750 images/s, one pair at
    # 1.01e-4.  Round 5, still available as CTDET_CTX_TILES=2,23: F(2x2,3x3) on bf16x3 with two accumulators (tile 23: per-layer
    # error vs fp64 4e-7 against 2e-6 for F(4x4,3x3)) except a fused fp32 F(4x4) on the short channel sums (f4_max_cin): 18 / 18
    # inside 1e-4 too (worst 9.2e-5), at 2 560 images/s.  Layers without 16-channel chunks keep F(2x2,3x3) on the fp32 MFMA.
    tile_set: Optional[Tuple[int, ...]] = None
    # Layers of a Context-Transformer network with at most this many input channels keep a fused F(4x4,3x3) kernel where the
    # table picks one (f4_tile): its rounding error grows with the length of the channel sum, and on conv1_2 .. conv3_1
    # (64 / 128 input channels at 300 x 300 .. 75 x 75) F(2x2,3x3) costs the most time.  Chosen by the round-5 sweeps
    # (profiles/r05_ctx_policy.txt: RFBNet-300 + Context-Transformer bs 32, 9 randn cases, every case judged against the fp32 CPU
    # path at 8 AND at 128 reference threads; three-kernel form off; (f4_tile, this cap) on the committed table):
    #   (4, 128)   2 570 images/s   worst GPU-CPU32 9.0e-5 at 8 threads, 9.2e-5 at 128   all 18 inside 1e-4   <- default
    #   (4, 256)   2 619            1.02e-4 / 1.07e-4    3 of 18 above 1e-4 (conv3_2 / conv3_3: 256-channel sums on the fp32 MFMA)
    #   (46, 128)  2 670            1.01e-4 / 9.5e-5     1 of 18 above
    #   (46, 256)  2 769            1.01e-4 / 9.7e-5     1 of 18 above
    #   cap 0 (every Winograd layer on F(2x2,3x3) / bf16x3): 2 353, 9.7e-5 / 1.02e-4, 1 of 18 above
    #   round 4's policy (three-kernel F(4x4) from 128 channels up): 2 898, 1.03e-4 / 1.05e-4, 3 of 18 above
    # All of them are within 7.7e-5 of the fp64 evaluation; which side of 1e-4 the worst of 7e5 elements lands on against a
    # reference that is itself 4.8..7.2e-5 from fp64 is decided by single layers' summation orders.  CTDET_CTX_F4_MAX_CIN;
    # 0 = none (and without a tile set).
    f4_max_cin: int = 0
    # Which F(4x4,3x3) kernel the layers below f4_max_cin run: 4 = fused on the fp32 MFMA (csrc/ct_wino4.hip), 46 = fused on
    # bf16x3 (csrc/ct_wino4f.hip; layers without 16-channel chunks keep 4).  CTDET_CTX_F4_TILE.
    f4_tile: int = 4
    # Layers of a Context-Transformer network with at least this many input channels that the table runs on F(4x4,3x3)
    # (fused or three-kernel) use the three-kernel bf16x3 form with two accumulators (tile 44: error vs fp64 2e-6 per layer
    # against 3-4e-7 for F(2x2,3x3) / bf16x3 with two accumulators, at 1.7x the speed on the wide layers).  Default 0 = never:
    # with tile 44 on the 512-channel layers one to three of the 18 (case, reference thread count) pairs of the sweep land at
    # 1.03-1.05e-4 from the fp32 CPU path (f4_max_cin has the table), and north_star's contract is a flat 1e-4.
    # CTDET_CTX_W4S_MIN_CIN=128 CTDET_CTX_F4_MAX_CIN=128 is the round-4 policy: +17 % images/s for callers who accept that.
    w4s_min_cin: int = 0
    # Context-Transformer networks with w4s_min_cin > 0: their dilated layers (conv6, the RFB branches) on the three-kernel form
    # too, from that many input channels up (CTDET_CTX_DIL_W4S=0: never)
    dil_w4s: bool = True
    # A fused bf16x3 F(4x4,3x3) table entry (tiles 46 / 48) only up to this many input channels; None = everywhere.  The
    # training runtime of a Context-Transformer network: CTDET_TRAIN_CTX_W4F_MAX_CIN, default 128 -- the fused bf16x3 kernel has
    # ONE accumulator, 3.4e-6 of the output range at 256 input channels and 4.6e-6 at 512 against 1.3-2.0e-6 for the
    # three-kernel form, and the block's backward amplifies that (conf.3's gradient 2.5e-4 from fp64 instead of <= 1.4e-4 at
    # RFBNet-512 bs 8) -- its wide layers stay on the three-kernel form.  Inference: only for a network with the block and only
    # when CTDET_CTX_W4F_MAX_CIN is set (experiments).
    w4f_max_cin: Optional[int] = None
    # CTDET_WINO_FORCE = tile code (experiments, tools/ctx_parity.py): every layer that runs on a Winograd kernel and has the
    # geometry for it is moved to that variant; 0 = off
    force_tile: int = 0
    # ---- training only
    # CTDET_TRAIN_WINO4=0 keeps forward and data-gradient convolutions on F(2x2,3x3) where the table says F(4x4,3x3)
    wino4: bool = True
    # the data gradient on the three-kernel form (tiles 44 / 47) where the forward launch runs it; CTDET_TRAIN_W4S=0 keeps the
    # fused kernel
    dgrad_w4s: bool = True
    # ... and on the fused bf16x3 F(4x4,3x3) kernel (tiles 46 / 48) where the forward launch runs that one (CTDET_TRAIN_W4F=0)
    dgrad_w4f: bool = True
    # ... and the dilated layers' data gradients on the three-kernel form (CTDET_TRAIN_W4S_DIL=0)
    dgrad_w4s_dil: bool = True


def has_ctx_block(net):
    return getattr(net, 'method', None) == 'ours' and getattr(net, 'phase', 1) == 2


def resolve(net, batch, env, training=False):
    """The policy of a runtime for `net` at `batch`, from the CTDET_* variables in `env`.  net=None: of a backend no runtime
    has bound (the bf16x3 forms).  batch=None: the operand form of a batch above the threshold."""
    ctx = net is not None and has_ctx_block(net)
    ctx_tiles = env.get('CTDET_CTX_TILES', CTX_TILES_DEFAULT) if ctx else None
    tiles = env.get('CTDET_WINO_TILES')
    mode = env.get('CTDET_H2', '1')
    if net is None or mode == '0' or (ctx_tiles is not None and ctx_tiles not in ('h2', 'any')):
        h2 = h2_direct = False
    elif ctx_tiles == 'h2':
        h2, h2_direct = True, False
    else:
        size = int(getattr(net, 'size', 300) or 300)
        h2 = mode == '2' or batch is None or batch * size * size >= H2_MIN_PIXELS
        h2_direct = h2 and env.get('CTDET_H2_X3', '1') != '0'
    common = dict(wino=env.get('CTDET_WINO', '1') != '0', x3=env.get('CTDET_X3', '1') != '0',
                  tiles_env=None if tiles is None else tuple(int(t) for t in tiles.split(',') if t), ctx_tiles=ctx_tiles,
                  f4_tile=int(env.get('CTDET_CTX_F4_TILE', CTX_F4_TILE_DEFAULT)),
                  dil_w4s=env.get('CTDET_CTX_DIL_W4S', CTX_DIL_W4S_DEFAULT) != '0',
                  force_tile=int(env.get('CTDET_WINO_FORCE', '0') or 0))
    if training:
        return ConvPolicy(h2=env.get('CTDET_TRAIN_H2', '1') != '0' and h2, h2_direct=False,
                          w4f_max_cin=int(env.get('CTDET_TRAIN_CTX_W4F_MAX_CIN', '128')) if ctx else None,
                          wino4=env.get('CTDET_TRAIN_WINO4', '1') != '0', dgrad_w4s=env.get('CTDET_TRAIN_W4S', '1') != '0',
                          dgrad_w4f=env.get('CTDET_TRAIN_W4F', '1') != '0',
                          dgrad_w4s_dil=env.get('CTDET_TRAIN_W4S_DIL', '1') != '0', **common)
    tile_set = None if ctx_tiles in (None, 'any', 'h2') else tuple(int(t) for t in ctx_tiles.split(',') if t)
    return ConvPolicy(h2=h2, h2_direct=h2_direct, tile_set=tile_set,
                      f4_max_cin=int(env.get('CTDET_CTX_F4_MAX_CIN', CTX_F4_MAX_CIN_DEFAULT)) if tile_set is not None else 0,
                      w4s_min_cin=int(env.get('CTDET_CTX_W4S_MIN_CIN', CTX_W4S_MIN_CIN_DEFAULT)) if tile_set is not None else 0,
                      w4f_max_cin=int(env['CTDET_CTX_W4F_MAX_CIN']) if ctx and env.get('CTDET_CTX_W4F_MAX_CIN') else None,
                      **common)


@dataclass(frozen=True)
class Kernels:
    """What the library offers, asked once per backend: names by config index."""
    direct: Tuple[str, ...]         # ct_conv2d_fwd tiles (desc.config = index + 1)
    x3: Tuple[str, ...]             # ct_conv2d_x3_fwd configs: 'x3:<tile>' on bf16x3, 'h2:<tile>' their f16x2 twins
    x3_bk: Tuple[int, ...]          # ... each one's k-step (must divide cin)
    x3_h2: Tuple[bool, ...]

    @classmethod
    def of(cls, lib):
        nx = range(lib.ct_conv_x3_num_configs())
        return cls(tuple(lib.ct_conv_config_name(i).decode() for i in range(lib.ct_conv_num_configs())),
                   tuple(lib.ct_conv_x3_config_name(i).decode() for i in nx), tuple(lib.ct_conv_x3_config_bk(i) for i in nx),
                   tuple(bool(lib.ct_conv_x3_config_h2(i)) for i in nx))


@dataclass(frozen=True)
class Layer:
    """What the rules read of a convolution.  geo: the geometry flags of its forward descriptor (wino_ok, winox_ok, wino4s_ok,
    wino4f_ok: st.rt of a prepared step).  The second group is read for the data gradient only."""
    key: str = ''                   # ConvStep.tune_key(batch)
    cin: int = 0
    kh: int = 3
    kw: int = 3
    stride: int = 1
    dil: int = 1
    has_res: bool = False
    geo: dict = field(default_factory=dict)
    ph: int = 1
    pw: int = 1
    h: int = 0                      # input map (the data gradient's output)
    w: int = 0
    oh: int = 0
    ow: int = 0
    batch: int = 0
    zc: int = 0                     # channels of the dZ buffer (cout, zero-padded to 16 on the multibox heads)
    segs: bool = False              # a multibox head
    is_bn: bool = False

    @classmethod
    def of(cls, st, batch, zc=0, is_bn=False):
        return cls(st.tune_key(batch), st.cin, st.kh, st.kw, st.stride, st.dil, st.res is not None, st.rt, st.ph, st.pw, st.h, st.w,
                   st.oh, st.ow, batch, zc, bool(st.segs), is_bn)


@dataclass(frozen=True)
class Choice:
    kind: str                       # 'wino' / 'x3' / 'direct'
    value: int                      # st.rt['wino'] code / ct_conv2d_x3_fwd config / desc.config
    via: Tuple[str, ...] = ()       # table names it fell back through


def x3_allowed(policy, layer):
    return policy.x3 and layer.cin >= 16 and layer.cin % 16 == 0


def wino_tiles(policy, layer=None):
    """Winograd codes the tuner / the table may use (ConvPolicy.tiles_env has the why), on `layer` if given."""
    env = policy.tiles_env
    tiles = env or WINO_TILES_DEFAULT
    if env is None and policy.h2:
        tiles = tiles + tuple(H2_OF_TILE.values())
    if policy.tile_set is not None:     # a runtime's accuracy policy: its set, narrowed by an explicit CTDET_WINO_TILES
        tiles = tuple(t for t in policy.tile_set if env is None or t in tiles)
        cap, f4 = policy.f4_max_cin, policy.f4_tile
        if cap and layer is not None and layer.cin <= cap:
            if f4 in WINO4F_TILES and not layer.geo.get('wino4f_ok'):
                f4 = 4                  # the fused bf16x3 kernel needs 16-channel chunks: such layers keep the fp32 fused kernel
            if f4 not in tiles and (env is None or f4 in env):
                tiles = tiles + (f4,)   # short channel sums: F(4x4) costs little accuracy there
    if layer is not None:               # each form's geometry (dilated 3x3: only the three-kernel form)
        tiles = tuple(t for t in tiles if geometry_ok(layer.geo, t) and (t not in FORMS or layer.geo.get(FORMS[t].ok)))
    return tiles


def choose_forward(policy, table, kernels, layer):
    """The committed choice for a layer's shape under `policy`; None if the table has none.  policy.wino4=False maps an
    F(4x4,3x3) entry to F(2x2,3x3).  A Winograd entry the policy excludes (tile_set) becomes the most accurate allowed variant:
    F(2x2) on bf16x3 with two accumulators where the layer has 16-channel chunks, else F(2x2) on the fp32 MFMA."""
    L, via = layer, []
    cfg = table.get(L.key)
    if policy.h2:
        # a runtime on the f16x2 operand forms: where the forms' different speed-ups change which KERNEL FAMILY wins a shape
        # (tools/tune_convs.py --h2), the table holds that choice under '<key>|h2' (same names: mapped to the f16x2 twins below)
        cfg = table.get(L.key + '|h2', cfg)
    usable = cfg in WINO_CODE and geometry_ok(L.geo, WINO_CODE[cfg]) and policy.wino
    if usable and L.dil > 1:
        # dilated layer on the three-kernel form: where tile 44 is allowed as such; a runtime with an accuracy policy
        # (Context-Transformer networks) takes it from w4s_min_cin input channels up (dil_w4s off: never -- the layer then runs
        # the table's previous choice, '|alt').  Only tile 44 (and its f16x2 twin 47) exists for these layers: a caller that rules
        # out F(4x4) (wino4=False) gets the '|alt' entry as well.
        if policy.tile_set is not None:
            usable = policy.dil_w4s and L.cin >= policy.w4s_min_cin > 0
        else:
            usable = WINO_CODE[cfg] in wino_tiles(policy, L)
        usable = usable and policy.wino4
    if cfg in WINO_CODE and not usable:
        via.append(cfg)
        cfg = table.get(L.key + '|alt')     # what the layer ran on before the three-kernel form took it
    if usable:
        allowed = wino_tiles(policy, L)
        want = WINO_CODE[cfg]
        if want in F4_TILES and not policy.wino4:
            want = 2
        if policy.tile_set is not None:
            # accuracy policy of this runtime: F(4x4) / fp32 survives only where the policy allows it (short channel sums),
            # everything else runs the most accurate allowed variant
            f4 = policy.f4_tile if policy.f4_tile in allowed else 4     # tile 46 needs 16-channel chunks
            if want in F4_TILES and policy.w4s_min_cin and L.cin >= policy.w4s_min_cin and L.geo.get('wino4s_ok'):
                want = 44                   # three-kernel F(4x4) with two accumulators: 0.4x the rounding of the fused fp32 form
            elif want in (4,) + WINO4F_TILES and f4 in allowed:
                want = f4                   # a fused F(4x4) entry below f4_max_cin input channels (wino_tiles put f4 into the set)
            else:
                want = 23 if 23 in allowed else 2 if 2 in allowed or not allowed else allowed[0]
        elif want in WINO4F_TILES and L.cin > (policy.w4f_max_cin or 1 << 30):
            want = 44 if L.geo.get('wino4s_ok') and 44 in allowed else 4 if 4 in allowed else 2     # (ConvPolicy.w4f_max_cin)
        elif want not in allowed:
            # a three-kernel / fused-bf16x3 F(4x4) entry without its tile in the set (CTDET_WINO_TILES=2,4) is the fused fp32
            # F(4x4) kernel's layer
            want = 4 if want in WINO4S_TILES + WINO4F_TILES and 4 in allowed else 2 if 2 in allowed or not allowed else allowed[0]
        if policy.h2 and H2_OF_TILE.get(want) in allowed:
            want = H2_OF_TILE[want]         # the same kernel on the f16x2 operand form
        return Choice('wino', want, tuple(via))

    def x3_config(name):                    # index of a bf16x3 / f16x2 config this layer can run (the k-step must divide cin)
        i = kernels.x3.index(name) if name in kernels.x3 else None
        return i if i is not None and x3_allowed(policy, L) and L.cin % kernels.x3_bk[i] == 0 else None
    if isinstance(cfg, str) and cfg.startswith('h2:'):
        # the f16x2 twin of a direct-kernel tile: only from a '<key>|h2' entry (tools/tune_convs.py --h2 times it against the
        # bf16x3 tile per shape: it wins from batch 8-16 up, not on the launch-bound small batches)
        i = x3_config(cfg)
        if policy.h2_direct and i is not None:
            return Choice('x3', i, tuple(via))
        via.append(cfg)
        cfg = 'x3:' + cfg[3:]
    if isinstance(cfg, str) and cfg.startswith('x3:'):
        i = x3_config(cfg)
        if i is not None:
            return Choice('x3', i, tuple(via))
        via.append(cfg)
        cfg = table.get(L.key + '|f32')     # the best fp32-MFMA tile, recorded next to it
    if cfg == 'valu' and not (L.cin == 3 and (L.kh, L.kw, L.stride, L.dil) == (3, 3, 1, 1) and not L.has_res):
        cfg = None                          # the vector-ALU kernel exists for the 3-channel image layer only
    if cfg in kernels.direct:
        return Choice('direct', kernels.direct.index(cfg) + 1, tuple(via))
    return None


def choose_dgrad(policy, layer, fwd_tile, supported):
    """(Winograd code or None, bf16x3 config or None) of a training layer's data-gradient launch; both None: ct_conv2d_fwd in
    transposed mode.  fwd_tile: the Winograd code of the layer's forward launch (falsy: none).  supported(form): the library's
    geometry check 'ct_conv_<form>_supported' on the data gradient written as a forward convolution on dZ."""
    L, tile = layer, None
    if (L.kh, L.kw, L.stride, L.dil, L.ph, L.pw) == (3, 3, 1, 1, 1, 1) and L.zc % 8 == 0 and L.oh * L.ow >= 19 * 19:
        # 3x3 / stride 1 / pad 1 layers: the data gradient is itself such a convolution (channels swapped, taps rotated) ->
        # Winograd kernel on dY with ct_conv_pack_weights_wino_dgrad
        if supported('wino'):
            # F(4x4,3x3) where the forward launch of this layer uses it (same map, channels swapped) and on the multibox heads
            # from 19x19 maps up (their forward launch is a bf16x3 / F(2x2) one chosen for cout = 156; the data gradient has
            # cout = the source's channel count)
            tile = 4 if supported('wino4') and (fwd_tile in F4_TILES or (policy.wino4 and L.segs and L.oh * L.ow >= 361)) else 2
            # ... and its three-kernel bf16x3 form (tile 44) where the forward launch runs that one
            if fwd_tile in WINO4S_TILES and policy.dgrad_w4s and supported('wino4s'):
                tile = 47 if policy.h2 else 44
            elif fwd_tile in WINO4F_TILES and policy.dgrad_w4f and L.zc <= (policy.w4f_max_cin or 1 << 30) and supported('wino4f'):
                # ... and the fused bf16x3 F(4x4,3x3) kernel (tile 46) where the forward launch runs it: the narrow layers on
                # the big maps, whose data gradients were 7 launches x 1.13 ms of the 37.8 ms step on the fp32 kernel
                # (profiles/r05_train_kernel_stats.md)
                # (f16x2, tile 48: where dZ comes from ct_bias_act_backward_amax, which leaves the maxima the fused kernel
                # needs -- the VGG trunk; a BatchNorm layer's dZ has none: bf16x3)
                tile = 48 if policy.h2 and not L.is_bn and not L.segs else 46
    elif (L.kh, L.kw, L.stride) == (3, 3, 1) and L.dil > 1 and L.ph == L.pw == L.dil and L.zc % 16 == 0 and \
            fwd_tile in WINO4S_TILES and policy.dgrad_w4s and policy.dgrad_w4s_dil and supported('wino4s'):
        # dilated 3x3 layers (pad = dilation) whose forward launch runs the three-kernel form: their data gradient is the same
        # dilated convolution with channels swapped and taps rotated -> the same kernels (tiles on the dilation sub-lattices)
        tile = 47 if policy.h2 else 44
    x3 = None
    if tile is None and L.stride <= 2 and policy.x3 and L.zc % 16 == 0 and L.zc >= 32:
        # direct data gradients on the bf16 matrix pipe (bf16x3, ct_conv2d_x3_fwd transposed): every layer without a Winograd
        # data gradient whose channel counts fit the k-step; CTDET_X3=0 keeps ct_conv2d_fwd
        npix = L.batch * L.h * L.w
        x3 = 0 if -(-L.cin // 128) * -(-npix // 128) >= 512 else 3 if L.zc % 32 == 0 and -(-L.cin // 64) * -(-npix // 128) < 384 else 1
    return tile, x3

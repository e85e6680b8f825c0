"""The weight-gradient routes of the training engine: one record per entry point, the rule that picks one for a layer, and the
launch (the forward and data-gradient launches have ctdet/wino_forms.py).

  direct   ct_conv2d_wgrad: the fp32 MFMA GEMM with atomics, every filter size (csrc/ct_wgrad.hip)
  wino2    Winograd F(3x3, 2x2) fused on the fp32 MFMA (csrc/ct_wino_wgrad.hip)
  wino4    Winograd F(3x3, 4x4) fused on the fp32 MFMA (csrc/ct_wino4_wgrad.hip)
  wino4s   F(3x3, 4x4) as transform kernels + the bf16x3 GEMM, also the dilated 3x3 layers (csrc/ct_wino4s.hip)
  h2       the 1x1 layers on the f16 matrix pipe, f16x2 operand form, opt-in (csrc/ct_wgrad_h2.hip)
  direct_det, wino2_det, wino4_det   the deterministic twins of the first three: the same kernels with one slab per split in
           place of the atomics, the slabs added in order (CTDET_TRAIN_DETERMINISTIC=1; include/ctdet.h)

A route's workspace is one of three kinds: none; the accumulating float dU workspace (`zeroed`: TrainRuntime.wgrad_ws, or under
CTDET_PREZERO a slice of wgrad_ws_all per layer, zeroed once per step); a byte workspace shared by all layers of the route
(weight gradients run in stream order) and passed with its size."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional


@dataclass(frozen=True)
class Route:
    name: str
    launch: str
    label: str                          # what _lib.check appends to the layer's name
    supported: Optional[str] = None     # geometry query (None: takes every layer)
    size: Optional[str] = None          # workspace size query, in bytes
    ws: Optional[str] = None            # TrainRuntime attribute of the shared workspace (None: no workspace)
    zeroed: bool = False                # the float dU workspace, passed without a size
    dz_amax: bool = False               # takes dZ's per-image maxima (and X's, through desc.in_absmax)
    partials: bool = False              # the size query also reports the partial sums per output (a second argument)

    def workspace_bytes(self, lib, desc):
        if not self.size:
            return 0
        return int(getattr(lib, self.size)(C.byref(desc), *((None,) if self.partials else ())))

    def run(self, lib, desc, dz, ctot, dw, ws, dz_amax, stream):
        """Launch on desc: dZ = channels [0, ctot) of tensor dz, dw dense; ws = the workspace tensor of this layer (None: none)."""
        args = (C.byref(desc), dz.data_ptr(), ctot, 0) + ((dz_amax,) if self.dz_amax else ()) + (dw.data_ptr(),)
        if self.ws is not None:
            args += (ws.data_ptr(),) if self.zeroed else (ws.data_ptr(), ws.numel())
        return getattr(lib, self.launch)(*args, stream)


ROUTES = {r.name: r for r in (
    Route('direct', 'ct_conv2d_wgrad', ' wgrad'),
    Route('wino2', 'ct_conv2d_wgrad_wino', ' wgrad (winograd)', 'ct_conv_wgrad_wino_supported', 'ct_conv_wgrad_wino_workspace_bytes',
          'wgrad_ws', zeroed=True),
    Route('wino4', 'ct_conv2d_wgrad_wino4', ' wgrad (winograd)', 'ct_conv_wgrad_wino4_supported',
          'ct_conv_wgrad_wino4_workspace_bytes', 'wgrad_ws', zeroed=True),
    Route('wino4s', 'ct_conv2d_wgrad_wino4s', ' wgrad (winograd 4s)', 'ct_conv_wgrad_wino4s_supported',
          'ct_conv_wgrad_wino4s_workspace_bytes', 'wgrad_ws4s'),
    Route('h2', 'ct_conv2d_wgrad_h2', ' wgrad (f16x2)', 'ct_conv_wgrad_h2_supported', 'ct_conv_wgrad_h2_workspace_bytes', 'wgrad_wsh2',
          dz_amax=True),
)}
# deterministic twins, by the name of the route they replace; ONE slab workspace for the three (weight gradients run in stream order)
DET_ROUTES = {r.name[:-4]: r for r in (
    Route('direct_det', 'ct_conv2d_wgrad_det', ' wgrad (det)', None, 'ct_conv_wgrad_det_workspace_bytes', 'wgrad_wsdet', partials=True),
    Route('wino2_det', 'ct_conv2d_wgrad_wino_det', ' wgrad (winograd, det)', 'ct_conv_wgrad_wino_supported',
          'ct_conv_wgrad_wino_det_workspace_bytes', 'wgrad_wsdet', partials=True),
    Route('wino4_det', 'ct_conv2d_wgrad_wino4_det', ' wgrad (winograd, det)', 'ct_conv_wgrad_wino4_supported',
          'ct_conv_wgrad_wino4_det_workspace_bytes', 'wgrad_wsdet', partials=True),
)}


def h2_enabled(env):
    """CTDET_WGRAD_H2=1 (opt-in): the 1x1 layers that otherwise fall through to ct_conv2d_wgrad run ct_conv2d_wgrad_h2 (the f16x2
    GEMM of csrc/ct_wgrad_h2.hip: no atomics, bit-reproducible)."""
    return env.get('CTDET_WGRAD_H2', '0') not in ('', '0')


def choose(lib, st, desc, ctot, env, deterministic=False):
    """The route of plan step st (a fused conv of ctot output channels) with weight-gradient descriptor desc.  deterministic
    (TrainSwitches.deterministic): the same choice, then direct / wino2 / wino4 become their slab twins; wino4s and h2 have no
    atomics and stay."""
    def ok(route):
        return bool(getattr(lib, route.supported)(C.byref(desc)))
    hw = st.oh * st.ow
    route = ROUTES['direct']
    # 3x3 / stride 1 / pad 1: Winograd F(3x3, 2x2) weight gradient.  Maps below 10x10 stay on the direct kernel (tile padding
    # costs more than the transform saves there); CTDET_WGRAD_WINO=0 keeps the direct kernel everywhere.
    if bool(int(env.get('CTDET_WGRAD_WINO', '1'))) and hw >= 100 and ok(ROUTES['wino2']):
        # F(3x3, 4x4) from 19x19 maps up (15-20 % faster than F(3x3, 2x2) there, tools/wgrad_probe.py; slower on 10x10; the same
        # geometry); CTDET_WGRAD_WINO4=0 keeps F(3x3, 2x2)
        route = ROUTES['wino4'] if hw >= 361 and env.get('CTDET_WGRAD_WINO4', '1') != '0' else ROUTES['wino2']
    # the three-kernel bf16x3 form (ct_conv2d_wgrad_wino4s) for the wide layers: from CTDET_WGRAD_W4S_MIN_CIN input
    # channels up (default 256; 0 = never) where cin x cout >= 2^17 -- conv4_x, conv5_x, the 19x19 RFB layers
    # (profiles/r04_wgrad_probe.txt: 512 -> 512 @38x38 778 -> 503 us, 512 -> 512 @19x19 253 -> 184, 256 -> 512 @38x38
    # 437 -> 366; the multibox heads (cout 126..156: 238 -> 353) and 256 -> 256 @75x75 (750 -> 804) stay fused)
    w4s_min = int(env.get('CTDET_WGRAD_W4S_MIN_CIN', '256') or 0)
    # dilated 3x3 layers (conv6: 512 -> 1024, dilation 6) have no fused Winograd weight gradient; the three-kernel form
    # takes them with the tiles on the dilation sub-lattices, under the same size rule
    dilated = (st.kh, st.kw, st.stride) == (3, 3, 1) and st.dil > 1 and st.ph == st.pw == st.dil and \
        env.get('CTDET_TRAIN_W4S_DIL', '1') != '0'
    # dilated layers: the alternative is the direct fp32 kernel, so the rule is looser -- conv6 and the 256-channel RFB
    # branches (same-box A/B of the step: 2^17 / 2^16 / 2^14 with 128 channels: 38.2-40.1 / 37.7-38.2 / 38.4-38.5 ms)
    dil_prod = int(env.get('CTDET_WGRAD_W4S_DIL_PROD', str(1 << 16)))
    dil_cin = int(env.get('CTDET_WGRAD_W4S_DIL_CIN', '256'))
    if ((route.name == 'wino4' and st.cin >= w4s_min and st.cin * ctot >= (1 << 17)) or
            (dilated and st.cin >= dil_cin and st.cin * ctot >= dil_prod)) and w4s_min and ok(ROUTES['wino4s']):
        route = ROUTES['wino4s']
    # f16x2 where it wins (profiles/wgrad_h2_probe.txt): stride 1 on maps from 19x19 up.  The stride-2 layers (one gathered
    # load per pixel: 1024 -> 768 @19x19 86 -> 118 us) and the maps below 19x19 (20-45 us launches, where the two
    # maxima passes a BatchNorm layer's dZ needs cost 10 us) stay on ct_conv2d_wgrad.
    if route.name == 'direct' and h2_enabled(env) and st.stride == 1 and hw >= 361 and ok(ROUTES['h2']):
        route = ROUTES['h2']
    if deterministic:
        route = DET_ROUTES.get(route.name, route)
    return route

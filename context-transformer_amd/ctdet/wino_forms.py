"""The Winograd conv forms of the engine: one record per st.rt['wino'] code, for the forward launch and the data gradient.

  2, 4   F(2x2,3x3) / F(4x4,3x3) fused on the fp32 MFMA (csrc/ct_wino.hip, ct_wino4.hip)
  23     F(2x2,3x3) fused on the bf16 matrix pipe (bf16x3), two accumulators, eight waves (csrc/ct_wino_x3.hip)
  44     F(4x4,3x3) as transform / bf16x3 GEMM / transform kernels, two accumulators (csrc/ct_wino4s.hip)
  46     F(4x4,3x3) fused on bf16x3, one 64-cout block per workgroup (csrc/ct_wino4f.hip): the narrow layers on big maps
  47, 48 44 / 46 on the f16x2 operand form (two binary16 pieces, three products; csrc/ct_f16x2.h)
(codes 24 and 45, the one-accumulator variants of 23 and 44, existed in rounds 4-5: never selected, removed in round 6)
"""
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass(frozen=True)
class Form:
    code: int
    name: str                   # tune-table name
    config: int                 # ConvStep.rt['config'] value selecting it
    ok: str                     # st.rt flag of its geometry check
    path: str                   # ... named in the error when that check fails
    key: str                    # st.rt key of the forward packed weights
    size: str                   # size query of a packed buffer (cin, cout)
    floats: bool                # ... in floats (else bytes)
    pack: str
    pack_dgrad: Optional[str]   # None: no data-gradient form
    launch: Optional[str]       # None: the pool entry point with no pool
    launch_pool: str            # with the fused MaxPool2d(2, 2)
    variant: Optional[int] = None   # the `variant` / `dual` argument of the launch
    split: bool = False         # three-kernel form: shared V / M workspace; also takes dilated 3x3 layers (pad = dilation)
    h2: bool = False            # f16x2 operand form: reads desc.in_absmax
    own_max: bool = False       # ... takes the maxima itself, inside its launch, where in_absmax is unset
    plain: Optional[int] = None     # the same kernel on bf16x3 (an f16x2 form's twin)
    tracks: bool = False        # folds max |output| into desc.out_absmax
    f4: bool = False            # F(4x4,3x3)'s rounding (accuracy policies treat these alike)

    def alloc(self, lib, alloc, cin, cout, dgrad=False):
        """The packed-weight buffer of a (cin -> cout) forward layer; dgrad: of a data gradient (cin = the dZ channels)."""
        n = getattr(lib, self.size)(cin, cout)
        if self.floats:
            return alloc((n,))
        return alloc(((n + 3) // 4,)) if dgrad else alloc((n,), torch.uint8)

    def pack_weights(self, lib, ptrs, couts, n, cin, dst, stream, dgrad=False):
        return getattr(lib, self.pack_dgrad if dgrad else self.pack)(ptrs, couts, n, cin, dst, stream)

    def run(self, lib, desc, U, ws, pool, stream):
        """Launch on C.byref(desc) with packed weights U; ws = the V / M workspace tensor of a split form; pool = (pooled
        buffer, oh, ow, write_full) or None."""
        args = (desc, U) + ((ws.data_ptr(), ws.numel()) if self.split else ()) + \
            ((self.variant,) if self.variant is not None else ())
        if pool is not None:
            t, poh, pow_, full = pool
            return getattr(lib, self.launch_pool)(*args, t.data_ptr(), t.shape[1], 0, poh, pow_, int(full), stream)
        if self.launch is None:
            return getattr(lib, self.launch_pool)(*args, None, 0, 0, 0, 0, 1, stream)
        return getattr(lib, self.launch)(*args, stream)


_F32, _X3, _4S, _4F = 'Winograd path', 'Winograd bf16x3 path (cin % 16)', 'three-kernel Winograd path (cin % 16)', \
    'fused F(4x4,3x3) bf16x3 path (cin % 16)'
FORMS = {f.code: f for f in (
    Form(2, 'wino', -1, 'wino_ok', _F32, 'U', 'ct_conv_wino_packed_floats', True, 'ct_conv_pack_weights_wino',
         'ct_conv_pack_weights_wino_dgrad', 'ct_conv2d_wino_fwd', 'ct_conv2d_wino_pool_fwd'),
    Form(4, 'wino4', -2, 'wino_ok', _F32, 'U4', 'ct_conv_wino4_packed_floats', True, 'ct_conv_pack_weights_wino4',
         'ct_conv_pack_weights_wino4_dgrad', 'ct_conv2d_wino4_fwd', 'ct_conv2d_wino4_pool_fwd', f4=True),
    Form(23, 'winox', -3, 'winox_ok', _X3, 'UX', 'ct_conv_wino_x3_packed_bytes', False, 'ct_conv_pack_weights_wino_x3',
         None, 'ct_conv2d_wino_x3_fwd', 'ct_conv2d_wino_x3_pool_fwd', variant=1),
    Form(44, 'wino4s', -6, 'wino4s_ok', _4S, 'U4S', 'ct_conv_wino4s_packed_bytes', False, 'ct_conv_pack_weights_wino4s',
         'ct_conv_pack_weights_wino4s_dgrad', 'ct_conv2d_wino4s_fwd', 'ct_conv2d_wino4s_pool_fwd', variant=1, split=True,
         tracks=True, f4=True),
    Form(46, 'wino4f', -8, 'wino4f_ok', _4F, 'U4F', 'ct_conv_wino4f_packed_bytes', False, 'ct_conv_pack_weights_wino4f',
         'ct_conv_pack_weights_wino4f_dgrad', None, 'ct_conv2d_wino4f_pool_fwd_v', variant=1, f4=True),
    Form(47, 'wino4h', -9, 'wino4s_ok', _4S, 'U4H', 'ct_conv_wino4s_h2_packed_bytes', False, 'ct_conv_pack_weights_wino4s_h2',
         'ct_conv_pack_weights_wino4s_h2_dgrad', 'ct_conv2d_wino4s_fwd', 'ct_conv2d_wino4s_pool_fwd', variant=3, split=True,
         h2=True, own_max=True, plain=44, tracks=True, f4=True),
    Form(48, 'wino4fh', -10, 'wino4f_ok', _4F, 'U4FH', 'ct_conv_wino4f_h2_packed_bytes', False, 'ct_conv_pack_weights_wino4f_h2',
         'ct_conv_pack_weights_wino4f_h2_dgrad', None, 'ct_conv2d_wino4f_pool_fwd_v', variant=2, h2=True, plain=46, tracks=True,
         f4=True),
)}


def geometry_ok(rt, code):
    """Whether a conv with runtime state rt can run Winograd form `code` at all: the fused forms need a 3x3 s1 d1 p1 layer, the
    three-kernel form also takes dilated ones."""
    f = FORMS.get(code)
    return bool(rt.get('wino_ok') or (f is not None and f.split and rt.get('wino4s_ok')))

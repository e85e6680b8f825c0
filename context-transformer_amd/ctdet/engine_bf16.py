"""bf16 channels-last execution of the RFBNet plan (BASELINE.json configs[4]: "bf16 MFMA convs + fp32 NMS").

Same Plan / Runtime / two-stream schedule as the fp32 path (ctdet/engine.py); only the storage and the conv kernel
differ: every activation map is [batch, H, W, C] bfloat16 (C padded to a multiple of 8, so the 8 input channels an
MFMA lane needs at a filter tap are one 16-byte load and `torch.cat` is still a channel offset), convolutions run
`ct_conv2d_bf16_fwd` (v_mfma_f32_32x32x16_bf16, fp32 accumulate + fp32 epilogue), the multibox heads write their
fp32 channels-last outputs exactly as the fp32 kernels do, and everything after them (softmax, decode, NMS,
Context-Transformer block) is the unchanged fp32 code.  What models/RFB_Net_vgg.py:219-248 computes, at bf16
activation precision: select with `net.conv_dtype = 'bf16'` (or CTDET_DTYPE=bf16) before the first forward.

CTDET_BF16_WINO=1 (read once, when the backend is created; default 0 = the direct kernel everywhere, bit for bit as before):
the 3x3 / stride 1 layers with a plain bf16 output that the measured rule below selects (WINO_MIN_CIN input channels or more, at
most WINO_MAX_TILES tiles per launch; CTDET_BF16_WINO_MIN_CIN overrides it)
run `ct_conv2d_bf16_wino_fwd` instead -- Winograd F(4x4,3x3) with single binary16 operands in the transform domain on the f16
matrix pipe (csrc/ct_wino_bf16.hip), all such layers of a stream sharing one V / M workspace.  The per-image maxima the route
scales its operands by travel from a Winograd layer to the next one (directly or through a max-pool); any other input is
measured by the launch itself.
"""
import ctypes as C
import os

import torch

from . import _lib
from .engine import HipBackend, weight_parts, wire_absmax

# Which supported layers take the Winograd route when CTDET_BF16_WINO=1: the rule measured by tools/bf16_wino_probe.py
# (profiles/bf16_wino_probe.txt, every 3x3 / stride 1 shape of RFBNet-300 bs 32 and RFBNet-512 bs 16).  The three-kernel form moves
# 2 + 2 bytes of V and 4 + 4 of M per (tile, point, channel), so its bytes per flop grow as 1 / cin: it beats the direct kernel
# only at 512 input channels (1.08 - 1.19x at 19 x 19 / 38 x 38 bs 32 and 32 x 32 bs 16: 800 - 3 200 tiles per launch), is 0.96x
# at 64 x 64 bs 16 (4 096 tiles) and 0.33 - 0.92x on every narrower layer.  CTDET_BF16_WINO_MIN_CIN (the probe, experiments)
# replaces the channel rule and lifts the tile limit.
WINO_MIN_CIN = 512
WINO_MAX_TILES = 3200


class HipBackendBF16(HipBackend):
    tune_conv = None                 # one tile shape: nothing to tune

    def __init__(self, device):
        super().__init__(device)
        self._read_switches()

    def _read_switches(self):
        self.bf16_wino = os.environ.get('CTDET_BF16_WINO', '0') == '1'
        forced = os.environ.get('CTDET_BF16_WINO_MIN_CIN')
        self.bf16_wino_min_cin = int(forced) if forced else WINO_MIN_CIN
        self.bf16_wino_max_tiles = None if forced else WINO_MAX_TILES

    def alloc(self, shape, dtype=torch.float32):
        if len(shape) == 4 and dtype == torch.float32:          # (batch, C, H, W) of the plan -> NHWC bf16
            b, c, h, w = shape
            return torch.zeros((b, h, w, (c + 7) // 8 * 8), device=self.device, dtype=torch.bfloat16)
        return super().alloc(shape, dtype)

    def load_input(self, xbuf, x):
        b, c, h, w = x.shape
        _lib.check(self.lib.ct_nchw_f32_to_nhwc_bf16(x.data_ptr(), b, c, h * w, xbuf.shape[3], xbuf.data_ptr(),
                                                     self._stream()), 'input -> NHWC bf16')

    def prepare_conv(self, st, bufs, batch):
        lib, rt = self.lib, st.rt
        src = bufs[st.src]
        cin_buf = src.shape[3] if st.src == 'x' else st.cin      # the image is stored with 8 channels (5 zero)
        if st.src_coff % 8 or cin_buf % 8:
            raise _lib.CtdetError('%s: bf16 path needs channel slices in multiples of 8 (offset %d, %d channels)'
                                  % (st.name, st.src_coff, cin_buf))
        mpad = lib.ct_conv_mpad(st.cout)
        rt['wpk16'] = torch.empty(lib.ct_conv_bf16_packed_elems(st.cin, st.cout, st.kh, st.kw), dtype=torch.int16,
                                  device=self.device)
        rt['scale'] = torch.ones(mpad, device=self.device)
        rt['shift'] = torch.zeros(mpad, device=self.device)
        relus = [p.relu for p in st.parts]
        rt['lo'] = self._relu_floor(st, mpad)
        rt['mpad'] = mpad
        self.pack_conv(st)
        d = _lib.ConvDesc()
        d.in_ = src.data_ptr()
        d.batch, d.cin, d.h, d.w = batch, cin_buf, st.h, st.w
        d.in_ctot, d.in_coff = src.shape[3], st.src_coff
        d.wpacked, d.scale, d.shift = rt['wpk16'].data_ptr(), rt['scale'].data_ptr(), rt['shift'].data_ptr()
        d.cout = st.cout
        d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = st.kh, st.kw, st.stride, st.ph, st.pw, st.dil
        d.oh, d.ow = st.oh, st.ow
        if st.segs:
            d.nseg = len(st.segs)
            for g, sg in enumerate(st.segs):
                t = bufs[sg.dst]
                d.seg[g].ptr = t.data_ptr()
                d.seg[g].co_begin, d.seg[g].co_end = sg.co_begin, sg.co_end
                d.seg[g].pix_stride, d.seg[g].img_stride, d.seg[g].base = sg.pix_stride, t.shape[1], sg.base
        else:
            dst = bufs[st.dst]
            assert dst.shape[1] == st.oh and dst.shape[2] == st.ow, (st.name, dst.shape, st.oh, st.ow)
            d.out, d.out_ctot, d.out_coff = dst.data_ptr(), dst.shape[3], st.dst_coff
        if st.res is not None:
            r = bufs[st.res]
            d.res, d.res_ctot, d.res_coff, d.res_scale = r.data_ptr(), r.shape[3], st.res_coff, st.res_scale
        d.relu = int(all(relus))
        d.lo = rt['lo'].data_ptr() if rt['lo'] is not None else None
        npix = batch * st.oh * st.ow
        if int(os.environ.get('CTDET_KSPLIT', '1')) and st.cout * npix <= (2 << 20):
            rt['ksws'] = torch.empty(16 * st.cout * npix, device=self.device)     # split-K slabs (small maps)
            d.ksplit, d.ksplit_ws, d.ksplit_ws_floats = -1, rt['ksws'].data_ptr(), rt['ksws'].numel()
        rt['desc'] = d
        rt['wino_ok'] = False
        if getattr(self, 'bf16_wino', False):
            rt['wino_ok'] = bool(lib.ct_conv_bf16_wino_supported(C.byref(d)))
            tiles = batch * ((st.h + 3) // 4) * ((st.w + 3) // 4)
            if rt['wino_ok'] and st.cin >= self.bf16_wino_min_cin and \
                    (self.bf16_wino_max_tiles is None or tiles <= self.bf16_wino_max_tiles):
                self.enable_wino(st, True)

    def pack_conv(self, st):
        rt, lib = st.rt, self.lib
        for wt in [p.weight.detach() for p in st.parts]:
            if not (wt.device.type == self.device.type and wt.is_contiguous() and wt.dtype == torch.float32):
                raise _lib.CtdetError('%s: parameters must be contiguous fp32 on the HIP device' % st.name)
        ptrs, couts, n = weight_parts(st.parts)
        _lib.check(lib.ct_conv_pack_weights_bf16(ptrs, couts, n, st.cin, st.kh, st.kw, rt['wpk16'].data_ptr(),
                                                 self._stream()), 'ct_conv_pack_weights_bf16')
        self._fold_epilogue(st)
        if rt.get('bf16_wino'):
            _lib.check(lib.ct_conv_pack_weights_bf16_wino(ptrs, couts, n, st.cin, rt['UW16'].data_ptr(), self._stream()),
                       'ct_conv_pack_weights_bf16_wino')
        rt['versions'] = self.param_versions(st)

    def enable_wino(self, st, on=True, tile=None):
        """Route this conv through ct_conv2d_bf16_wino_fwd (CTDET_BF16_WINO=1 only) or back to the direct kernel."""
        rt = st.rt
        if not getattr(self, 'bf16_wino', False):
            if on:
                raise _lib.CtdetError('the bf16 path has no Winograd routing (CTDET_BF16_WINO=1 enables it)')
            return
        self.kernel_epoch += 1
        if not on:
            rt['bf16_wino'] = False
            rt.pop('ws4s_bytes', None)
            return
        if not rt.get('wino_ok'):
            raise _lib.CtdetError('%s: geometry has no bf16 Winograd path' % st.name)
        if 'UW16' not in rt:
            rt['UW16'] = torch.empty(self.lib.ct_conv_bf16_wino_packed_bytes(st.cin, st.cout), dtype=torch.uint8,
                                     device=self.device)
            dw = _lib.ConvDesc.from_buffer_copy(rt['desc'])      # the same launch geometry, the other weight layout
            dw.wpacked = rt['UW16'].data_ptr()
            dw.ksplit, dw.ksplit_ws, dw.ksplit_ws_floats = 0, None, 0
            rt['desc_w'] = dw
        rt['ws4s_bytes'] = self.lib.ct_conv_bf16_wino_workspace_bytes(C.byref(rt['desc_w']))
        self.ws_reserve(rt.get('ws_key', 0), rt['ws4s_bytes'])
        rt['bf16_wino'] = True
        self.pack_conv(st)

    @staticmethod
    def uses_ws(st):
        return bool(st.rt.get('bf16_wino'))

    def wire_absmax(self, runtime):
        """Maxima of |activation| per image (ct_conv_desc.in_absmax / out_absmax) between the Winograd launches: a buffer whose
        ONLY writers are Winograd launches -- seen directly or through max-pool steps, whose output the input bounds -- gets a
        slot that its writers fill and its Winograd readers scale by; every other Winograd layer measures its input itself."""
        return wire_absmax(self, runtime.batch, runtime.plan.steps, runtime.conv_steps(), lambda st: st.rt.get('desc_w'),
                           lambda st: bool(st.rt.get('bf16_wino')),
                           lambda w: w.kind == 'conv' and not w.segs and bool(w.rt.get('bf16_wino')))

    def policy_extra(self, steps):
        return {'bf16_wino': {'switch': 'CTDET_BF16_WINO', 'on': bool(getattr(self, 'bf16_wino', False)),
                              'min_cin': getattr(self, 'bf16_wino_min_cin', None),
                              'max_tiles': getattr(self, 'bf16_wino_max_tiles', None),
                              'layers': sum(1 for st in steps if st.rt.get('bf16_wino'))}}

    def run_conv(self, st):
        rt = st.rt
        if rt.get('bf16_wino'):
            ws = self.ws_pool[rt.get('ws_key', 0)]
            _lib.check(self.lib.ct_conv2d_bf16_wino_fwd(C.byref(rt['desc_w']), ws.data_ptr(), ws.numel(), self._stream()),
                       st.name)
            return
        _lib.check(self.lib.ct_conv2d_bf16_fwd(C.byref(rt['desc']), self._stream()), st.name)

    def run_pool(self, st, bufs, batch):
        src, dst = bufs[st.src], bufs[st.dst]
        assert src.shape[3] == dst.shape[3]
        _lib.check(self.lib.ct_maxpool2d_nhwc_bf16(src.data_ptr(), dst.data_ptr(), batch, src.shape[3], st.h, st.w,
                                                   st.oh, st.ow, st.k, st.stride, st.pad, self._stream()), st.name)

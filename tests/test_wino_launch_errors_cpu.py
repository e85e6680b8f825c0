"""The argument checks of the five Winograd forward launchers (csrc/ct_wino_launch.h and the checks each launcher keeps for
itself) without a device: every rejected call returns before any HIP call, so the library loads and answers on the CPU.  One valid
descriptor per entry point, then one thing broken at a time: the return code, the key word of ct_last_error_string() and the
entry point it names.  The pairs at the end break two things at once and pin which error wins."""
import ctypes as C
import re

import pytest

from ctdet import _lib

INVALID, UNSUPPORTED = 1, 4
IN, OUT, U, WS, SCALE, SHIFT, POOL, RES, SEG, AMAX = (0x10000 * i for i in range(1, 11))
GIB2_CTOT = 1 << 23             # x 8 x 8 x 4 bytes = 2 GiB per image


def _desc(**kw):
    """3x3, stride 1, pad 1, 16 -> 24 channels, 8x8, batch 2, fake non-null pointers."""
    d = _lib.ConvDesc()
    d.in_, d.out, d.scale, d.shift = IN, OUT, SCALE, SHIFT
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = 2, 16, 8, 8, 16, 0
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = 24, 3, 3, 1, 1, 1, 1
    d.oh, d.ow, d.out_ctot, d.out_coff = 8, 8, 24, 0
    seg = kw.pop('seg', None)
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    if d.kh == 1:
        d.pad_h = d.pad_w = 0
    if d.stride == 2:
        d.oh = d.ow = 4
    if d.dil == 2:
        d.pad_h = d.pad_w = 2
    if d.nseg:
        d.seg[0].ptr, d.seg[0].co_begin, d.seg[0].co_end, d.seg[0].pix_stride, d.seg[0].img_stride = seg, 0, 24, 24, 24 * 64
    return d


class Form:
    """One entry point (and variant): call(**what_to_break) -> (return code, message)."""

    def __init__(self, entry, variant=None, workspace=False, amax=False):
        self.entry, self.variant, self.workspace, self.amax = entry, variant, workspace, amax
        self.id = entry[len('ct_conv2d_'):] + ('' if variant is None else '-v%d' % variant)

    def desc(self, **kw):
        if self.amax:
            kw.setdefault('in_absmax', AMAX)
        return _desc(**kw)

    def call(self, d='valid', u=U, variant='valid', ws=WS, ws_bytes=None, pool=None, ctot=24, coff=0, oh=4, ow=4, write_full=1, **kw):
        lib = _lib.lib()
        d = self.desc(**kw) if d == 'valid' else d
        args = [C.byref(d) if d is not None else None, u]
        if self.workspace:
            args += [ws, lib.ct_conv_wino4s_workspace_bytes(C.byref(self.desc())) if ws_bytes is None else ws_bytes]
        if self.variant is not None:
            args.append(self.variant if variant == 'valid' else variant)
        rc = getattr(lib, self.entry)(*args, pool, ctot, coff, oh, ow, write_full, None)
        return rc, lib.ct_last_error_string().decode()


FORMS = [Form('ct_conv2d_wino_pool_fwd'), Form('ct_conv2d_wino4_pool_fwd'), Form('ct_conv2d_wino_x3_pool_fwd', 1),
         Form('ct_conv2d_wino4f_pool_fwd_v', 1), Form('ct_conv2d_wino4f_pool_fwd_v', 2, amax=True),
         Form('ct_conv2d_wino4s_pool_fwd', 1, workspace=True), Form('ct_conv2d_wino4s_pool_fwd', 3, workspace=True)]

# (what to break, return code, key word of the message)
ONE = [
    (dict(d=None), INVALID, 'null pointer'),
    (dict(u=None), INVALID, 'null pointer'),
    (dict(in_=None), INVALID, 'null tensor'),
    (dict(out=None), INVALID, 'null tensor'),
    (dict(scale=None), INVALID, 'null tensor'),
    (dict(kh=1, kw=1), UNSUPPORTED, 'needs 3x3'),
    (dict(stride=2), UNSUPPORTED, 'needs 3x3'),
    (dict(cin=12), UNSUPPORTED, 'needs 3x3'),
    (dict(batch=0), INVALID, 'bad shape'),
    (dict(cout=0), INVALID, 'bad shape'),
    (dict(write_full=0), INVALID, 'nothing to write'),
    (dict(pool=POOL, ctot=23), INVALID, 'pooled output slice'),
    (dict(pool=POOL, ctot=30, coff=7), INVALID, 'pooled output slice'),
    (dict(pool=POOL, coff=-1), INVALID, 'pooled output slice'),
    (dict(pool=POOL, oh=3, ow=4), INVALID, 'pooled size 3x4 for a 8x8 map'),
    (dict(in_ctot=20, in_coff=5), INVALID, 'input slice'),
    (dict(out_coff=-1), INVALID, 'output slice'),
    (dict(nseg=1, seg=None), INVALID, 'null segment'),
    (dict(nseg=1, seg=SEG, pool=POOL), INVALID, 'pooling with segmented output'),
    (dict(nseg=1, seg=SEG, write_full=0, pool=POOL), INVALID, 'pooling with segmented output'),
    (dict(res=RES, res_ctot=24, res_coff=4), INVALID, 'residual slice'),
    (dict(in_ctot=GIB2_CTOT), INVALID, 'one image exceeds 2 GiB'),
    (dict(out_ctot=GIB2_CTOT), INVALID, 'one image exceeds 2 GiB'),
    (dict(res=RES, res_ctot=GIB2_CTOT), INVALID, 'one image exceeds 2 GiB'),
]
# two things at once: (what to break, return code, the word of the error that wins)
TWO = [
    (dict(in_=None, kh=1, kw=1), INVALID, 'null tensor'),
    (dict(u=None, cin=12), INVALID, 'null pointer'),
    (dict(kh=1, kw=1, batch=0), UNSUPPORTED, 'needs 3x3'),
    (dict(batch=0, in_ctot=20, in_coff=5), INVALID, 'bad shape'),
    (dict(write_full=0, out_coff=-1), INVALID, 'nothing to write'),
    (dict(pool=POOL, ctot=23, in_ctot=20, in_coff=5), INVALID, 'pooled output slice'),
    (dict(pool=POOL, ctot=23, oh=3), INVALID, 'pooled output slice'),
    (dict(in_ctot=20, in_coff=5, out_coff=-1), INVALID, 'input slice'),
    (dict(out_coff=-1, res=RES, res_ctot=24, res_coff=4), INVALID, 'output slice'),
    (dict(res=RES, res_ctot=24, res_coff=4, in_ctot=GIB2_CTOT), INVALID, 'residual slice'),
]


def _check(form, kw, code, word):
    rc, msg = form.call(**kw)
    assert rc == code, (form.id, kw, rc, msg)
    assert word in msg, (form.id, kw, msg)
    assert msg.startswith(form.entry + ': '), (form.id, kw, msg)


@pytest.mark.parametrize('form', FORMS, ids=[f.id for f in FORMS])
def test_one_thing_broken(form):
    for kw, code, word in ONE:
        if form.amax and 'd' in kw:             # the f16x2 form of wino4f asks for d->in_absmax before the null checks
            word = 'in_absmax'
        _check(form, kw, code, word)


@pytest.mark.parametrize('form', FORMS, ids=[f.id for f in FORMS])
def test_two_things_broken_the_first_check_wins(form):
    for kw, code, word in TWO:
        _check(form, kw, code, word)


@pytest.mark.parametrize('form', [f for f in FORMS if f.variant is not None], ids=[f.id for f in FORMS if f.variant is not None])
def test_bad_variant(form):
    for v in (0, 4, 2 if form.workspace else 3, -1):
        _check(form, dict(variant=v), INVALID, 'variant %d' % v)


def test_variant_check_position():
    x3, f1, f2, s1, s3 = FORMS[2:]
    # x3 and wino4f look at the variant before anything else, the descriptor included
    for form in (x3, f1, f2):
        _check(form, dict(variant=7, d=None), INVALID, 'variant 7')
        _check(form, dict(variant=7, kh=1, kw=1), INVALID, 'variant 7')
    # wino4s: after the pointers and the geometry, before the shape
    for form in (s1, s3):
        _check(form, dict(variant=2, d=None), INVALID, 'null pointer')
        _check(form, dict(variant=2, in_=None), INVALID, 'null tensor')
        _check(form, dict(variant=2, kh=1, kw=1), UNSUPPORTED, 'needs 3x3')
        _check(form, dict(variant=2, batch=0), INVALID, 'variant 2')
        _check(form, dict(variant=2, write_full=0), INVALID, 'variant 2')


def test_wino4f_f16x2_needs_the_input_maxima():
    f1, f2 = FORMS[3:5]
    _check(f2, dict(in_absmax=None), INVALID, 'in_absmax')
    _check(f2, dict(d=None), INVALID, 'in_absmax')                     # asked before the null checks
    _check(f2, dict(in_absmax=None, u=None), INVALID, 'in_absmax')
    _check(f2, dict(in_absmax=None, variant=3), INVALID, 'variant 3')
    rc, msg = f1.call(in_absmax=None, batch=0)                          # the bf16x3 variant does not ask
    assert rc == INVALID and 'bad shape' in msg, msg


@pytest.mark.parametrize('form', FORMS[5:], ids=[f.id for f in FORMS[5:]])
def test_wino4s_workspace_and_dilated_pooling(form):
    lib = _lib.lib()
    _check(form, dict(ws=None), INVALID, 'null pointer')
    rc, msg = form.call(ws_bytes=0)
    assert rc == INVALID and 'workspace of 0 bytes' in msg, msg
    need = int(re.search(r'needs (\d+)', msg).group(1))
    assert 0 < need <= lib.ct_conv_wino4s_workspace_bytes(C.byref(form.desc()))
    _check(form, dict(ws_bytes=need - 1), INVALID, 'workspace of %d bytes, needs %d' % (need - 1, need))
    # the workspace is looked at last
    _check(form, dict(ws_bytes=need - 1, in_ctot=GIB2_CTOT), INVALID, 'one image exceeds 2 GiB')
    _check(form, dict(ws_bytes=need - 1, res=RES, res_ctot=24, res_coff=4), INVALID, 'residual slice')
    # dilation 2: supported as a plain layer, not with the fused pooling
    rc, msg = form.call(dil=2, batch=0)
    assert rc == INVALID and 'bad shape' in msg, msg
    _check(form, dict(dil=2, pool=POOL), INVALID, 'fused pooling on a dilated layer')
    _check(form, dict(dil=2, pool=POOL, ctot=23), INVALID, 'fused pooling on a dilated layer')
    _check(form, dict(dil=2, pool=POOL, in_ctot=20, in_coff=5), INVALID, 'fused pooling on a dilated layer')
    _check(form, dict(dil=2, pool=POOL, variant=2), INVALID, 'variant 2')
    _check(form, dict(dil=2, write_full=0), INVALID, 'nothing to write')

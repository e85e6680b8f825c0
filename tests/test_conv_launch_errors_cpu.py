"""The argument checks of the three direct convolution launchers (ct_conv2d_fwd, ct_conv2d_x3_fwd, ct_conv2d_bf16_fwd: the shared
ones of csrc/ct_conv_launch.h and the checks each launcher keeps for itself) without a device: every rejected call returns before
any HIP call, so the library loads and answers on the CPU.  One valid descriptor per entry point, then one thing broken at a time:
the return code, the key word of ct_last_error_string() and the entry point it names.  The pairs break two things at once and pin
which error wins, i.e. the order of the checks.  (No call here passes a descriptor that is valid: that one would launch.)"""
import ctypes as C

import pytest

from ctdet import _lib

INVALID, UNSUPPORTED = 1, 4
IN, OUT, W, SCALE, SHIFT, RES, SEG, AMAX, WX3 = (0x10000 * i for i in range(1, 10))
GIB2_CTOT = 1 << 23             # x 8 x 8 x 4 bytes = 2 GiB per fp32 image
X3_BK16, X3_BK32, H2_BK16 = 0, 2, 6      # ct_conv_x3_config_name: x3:128x128k16d, x3:128x64k32d, h2:128x128k16d
RES_BAD = dict(res=RES, res_ctot=24, res_coff=4)
FIVE = dict(kh=5, kw=5, pad_h=2, pad_w=2)                # a consistent 5x5 layer: no such direct kernel


def _desc(**kw):
    """3x3, stride 1, pad 1, 16 -> 24 channels, 8x8, batch 2, fake non-null pointers, packed sizes of ct_conv2d_fwd."""
    lib = _lib.lib()
    d = _lib.ConvDesc()
    d.in_, d.out, d.wpacked, d.scale, d.shift = IN, OUT, W, SCALE, SHIFT
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = 2, 16, 8, 8, 16, 0
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = 24, 3, 3, 1, 1, 1, 1
    d.oh, d.ow, d.out_ctot, d.out_coff = 8, 8, 24, 0
    d.m_pad, d.k_pad = lib.ct_conv_mpad(24), lib.ct_conv_kpad(16, 3, 3)
    seg = kw.pop('seg', SEG)
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    for g in range(max(0, min(d.nseg, 3))):
        d.seg[g].ptr, d.seg[g].co_begin, d.seg[g].co_end, d.seg[g].pix_stride, d.seg[g].img_stride = seg, 8 * g, 8 * g + 8, 8, 8 * 64
    return d


class Entry:
    """One entry point: call(**what_to_break) -> (return code, message)."""

    def __init__(self, name):
        self.name = name

    def call(self, d='valid', wx3=WX3, **kw):
        lib = _lib.lib()
        x3 = self.name == 'ct_conv2d_x3_fwd'
        config = kw.pop('config', X3_BK16) if x3 else None          # an argument there, desc->config (ignored there) elsewhere
        d = _desc(**kw) if d == 'valid' else d
        args = [C.byref(d) if d is not None else None]
        if x3:
            args += [wx3, config]
        rc = getattr(lib, self.name)(*args, None)
        return rc, lib.ct_last_error_string().decode()

    def check(self, kw, code, word):
        rc, msg = self.call(**kw)
        assert rc == code, (self.name, kw, rc, msg)
        assert word in msg, (self.name, kw, msg)
        assert msg.startswith(self.name) and msg[len(self.name)] in ':(', (self.name, kw, msg)      # "entry: " or "entry(transposed): "


FWD, X3, BF16 = Entry('ct_conv2d_fwd'), Entry('ct_conv2d_x3_fwd'), Entry('ct_conv2d_bf16_fwd')

# what ct_conv2d_fwd and ct_conv2d_x3_fwd check alike: (what to break, return code, key word of the message)
SHARED = [
    (dict(in_=None), INVALID, 'null tensor'),
    (dict(scale=None), INVALID, 'null tensor'),
    (dict(shift=None), INVALID, 'null tensor'),
    (dict(batch=0), INVALID, 'bad shape'),
    (dict(cin=0), INVALID, 'bad shape'),
    (dict(cout=0), INVALID, 'bad shape'),
    (dict(h=0), INVALID, 'bad shape'),
    (dict(w=-1), INVALID, 'bad shape'),
    (dict(oh=7), INVALID, 'oh/ow 7x8 != expected 8x8'),
    (dict(ow=9), INVALID, 'oh/ow 8x9 != expected 8x8'),
    (dict(stride=2), INVALID, 'oh/ow 8x8 != expected 4x4'),
    (dict(transposed=1, oh=9, ow=9), INVALID, '(transposed): dY 8x8 != forward output 9x9 of a 9x9 input'),
    (dict(transposed=1, stride=2), INVALID, '(transposed): dY 8x8 != forward output 4x4 of a 8x8 input'),
    (dict(in_ctot=20, in_coff=5), INVALID, 'input slice'),
    (dict(in_coff=-1), INVALID, 'input slice'),
    (dict(nseg=4), INVALID, 'nseg'),
    (dict(nseg=-1), INVALID, 'nseg'),
    (dict(out=None), INVALID, 'output slice'),
    (dict(out_coff=-1), INVALID, 'output slice'),
    (dict(out_ctot=23), INVALID, 'output slice'),
    (RES_BAD, INVALID, 'residual slice'),
    (dict(res=RES, res_ctot=24, res_coff=-1), INVALID, 'residual slice'),
    (dict(nseg=1, res=RES, res_ctot=24), INVALID, 'residual with segmented output'),
    (dict(nseg=1, seg=None), INVALID, 'null segment'),
    (dict(nseg=3, out=None, seg=None), INVALID, 'null segment'),
    (dict(in_ctot=GIB2_CTOT), INVALID, 'one image exceeds 2 GiB'),
]
SHARED_TWO = [
    (dict(in_=None, batch=0), INVALID, 'null tensor'),
    (dict(batch=0, stride=0), INVALID, 'bad shape'),
    (dict(cout=0, oh=7), INVALID, 'bad shape'),
    (dict(oh=7, in_coff=-1), INVALID, 'oh/ow 7x8'),
    (dict(transposed=1, oh=9, ow=9, in_coff=-1), INVALID, 'dY 8x8'),
    (dict(in_coff=-1, nseg=4), INVALID, 'input slice'),
    (dict(nseg=4, out_coff=-1), INVALID, 'nseg'),
    (dict(out_coff=-1, **RES_BAD), INVALID, 'output slice'),
    (dict(nseg=1, seg=None, res=RES, res_ctot=24), INVALID, 'residual with segmented output'),
    (dict(in_ctot=GIB2_CTOT, **RES_BAD), INVALID, 'residual slice'),
    (dict(in_ctot=GIB2_CTOT, nseg=2, seg=None), INVALID, 'null segment'),
]


@pytest.mark.parametrize('entry', [FWD, X3], ids=['fwd', 'x3'])
def test_shared_checks_one_thing_broken(entry):
    for kw, code, word in SHARED:
        entry.check(kw, code, word)


@pytest.mark.parametrize('entry', [FWD, X3], ids=['fwd', 'x3'])
def test_shared_checks_the_first_one_wins(entry):
    for kw, code, word in SHARED_TWO:
        entry.check(kw, code, word)


def test_fwd_own_checks():
    lib = _lib.lib()
    kpad = lib.ct_conv_kpad(16, 3, 3)
    nvalu = lib.ct_conv_num_configs()                               # the last configuration is 'valu'
    assert lib.ct_conv_config_name(nvalu - 1) == b'valu'
    one = [
        (dict(d=None), INVALID, 'null descriptor'),
        (dict(wpacked=None), INVALID, 'null tensor'),
        (dict(stride=0), INVALID, 'stride/dilation'),
        (dict(dil=0), INVALID, 'stride/dilation'),
        (dict(dil=-1), INVALID, 'stride/dilation'),
        (dict(m_pad=20), INVALID, 'm_pad'),
        (dict(m_pad=34), INVALID, 'm_pad'),
        (FIVE, UNSUPPORTED, '5x5 filters not built'),
        (dict(k_pad=kpad + 4), INVALID, 'k_pad=%d, expected %d' % (kpad + 4, kpad)),
        (dict(k_pad=0), INVALID, 'k_pad=0, expected %d' % kpad),
        (dict(m_pad=1 << 26), INVALID, 'weights too large'),
        (dict(config=nvalu + 1), INVALID, 'config %d' % (nvalu + 1)),
        (dict(config=99), INVALID, 'config 99'),
        (dict(config=nvalu), UNSUPPORTED, "config 'valu' is for 3x3 convolutions of 3 input channels"),
    ]
    for kw, code, word in one:
        FWD.check(kw, code, word)
    # where the launcher's own checks stand among the shared ones
    two = [
        (dict(wpacked=None, cin=0), INVALID, 'null tensor'),
        (dict(batch=0, stride=0), INVALID, 'bad shape'),
        (dict(dil=0, oh=7), INVALID, 'stride/dilation'),
        (dict(in_coff=-1, m_pad=20), INVALID, 'input slice'),
        (dict(m_pad=20, **FIVE), INVALID, 'm_pad'),
        (dict(m_pad=20, k_pad=0), INVALID, 'm_pad'),
        (dict(nseg=4, **FIVE), UNSUPPORTED, '5x5 filters not built'),
        (dict(k_pad=0, **FIVE), UNSUPPORTED, '5x5 filters not built'),
        (dict(k_pad=0, nseg=4), INVALID, 'k_pad=0'),
        (dict(k_pad=0, out_coff=-1), INVALID, 'k_pad=0'),
        (dict(m_pad=1 << 26, **RES_BAD), INVALID, 'residual slice'),
        (dict(m_pad=1 << 26, nseg=1, seg=None), INVALID, 'null segment'),
        (dict(m_pad=1 << 26, in_ctot=GIB2_CTOT), INVALID, 'weights too large'),
        (dict(in_ctot=GIB2_CTOT, config=99), INVALID, 'one image exceeds 2 GiB'),
        (dict(cout=20, config=nvalu), UNSUPPORTED, "config 'valu'"),
    ]
    for kw, code, word in two:
        FWD.check(kw, code, word)


def test_x3_own_checks():
    lib = _lib.lib()
    n = lib.ct_conv_x3_num_configs()
    assert lib.ct_conv_x3_config_bk(X3_BK16) == 16 and lib.ct_conv_x3_config_bk(X3_BK32) == 32
    assert lib.ct_conv_x3_config_h2(H2_BK16) == 1 and lib.ct_conv_x3_config_bk(H2_BK16) == 16
    big = dict(cout=1 << 24, out_ctot=1 << 24)                     # 9 x 3 x 16 x 2^24 x 2 bytes of split weights
    one = [
        (dict(d=None), INVALID, 'null pointer'),
        (dict(wx3=None), INVALID, 'null pointer'),
        (dict(config=-1), INVALID, 'config -1 (0..%d)' % (n - 1)),
        (dict(config=n), INVALID, 'config %d (0..%d)' % (n, n - 1)),
        (dict(kh=0), INVALID, 'filter geometry'),
        (dict(kw=0), INVALID, 'filter geometry'),
        (dict(stride=0), INVALID, 'filter geometry'),
        (dict(dil=0), INVALID, 'filter geometry'),
        (dict(transposed=1, stride=3), UNSUPPORTED, '(transposed): stride 3 (1 or 2)'),
        (dict(config=H2_BK16), INVALID, 'in_absmax'),
        (dict(config=H2_BK16, in_absmax=AMAX, transposed=1), INVALID, 'forward-only'),
        (dict(cin=24, in_ctot=24), UNSUPPORTED, 'cin=24 is not a multiple of the k-step (16 channels)'),
        (dict(config=X3_BK32), UNSUPPORTED, 'cin=16 is not a multiple of the k-step (32 channels)'),
        (dict(config=H2_BK16, in_absmax=AMAX, cin=24, in_ctot=24), UNSUPPORTED, 'cin=24 is not a multiple'),
        (big, INVALID, 'weights too large'),
        (dict(config=H2_BK16, in_absmax=AMAX, **big), INVALID, 'weights too large'),
        (dict(wpacked=None, in_ctot=GIB2_CTOT), INVALID, 'one image exceeds 2 GiB'),      # d->wpacked is not looked at
    ]
    for kw, code, word in one:
        X3.check(kw, code, word)
    two = [
        (dict(d=None, config=-1), INVALID, 'null pointer'),
        (dict(in_=None, config=-1), INVALID, 'null tensor'),
        (dict(config=-1, batch=0), INVALID, 'config -1'),
        (dict(batch=0, kh=0), INVALID, 'bad shape'),
        (dict(dil=0, oh=7), INVALID, 'filter geometry'),
        (dict(transposed=1, stride=3, dil=0), INVALID, 'filter geometry'),
        (dict(transposed=1, stride=3, batch=0), INVALID, 'bad shape'),
        (dict(transposed=1, stride=3, oh=9, ow=9), UNSUPPORTED, 'stride 3'),
        (dict(transposed=1, stride=3, in_coff=-1), UNSUPPORTED, 'stride 3'),
        (dict(config=H2_BK16, nseg=1, seg=None), INVALID, 'null segment'),
        (dict(config=H2_BK16, **RES_BAD), INVALID, 'residual slice'),
        (dict(config=H2_BK16, transposed=1), INVALID, 'in_absmax'),
        (dict(config=H2_BK16, in_absmax=AMAX, transposed=1, cin=24, in_ctot=24), INVALID, 'forward-only'),
        (dict(cin=24, in_ctot=24, **big), UNSUPPORTED, 'not a multiple'),
        (dict(cin=24, in_ctot=GIB2_CTOT), UNSUPPORTED, 'not a multiple'),
        (dict(in_ctot=GIB2_CTOT, **big), INVALID, 'weights too large'),
    ]
    for kw, code, word in two:
        X3.check(kw, code, word)


def test_bf16_checks():
    """NHWC bf16, forward only, the whole batch under one descriptor: a contract and a list of checks of its own."""
    one = [
        (dict(d=None), INVALID, 'null tensor'),
        (dict(in_=None), INVALID, 'null tensor'),
        (dict(wpacked=None), INVALID, 'null tensor'),
        (dict(scale=None), INVALID, 'null tensor'),
        (dict(shift=None), INVALID, 'null tensor'),
        (dict(batch=0), INVALID, 'bad shape'),
        (dict(cin=0), INVALID, 'bad shape'),
        (dict(cout=0), INVALID, 'bad shape'),
        (dict(transposed=1), INVALID, 'bad shape'),
        (dict(cin=12), INVALID, 'multiples of 8 (16-byte loads), got ctot 16 coff 0 cin 12'),
        (dict(in_ctot=20), INVALID, 'multiples of 8'),
        (dict(in_ctot=24, in_coff=4), INVALID, 'multiples of 8'),
        (dict(in_ctot=24, in_coff=16), INVALID, 'input slice'),
        (dict(in_coff=-8), INVALID, 'input slice'),
        (dict(oh=7), INVALID, 'oh/ow mismatch'),
        (dict(stride=2), INVALID, 'oh/ow mismatch'),
        (dict(h=0), INVALID, 'oh/ow mismatch'),
        (dict(out=None), INVALID, 'output slice'),
        (dict(out_coff=-1), INVALID, 'output slice'),
        (dict(out_ctot=23), INVALID, 'output slice'),
        (dict(nseg=4), INVALID, 'segments'),
        (dict(nseg=1, res=RES, res_ctot=24), INVALID, 'segments'),
        (dict(in_ctot=1 << 24), INVALID, 'input above 2 GiB'),
    ]
    for kw, code, word in one:
        BF16.check(kw, code, word)
    two = [
        (dict(in_=None, batch=0), INVALID, 'null tensor'),
        (dict(batch=0, cin=12), INVALID, 'bad shape'),
        (dict(transposed=1, oh=7), INVALID, 'bad shape'),
        (dict(cin=12, oh=7), INVALID, 'multiples of 8'),
        (dict(in_ctot=24, in_coff=16, oh=7), INVALID, 'input slice'),
        (dict(oh=7, out=None), INVALID, 'oh/ow mismatch'),
        (dict(oh=7, nseg=4), INVALID, 'oh/ow mismatch'),
        (dict(out_coff=-1, in_ctot=1 << 24), INVALID, 'output slice'),
        (dict(nseg=4, in_ctot=1 << 24), INVALID, 'segments'),
    ]
    for kw, code, word in two:
        BF16.check(kw, code, word)

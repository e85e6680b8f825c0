"""The argument checks of the five weight-gradient launchers (csrc/ct_wgrad_launch.h and the checks each launcher keeps for
itself) without a device: every rejected call returns before any HIP call, so the library loads and answers on the CPU.  One valid
descriptor per entry point, then one thing broken at a time: the return code, the key word of ct_last_error_string() and the
entry point it names; then pairs, which pin the error that wins.  The return codes are those the launchers gave before they
shared their checks, with one exception: ct_conv2d_wgrad accepted a bad input channel slice.  Where two broken things both give
CT_ERR_INVALID the order is the shared one: pointers, shape, input slice, dz slice.  (ct_conv2d_wgrad looks at the filter size only
after its first HIP call, so it has no "wrong geometry" row.)  Last, the workspace sizes: for the three-kernel form and the f16x2
GEMM they hold the split count, the part of the launch plan that shows without a device."""
import ctypes as C

import pytest

from ctdet import _lib

INVALID, WORKSPACE, UNSUPPORTED = 1, 3, 4
IN, DZ, DW, WS = 0x10000, 0x20000, 0x30000, 0x40000
GIB2_CTOT = 1 << 23             # x 8 x 8 x 4 bytes = 2 GiB per image


def _desc(k, **kw):
    """k x k, stride 1, pad k / 2, 16 -> 24 channels, 8x8, batch 2, a fake non-null input."""
    d = _lib.ConvDesc()
    d.in_ = IN
    d.batch, d.cin, d.h, d.w, d.in_ctot, d.in_coff = 2, 16, 8, 8, 16, 0
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = 24, k, k, 1, k // 2, k // 2, 1
    d.oh, d.ow = 8, 8
    for a, v in kw.items():
        assert hasattr(d, a), a
        setattr(d, a, v)
    return d


class Entry:
    """One entry point: call(**what_to_break) -> (return code, message).  group: D direct, F the two fused Winograd kernels,
    S the three-kernel form, H the f16x2 GEMM of the 1x1 layers."""

    def __init__(self, name, group, k=3, workspace=False, sized=None):
        self.name, self.group, self.k, self.workspace, self.sized = name, group, k, workspace, sized
        self.id = name[len('ct_conv2d_'):]

    def call(self, d='valid', dz=DZ, ctot=24, coff=0, dw=DW, ws=WS, short=0, **kw):
        lib = _lib.lib()
        d = _desc(self.k, **kw) if d == 'valid' else d
        args = [C.byref(d) if d is not None else None, dz, ctot, coff] + ([None] if self.group == 'H' else []) + [dw]
        if self.workspace:
            args.append(ws)
        if self.sized:
            args.append(getattr(lib, self.sized)(C.byref(_desc(self.k))) - short)
        rc = getattr(lib, self.name)(*args, None)
        return rc, lib.ct_last_error_string().decode()


ENTRIES = [Entry('ct_conv2d_wgrad', 'D'), Entry('ct_conv2d_wgrad_wino', 'F', workspace=True),
           Entry('ct_conv2d_wgrad_wino4', 'F', workspace=True),
           Entry('ct_conv2d_wgrad_wino4s', 'S', workspace=True, sized='ct_conv_wgrad_wino4s_workspace_bytes'),
           Entry('ct_conv2d_wgrad_h2', 'H', k=1, workspace=True, sized='ct_conv_wgrad_h2_workspace_bytes')]
IDS = [e.id for e in ENTRIES]

K1, K3 = dict(kh=1, kw=1, pad_h=0, pad_w=0), dict(kh=3, kw=3, pad_h=1, pad_w=1)
S2, S3, D2 = dict(stride=2, oh=4, ow=4), dict(stride=3, oh=3, ow=3), dict(dil=2, pad_h=2, pad_w=2)
BAD_IN, BAD_DZ = dict(in_ctot=20, in_coff=5), dict(ctot=23)
GEO3, GEO1 = 'needs 3x3', 'geometry of d: needs a 1x1'
# (what to break, the groups it applies to, return code, key word of the message)
ONE = [
    (dict(d=None), 'DFSH', INVALID, 'd is null'),
    (dict(in_=None), 'DFSH', INVALID, 'd->in is null'),
    (dict(dz=None), 'DFSH', INVALID, 'dz is null'),
    (dict(dw=None), 'DFSH', INVALID, 'dw is null'),
    (dict(ws=None), 'FSH', INVALID, 'workspace is null'),
    (dict(batch=0), 'DFSH', INVALID, 'bad shape'),
    (dict(cout=0), 'DH', INVALID, 'bad shape'),
    (dict(cout=0), 'FS', UNSUPPORTED, GEO3),            # cin, cout >= 1 belong to their geometry predicate
    (dict(cin=0), 'DH', INVALID, 'bad shape'),
    (dict(cin=0), 'FS', UNSUPPORTED, GEO3),
    (BAD_IN, 'DFSH', INVALID, 'input slice'),           # D: accepted before the launchers shared their checks
    (dict(in_coff=-1), 'DFSH', INVALID, 'input slice'),
    (BAD_DZ, 'DFSH', INVALID, 'dz slice'),
    (dict(coff=-1), 'DFSH', INVALID, 'dz slice'),
    (dict(ctot=30, coff=7), 'DFSH', INVALID, 'dz slice'),
    (K1, 'FS', UNSUPPORTED, GEO3),
    (S2, 'FS', UNSUPPORTED, GEO3),
    (S3, 'FS', UNSUPPORTED, GEO3),
    (D2, 'F', UNSUPPORTED, GEO3),
    (dict(cin=24, in_ctot=24), 'S', UNSUPPORTED, 'cin % 16'),
    (K3, 'H', UNSUPPORTED, GEO1),
    (S3, 'H', UNSUPPORTED, GEO1),
    (D2, 'H', UNSUPPORTED, GEO1),
    (dict(in_ctot=GIB2_CTOT), 'D', INVALID, 'one image exceeds 2 GiB'),
    (dict(in_ctot=GIB2_CTOT), 'FS', UNSUPPORTED, GEO3),                 # the predicate bounds the input image
    (dict(in_ctot=GIB2_CTOT), 'H', UNSUPPORTED, 'above 2 GiB'),
    (dict(ctot=GIB2_CTOT), 'DFS', INVALID, 'exceeds 2 GiB'),
    (dict(ctot=GIB2_CTOT), 'H', UNSUPPORTED, 'above 2 GiB'),
    (dict(oh=7), 'DH', INVALID, 'oh/ow'),
    (dict(oh=7), 'FS', UNSUPPORTED, GEO3),
    (dict(short=1), 'S', INVALID, 'workspace of 4128767 bytes, needs 4128768'),
    (dict(short=1), 'H', WORKSPACE, 'workspace_bytes is 2047, needs 2048'),
]
# two things at once: the error that wins
TWO = [
    # different codes: as the launchers always answered
    (dict(batch=0, **K3), 'H', INVALID, 'bad shape'),
    (dict(batch=0, **K1), 'FS', UNSUPPORTED, GEO3),
    (dict(dz=None, **K1), 'FS', INVALID, 'dz is null'),
    (dict(dz=None, **K3), 'H', INVALID, 'dz is null'),
    (dict(ws=None, **S3), 'FSH', INVALID, 'workspace is null'),
    (dict(**S3, **BAD_DZ), 'FS', UNSUPPORTED, GEO3),
    (dict(**S3, **BAD_DZ), 'H', UNSUPPORTED, GEO1),
    (dict(**S3, **BAD_IN), 'FS', UNSUPPORTED, GEO3),
    (dict(**S3, **BAD_IN), 'H', UNSUPPORTED, GEO1),
    (dict(oh=7, batch=0), 'FS', UNSUPPORTED, GEO3),
    (dict(oh=7, batch=0), 'DH', INVALID, 'bad shape'),
    (dict(oh=7, **BAD_DZ), 'FS', UNSUPPORTED, GEO3),
    (dict(oh=7, **BAD_DZ), 'H', INVALID, 'oh/ow'),          # its size check sits before the slices
    (dict(oh=7, **BAD_IN), 'H', INVALID, 'oh/ow'),
    (dict(in_ctot=GIB2_CTOT, **BAD_DZ), 'FS', UNSUPPORTED, GEO3),
    (dict(in_ctot=GIB2_CTOT, **BAD_DZ), 'H', INVALID, 'dz slice'),
    (dict(short=1, **BAD_DZ), 'SH', INVALID, 'dz slice'),   # the workspace size is looked at last
    (dict(short=1, in_ctot=GIB2_CTOT), 'S', UNSUPPORTED, GEO3),
    (dict(short=1, in_ctot=GIB2_CTOT), 'H', UNSUPPORTED, 'above 2 GiB'),
    (dict(short=1, ctot=GIB2_CTOT), 'S', INVALID, 'exceeds 2 GiB'),
    (dict(short=1, ctot=GIB2_CTOT), 'H', UNSUPPORTED, 'above 2 GiB'),
    # CT_ERR_INVALID twice: pointers -> shape -> input slice -> dz slice -> the launcher's sizes and limits
    (dict(dw=None, in_ctot=GIB2_CTOT), 'DFSH', INVALID, 'dw is null'),
    (dict(dz=None, batch=0), 'DFSH', INVALID, 'dz is null'),
    (dict(batch=0, **BAD_IN), 'DFSH', INVALID, 'bad shape'),
    (dict(**BAD_IN, **BAD_DZ), 'DFSH', INVALID, 'input slice'),
    (dict(oh=7, **BAD_IN), 'D', INVALID, 'input slice'),
    (dict(oh=7, **BAD_DZ), 'D', INVALID, 'dz slice'),
    (dict(in_ctot=GIB2_CTOT, **BAD_DZ), 'D', INVALID, 'dz slice'),
    (dict(ctot=GIB2_CTOT, coff=-1), 'DFSH', INVALID, 'dz slice'),
]


def _check(entry, kw, code, word):
    rc, msg = entry.call(**kw)
    assert rc == code, (entry.id, kw, rc, msg)
    assert word in msg, (entry.id, kw, msg)
    assert msg.startswith(entry.name + ': '), (entry.id, kw, msg)


@pytest.mark.parametrize('entry', ENTRIES, ids=IDS)
def test_one_thing_broken(entry):
    rows = [r for r in ONE if entry.group in r[1]]
    assert len(rows) >= 15
    for kw, _, code, word in rows:
        _check(entry, kw, code, word)


@pytest.mark.parametrize('entry', ENTRIES, ids=IDS)
def test_two_things_broken_the_first_check_wins(entry):
    rows = [r for r in TWO if entry.group in r[1]]
    assert len(rows) >= 8
    for kw, _, code, word in rows:
        _check(entry, kw, code, word)


def _wdesc(cin, cout, hw, batch, k=3, stride=1, dil=1):
    pad = dil * (k // 2)
    d = _desc(k, batch=batch, cin=cin, in_ctot=cin, cout=cout, h=hw, w=hw, stride=stride, dil=dil, pad_h=pad, pad_w=pad)
    d.oh = d.ow = (hw + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return d


# (cin, cout, map, batch) -> bytes, as the queries answered before the launchers shared their plan code
WS_3X3 = [(16, 24, 8, 2), (64, 64, 38, 2), (64, 64, 300, 32), (512, 512, 38, 32), (256, 512, 19, 32), (33, 20, 10, 8),
          (1024, 126, 19, 32), (128, 192, 5, 3)]
WS_WINO = [24576, 262144, 262144, 16777216, 8388608, 42240, 8257536, 1572864]
WS_WINO4 = [55296, 589824, 589824, 37748736, 18874368, 95040, 18579456, 3538944]
# (cin, cout, map, batch, dilation); the last one has cin % 16 != 0
WS_WINO4S = [((16, 24, 8, 2, 1), 4128768), ((256, 512, 19, 32, 1), 245956608), ((512, 512, 38, 32, 1), 821035008),
             ((512, 1024, 19, 32, 6), 533200896), ((256, 256, 19, 2, 2), 20054016), ((48, 20, 10, 8, 1), 7667712),
             ((1024, 126, 19, 32, 1), 312311808), ((128, 128, 37, 3, 2), 22413312), ((24, 24, 8, 2, 1), 0)]
# (cin, cout, map, batch, stride)
WS_H2 = [((64, 96, 19, 2, 1), 147968), ((16, 24, 8, 2, 1), 2048), ((512, 128, 38, 32, 1), 33562624), ((1024, 256, 19, 32, 1), 33562624),
         ((1024, 768, 19, 32, 2), 33562624), ((33, 20, 10, 8, 1), 17920), ((128, 128, 75, 32, 1), 33562624), ((48, 64, 38, 2, 2), 74240),
         ((2048, 2048, 1, 8, 1), 16779264)]


def test_workspace_bytes():
    lib = _lib.lib()
    for name, want in (('ct_conv_wgrad_wino_workspace_bytes', WS_WINO), ('ct_conv_wgrad_wino4_workspace_bytes', WS_WINO4)):
        assert [getattr(lib, name)(C.byref(_wdesc(*c))) for c in WS_3X3] == want, name
    for (cin, cout, hw, batch, dil), want in WS_WINO4S:
        assert lib.ct_conv_wgrad_wino4s_workspace_bytes(C.byref(_wdesc(cin, cout, hw, batch, dil=dil))) == want, (cin, cout, hw, dil)
    for (cin, cout, hw, batch, stride), want in WS_H2:
        assert lib.ct_conv_wgrad_h2_workspace_bytes(C.byref(_wdesc(cin, cout, hw, batch, k=1, stride=stride))) == want, (cin, cout, hw)
    assert lib.ct_conv_wgrad_wino_workspace_bytes(None) == lib.ct_conv_wgrad_wino4s_workspace_bytes(None) == 0

"""The C surface of synchronized BatchNorm without a device: the four ct_bn_sync_* entries are exported, declared in
include/ctdet.h and bound in ctdet._lib, the ABI is still 1, and every refusal include/ctdet.h lists is taken before any HIP call
(the pointers handed in are never dereferenced: a call that got past its checks would fault here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ctdet import _lib, train_engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('ct_bn_sync_stats_local', 'ct_bn_sync_stats_finish', 'ct_bn_sync_backward_local', 'ct_bn_sync_backward_apply')
CT_ERR_INVALID, CT_ERR_WORKSPACE = 1, 3
P = 0x10000
B, CH, HW = 8, 64, 5625             # 16 slices: the scratch is needed
NAN, INF = float('nan'), float('inf')


def test_exports_signatures_and_header():
    out = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == 'T'}
    header = open(os.path.join(REPO, 'include', 'ctdet.h')).read()
    for n in ENTRIES:
        assert n in exported, n
        assert n in _lib.SIGNATURES and _lib.SIGNATURES[n][0] is C.c_int and _lib.SIGNATURES[n][1][-1] is _lib._P, n
        assert re.search(r'\bint\s+%s\s*\(' % n, header), n
    # the header's argument lists and the table agree on the number of arguments
    for n in ENTRIES:
        decl = re.search(r'\bint\s+%s\s*\(([^;]*)\);' % n, header).group(1)
        assert len(decl.split(',')) == len(_lib.SIGNATURES[n][1]), n
    assert re.search(r'#define\s+CTDET_ABI_VERSION\s+1\b', header)
    assert _lib.lib().ct_abi_version() == 1


def _need():
    return int(_lib.lib().ct_bn_det_scratch_bytes(B, CH, HW, None))


def _stats_local(z=P, batch=B, channels=CH, hw=HW, sums=P, scratch=P, nbytes=None):
    return _lib.lib().ct_bn_sync_stats_local(z, batch, channels, 0, channels, hw, sums, scratch, _need() if nbytes is None else nbytes,
                                             None)


def _finish(sums=P, count=float(B * HW), channels=CH, mean=P, var=P):
    return _lib.lib().ct_bn_sync_stats_finish(sums, count, channels, mean, var, 0.01, None, None, None)


def _bwd_local(dy=P, y=P, z=P, mean=P, var=P, relu=1, batch=B, channels=CH, hw=HW, sums=P, dgamma=P, dbeta=P, scratch=P, nbytes=None):
    return _lib.lib().ct_bn_sync_backward_local(dy, channels, 0, y, channels, 0, z, mean, var, 1e-5, relu, None, 1.0, channels, 0, batch,
                                                channels, hw, sums, dgamma, dbeta, scratch, _need() if nbytes is None else nbytes, None)


def _bwd_apply(dy=P, y=P, z=P, mean=P, var=P, gamma=P, relu=1, dz=P, batch=B, channels=CH, hw=HW, sums=P, count=float(B * HW)):
    return _lib.lib().ct_bn_sync_backward_apply(dy, channels, 0, y, channels, 0, z, mean, var, gamma, 1e-5, relu, None, 1.0, None, 0, 0, 0,
                                                dz, channels, 0, batch, channels, hw, sums, count, None)


SIZES = [dict(batch=0), dict(batch=-1), dict(channels=0), dict(hw=0), dict(hw=-3)]
COUNTS = [dict(count=0.0), dict(count=0.5), dict(count=-4.0), dict(count=NAN), dict(count=INF)]
SCRATCH = [(dict(scratch=None), CT_ERR_INVALID, 'scratch is null'), (dict(scratch=P + 4), CT_ERR_INVALID, 'aligned'),
           (dict(nbytes=16 * 2 * CH * 8 - 1), CT_ERR_WORKSPACE, 'scratch_bytes'), (dict(nbytes=0), CT_ERR_WORKSPACE, 'scratch_bytes')]
REFUSALS = (
    [('ct_bn_sync_stats_local', _stats_local, kw, CT_ERR_INVALID, None) for kw in [dict(z=None), dict(sums=None)] + SIZES]
    + [('ct_bn_sync_stats_local', _stats_local, kw, code, word) for kw, code, word in SCRATCH]
    + [('ct_bn_sync_stats_finish', _finish, kw, CT_ERR_INVALID, None)
       for kw in [dict(sums=None), dict(mean=None), dict(var=None), dict(channels=0), dict(channels=-2)] + COUNTS]
    + [('ct_bn_sync_backward_local', _bwd_local, kw, CT_ERR_INVALID, None)
       for kw in [dict(dy=None), dict(z=None), dict(mean=None), dict(var=None), dict(sums=None), dict(dgamma=None), dict(dbeta=None),
                  dict(y=None)] + SIZES]
    + [('ct_bn_sync_backward_local', _bwd_local, kw, code, word) for kw, code, word in SCRATCH]
    + [('ct_bn_sync_backward_apply', _bwd_apply, kw, CT_ERR_INVALID, None)
       for kw in [dict(dy=None), dict(z=None), dict(mean=None), dict(var=None), dict(gamma=None), dict(dz=None), dict(sums=None),
                  dict(y=None)] + SIZES + COUNTS]
)


@pytest.mark.parametrize('name,call,kw,code,word', REFUSALS, ids=['%s-%s' % (r[0][11:], ','.join('%s=%s' % kv for kv in r[2].items()))
                                                                  for r in REFUSALS])
def test_refusals_come_before_any_hip_call(name, call, kw, code, word):
    lib = _lib.lib()
    assert call(**kw) == code, (name, kw)
    msg = lib.ct_last_error_string().decode()
    assert msg.startswith(name + ':'), msg
    if word:
        assert word in msg, msg


def test_a_misaligned_scratch_is_refused_even_where_one_slice_needs_none():
    assert _stats_local(batch=2, hw=9, scratch=P + 4) == CT_ERR_INVALID
    assert _bwd_local(batch=2, hw=9, scratch=P + 4) == CT_ERR_INVALID


def test_switch_defaults_to_off_and_is_read_with_the_other_training_switches():
    of = train_engine.TrainSwitches.of
    assert of({}).sync_bn is False and of({'CTDET_SYNC_BN': '0'}).sync_bn is False and of({'CTDET_SYNC_BN': ''}).sync_bn is False
    assert of({'CTDET_SYNC_BN': '1'}).sync_bn is True
    assert of({'CTDET_SYNC_BN': '1'}).deterministic is False and of({'CTDET_TRAIN_DETERMINISTIC': '1'}).sync_bn is False

"""tools/sync_bn_probe.py starts one process per rank; when one of them fails, none may stay behind on a device.  The launcher
(run_ranks) is run here with stand-in workers that need no GPU: the first rank that ends with a non-zero status ends the run at
once, and the rank that would have gone on for minutes -- the python under its `timeout` wrapper, not only the wrapper -- is gone
when run_ranks returns."""
import importlib.util
import os
import sys
import time

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STANDIN = r'''
import os, sys, time
rank, out = int(os.environ['RANK']), sys.argv[1]
open(os.path.join(out, 'pid%d' % rank), 'w').write(str(os.getpid()))
mode = sys.argv[2]
if mode == 'ok':
    if rank == 0:
        print('SYNC_BN_PROBE {"ms_per_step": 1.5}', flush=True)
    sys.exit(0)
if rank == int(mode):
    while not os.path.exists(os.path.join(out, 'pid%d' % (1 - rank))):
        time.sleep(0.01)
    sys.exit(3)
time.sleep(600)             # a rank blocked in a collective its peer never joins
'''


@pytest.fixture(scope='module')
def probe():
    spec = importlib.util.spec_from_file_location('sync_bn_probe', os.path.join(REPO, 'tools', 'sync_bn_probe.py'))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = path
    return mod


def _alive(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    # a killed child of another process may linger as a zombie until it is reaped
    try:
        return open('/proc/%d/stat' % pid).read().rsplit(')', 1)[1].split()[0] != 'Z'
    except OSError:
        return False


def _cmd(tmp_path):
    script = tmp_path / 'standin.py'
    script.write_text(STANDIN)
    return [sys.executable, str(script)]


def test_all_ranks_succeeding_gives_rank_zeros_line(probe, tmp_path):
    assert probe.run_ranks([str(tmp_path), 'ok'], 2, 60, cmd=_cmd(tmp_path)) == {'ms_per_step': 1.5}


@pytest.mark.parametrize('failing', [0, 1])
def test_a_failing_rank_ends_the_others_before_the_run_stops(probe, tmp_path, failing):
    t0 = time.monotonic()
    with pytest.raises(SystemExit) as e:
        probe.run_ranks([str(tmp_path), str(failing)], 2, 300, cmd=_cmd(tmp_path))
    took = time.monotonic() - t0
    assert 'rank %d' % failing in str(e.value) and 'status 3' in str(e.value)
    other = int((tmp_path / ('pid%d' % (1 - failing))).read_text())
    assert not _alive(other), 'the worker under the timeout wrapper outlived the run'
    assert took < 30, took          # far below the ranks' own limit (300 s) and the stand-in's 600 s

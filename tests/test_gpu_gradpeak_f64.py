"""GradPeak on float64 frames against the reference run in float64 (tests/golden/f17_gradpeak_f64.npz, make_golden_f64.py):
toa_detect / grad_peak_detect / GradPeak keep a float64 input in double end to end, as the reference does.  Onset and
peak indices must be identical on every row, amplitudes within 1e-12 (inputs have max-abs ~1); the fixture keeps every
smoothed-gradient sample at least 1e-9 x max|grad| away from the thresholds, so exact indices are a fair bar."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden
import f64_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f17_gradpeak_f64')


def assert_echoes(got, want):
    got = got.cpu()
    assert got.dtype == torch.float64
    got = got.numpy()
    assert got.shape == want.shape
    assert np.array_equal(got[..., :2], want[..., :2])             # onset / peak indices, every row
    assert np.max(np.abs(got[..., 2] - want[..., 2]), initial=0.0) <= 1e-12


def toa_input(g, rf, dev):
    return torch.from_numpy(f64_inputs.echo_frames(1024, 2000, int(g[f'toa_rf{rf}_seed']))).to(dev)


@pytest.mark.parametrize('rf', [10, 20])
@pytest.mark.parametrize('thn,th', [('th1e-3', 1e-3), ('thdef', None)])
def test_toa_detect_f64_matches_reference(dev, g, rf, thn, th):
    from stofnet_amd import toa_detect
    assert_echoes(toa_detect(toa_input(g, rf, dev), threshold=th, rescale_factor=rf), g[f'toa_rf{rf}_{thn}'])


def test_toa_detect_f64_long_rows(dev, g):
    from stofnet_amd import toa_detect
    x = torch.from_numpy(f64_inputs.echo_frames(64, 30720, int(g['long_rf20_seed']))).to(dev)
    assert_echoes(toa_detect(x, threshold=None, rescale_factor=20), g['long_rf20_thdef'])


def test_grad_peak_detect_f64_envelope_default_args(dev, g):
    from stofnet_amd import grad_peak_detect
    env = torch.from_numpy(f64_inputs.envelopes(256, 1536, 1703)).to(dev)
    assert_echoes(grad_peak_detect(env), g['gpd_env'])               # Kmax 238: the re-run past the first cap


def test_gradpeak_module_chirp_and_pala_settings(dev, g):
    from stofnet_amd import GradPeak
    x = torch.from_numpy(f64_inputs.echo_frames(512, 2000, 1704)[:, None, :]).to(dev)
    on = GradPeak(threshold=None, rescale_factor=10, echo_max=1, onset_opt=True)(x)
    assert int(g['chirp_kmax']) > 1                                  # the echo_max reduction ran
    assert on.dtype == torch.float64 and np.array_equal(on.cpu().numpy(), g['chirp'])
    xp = torch.from_numpy(f64_inputs.pala_frames(2, 16, 30720, 1201)).to(dev)
    pk = GradPeak(threshold=1e-5, rescale_factor=20, echo_max=float('inf'), onset_opt=False)(xp)
    assert pk.dtype == torch.float64 and np.array_equal(pk.cpu().numpy(), g['pala'])


def test_discriminating_threshold_needs_float64(dev, g):
    """th sits 1e-10 relative below one smoothed-gradient sample: the reference's float32 run gets other indices there
    (asserted by the generator), its float64 run is the fixture"""
    from stofnet_amd import toa_detect
    x = torch.from_numpy(f64_inputs.echo_frames(16, 2000, 1705)).to(dev)
    assert_echoes(toa_detect(x, threshold=float(g['disc_th']), rescale_factor=10), g['disc'])


@pytest.mark.parametrize('case,rf', [('toa_rf10_thdef', 10), ('toa_rf20_thdef', 20)])
def test_default_threshold_on_device_f64(dev, g, case, rf):
    """moments -> threshold through the ABI: within 1e-12 relative of the reference's std()**16 * 1.2e13, bitwise repeatable"""
    from stofnet_amd import _lib
    from stofnet_amd.gradpeak import _taps_on
    from stofnet_amd.hilbert import hilbert_envelope
    lib = _lib.lib()
    env = hilbert_envelope(toa_input(g, rf, dev))
    n, L = env.shape
    gs = rf // 6 * 5
    taps = _taps_on(dev, gs, torch.float64)
    ws = torch.empty(lib.stof_gradpeak_moments_f64_workspace_bytes(n), dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr(dev)
    ths = []
    for _ in range(2):
        stats = torch.tensor([0.0, 0.0, float(n * L)], dtype=torch.float64, device=dev)
        th = torch.empty(1, dtype=torch.float64, device=dev)
        assert lib.stof_gradpeak_moments_f64(_lib.ptr(env), n, L, gs, _lib.ptr(taps), (taps.numel() - 1) // 2, _lib.ptr(stats),
                                             _lib.ptr(ws), ws.numel(), stream) == 0
        assert lib.stof_gradpeak_threshold_f64(_lib.ptr(stats), _lib.ptr(th), stream) == 0
        ths.append((stats.cpu().numpy().tobytes(), float(th.cpu())))
    assert ths[0] == ths[1]
    want = float(g[case + '_th'])
    assert abs(ths[0][1] - want) <= 1e-12 * want


def test_degenerate_inputs_f64(dev):
    from stofnet_amd import grad_peak_detect, toa_detect
    flat = torch.zeros(5, 2000, dtype=torch.float64, device=dev)
    out = toa_detect(flat, threshold=1e-3, rescale_factor=10)        # no edges at all
    assert out.dtype == torch.float64 and tuple(out.shape) == (5, 0)
    # Q9: rising and falling edges 700 samples apart, outside the gate (1, 6) -> the reference's empty float32 [3, 0]
    e = np.zeros(1536)
    e[500:800] = np.linspace(0, 1, 300)
    e[800:1200] = 1
    e[1200:1500] = np.linspace(1, 0, 300)
    q9 = grad_peak_detect(torch.from_numpy(np.stack([e] * 3)).to(dev), threshold=1e-5)
    assert tuple(q9.shape) == (3, 0) and q9.dtype == torch.float32 and q9.device.type == 'cpu'
    empty = toa_detect(torch.zeros(0, 2000, dtype=torch.float64, device=dev), threshold=1e-3, rescale_factor=10)
    assert empty.dtype == torch.float64 and tuple(empty.shape) == (0, 0)


def test_odd_batch_and_single_row_equal_their_rows(dev, g):
    from stofnet_amd import toa_detect
    x = toa_input(g, 10, dev)
    full = toa_detect(x, threshold=1e-3, rescale_factor=10).cpu()
    for lo, hi in ((0, 1), (100, 101), (3, 40), (500, 1023)):
        part = toa_detect(x[lo:hi].contiguous(), threshold=1e-3, rescale_factor=10).cpu()
        k = part.shape[1]
        assert torch.equal(part, full[lo:hi, :k]) and not full[lo:hi, k:].any()


CHILD = r'''
import datetime, os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import f64_inputs
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=120))
from stofnet_amd import GradPeak, toa_detect
x = torch.from_numpy(f64_inputs.echo_frames(256, 2000, 1701)).to(dev)
local = toa_detect(x, threshold=None, rescale_factor=10)
shard = toa_detect(x, threshold=None, rescale_factor=10, sharded=True)
assert shard.dtype == torch.float64 and torch.equal(local, shard)
m = GradPeak(threshold=None, rescale_factor=10, echo_max=1, onset_opt=True, sharded=True)
assert torch.equal(m(x[:, None]), GradPeak(threshold=None, rescale_factor=10, echo_max=1, onset_opt=True)(x[:, None]))
dist.destroy_process_group()
print('ok')
'''


def test_sharded_f64_one_rank_rccl(dev):
    """sharded=True on float64 under a one-rank nccl group with the collectives forced on: the float64 moment triple
    goes through RCCL's SUM all-reduce and the result equals the unsharded call (child process, as test_rccl_one_rank)"""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', LOCAL_WORLD_SIZE='1', MASTER_ADDR='127.0.0.1',
               MASTER_PORT=str(port), STOF_FORCE_COLLECTIVES='1',
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'),
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

"""ZonziniNetSmall / ZonziniNetLarge on the gfx950 kernels against the reference's fp32 outputs
(tests/golden/f18_zonzini.npz, make_golden_zonzini.py) and the float64 restatement of test_zonzini_cpu.py: outputs and
pooled features within 1e-5 x max|ref|; the error contract (short rows, dtypes, devices, training); bitwise batch
invariance and determinism; NaN isolation; re-packing after a weight change; `main.py model=zonzini`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden, load_weights
import zonzini_inputs as zi
from test_zonzini_cpu import CASES, forward64, weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f18_zonzini')


def make(net, sd, dev):
    from stofnet_amd import ZonziniNetLarge, ZonziniNetSmall
    m = ZonziniNetSmall() if net == 'small' else ZonziniNetLarge()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def small(dev):
    return make('small', load_weights('graceful-wave'), dev)


@pytest.mark.parametrize('name,net,n,L', CASES)
def test_matches_reference(dev, g, name, net, n, L):
    sd = weights(net, g)
    m = make(net, sd, dev)
    x = zi.echo_frames(n, L, int(g[f'{name}_seed']))
    with torch.no_grad():
        y, f = m.forward_with_features(torch.from_numpy(x).to(dev))
    y, f = y.cpu().numpy(), f.cpu().numpy()
    ry, rf = g[f'{name}_y'], g[f'{name}_feat']
    y64, f64 = forward64(sd, x)
    assert y.shape == ry.shape == (n, 1) and f.shape == rf.shape
    ey, ef = np.abs(y - ry).max() / np.abs(ry).max(), np.abs(f - rf).max() / np.abs(rf).max()
    ey64, ef64 = np.abs(y - y64).max() / np.abs(y64).max(), np.abs(f - f64).max() / np.abs(f64).max()
    print(f'{name}: y {ey:.2e} vs ref fp32, {ey64:.2e} vs f64 (ref fp32 vs f64 {np.abs(ry - y64).max() / np.abs(y64).max():.2e}); '
          f'features {ef:.2e} / {ef64:.2e}')
    assert max(ey, ey64, ef, ef64) <= 1e-5
    assert torch.equal(m(torch.from_numpy(x).to(dev)), torch.from_numpy(y).to(dev))      # eval mode, grad enabled


@pytest.mark.parametrize('net,L', [('small', 935), ('small', 10), ('large', 3751), ('large', 936)])
def test_too_short_rows_raise(dev, net, L):
    m = make(net, zi.seeded_weights(zi.SMALL_CHANNELS if net == 'small' else zi.LARGE_CHANNELS, 3), dev)
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 1, L, device=dev))


def test_batch_invariance_and_chunking(dev, g, small):
    x = torch.from_numpy(zi.echo_frames(256, 2000, int(g['small_chirp_seed']))).to(dev)
    full = small(x)
    for r in (0, 1, 100, 255):
        assert torch.equal(small(x[r:r + 1]), full[r:r + 1])
    assert torch.equal(small(x[50:57]), full[50:57])
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(0)).to(dev)
    assert torch.equal(small(x[perm]), full[perm])
    small.max_workspace_bytes = 200_000                                       # about 5 rows per chunk
    try:
        y, f = small.forward_with_features(x)
    finally:
        del small.max_workspace_bytes
    assert torch.equal(y, full)
    assert torch.equal(small(x), full)                                        # deterministic across calls


def test_nan_isolation(dev, g, small):
    x = torch.from_numpy(zi.echo_frames(8, 2000, 5)).to(dev)
    ref = small(x)
    x[3, 0, 777] = float('nan')
    y = small(x)
    assert torch.isnan(y[3]).all()
    keep = torch.arange(8, device=dev) != 3
    assert torch.equal(y[keep], ref[keep])


def test_dtype_device_and_training_errors(dev, small):
    x = torch.zeros(2, 1, 2000, device=dev)
    with pytest.raises(TypeError):
        small(x.double())
    with pytest.raises(TypeError):
        small(x.half())
    with pytest.raises(RuntimeError, match='ROCm device'):
        small(x.cpu())
    from stofnet_amd import ZonziniNetSmall
    m = ZonziniNetSmall().to(dev).eval().double()
    with pytest.raises(TypeError):
        m(x)
    small.train()
    try:
        with pytest.raises(NotImplementedError, match='training is not implemented'):
            small(x)
        with torch.no_grad():
            y = small(x)                                                      # train mode under no_grad: inference
        assert not y.requires_grad
    finally:
        small.eval()
    with pytest.raises(NotImplementedError):
        small(x.clone().requires_grad_(True))
    assert all(p.requires_grad for p in small.parameters())
    y = small(x)                                                              # eval mode, grad enabled: a plain tensor
    assert not y.requires_grad and y.grad_fn is None


def test_repacks_after_weight_change(dev, g):
    x = torch.from_numpy(zi.echo_frames(16, 2000, 11)).to(dev)
    sd_a, sd_b = load_weights('graceful-wave'), zi.seeded_weights(zi.SMALL_CHANNELS, 99)
    m = make('small', sd_a, dev)
    ya = m(x)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_b.items()}, strict=True)
    yb = m(x)
    assert torch.equal(yb, make('small', sd_b, dev)(x))
    assert not torch.equal(ya, yb)
    with torch.no_grad():
        m.fc2.bias.add_(1.0)                                                  # in-place edit
    assert torch.allclose(m(x), yb + 1.0, rtol=0, atol=1e-4)
    m.invalidate_packed()
    assert torch.allclose(m(x), yb + 1.0, rtol=0, atol=1e-4)


def run_main(tmp_path, args):
    ck = tmp_path / 'ckpts'
    ck.mkdir(exist_ok=True)
    torch.save({k: torch.from_numpy(v) for k, v in load_weights('graceful-wave').items()},
               ck / 'graceful-wave-1444_rf-scale10_epoch_32.pth')
    out = tmp_path / 'es.npy'
    code = ('import sys, json, numpy as np; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[3:]); np.save(sys.argv[2], es); print(json.dumps(s))')
    res = subprocess.run([sys.executable, '-c', code, ROOT, str(out), 'model=zonzini', 'evaluate=True', f'ckpt_dir={ck}'] + args,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    return np.load(out), json.loads(res.stdout.strip().splitlines()[-1])


def test_main_zonzini_chirp_selects_small(dev, tmp_path, small):
    from stofnet_amd import synth
    es, summary = run_main(tmp_path, ['model_file=graceful-wave', 'data_dir=./datasets/stof_chirp101_dataset',
                                      'batch_size=4', 'num_waveforms=10', 'num_samples=2000', 'seed=5'])
    assert summary['model'] == 'zonzini' and summary['waveforms'] == 8
    x = torch.from_numpy(synth.synth_echo(10, 2000, seed=5)[:8]).to(dev)
    assert np.array_equal(es, small(x).cpu().numpy())


def test_main_zonzini_pala_selects_large(dev, tmp_path):
    from stofnet_amd import ZonziniNetLarge, synth
    es, summary = run_main(tmp_path, ['data_dir=./PALA_data_InSilicoFlow', 'batch_size=2', 'num_waveforms=4',
                                      'num_samples=4000', 'seed=6'])
    assert summary['model'] == 'zonzini' and es.shape == (4, 1)
    torch.manual_seed(6)                                                      # main.py seeds before it builds the model
    m = ZonziniNetLarge().to(dev).eval()
    x = torch.from_numpy(synth.synth_echo(4, 4000, seed=6)).to(dev)
    assert np.array_equal(es, m(x).cpu().numpy())

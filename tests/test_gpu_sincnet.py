"""SincNet on the gfx950 kernels against the reference's fp32 outputs (tests/golden/f19_sincnet.npz,
make_golden_sincnet.py) and the float64 restatement of test_sincnet_cpu.py: outputs within 1e-5 x max|y| of both, the
per-layer outputs of the chirp case; the error contract (dtypes, devices, training); bitwise batch and chunk invariance
and determinism; NaN isolation; re-packing after a weight change; `main.py model=sincnet`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden
import sincnet_inputs as si
from test_sincnet_cpu import CASE_IDS, case, forward64, weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f19_sincnet')


def make(sd, fs, dev, L=2000):
    from stofnet_amd import SincNet
    m = SincNet(si.options(fs, L))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def brook(dev):
    return make(si.checkpoint_weights('pretty-brook'), 1e6, dev)


@pytest.mark.parametrize('name', CASE_IDS)
def test_matches_reference(dev, g, name):
    _, wkey, fs, shape, seed, step = case(name)
    sd = weights(wkey)
    m = make(sd, fs, dev, shape[-1])
    x = si.frames(shape, seed)
    with torch.no_grad():
        yall = m(torch.from_numpy(x).to(dev)).cpu().numpy()               # the whole batch runs
    assert yall.shape == (shape[0], 1, shape[-1])
    y, ry = yall[::step], g[f'{name}_y']                                   # the fixture keeps every step-th row
    y64, _ = forward64(sd, fs, x[::step])
    assert y.shape == ry.shape
    e = np.abs(y - ry).max() / np.abs(ry).max()
    e64 = np.abs(y - y64).max() / np.abs(y64).max()
    print(f'{name}: {e:.2e} vs ref fp32, {e64:.2e} vs f64 (ref fp32 vs f64 {np.abs(ry - y64).max() / np.abs(y64).max():.2e})')
    assert max(e, e64) <= 1e-5
    assert torch.equal(m(torch.from_numpy(x).to(dev)).cpu(), torch.from_numpy(yall))   # eval mode, grad enabled


def test_layer_outputs(dev, g, brook):
    _, _, _, shape, seed, _ = case(si.LAYER_CASE)
    x = torch.from_numpy(si.frames(shape, seed)[:2]).to(dev)
    with torch.no_grad():
        acts = brook.forward_layers(x)
        y = brook(x)
    e = si.LAYER_EDGE
    for i in range(3):
        assert acts[i].shape == (2, 128, shape[-1])
        got = torch.cat([acts[i][0, :, :e], acts[i][0, :, -e:]], -1).cpu().numpy()
        ref = g['layers'][i]
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f'layer {i}: {err:.2e}')
        assert err <= 1e-5
    assert torch.equal(brook(x), y)                                   # the diagnostic runs leave the forward unchanged


def test_batch_invariance_chunking_and_determinism(dev, g, brook):
    x = torch.from_numpy(si.frames((64, 1, 2000), 3101)).to(dev)
    full = brook(x)
    for r in (0, 1, 33, 63):
        assert torch.equal(brook(x[r:r + 1]), full[r:r + 1])
    assert torch.equal(brook(x[10:17]), full[10:17])
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0)).to(dev)
    assert torch.equal(brook(x[perm]), full[perm])
    brook.max_workspace_bytes = 5 * 2 * 512 * 2008                      # 4 rows per chunk
    try:
        assert torch.equal(brook(x), full)
    finally:
        del brook.max_workspace_bytes
    assert torch.equal(brook(x), full)
    assert torch.equal(brook(x[:, 0, :]), full)                         # [N, L] input
    big = torch.cat([x, x[:32]])                                        # 96 rows: past NARROW_M, 4 N tiles per wave
    assert torch.equal(brook(big), torch.cat([full, full[:32]]))


def test_nan_isolation(dev, brook):
    x = torch.from_numpy(si.frames((8, 1, 2000), 5)).to(dev)
    ref = brook(x)
    x[3, 0, 777] = float('nan')
    y = brook(x)
    assert torch.isnan(y[3]).any()
    assert not torch.isnan(y[3, 0, :777 - 511 - 5 - 4 - 3]).any()     # outside the receptive field of sample 777
    keep = torch.arange(8, device=dev) != 3
    assert torch.equal(y[keep], ref[keep])


def test_dtype_device_and_training_errors(dev, brook):
    x = torch.zeros(2, 1, 2000, device=dev)
    with pytest.raises(TypeError):
        brook(x.double())
    with pytest.raises(TypeError):
        brook(x.half())
    with pytest.raises(RuntimeError, match='ROCm device'):
        brook(x.cpu())
    with pytest.raises(RuntimeError):
        brook(torch.zeros(2, 2, 100, device=dev))
    m = make(si.checkpoint_weights('pretty-brook'), 1e6, dev).double()
    with pytest.raises(TypeError):
        m(x)
    brook.train()
    try:
        with torch.no_grad():
            with pytest.raises(NotImplementedError, match='training'):
                brook(x)
    finally:
        brook.eval()
    with pytest.raises(NotImplementedError):
        brook(x.clone().requires_grad_(True))
    y = brook(x)
    assert not y.requires_grad and y.grad_fn is None
    assert brook(torch.zeros(0, 1, 50, device=dev)).shape == (0, 1, 50)


def test_repacks_after_weight_change(dev):
    x = torch.from_numpy(si.frames((8, 1, 2000), 11)).to(dev)
    sd_a, sd_b = si.checkpoint_weights('pretty-brook'), si.checkpoint_weights('noble-monkey')
    m = make(sd_a, 1e6, dev)
    ya = m(x)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_b.items()}, strict=True)
    yb = m(x)
    assert torch.equal(yb, make(sd_b, 1e6, dev)(x))
    assert not torch.equal(ya, yb)
    with torch.no_grad():
        m.bn[3].bias.add_(1.0)                                           # in-place edit of a BatchNorm parameter
    assert torch.allclose(m(x), yb + 1.0, rtol=0, atol=1e-4)
    with torch.no_grad():
        m.conv[0].low_hz_.mul_(1.5)                                      # the filter bank is re-synthesised
    yc = m(x)
    assert torch.equal(yc, make({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, 1e6, dev)(x))


def test_main_sincnet(dev, tmp_path, brook):
    from stofnet_amd import mask2coords, synth
    ck = tmp_path / 'ckpts'
    ck.mkdir()
    torch.save({k: torch.from_numpy(v) for k, v in si.checkpoint_weights('pretty-brook').items()}, ck / si.CHECKPOINTS['pretty-brook'])
    out = tmp_path / 'es.npy'
    code = ('import sys, json, numpy as np; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[3:]); np.save(sys.argv[2], es); print(json.dumps(s))')
    args = ['model=sincnet', 'model_file=pretty-brook', 'fs=1e5', 'rf_scale_factor=10', f'ckpt_dir={ck}', 'batch_size=4',
            'num_waveforms=10', 'num_samples=2000', 'seed=5', 'th=Null']
    res = subprocess.run([sys.executable, '-c', code, ROOT, str(out)] + args, capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    es, summary = np.load(out), json.loads(res.stdout.strip().splitlines()[-1])
    assert summary['model'] == 'sincnet' and summary['waveforms'] == 8
    x = torch.from_numpy(synth.synth_echo(10, 2000, seed=5)[:8]).to(dev)
    with torch.no_grad():
        ref = mask2coords(brook(x), window_size=20, threshold=None, upsample_factor=1).cpu().numpy()
    assert np.array_equal(es, ref.reshape(8, -1))

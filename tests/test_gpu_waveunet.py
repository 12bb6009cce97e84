"""WaveUnet on the gfx950 kernels of csrc/waveunet.hip against the reference's fp32 outputs (tests/golden/f23_waveunet.npz,
make_golden_waveunet.py) and the float64 restatement of test_waveunet_cpu.py: output, logits and the middle block's
output within 1e-5 x max|ref| of both; routing of `forward`; bitwise batch and chunk invariance and determinism; NaN
isolation; re-packing after a change of the weights or of the running statistics; the error contract;
`main.py model=unet`.

The bound is the one test_gpu_riders.py and test_gpu_zonzini.py use: the reference's own fp32 result is within 1.6e-6 x
max of float64, and an fp32 forward with BatchNorm folded in double within 1.7e-6 x max of the reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden
import waveunet_inputs as wi
from test_waveunet_cpu import case64, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'waveunet.jsonl')
_errors = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f23_waveunet')


def make(sd, n, dev):
    from stofnet_amd import WaveUnet
    m = WaveUnet(n, 16)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def net2(dev):
    return make(wi.seeded_waveunet(2, 802), 2, dev)


@pytest.fixture(scope='module')
def x8(dev):
    return torch.from_numpy(wi.frames(8, 2000, 5)).to(dev)


def record(name, errs):
    """print the achieved errors and keep them in profiles/waveunet.jsonl (one `parity` line, rewritten as cases come in)"""
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    _errors[name] = {k: float(f'{v:.3e}') for k, v in errs.items()}
    lines = []
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'parity']
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines + [json.dumps({'kind': 'parity', 'bound': 1e-5, 'rel_err': _errors})]) + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('name', wi.IDS)
def test_matches_reference(dev, g, name):
    _, n, _, N, L, _ = wi.case(name)
    sd, x, (y64, l64, b64) = case64(g, name)
    m = make(sd, n, dev)
    xd = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        y, bott, logits = m.forward_with_taps(xd)                        # the whole batch runs
        assert y.shape == logits.shape == (N, 1, L) and bott.shape == (N, 16 * n, L >> n)
        assert torch.equal(m(xd), y) and torch.equal(m.forward_kernels(xd), y)     # routing
    rows = wi.kept_rows(N, L)
    y, bott, logits = y.cpu().numpy(), bott.cpu().numpy(), logits.cpu().numpy()
    errs = {'y_ref': rel(y[rows], g[f'{name}_y']), 'y_f64': rel(y, y64),
            'logits_ref': rel(logits[rows], g[f'{name}_logits']), 'logits_f64': rel(logits, l64),
            'bott_ref': rel(wi.bott_edges(bott[rows]), g[f'{name}_bott']), 'bott_f64': rel(bott, b64)}
    record(name, errs)
    assert max(errs.values()) <= 1e-5


def test_routing(dev, x8):
    m = make(wi.seeded_waveunet(2, 802), 2, dev)
    x = x8[:2]
    with torch.no_grad():
        yk = m.forward_kernels(x)
        assert torch.equal(m(x), yk)                                     # eval + no_grad: kernels
    y = m(x)                                                             # eval mode, grad enabled: the ATen route
    assert y.grad_fn is not None and torch.equal(y, m.forward_aten(x))
    assert (y - yk).abs().max() <= 1e-4 * yk.abs().max()                 # two fp32 implementations of one network
    assert m(x.clone().requires_grad_(True)).grad_fn is not None
    m.requires_grad_(False)
    yp = m(x)
    assert yp.grad_fn is None and not yp.requires_grad and torch.equal(yp, yk)
    m.train()
    mean0 = m.middle[1].running_mean.clone()
    with torch.no_grad():
        yt = m(x)                                                        # train mode: batch statistics on ATen
    assert not torch.allclose(yt, yk, atol=1e-3) and not torch.equal(m.middle[1].running_mean, mean0)
    m.eval()
    with torch.no_grad():
        assert not torch.equal(m(x), yk)                                 # the running statistics moved: re-packed
        with pytest.raises(RuntimeError):
            m(torch.zeros(2, 1, 6, device=dev))                          # the reference's torch.cat failure, via forward


def test_kernels_supported_and_errors(dev, net2, x8):
    m = net2
    assert m.kernels_supported(x8)
    assert not m.kernels_supported(x8.double()) and not m.kernels_supported(x8.cpu()) and not m.kernels_supported(x8[:, 0])
    assert not m.kernels_supported(x8.expand(8, 2, 2000)) and not m.kernels_supported(x8[:, :, :1998])
    cpu_net = make(wi.seeded_waveunet(2, 802), 2, torch.device('cpu'))
    assert not cpu_net.kernels_supported(x8)
    with pytest.raises(TypeError):
        m.forward_kernels(x8.double())
    with pytest.raises(TypeError):
        m.forward_kernels(x8.half())
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.forward_kernels(x8.cpu())
    with pytest.raises(RuntimeError):
        m.forward_kernels(torch.zeros(2, 2, 100, device=dev))
    with pytest.raises(RuntimeError, match='forward_aten'):
        m.forward_kernels(x8[:, :, :1998])
    with pytest.raises(TypeError):
        make(wi.seeded_waveunet(2, 802), 2, dev).double().forward_kernels(x8)
    with pytest.raises(RuntimeError, match='ROCm device'):
        cpu_net.forward_kernels(x8)
    y = m.forward_kernels(x8.clone().requires_grad_(True))               # explicit call: no graph, whatever the grad mode
    assert y.grad_fn is None and not y.requires_grad


def test_batch_invariance_chunking_and_determinism(dev, net2, x8):
    m = net2
    with torch.no_grad():
        full = m(x8)
        assert torch.equal(m(x8), full)                                  # determinism
        for r in (0, 1, 7):
            assert torch.equal(m(x8[r:r + 1]), full[r:r + 1])
        assert torch.equal(m(x8[2:5]), full[2:5])
        perm = torch.randperm(8, generator=torch.Generator().manual_seed(0)).to(dev)
        assert torch.equal(m(x8[perm]), full[perm])
        taps = m.forward_with_taps(x8)
        per_row = 4 * (2000 * 16 + 1000 * 32 + 500 * 32 + 2 * 2000 * 16)    # floats of one row's workspace
        m.max_workspace_bytes = 3 * per_row + 4096                       # 3 rows per chunk
        try:
            assert torch.equal(m(x8), full)
            chunked = m.forward_with_taps(x8)
        finally:
            del m.max_workspace_bytes
        assert all(torch.equal(a, b) for a, b in zip(taps, chunked)) and torch.equal(taps[0], full)
        side = torch.cuda.Stream(dev)                                    # launches go on the current stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ys = m(x8)
        side.synchronize()
        assert torch.equal(ys, full)
        assert m(torch.zeros(0, 1, 2000, device=dev)).shape == (0, 1, 2000)


def test_nan_isolation(dev, net2, x8):
    x = x8.clone()
    with torch.no_grad():
        ref = net2(x)
        x[3, 0, 777] = float('nan')
        y = net2(x)
    assert torch.isnan(y[3, 0, 777])
    keep = torch.arange(8, device=dev) != 3
    assert torch.equal(y[keep], ref[keep])


def test_repacks_after_weight_change(dev, x8):
    sd_a, sd_b = wi.seeded_waveunet(2, 802), wi.seeded_waveunet(2, 803)
    fresh = lambda net: make({k: v.cpu().numpy() for k, v in net.state_dict().items()}, 2, dev)
    with torch.no_grad():
        m = make(sd_a, 2, dev)
        ya = m(x8)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_b.items()}, strict=True)
        yb = m(x8)
        assert torch.equal(yb, make(sd_b, 2, dev)(x8)) and not torch.equal(ya, yb)
        m.decoder[1].main[1].running_var.mul_(2)                         # a buffer, not a parameter
        yc = m(x8)
        assert not torch.equal(yc, yb) and torch.equal(yc, fresh(m)(x8))
        lc = m.forward_with_taps(x8)[2]
        m.out[0].bias.add_(0.25)
        yd, _, ld = m.forward_with_taps(x8)
        assert torch.allclose(ld, lc + 0.25, rtol=0, atol=1e-5) and torch.equal(yd, fresh(m)(x8))
        m.invalidate_packed()
        assert m._packed is None and torch.equal(m(x8), yd)


def test_main_entry_point(dev, tmp_path):
    from stofnet_amd import mask2coords, synth
    sd = wi.seeded_waveunet(10, 810)
    ck = tmp_path / 'ckpts'
    ck.mkdir()
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ck / 'seeded-unet-1_rf-scale10_epoch_1.pth')
    out = tmp_path / 'es.npy'
    code = ('import sys, json, numpy as np; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[3:]); np.save(sys.argv[2], es); print(json.dumps(s))')
    args = ['model=unet', 'model_file=seeded-unet-1', 'data_dir=./datasets/pala', 'rf_scale_factor=10', 'upsample_factor=4',
            f'ckpt_dir={ck}', 'batch_size=4', 'num_waveforms=10', 'num_samples=2048', 'seed=5', 'evaluate=True', 'th=Null']
    res = subprocess.run([sys.executable, '-c', code, ROOT, str(out)] + args, capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    es, summary = np.load(out), json.loads(res.stdout.strip().splitlines()[-1])
    assert summary['model'] == 'unet' and summary['waveforms'] == 8
    m = make(sd, 10, dev)
    x = torch.from_numpy(synth.synth_echo(10, 2048, seed=5)[:8]).to(dev)
    with torch.no_grad():
        ref = mask2coords(m.forward_kernels(x), window_size=20, threshold=None, upsample_factor=1).cpu().numpy()
    assert np.array_equal(es, ref.reshape(8, -1))

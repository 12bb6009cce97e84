"""Kuleshov on the gfx950 kernels of csrc/kuleshov.hip against the reference's fp32 taps (tests/golden/f24_kuleshov.npz,
make_golden_kuleshov.py) and the float64 restatement of kuleshov_inputs.forward64: output, bottleneck, the input of
final_conv around its edges and its seam, and final_conv's output, each within max(1e-5, 8 e_ref) x max|ref| of both
(the bound is derived in test_kuleshov_cpu.py); routing of `forward`; bitwise batch, chunk and wave-tile invariance and
determinism; NaN isolation; re-packing after a change of a weight or of a running statistic; the error contract; the
crop; `main.py model=kuleshov`."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden
import kuleshov_inputs as ki
from test_kuleshov_cpu import bound, case64, make, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'kuleshov.jsonl')
_errors = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f24_kuleshov')


@pytest.fixture(scope='module')
def net(dev):
    return make(ki.seeded_kuleshov(641, 64), 641, 64, dev)


@pytest.fixture(scope='module')
def x5(dev):
    return torch.from_numpy(ki.frames(5, 641, 11)).to(dev)


def record(name, errs, bounds):
    """print the achieved errors and keep them in profiles/kuleshov.jsonl (one `parity` line, rewritten as cases come in)"""
    print(name, ' '.join(f'{k} {v:.2e} (<= {bounds[k]:.2e})' for k, v in errs.items()))
    _errors[name] = {k: float(f'{v:.3e}') for k, v in errs.items()}
    lines = []
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'parity']
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines + [json.dumps({'kind': 'parity', 'bound': 'max(1e-5, 8 e_ref)', 'rel_err': _errors})]) + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('name', ki.IDS)
def test_matches_reference(dev, g, name):
    from stofnet_amd.kuleshov import chain_lengths
    _, N, L, O, X, _ = ki.case(name)
    sd, x, t64 = case64(g, name)
    m = make(sd, L, O, dev)
    xd = torch.from_numpy(x).to(dev)
    d = chain_lengths(L)
    with torch.no_grad():
        y, bott, fin_in, fin = m.forward_with_taps(xd)                   # the whole batch runs
        assert y.shape == (N, 1, O) and bott.shape == (N, 512, d['bottleneck'])
        assert fin_in.shape == (N, 128, d['cat'][-1]) and fin.shape == (N, 2, d['final'])
        assert torch.equal(m(xd), y) and torch.equal(m.forward_kernels(xd), y)     # routing
    rows = ki.kept_rows(N, L)
    got = {'y': y.cpu().numpy()[rows], 'bott': bott.cpu().numpy()[rows],
           'fin_in': ki.final_in_window(fin_in.cpu().numpy()[rows], L), 'fin': fin.cpu().numpy()[rows]}
    errs, bounds = {}, {}
    for tap in ki.TAPS:
        assert got[tap].shape == g[f'{name}_{tap}'].shape == t64[tap].shape, tap
        errs[tap + '_ref'], errs[tap + '_f64'] = rel(got[tap], g[f'{name}_{tap}']), rel(got[tap], t64[tap])
        bounds[tap + '_ref'] = bounds[tap + '_f64'] = bound(name, tap)
    record(name, errs, bounds)
    for k, v in errs.items():
        assert v <= bounds[k], k


def test_routing(dev, x5):
    m = make(ki.seeded_kuleshov(641, 64), 641, 64, dev)
    x = x5[:2]
    with torch.no_grad():
        yk = m.forward_kernels(x)
        assert torch.equal(m(x), yk)                                     # eval + no_grad: kernels
    y = m(x)                                                             # eval mode, grad enabled: the ATen route
    assert y.grad_fn is not None                                         # (MIOpen's results are not bitwise repeatable)
    assert (y - yk).abs().max() <= 1e-4 * yk.abs().max()                 # two fp32 implementations of one network
    assert m(x.clone().requires_grad_(True)).grad_fn is not None
    m.requires_grad_(False)
    yp = m(x)
    assert yp.grad_fn is None and not yp.requires_grad and torch.equal(yp, yk)
    m.up_bn1.eps = 1e-3                                                  # two different eps: no kernels
    with torch.no_grad():
        assert not m.kernels_supported(x) and not torch.equal(m(x), yk)
    m.up_bn1.eps = 1e-5
    m.train()
    mean0 = m.up_bn2.running_mean.clone()
    with torch.no_grad():
        yt = m(x)                                                        # train mode: batch statistics on ATen
    assert not torch.allclose(yt, yk, atol=1e-3) and not torch.equal(m.up_bn2.running_mean, mean0)
    m.eval()
    with torch.no_grad():
        assert not torch.equal(m(x), yk)                                 # the running statistics moved: re-packed


def test_kernels_supported_and_errors(dev, net, x5):
    m = net
    assert m.kernels_supported(x5)
    assert not m.kernels_supported(x5.double()) and not m.kernels_supported(x5.cpu()) and not m.kernels_supported(x5[:, 0])
    assert not m.kernels_supported(x5.expand(5, 2, 641)) and not m.kernels_supported(x5[:, :, :640])
    cpu_net = make(ki.seeded_kuleshov(641, 64), 641, 64)
    assert not cpu_net.kernels_supported(x5)
    with pytest.raises(TypeError):
        m.forward_kernels(x5.double())
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.forward_kernels(x5.cpu())
    with pytest.raises(RuntimeError, match='forward_aten'):
        m.forward_kernels(x5[:, :, :640])                                # a short row
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            m(x5[:, :, :640])                                            # ... fails on the ATen route too, as in the reference
    with pytest.raises(RuntimeError, match='ROCm device'):
        cpu_net.forward_kernels(x5)
    y = m.forward_kernels(x5.clone().requires_grad_(True))               # explicit call: no graph, whatever the grad mode
    assert y.grad_fn is None and not y.requires_grad
    empty = torch.zeros(0, 1, 641, device=dev)
    with torch.no_grad():
        assert m(empty).shape == m.forward_kernels(empty).shape == (0, 1, 64)


def test_crop_by_stride(dev, net, x5):
    long = torch.cat([x5, torch.full((5, 1, 59), float('nan'), device=dev)], -1)     # what lies behind must not be read
    with torch.no_grad():
        full = net(x5)
        assert torch.equal(net(long), full)
        assert torch.equal(net(long[1:2]), full[1:2]) and torch.equal(net(long[::2]), full[::2])
        assert torch.allclose(net.forward_aten(long), full, rtol=0, atol=1e-4 * float(full.abs().max()))


def test_batch_chunk_and_tile_invariance(dev, net, x5):
    from stofnet_amd import _lib
    m = net
    x40 = torch.from_numpy(ki.frames(40, 641, 12)).to(dev)               # more than 32 rows: the Linear layer's 4-tile path
    x40[:5] = x5
    with torch.no_grad():
        full = m(x5)
        assert torch.equal(m(x5), full)                                  # determinism
        for r in (0, 1, 4):
            assert torch.equal(m(x5[r:r + 1]), full[r:r + 1])
        assert torch.equal(m(x5[2:5]), full[2:5])
        perm = torch.randperm(5, generator=torch.Generator().manual_seed(0)).to(dev)
        assert torch.equal(m(x5[perm]), full[perm])
        taps = m.forward_with_taps(x40)
        assert torch.equal(taps[0][:5], full) and torch.equal(m(x40), taps[0])
        desc = m._desc()
        per_row = int(_lib.lib().stof_kuleshov_workspace_bytes(ctypes.byref(desc), 1))
        m.max_workspace_bytes = 3 * per_row + 4096                       # 3 rows per chunk
        try:
            chunked = m.forward_with_taps(x40)
        finally:
            del m.max_workspace_bytes
        assert all(torch.equal(a, b) for a, b in zip(taps, chunked))
        for variant in (1, 2, 3):                                        # every wave tile runs the same k order
            m.tile_variant = variant
            try:
                tiled = m.forward_with_taps(x40)
            finally:
                del m.tile_variant
            assert all(torch.equal(a, b) for a, b in zip(taps, tiled)), variant
        side = torch.cuda.Stream(dev)                                    # launches go on the current stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ys = m(x5)
        side.synchronize()
        assert torch.equal(ys, full)


def test_nan_isolation(dev, net, x5):
    x = x5.clone()
    with torch.no_grad():
        ref = net(x)
        x[3, 0, 333] = float('nan')
        y = net(x)
    assert torch.isnan(y[3]).all()                                       # the Linear layer spreads it over the row
    keep = torch.arange(5, device=dev) != 3
    assert torch.equal(y[keep], ref[keep])


def test_repacks_after_weight_change(dev, x5):
    fresh = lambda net: make({k: v.cpu().numpy() for k, v in net.state_dict().items()}, 641, 64, dev)   # noqa: E731
    with torch.no_grad():
        m = make(ki.seeded_kuleshov(641, 64), 641, 64, dev)
        ya = m(x5)
        m.up_conv2.weight.mul_(1.5)                                      # a weight, in place
        yb = m(x5)
        assert not torch.equal(ya, yb) and torch.equal(yb, fresh(m)(x5))
        m.down_bn1.running_var.mul_(2)                                   # a buffer, not a parameter
        yc = m(x5)
        assert not torch.equal(yc, yb) and torch.equal(yc, fresh(m)(x5))
        m.output_fc.bias.add_(0.25)
        yd = m(x5)
        assert torch.allclose(yd, yc + 0.25, rtol=0, atol=1e-5) and torch.equal(yd, fresh(m)(x5))
        m.invalidate_packed()
        assert m._packed is None and torch.equal(m(x5), yd)


def test_main_entry_point(dev, tmp_path):
    from stofnet_amd import Kuleshov, mask2coords, synth
    out = tmp_path / 'es.npy'
    code = ('import sys, json, numpy as np; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[3:]); np.save(sys.argv[2], es); print(json.dumps(s))')
    args = ['model=kuleshov', 'upsample_factor=2', 'batch_size=2', 'num_waveforms=5', 'num_samples=700', 'seed=5',
            'evaluate=False', 'th=Null']
    res = subprocess.run([sys.executable, '-c', code, ROOT, str(out)] + args, capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    es, summary = np.load(out), json.loads(res.stdout.strip().splitlines()[-1])
    assert summary['model'] == 'kuleshov' and summary['waveforms'] == 4 and 'train_history' not in summary
    torch.manual_seed(5)                                                 # main.py seeds, then builds the model
    m = Kuleshov(input_length=700, output_length=1400).to(dev).eval()
    x = torch.from_numpy(synth.synth_echo(5, 700, seed=5)[:4]).to(dev)
    with torch.no_grad():
        ref = mask2coords(m.forward_kernels(x), window_size=20, threshold=None, upsample_factor=2).cpu().numpy()
    assert np.array_equal(es, ref.reshape(4, -1))

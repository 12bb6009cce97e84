"""EDSR_1D / ESPCN_1D on the gfx950 kernels of csrc/riders.hip against the reference's fp32 outputs
(tests/golden/f21_riders.npz, make_golden_riders.py) and the float64 restatement of test_riders_cpu.py: outputs and the
hooked intermediates (EDSR: the input of `upscale`; ESPCN: the logits) within 1e-5 x max|ref| of both; routing of
`forward`; bitwise batch and chunk invariance and determinism; NaN isolation; re-packing after a weight change; the
autograd routing; the error contract; `main.py model=edsr|espcn`.

The bound is the one test_gpu_zonzini.py and test_shuffle_riders_match_reference use; the reference's own fp32 result
is within 2.4e-6 x max of float64 (logits 5.1e-7), an fp32 chain of K = 192 products sits at about sqrt(192) x 2^-24 =
8e-7 per layer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden, load_weights
import riders_inputs as ri
from test_riders_cpu import EDSR_IDS, ESPCN_IDS, edsr64, edsr_case, espcn64, espcn_case, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'riders.jsonl')
_errors = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f21_riders')


def make_edsr(sd, b, r, dev):
    from stofnet_amd import EDSR_1D
    m = EDSR_1D(1, 64, b, r)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def make_espcn(sd, r, dev):
    from stofnet_amd import ESPCN_1D
    m = ESPCN_1D(r)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def cherry(dev):
    return make_edsr(load_weights('proud-cherry'), 8, 4, dev)


@pytest.fixture(scope='module')
def puddle(dev):
    return make_espcn(load_weights('vital-puddle'), 4, dev)


@pytest.fixture(scope='module')
def x8(dev):
    return torch.from_numpy(ri.frames(8, 2000, 5)).to(dev)


def record(name, errs):
    """print the achieved errors and keep them in profiles/riders.jsonl (one `parity` line, rewritten as cases come in)"""
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


@pytest.mark.parametrize('name', EDSR_IDS)
def test_edsr_matches_reference(dev, g, name):
    _, wkey, b, r, n, L, _ = edsr_case(name)
    sd = ri.weights(wkey, load_weights, b, r)
    m = make_edsr(sd, b, r, dev)
    x = ri.frames(n, L, int(g[f'{name}_seed']))
    xd = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        y, trunk = m.forward_with_trunk(xd)                               # the whole batch runs
        assert y.shape == (n, 1, L * r) and trunk.shape == (n, 64, L)
        assert torch.equal(m(xd), y) and torch.equal(m.forward_kernels(xd), y)     # routing
    rows = ri.kept_rows(n, L, r)
    y, trunk = y.cpu().numpy(), trunk.cpu().numpy()
    y64, t64 = edsr64(sd, b, r, x)
    te = ri.trunk_edges(trunk[rows[-1]])
    errs = {'y_ref': rel(y[rows], g[f'{name}_y']), 'y_f64': rel(y, y64), 'trunk_ref': rel(te, g[f'{name}_trunk']),
            'trunk_f64': rel(trunk, t64)}
    record(name, errs)
    assert max(errs.values()) <= 1e-5


@pytest.mark.parametrize('name', ESPCN_IDS)
def test_espcn_matches_reference(dev, g, name):
    _, wkey, r, n, L, _ = espcn_case(name)
    sd = ri.weights(wkey, load_weights, r)
    m = make_espcn(sd, r, dev)
    x = ri.frames(n, L, int(g[f'{name}_seed']))
    xd = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        y, logits = m.forward_with_logits(xd)
        assert y.shape == logits.shape == (n, 1, L * r)
        assert torch.equal(m(xd), y) and torch.equal(m.forward_kernels(xd), y)     # routing
    rows = ri.kept_rows(n, L, r)
    y, logits = y.cpu().numpy(), logits.cpu().numpy()
    y64, l64 = espcn64(sd, r, x)
    errs = {'y_ref': rel(y[rows], g[f'{name}_y']), 'y_f64': rel(y, y64), 'logits_ref': rel(logits[rows], g[f'{name}_logits']),
            'logits_f64': rel(logits, l64)}
    record(name, errs)
    assert max(errs.values()) <= 1e-5


def test_kernels_supported(dev, cherry, puddle, x8):
    from stofnet_amd import EDSR_1D, ESPCN_1D
    assert cherry.kernels_supported(x8) and puddle.kernels_supported(x8)
    for m in (cherry, puddle):
        assert not m.kernels_supported(x8.double()) and not m.kernels_supported(x8.cpu()) and not m.kernels_supported(x8[:, 0])
        assert not m.kernels_supported(x8.expand(8, 2, 2000))
    assert not EDSR_1D(1, 16, 2, 4).to(dev).kernels_supported(x8)
    assert not EDSR_1D(2, 64, 1, 4).to(dev).kernels_supported(x8)
    assert not EDSR_1D(1, 64, 1, 4).to(dev).double().kernels_supported(x8)
    assert not EDSR_1D(1, 64, 1, 4).kernels_supported(x8)               # parameters on the CPU
    assert not ESPCN_1D(65).to(dev).kernels_supported(x8)
    with torch.no_grad():                                                # unsupported widths stay on the ATen route
        m = EDSR_1D(1, 16, 2, 4).to(dev)
        assert torch.equal(m(x8), m.forward_aten(x8))
        with pytest.raises(RuntimeError, match='forward_aten'):
            m.forward_kernels(x8)


@pytest.mark.parametrize('which', ['edsr', 'espcn'])
def test_batch_invariance_chunking_and_determinism(dev, cherry, puddle, x8, which):
    m = cherry if which == 'edsr' else puddle
    with torch.no_grad():
        full = m(x8)
        assert torch.equal(m(x8), full)                                  # determinism
        for r in (0, 1, 7):
            assert torch.equal(m(x8[r:r + 1]), full[r:r + 1])
        assert torch.equal(m(x8[2:5]), full[2:5])
        perm = torch.randperm(8, generator=torch.Generator().manual_seed(0)).to(dev)
        assert torch.equal(m(x8[perm]), full[perm])
        if which == 'edsr':
            m.max_workspace_bytes = 3 * 3 * 256 * 2001 + 1024               # 3 rows per chunk
            try:
                assert torch.equal(m(x8), full)
                y, trunk = m.forward_with_trunk(x8)
            finally:
                del m.max_workspace_bytes
            y2, trunk2 = m.forward_with_trunk(x8)
            assert torch.equal(y, full) and torch.equal(y2, full) and torch.equal(trunk, trunk2)
            big = torch.cat([x8] * 5)                                    # 80000 outputs: past NARROW_M, two N tiles per wave
            assert torch.equal(m(big), torch.cat([full] * 5))
        side = torch.cuda.Stream(dev)                                    # launches go on the current stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ys = m(x8)
        side.synchronize()
        assert torch.equal(ys, full)
        assert m(torch.zeros(0, 1, 50, device=dev)).shape == (0, 1, 200)


@pytest.mark.parametrize('which', ['edsr', 'espcn'])
def test_nan_isolation(dev, cherry, puddle, x8, which):
    m = cherry if which == 'edsr' else puddle
    x = x8.clone()
    with torch.no_grad():
        ref = m(x)
        x[3, 0, 777] = float('nan')
        y = m(x)
    assert torch.isnan(y[3, 0, 777 * 4:777 * 4 + 4]).all()
    assert not torch.isnan(y[3, 0, :(777 - 20) * 4]).any()                # outside the receptive field (19 / 4 samples)
    keep = torch.arange(8, device=dev) != 3
    assert torch.equal(y[keep], ref[keep])


def test_repacks_after_weight_change(dev, x8):
    with torch.no_grad():
        for make, keys, shape in ((make_edsr, ri.EDSR_CKPTS, (8, 4)), (make_espcn, ri.ESPCN_CKPTS, (4,))):
            sd_a, sd_b = load_weights(keys[0]), load_weights(keys[1])
            m = make(sd_a, *shape, dev)
            ya = m(x8)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_b.items()}, strict=True)
            yb = m(x8)
            assert torch.equal(yb, make(sd_b, *shape, dev)(x8)) and not torch.equal(ya, yb)
            last = list(m.parameters())[-1]                              # conv_output.bias | conv3.bias
            last.add_(0.5)                                               # in-place edit
            yc = m(x8)
            if make is make_edsr:
                assert torch.allclose(yc, yb + 0.5, rtol=0, atol=1e-5)
            else:
                lb = make(sd_b, *shape, dev).forward_with_logits(x8)[1]
                assert torch.allclose(m.forward_with_logits(x8)[1], lb + 0.5, rtol=0, atol=1e-4)
            assert torch.equal(yc, make({k: v.cpu().numpy() for k, v in m.state_dict().items()}, *shape, dev)(x8))
            m.invalidate_packed()
            assert m._packed is None and torch.equal(m(x8), yc)


@pytest.mark.parametrize('which', ['edsr', 'espcn'])
def test_autograd_routing(dev, x8, which):
    m = (make_edsr(load_weights('proud-cherry'), 8, 4, dev) if which == 'edsr'
         else make_espcn(load_weights('vital-puddle'), 4, dev))
    x = x8[:2]
    y = m(x)                                                             # eval mode, grad enabled: the ATen route
    assert y.grad_fn is not None
    assert torch.equal(y, m.forward_aten(x))
    with torch.no_grad():
        yk = m.forward_kernels(x)
        assert torch.equal(m(x), yk)
    assert (y - yk).abs().max() <= 1e-4 * yk.abs().max()                 # two fp32 implementations of one network
    m.requires_grad_(False)
    yp = m(x)
    assert yp.grad_fn is None and not yp.requires_grad and torch.equal(yp, yk)
    assert m(x.clone().requires_grad_(True)).grad_fn is not None         # an input that asks for a gradient: ATen
    m.train()
    assert torch.equal(m(x), yk)                                         # no BatchNorm / dropout: the mode does not matter


def test_dtype_and_device_errors(dev, cherry, puddle, x8):
    for m, make, key, shape in ((cherry, make_edsr, 'proud-cherry', (8, 4)), (puddle, make_espcn, 'vital-puddle', (4,))):
        with pytest.raises(TypeError):
            m.forward_kernels(x8.double())
        with pytest.raises(TypeError):
            m.forward_kernels(x8.half())
        with pytest.raises(RuntimeError, match='ROCm device'):
            m.forward_kernels(x8.cpu())
        with pytest.raises(RuntimeError):
            m.forward_kernels(torch.zeros(2, 2, 100, device=dev))
        with pytest.raises(TypeError):
            make(load_weights(key), *shape, dev).double().forward_kernels(x8)
        with pytest.raises(RuntimeError, match='ROCm device'):
            make(load_weights(key), *shape, torch.device('cpu')).forward_kernels(x8)
        y = m.forward_kernels(x8.clone().requires_grad_(True))           # explicit call: no graph, whatever the grad mode
        assert y.grad_fn is None and not y.requires_grad


@pytest.mark.parametrize('which,key', [('edsr', 'proud-cherry'), ('espcn', 'vital-puddle')])
def test_main_entry_point(dev, tmp_path, cherry, puddle, which, key):
    from stofnet_amd import mask2coords, synth
    ck = tmp_path / 'ckpts'
    ck.mkdir()
    torch.save({k: torch.from_numpy(v) for k, v in load_weights(key).items()}, ck / ri.CHECKPOINTS[key])
    out = tmp_path / 'es.npy'
    code = ('import sys, json, numpy as np; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[3:]); np.save(sys.argv[2], es); print(json.dumps(s))')
    args = [f'model={which}', f'model_file={key}', 'rf_scale_factor=10', 'upsample_factor=4', f'ckpt_dir={ck}', 'batch_size=4',
            'num_waveforms=10', 'num_samples=2000', 'seed=5', 'evaluate=True', 'th=Null']
    res = subprocess.run([sys.executable, '-c', code, ROOT, str(out)] + args, capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    es, summary = np.load(out), json.loads(res.stdout.strip().splitlines()[-1])
    assert summary['model'] == which and summary['waveforms'] == 8
    m = cherry if which == 'edsr' else puddle
    x = torch.from_numpy(synth.synth_echo(10, 2000, seed=5)[:8]).to(dev)
    with torch.no_grad():
        ref = mask2coords(m.forward_kernels(x), window_size=20, threshold=None, upsample_factor=4).cpu().numpy()
    assert np.array_equal(es, ref.reshape(8, -1))

"""Training ESPCN_1D on the gfx950 kernels (csrc/espcn_train.hip, stofnet_amd/espcn_training.py):

  * every new kernel alone against float64 torch at the bound of test_gpu_edsr_training.py (2e-6 x max|ref|), outputs and
    workspaces pre-filled with NaN patterns, out_scale = 0.25, each weight gradient twice (bitwise); the backward kernels and
    their float64 side start from the same saved fp32 activations, so tanh / sigmoid rounding of the forward does not enter;
  * the autograd boundary (`train_route = 'kernels'`) on every case of tests/golden/f27_espcn_training.npz against the
    reference's fp32 autograd: rel(y) < 2e-5, dx and all six parameter gradients within 2e-4 x max|ref|;
  * the same step on `train_route = 'aten'` within the same bounds of the kernel route;
  * routing, the error contract, freed activations, parameter edits, streams, determinism;
  * `main.py model=espcn evaluate=False` end to end, on both routes.

rel(a, b) = max|a - b| / max|b|.  The measured maxima go to profiles/espcn_training.jsonl (the `parity` line)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, load_weights
import espcn_training_inputs as pi
import riders_inputs as ri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'espcn_training.jsonl')
KERNEL_BOUND, Y_BOUND, GRAD_BOUND = 2e-6, 2e-5, 2e-4
SHAPES = [(3, 171, 4), (2, 1, 17), (1, 2, 33), (2, 3, 2), (2, 5, 1), (2, 40, 64), (2, 31, 10), (1, 130, 3)]
_errors = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib(dev):
    from stofnet_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def g():
    return golden('f27_espcn_training')


def rel(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def record(name, errs):
    """print the achieved errors and keep them in profiles/espcn_training.jsonl (one `parity` line, rewritten as cases come in)"""
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    _errors[name] = {k: float(f'{v:.3e}') for k, v in errs.items()}
    lines = []
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'parity']
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines + [json.dumps({'kind': 'parity', 'bounds': {'y': Y_BOUND, 'grad': GRAD_BOUND},
                                                    'rel_err': _errors})]) + '\n')
    except OSError:
        pass


def make_espcn(sd, r, dev, route='kernels'):
    from stofnet_amd import ESPCN_1D
    m = ESPCN_1D(r)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).train()
    m.train_route = route
    return m


def step(m, x, t, route='kernels', want_dx=True):
    """One forward + backward of loss = sum(y * t) -> (y, dx or None, {name: gradient})."""
    m.train_route = route
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(want_dx)
    y = m(xd)
    (y * t).sum().backward()
    return y.detach(), xd.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------- the kernels alone
def _nan(*shape, dev):
    return torch.full(shape, float('nan'), device=dev)


def _cl(t):
    """[N, C, L] float64 -> channel-last [N, L, C]"""
    return t.detach().permute(0, 2, 1)


@pytest.mark.parametrize('N,L', sorted({(n, L) for n, L, _ in SHAPES}))
def test_espcn_in_kernels_vs_torch(lib, dev, N, L):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    gen = torch.Generator().manual_seed(2000 * N + L)
    x = 0.5 * torch.randn(N, 1, L, generator=gen)
    w = 0.6 * torch.randn(64, 1, 5, generator=gen)
    b = 0.3 * torch.randn(64, generator=gen)
    g1 = torch.randn(N, L, 64, generator=gen)
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    pre = F.conv1d(x64, w64, b64, padding=2)
    xd, wd, bd, g1d = (t.to(dev).contiguous() for t in (x, w, b, g1))
    h1 = _nan(N, L, 64, dev=dev)
    _lib.check(lib.stof_train_espcn_in(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(h1), N, L, st), 'espcn_in')
    errs = {'h1': rel(h1, _cl(torch.tanh(pre)))}
    # backward: both sides start from the saved fp32 activation
    saved = h1.detach().cpu()
    pre.backward((g1.double() * (1.0 - saved.double() ** 2)).permute(0, 2, 1))
    ws = torch.empty(lib.stof_train_espcn_in_wgrad_workspace_bytes(), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        dw, db = _nan(64, 1, 5, dev=dev), _nan(64, dev=dev)
        ws.fill_(0xff)                                                  # NaN patterns: a partial that is read must have been written
        _lib.check(lib.stof_train_espcn_in_wgrad(_lib.ptr(xd), _lib.ptr(g1d), _lib.ptr(h1), _lib.ptr(dw), _lib.ptr(db), N, L, 0.25,
                                                 _lib.ptr(ws), ws.numel(), st), 'espcn_in_wgrad')
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # no float atomics
    errs['dw'], errs['db'] = rel(runs[0][0], 0.25 * w64.grad), rel(runs[0][1], 0.25 * b64.grad)
    dx = _nan(N, L, dev=dev)
    _lib.check(lib.stof_train_espcn_in_dgrad(_lib.ptr(g1d), _lib.ptr(h1), _lib.ptr(wd), _lib.ptr(dx), N, L, 0.25, st), 'espcn_in_dgrad')
    errs['dx'] = rel(dx, 0.25 * x64.grad[:, 0])
    print('espcn_in', (N, L), ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert max(errs.values()) < KERNEL_BOUND, errs


@pytest.mark.parametrize('N,L', sorted({(n, L) for n, L, _ in SHAPES}))
def test_espcn_mid_kernel_vs_torch(lib, dev, N, L):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    gen = torch.Generator().manual_seed(3000 * N + L)
    h1 = torch.tanh(torch.randn(N, L, 64, generator=gen))
    w = torch.randn(32, 64, 3, generator=gen) * (2.0 / 192) ** 0.5
    b = 0.3 * torch.randn(32, generator=gen)
    ref = torch.tanh(F.conv1d(h1.double().permute(0, 2, 1), w.double(), b.double(), padding=1))
    hd, wd, bd = (t.to(dev).contiguous() for t in (h1, w, b))
    frag = _nan(lib.stof_train_espcn_repack_floats(), dev=dev)
    _lib.check(lib.stof_train_espcn_repack(_lib.ptr(wd), _lib.ptr(frag), st), 'espcn_repack')
    assert sorted(frag.cpu().tolist()) == sorted(w.reshape(-1).tolist())             # a permutation of the weights
    h2 = _nan(N, L, 32, dev=dev)
    _lib.check(lib.stof_train_espcn_mid(_lib.ptr(hd), _lib.ptr(frag), _lib.ptr(bd), _lib.ptr(h2), N, L, st), 'espcn_mid')
    err = rel(h2, _cl(ref))
    print('espcn_mid', (N, L), f'h2 {err:.2e}')
    assert err < KERNEL_BOUND


@pytest.mark.parametrize('N,L,r', SHAPES)
def test_espcn_out_kernels_vs_torch(lib, dev, N, L, r):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    gen = torch.Generator().manual_seed(1000 * N + L + 7 * r)
    h2 = torch.tanh(torch.randn(N, L, 32, generator=gen))
    w = torch.randn(r, 32, 3, generator=gen) * (2.0 / 96) ** 0.5
    b = 0.3 * torch.randn(r, generator=gen)
    dy = torch.randn(N, L * r, generator=gen)
    h64, w64, b64 = h2.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    z = F.conv1d(h64.permute(0, 2, 1), w64, b64, padding=1)                  # [N, r, L]: y[n, l r + j] = sigmoid(z[n, j, l])
    hd, wd, bd, dyd = (t.to(dev).contiguous() for t in (h2, w, b, dy))
    y = _nan(N, L * r, dev=dev)
    _lib.check(lib.stof_train_espcn_out(_lib.ptr(hd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), N, L, r, st), 'espcn_out')
    errs = {'y': rel(y, _cl(torch.sigmoid(z)).reshape(N, L * r))}
    # backward: dz from the saved fp32 output on both sides; conv3^T(dz) without tanh' first, then times (1 - h2^2)
    ys = y.detach().cpu().double()
    dz = (dy.double() * ys * (1.0 - ys)).reshape(N, L, r)
    z.backward(dz.permute(0, 2, 1))
    g2_ref = h64.grad * (1.0 - h2.double() ** 2)
    g2 = _nan(N, L, 32, dev=dev)
    _lib.check(lib.stof_train_espcn_out_dgrad(_lib.ptr(y), _lib.ptr(dyd), _lib.ptr(hd), _lib.ptr(wd), _lib.ptr(g2), N, L, r, st),
               'espcn_out_dgrad')
    errs['g2'] = rel(g2, g2_ref)
    nbytes = lib.stof_train_espcn_out_wgrad_workspace_bytes(r)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        dw, db = _nan(r, 32, 3, dev=dev), _nan(r, dev=dev)
        ws.fill_(0xff)
        _lib.check(lib.stof_train_espcn_out_wgrad(_lib.ptr(hd), _lib.ptr(y), _lib.ptr(dyd), _lib.ptr(dw), _lib.ptr(db), N, L, r, 0.25,
                                                  _lib.ptr(ws), ws.numel(), st), 'espcn_out_wgrad')
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # no float atomics
    errs['dw'], errs['db'] = rel(runs[0][0], 0.25 * w64.grad), rel(runs[0][1], 0.25 * b64.grad)
    print('espcn_out', (N, L, r), ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert max(errs.values()) < KERNEL_BOUND, errs


def test_empty_batches_zero_the_gradients(lib, dev):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    for N, L in ((0, 8), (3, 0)):
        dw, db = torch.ones(64, 1, 5, device=dev), torch.ones(64, device=dev)
        assert lib.stof_train_espcn_in_wgrad(None, None, None, _lib.ptr(dw), _lib.ptr(db), N, L, 1.0, None, 0, st) == 0
        assert not dw.any() and not db.any()
        dw, db = torch.ones(10, 32, 3, device=dev), torch.ones(10, device=dev)
        assert lib.stof_train_espcn_out_wgrad(None, None, None, _lib.ptr(dw), _lib.ptr(db), N, L, 10, 1.0, None, 0, st) == 0
        assert not dw.any() and not db.any()


# --------------------------------------------------------------------------------------------- the autograd boundary
@pytest.fixture(scope='module')
def stepped(dev, g):
    """name -> (module, x, t, result of one kernel-route step), computed once per case and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            _, wkey, r, n, L, _ = pi.case(name)
            seed = int(g[f'{name}.seed'])
            m = make_espcn(ri.weights(wkey, load_weights, r), r, dev)
            x = torch.from_numpy(ri.frames(n, L, seed)).to(dev)
            t = torch.from_numpy(pi.cotangent(n, L * r, seed)).to(dev)
            cache[name] = (m, x, t, step(m, x, t, 'kernels'))
        return cache[name]
    return get


@pytest.mark.parametrize('name', pi.IDS)
def test_kernel_route_matches_reference_autograd(g, stepped, name):
    _, _, r, n, L, _ = pi.case(name)
    m, x, t, (y, dx, grads) = stepped(name)
    assert y.shape == (n, 1, L * r) and dx.shape == (n, 1, L)
    errs = {'y': rel(y, g[f'{name}.y']), 'dx': rel(dx, g[f'{name}.dx'])}
    for k in pi.PARAMS:
        errs[k] = rel(grads[k], g[f'{name}.grad.{k}'])
    record(name, {'y': errs['y'], 'dx': errs['dx'], 'grad_max': max(errs[k] for k in pi.PARAMS)})
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert errs.pop('y') < Y_BOUND
    assert max(errs.values()) < GRAD_BOUND, errs


@pytest.mark.parametrize('name', pi.IDS)
def test_aten_route_agrees_with_kernel_route(stepped, name):
    m, x, t, (y, dx, grads) = stepped(name)
    ya, dxa, ga = step(m, x, t, 'aten')
    m.train_route = 'kernels'
    errs = {'y': rel(ya, y), 'dx': rel(dxa, dx), **{k: rel(ga[k], grads[k]) for k in grads}}
    print(name, 'aten vs kernels', f"y {errs['y']:.2e} dx {errs['dx']:.2e} grad {max(errs[k] for k in grads):.2e}")
    assert errs.pop('y') < Y_BOUND
    assert max(errs.values()) < GRAD_BOUND, errs


# ------------------------------------------------------------------------------------------------------------ routing
@pytest.fixture(scope='module')
def puddle_sd():
    return load_weights('vital-puddle')


@pytest.fixture(scope='module')
def x2(dev):
    return torch.from_numpy(ri.frames(2, 300, 5)).to(dev)


def test_default_route_is_unchanged(dev, puddle_sd, x2):
    m = make_espcn(puddle_sd, 4, dev, route='aten')
    assert type(m).train_route == 'aten'
    y = m(x2)                                                            # a graph is recorded: ATen, as before
    assert y.grad_fn is not None and torch.equal(y, m.forward_aten(x2))
    del m.train_route                                                    # the class default
    assert torch.equal(m(x2), y)
    with torch.no_grad():
        yk = m.forward_kernels(x2)
        assert torch.equal(m(x2), yk)
        m.train_route = 'kernels'                                        # no graph: the inference kernel on either setting
        assert torch.equal(m(x2), yk)
    m.train_route = 'nope'
    with pytest.raises(ValueError, match='train_route'):
        m(x2)


def test_kernel_route_routing(dev, puddle_sd, x2):
    from stofnet_amd import ESPCN_1D
    from stofnet_amd import _lib
    from stofnet_amd.espcn_training import EspcnTrainEngine
    m = make_espcn(puddle_sd, 4, dev)
    y = m(x2)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith('EspcnFunction')
    assert y.shape == (2, 1, 1200) and torch.equal(y, m.forward_train_kernels(x2))
    with torch.no_grad():
        assert rel(y, m.forward_kernels(x2)) < Y_BOUND                   # the inference kernel computes the same network
    # no dx for a frame that does not ask for one: neither the argument nor the launch
    calls, launches = [], []
    orig = EspcnTrainEngine._backward_saved
    clib = _lib.lib()                                                    # the one loaded library object
    real = clib.stof_train_espcn_in_dgrad

    def spy(self, saved, dy, grads, dx=None):
        calls.append(dx is not None)
        return orig(self, saved, dy, grads, dx)

    def counted(*args):
        launches.append(1)
        return real(*args)
    EspcnTrainEngine._backward_saved = spy
    clib.stof_train_espcn_in_dgrad = counted
    try:
        t = torch.ones_like(y)
        _, dx, _ = step(m, x2, t, want_dx=False)
        assert dx is None and launches == []
        _, dx, _ = step(m, x2, t, want_dx=True)
        assert dx is not None and dx.shape == x2.shape and launches == [1]
    finally:
        EspcnTrainEngine._backward_saved = orig
        clib.stof_train_espcn_in_dgrad = real
    assert calls == [False, True]
    # frozen parameters, a frame that asks: still the kernels; nothing asks: the inference kernel, no graph
    m.requires_grad_(False)
    for p in m.parameters():
        p.grad = None
    xg = x2.clone().requires_grad_()
    yg = m(xg)
    assert type(yg.grad_fn).__name__.startswith('EspcnFunction')
    (yg * t).sum().backward()
    assert rel(xg.grad, dx) < 1e-6 and all(p.grad is None for p in m.parameters())
    assert m(x2).grad_fn is None
    m.requires_grad_(True)
    # unsupported models and inputs: `forward` falls back to ATen, the explicit call raises
    big = ESPCN_1D(128).to(dev)
    big.train_route = 'kernels'
    yb = big(x2)
    assert yb.grad_fn is not None and torch.equal(yb, big.forward_aten(x2))
    with pytest.raises(RuntimeError, match='forward_aten'):
        big.forward_train_kernels(x2)
    md = make_espcn(puddle_sd, 4, dev).double()
    assert torch.equal(md(x2.double()), md.forward_aten(x2.double()))
    with pytest.raises(TypeError):
        md.forward_train_kernels(x2.double())
    with pytest.raises(TypeError):
        m.forward_train_kernels(x2.double())
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.forward_train_kernels(x2.cpu())
    mc = make_espcn(puddle_sd, 4, torch.device('cpu'))
    with pytest.raises(RuntimeError, match='ROCm device'):
        mc.forward_train_kernels(x2)
    mc.forward_aten = lambda x: 'aten'                                   # CPU tensors: `forward` hands them to the ATen route
    assert mc(x2.cpu()) == 'aten'
    with pytest.raises(RuntimeError):
        m.forward_train_kernels(torch.zeros(2, 2, 100, device=dev))     # two channels
    # an empty batch
    for shape in ((0, 1, 50), (3, 1, 0)):
        for p in m.parameters():
            p.grad = None
        ye = m(torch.zeros(shape, device=dev))
        assert ye.shape == (shape[0], 1, 4 * shape[2])
        ye.sum().backward()
        assert all(p.grad is not None and not p.grad.any() for p in m.parameters())


def test_parameter_edit_between_forward_and_backward_raises(dev, puddle_sd, x2):
    """The backward reads the weights again (data gradients): as with torch's own convolutions, an in-place edit in between
    is an error, not a silently different gradient."""
    m = make_espcn(puddle_sd, 4, dev)
    for name in ('conv3.weight', 'conv2.weight', 'conv1.bias'):
        loss = m(x2).sum()
        with torch.no_grad():
            dict(m.named_parameters())[name].mul_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            loss.backward()
    m(x2).sum().backward()                                                # the next step is fine


def test_second_backward_raises(dev, puddle_sd, x2):
    m = make_espcn(puddle_sd, 4, dev)
    y = m(x2)
    loss = y.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()


def test_parameter_edit_stream_and_determinism(dev, puddle_sd, x2):
    m = make_espcn(puddle_sd, 4, dev)
    t = torch.randn((2, 1, 1200), generator=torch.Generator().manual_seed(3)).to(dev)
    y1, dx1, g1 = step(m, x2, t)
    y2, dx2, g2 = step(m, x2, t)                                          # two full runs: bitwise equal
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    side = torch.cuda.Stream(dev)                                         # launches follow the current stream
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        y3, dx3, g3 = step(m, x2, t)
    side.synchronize()
    assert torch.equal(y1, y3) and torch.equal(dx1, dx3) and all(torch.equal(g1[k], g3[k]) for k in g1)
    with torch.no_grad():                                                 # in-place edits: the two cached conv2 images and raw weights
        m.conv2.weight.mul_(1.5)
        m.conv1.weight.add_(0.01)
        m.conv3.bias.add_(0.5)
    y4, dx4, g4 = step(m, x2, t)
    fresh = make_espcn({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, 4, dev)
    y5, dx5, g5 = step(fresh, x2, t)
    assert not torch.equal(y4, y1)
    assert torch.equal(y4, y5) and torch.equal(dx4, dx5) and all(torch.equal(g4[k], g5[k]) for k in g4)


# ------------------------------------------------------------------------------------------------------------ main.py
def test_main_entry_point_trains_espcn(dev, tmp_path):
    from stofnet_amd import ESPCN_1D
    code = ('import sys, json; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[2:]); print(json.dumps(s))')
    base = ['model=espcn', 'evaluate=False', 'epochs=2', 'batch_size=4', 'num_waveforms=24', 'num_samples=256', 'upsample_factor=4',
            'seed=5', 'th=Null', 'logging=unit']
    first = {}
    for route, extra in (('kernels', []), ('aten', ['train_route=aten'])):
        ck = tmp_path / f'ckpts_{route}'
        run = f'espcntest{os.getpid()}{route}'
        log = os.path.join(ROOT, f'{run}_unit.jsonl')                    # RunLog without wandb: JSON lines next to main.py
        try:
            res = subprocess.run([sys.executable, '-c', code, ROOT] + base + extra + [f'ckpt_dir={ck}', f'run_name={run}'],
                                 capture_output=True, text=True, timeout=600, cwd=ROOT)
            assert res.returncode == 0, res.stdout + res.stderr
            recs = [json.loads(ln) for ln in open(log)]
        finally:
            if os.path.exists(log):
                os.remove(log)
        summary = json.loads(res.stdout.strip().splitlines()[-1])
        hist = summary['train_history']
        assert summary['model'] == 'espcn' and summary['train_route'] == route and summary['train_precision'] == 'fp32'
        assert len(hist) == 2 and all(np.isfinite(h['train_loss']) and np.isfinite(h['val_loss']) for h in hist)
        first[route] = next(r['train_loss'] for r in recs if 'train_loss' in r)
        assert np.isfinite(first[route])
        paths = sorted(ck.iterdir())
        assert [p.name for p in paths] == [f'{run}_rf-scale10_epoch_2.pth']
        sd = torch.load(str(paths[0]), map_location='cpu', weights_only=True)
        ESPCN_1D(4).load_state_dict(sd, strict=True)
        torch.manual_seed(5)
        init = ESPCN_1D(4).state_dict()                                   # main.py seeds torch, then builds the model
        moved = max(float((sd[k] - init[k]).abs().max()) for k in sd)
        assert 0.0 < moved < 0.05, moved                                  # ten AdamW steps at lr <= 5e-4 away from that initialisation
    # the first logged loss is one forward pass on identical parameters
    assert abs(first['kernels'] - first['aten']) <= 1e-5 * abs(first['aten']), first

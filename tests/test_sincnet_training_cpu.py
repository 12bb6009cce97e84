"""SincNet training, the parts that need no GPU:

  * `SincNet.forward_aten` (the reference's forward restated in torch on the module's own parameters) on the CPU in train mode
    against tests/golden/f29_sincnet_training.npz: y, the running statistics and num_batches_tracked on every case, dx and all 16
    parameter gradients on the cases with N L >= 128; in fp32 under the tolerance rule, in float64 to 1e-10 of
    `sincnet_training_inputs.restate64` (which the generator asserts to be the reference's float64 module);
  * `stof_sincnet_band_grad`, the host entry over the chain rule the device kernel runs, against float64 torch autograd of the
    restated synthesis (2e-6 x max), with clamped bands (d band_hz_ exactly 0) and a negative low_hz_;
  * the route contract of `SincNet.train_route`;
  * the inputs module reproduces the stored seeds.

Tolerance rule: |ours - ref64| <= max(B max|ref64|, 8 dev_T), dev_T the reference's own fp32-vs-float64 deviation of tensor T
(stored); B = 2e-5 for y and the running statistics, 2e-4 for dx and the gradients.  For the conv bias gradients
(analytically 0 under train-mode BatchNorm) dev_T is the largest of eight of the reference's own noise samples, see
sincnet_training_inputs.ZERO_GRADS.  ref64 is float64 autograd of the restated
network with the decisions (BatchNorm output > 0) of the run under test."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
import sincnet_inputs as si
import sincnet_training_inputs as ti

Y_BOUND, GRAD_BOUND, BAND_BOUND = 2e-5, 2e-4, 2e-6


@pytest.fixture(scope='module')
def g():
    return golden('f29_sincnet_training')


def make_net(sd, fs, L, route='aten', dev='cpu', dtype=torch.float32):
    from stofnet_amd import SincNet
    m = SincNet(si.options(fs, L))
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    m = m.to(device=dev)
    if dtype != torch.float32:
        m = m.to(dtype)
    m.train()
    m.train_route = route
    return m


def check_rule(name, key, ours, ref64, g, B, errs=None):
    """assert the tolerance rule for the stored tensor `key` of case `name`; `ours` / `ref64` as the fixture stores it"""
    ours, ref64 = np.asarray(ours, np.float64), np.asarray(ref64, np.float64)
    err, lim = float(np.abs(ours - ref64).max()), ti.bound(B, ref64, g[f'{name}.dev.{key}'])
    if errs is not None:
        errs[key] = err / max(float(np.abs(ref64).max()), 1e-300)
    print(f'{name} {key}: max err {err:.3e} bound {lim:.3e}')
    assert np.isfinite(ours).all() and err <= lim, (name, key, err, lim)


def check_step(name, g, y, dx, grads, run_mean, run_var, decisions, errs=None):
    """The whole comparison of one step of case `name` (numpy arrays; decisions per LeakyReLU layer [N, 128, L]) with float64
    autograd taken with those decisions.  -> the float64 runs (own decisions, the given ones)."""
    _, wkey, fs, n, L, seed = ti.case(name)
    sd, x, t = ti.weights(wkey, fs), ti.frames(n, L, seed), ti.cotangent(n, L, seed)
    own = ti.restate64(sd, fs, x, t)
    routed = own if all(np.array_equal(a, b) for a, b in zip(decisions, own['decisions'])) else ti.restate64(sd, fs, x, t, decisions)
    # a decision that differs from float64's lies within the stored margin; no more of them than float64 alone counts there
    for l in range(3):
        differ = decisions[l] != own['decisions'][l]
        assert (np.abs(own['bn_out'][l][differ]) < ti.MARGIN * g[f'{name}.bn_dev'][l]).all(), (name, l)
        assert int(differ.sum()) <= int(g[f'{name}.near'][l]), (name, l, int(differ.sum()))
    check_rule(name, 'y', y, routed['y'], g, Y_BOUND, errs)
    for i in range(4):
        check_rule(name, f'run_mean.{i}', run_mean[i], routed['run_mean'][i], g, Y_BOUND, errs)
        check_rule(name, f'run_var.{i}', run_var[i], routed['run_var'][i], g, Y_BOUND, errs)
    assert np.isfinite(dx).all() and all(np.isfinite(v).all() for v in grads.values())
    if name in ti.GRAD_IDS:
        check_rule(name, 'dx', dx, routed['dx'], g, GRAD_BOUND, errs)
        for p in ti.PARAMS:
            check_rule(name, f'grad.{p}', np.asarray(grads[p]).reshape(ti.SHAPES[p]), routed['grads'][p], g, GRAD_BOUND, errs)
    return own, routed


def check_against_reference_fp32(name, g, dx, grads):
    """where the decisions are float64's: the same rule against the reference's own fp32 results (the fixture)"""
    check_rule(name, 'dx', dx, g[f'{name}.dx'], g, GRAD_BOUND)
    for p in ti.PARAMS:
        check_rule(name, f'grad.{p}', ti.view_like_stored(p, grads[p]), ti.stored_grad(g, name, p), g, GRAD_BOUND)


def aten_step(m, x, t):
    outs = {}
    hooks = [m.bn[i].register_forward_hook(lambda mod, a, o, i=i: outs.__setitem__(i, (o.detach() > 0).cpu().numpy())) for i in range(3)]
    x = x.clone().requires_grad_(True)
    y = m(x)
    (y * t).sum().backward()
    for h in hooks:
        h.remove()
    return (y.detach().cpu().numpy(), x.grad.cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()},
            [b.running_mean.detach().cpu().numpy() for b in m.bn], [b.running_var.detach().cpu().numpy() for b in m.bn],
            [outs[i] for i in range(3)])


def test_inputs_module_reproduces_the_stored_seeds(g):
    for name, _, _, n, L, seed in ti.CASES:
        assert int(g[f'{name}.seed']) == seed
        assert g[f'{name}.y'].shape == (n, 1, L) and g[f'{name}.dx'].shape == (n, 1, L)
    assert ti.frames(2, 1, 7001).shape == (2, 1, 1) and ti.cotangent(3, 7, 1).shape == (3, 1, 7)


@pytest.mark.parametrize('name', ti.IDS)
def test_forward_aten_fp32_on_the_cpu_against_the_fixture(g, name):
    _, wkey, fs, n, L, seed = ti.case(name)
    m = make_net(ti.weights(wkey, fs), fs, L)
    y, dx, grads, rm, rv, dec = aten_step(m, torch.from_numpy(ti.frames(n, L, seed)), torch.from_numpy(ti.cotangent(n, L, seed)))
    assert y.shape == (n, 1, L) and y.dtype == np.float32
    assert int(m.bn[0].num_batches_tracked) == int(g[f'{name}.nbt']) and int(m.bn[3].num_batches_tracked) == int(g[f'{name}.nbt'])
    own, _ = check_step(name, g, y, dx, grads, rm, rv, dec)
    check_rule(name, 'y', y, g[f'{name}.y'], g, Y_BOUND)                       # ... and the reference's fp32 y itself
    if name in ti.GRAD_IDS and all(np.array_equal(a, b) for a, b in zip(dec, own['decisions'])):
        check_against_reference_fp32(name, g, dx, grads)


@pytest.mark.parametrize('name', ti.IDS)
def test_forward_aten_float64_is_the_restated_network(name):
    _, wkey, fs, n, L, seed = ti.case(name)
    sd, x, t = ti.weights(wkey, fs), ti.frames(n, L, seed), ti.cotangent(n, L, seed)
    m = make_net(sd, fs, L, dtype=torch.float64)
    y, dx, grads, rm, rv, dec = aten_step(m, torch.from_numpy(x).double(), torch.from_numpy(t).double())
    assert y.dtype == np.float64
    ref = ti.restate64(sd, fs, x, t)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))   # noqa: E731
    assert rel(y, ref['y']) <= 1e-10
    for i in range(4):
        assert np.abs(rm[i] - ref['run_mean'][i]).max() <= 1e-10 * max(1.0, np.abs(ref['run_mean'][i]).max())
        assert rel(rv[i], ref['run_var'][i]) <= 1e-10
    if name in ti.GRAD_IDS:
        assert rel(dx, ref['dx']) <= 1e-10
        for p in ti.PARAMS:
            if 'bias' in p and p.startswith('conv'):            # analytically 0 under train-mode BatchNorm: rounding noise on both sides
                assert np.abs(grads[p]).max() <= 1e-10 * max(float(np.abs(ref['grads'][f'bn.{p[5]}.bias']).max()), 1.0)
            else:
                assert rel(grads[p], ref['grads'][p]) <= 1e-10, p


BAND_SETS = [(w, fs) for w in ('pretty-brook', 'noble-monkey', 'init') for fs in (2e5, 1e6, 1.25e9)]


@pytest.mark.parametrize('wkey,fs', BAND_SETS)
def test_band_grad_host_entry_against_float64_autograd(wkey, fs):
    from stofnet_amd import _lib
    lib = _lib.lib()
    sd = ti.weights(wkey, fs)
    low, band = sd['conv.0.low_hz_'].astype(np.float32).copy(), sd['conv.0.band_hz_'].astype(np.float32).copy()
    low[5, 0] = -low[5, 0] - 1.0                                               # abs: the sign
    band[9, 0] = -band[9, 0] - 1.0
    G = np.random.default_rng(31 + int(fs) % 1000).standard_normal((128, 1023)).astype(np.float32)
    lp = torch.tensor(low, dtype=torch.float64, requires_grad=True)
    bp = torch.tensor(band, dtype=torch.float64, requires_grad=True)
    (ti.synth64(lp, bp, fs).view(128, 1023) * torch.from_numpy(G).double()).sum().backward()
    desc = _lib.SincNetDesc(float(fs), 1e-5, 0, 0)
    dlow, dband = np.full(128, np.nan), np.full(128, np.nan)
    low_c, band_c = np.ascontiguousarray(low.reshape(-1)), np.ascontiguousarray(band.reshape(-1))
    _lib.check(lib.stof_sincnet_band_grad(ctypes.byref(desc), low_c.ctypes.data, band_c.ctypes.data, G.ctypes.data, dlow.ctypes.data,
                                          dband.ctypes.data), 'stof_sincnet_band_grad')
    rl, rb = lp.grad.numpy().reshape(-1), bp.grad.numpy().reshape(-1)
    print(wkey, fs, 'max err / max', np.abs(dlow - rl).max() / np.abs(rl).max(), np.abs(dband - rb).max() / np.abs(rb).max())
    assert np.abs(dlow - rl).max() <= BAND_BOUND * np.abs(rl).max() and np.abs(dband - rb).max() <= BAND_BOUND * np.abs(rb).max()
    clamped = (50.0 + np.abs(low_c.astype(np.float64)) + 50.0 + np.abs(band_c.astype(np.float64))) > fs / 2
    if fs == 2e5 and wkey != 'init':
        assert clamped.any()                                                   # learned bands above this Nyquist
    assert not dband[clamped].any() and not rb[clamped].any()                  # exactly 0 through the clamp
    assert np.sign(dlow[5]) == np.sign(rl[5]) and rl[5] != 0


def test_route_contract():
    from stofnet_amd import SincNet
    m = SincNet(si.options(1e6, 8))
    assert SincNet.train_route is None and m.train_route is None
    x = torch.zeros(2, 1, 8)
    m.train()
    with pytest.raises(NotImplementedError, match='training is not implemented on the gfx950 path'):
        m(x)
    m.train_route = 'kernel'
    with pytest.raises(ValueError, match='train_route'):
        m(x)
    m.eval()
    with pytest.raises(ValueError, match='train_route'):
        m(x)
    for route in ('kernels', 'aten'):
        opts = si.options(1e6, 8)
        opts['cnn_drop'] = [0.0, 0.1, 0.0, 0.0]
        d = SincNet(opts).train()
        d.train_route = route
        with pytest.raises(NotImplementedError, match='cnn_drop'):
            d(x)
        m.train_route = route
        m.train()
        with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
            m(torch.zeros(1, 1, 1))
    m = SincNet(si.options(1e6, 8)).train()       # (torch's BatchNorm counts a batch before it raises: a fresh module)
    m.train_route = 'aten'
    y = m(torch.randn(2, 1, 8))
    assert y.shape == (2, 1, 8) and y.grad_fn is not None and int(m.bn[0].num_batches_tracked) == 1
    m.eval()
    assert m(torch.randn(2, 8, requires_grad=True)).shape == (2, 1, 8)         # an eval-mode graph: forward_aten under 'aten'

"""Training SincNet on the gfx950 kernels (csrc/sincnet_train.hip, stofnet_amd/sincnet_training.py):

  * every new kernel alone against float64 torch on the same Gaussian fp32 operands within 2e-6 x max|ref|, each twice
    (bitwise), at the tiny shapes and one below / on / one above every tile and chunk constant;
  * the statistics kernel on a channel with mean / std = 1e3 (1e-6 relative of float64 numpy);
  * the device-synthesised bank against the host packer's (one fp32 ulp of max|bank|);
  * the autograd boundary (`train_route = 'kernels'`) on every case of tests/golden/f29_sincnet_training.npz under the
    tolerance rule of test_sincnet_training_cpu.py, float64 autograd taken with the route's own decisions (a_l > 0 of the
    engine's saved tensors); where those equal float64's, also against the reference's own fp32 gradients;
  * the same kernels where a chunk outgrows its minimum (a work-group walks more rows, the bank gradient several tiles);
  * the device-packed inference blob against the host packer's: the same bytes, bitwise the same eval-mode output;
  * determinism, the 'aten' route, eval mode after AdamW steps (the stale-blob trap), the graph and error behaviour;
  * `main.py model=sincnet evaluate=False train_route=kernels` end to end in a child process, twice (bitwise).

The measured maxima go to profiles/sincnet_training.jsonl (the `parity` line)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
import sincnet_inputs as si
import sincnet_training_inputs as ti
from test_sincnet_training_cpu import (GRAD_BOUND, Y_BOUND, check_against_reference_fp32, check_rule, check_step, make_net)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'sincnet_training.jsonl')
KERNEL_BOUND = 2e-6
C, GAP = 128, 8
_errors, _runs, _direct = {}, {}, []


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f29_sincnet_training')


@pytest.fixture(scope='module')
def engine(dev):
    from stofnet_amd.sincnet_training import SincNetTrainEngine
    return SincNetTrainEngine(dev, 1e6)


def rel(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def record(name, errs):
    """print the achieved errors and keep them in profiles/sincnet_training.jsonl (one `parity` line, rewritten as cases come in)"""
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    _errors[name] = {k: float(f'{v:.3e}') for k, v in errs.items()}
    lines = []
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'parity']
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines + [json.dumps({'kind': 'parity', 'bounds': {'kernel': KERNEL_BOUND, 'y': Y_BOUND, 'grad': GRAD_BOUND},
                                                    'rel_err': _errors})]) + '\n')
    except OSError:
        pass


def step(m, x, t, route='kernels', want_dx=True, keep=None):
    """One forward + backward of loss = sum(y * t) -> (y, dx or None, {name: gradient}); keep: receives the route's saved state."""
    m.train_route = route
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(want_dx)
    y = m(xd)
    if keep is not None:
        keep['saved'] = y.grad_fn.saved
    (y * t).sum().backward()
    return y.detach(), xd.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------- the kernels alone
# the tiny shapes; 129 rows over three waveforms; one below / on / one above the 64-row (conv weight gradient), 128-sample (sinc
# tiles, bank gradient) and 256-row (layer 3 weight gradient, statistics) constants; a row longer than the filter
KERNEL_SHAPES = [(2, 1), (1, 2), (3, 7), (3, 43), (1, 63), (1, 64), (1, 65), (1, 127), (1, 128), (1, 129), (2, 129), (1, 255), (1, 256),
                 (1, 257), (2, 1025)]


def twice(fn):
    a, b = fn(), fn()
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    return a if len(a) > 1 else a[0]


@pytest.mark.parametrize('N,L', KERNEL_SHAPES)
def test_layer_kernels_vs_torch(dev, engine, N, L):
    e = engine
    gen = torch.Generator().manual_seed(4000 + 7 * N + L)
    rn = lambda *s: torch.randn(*s, generator=gen)                            # noqa: E731
    M = N * L
    errs = {}
    # --- statistics, apply, BatchNorm backward (128 channels and 1)
    for ch in (C, 1):
        z = rn(N, L, ch) * 2 + rn(ch)
        a_dec = rn(N, L, ch)                                                  # the saved activation: only its sign is read
        da = rn(N, L, ch)
        gamma, beta, rmean, rvar = rn(ch), rn(ch), rn(ch), rn(ch).abs() + 0.5
        z64 = z.double()
        mean, var = z64.mean((0, 1)), z64.var((0, 1), unbiased=False)
        xh = (z64 - mean) / torch.sqrt(var + 1e-5)
        v = xh * gamma.double() + beta.double()
        out64 = torch.where(v > 0, v, 0.2 * v) if ch == C else v
        g64 = da.double() * (torch.where(a_dec > 0, 1.0, 0.2).double() if ch == C else 1.0)
        dz64 = gamma.double() / torch.sqrt(var + 1e-5) * (g64 - g64.mean((0, 1)) - xh * (g64 * xh).mean((0, 1)))
        to_buf = (lambda t: e.from_rows(t.to(dev))) if ch == C else (lambda t: t.reshape(-1).to(dev).contiguous())
        of_buf = (lambda b: e.rows(b, N, L)) if ch == C else (lambda b: b.view(N, L, 1))
        zb, ab, dab = to_buf(z), to_buf(a_dec), to_buf(da)
        gd, bd, rmd, rvd = (t.to(dev) for t in (gamma, beta, rmean, rvar))
        stat, nm, nv = twice(lambda: e.stats(zb, N, L, ch, gd, bd, rmd, rvd))
        out = twice(lambda: e.apply(zb, N, L, ch, stat))
        dgam, dbet = torch.full((ch,), float('nan'), device=dev), torch.full((ch,), float('nan'), device=dev)
        dz = twice(lambda: e.bn_bwd(dab, ab if ch == C else None, zb, stat, gd, N, L, ch, dgam, dbet))
        k = f'c{ch}'
        errs[f'mean {k}'] = rel(stat[0], mean)
        errs[f'var {k}'] = rel(1.0 / stat[1].cpu() ** 2 - 1e-5, var)
        errs[f'apply {k}'] = rel(of_buf(out), out64)
        errs[f'run_mean {k}'] = rel(nm, 0.95 * rmean.double() + 0.05 * mean)
        errs[f'run_var {k}'] = rel(nv, 0.95 * rvar.double() + 0.05 * var * M / (M - 1))
        # (at N L = 2 xhat = +-1 for every element: dz is a difference of equal numbers, rounding noise, there alone over max|g|)
        errs[f'dz {k}'] = rel(of_buf(dz), dz64) if M > 2 else \
            float((of_buf(dz).cpu().double() - dz64).abs().max() / max(float(dz64.abs().max()), float(g64.abs().max())))
        errs[f'dgamma {k}'] = rel(dgam, (g64 * xh).sum((0, 1)))
        errs[f'dbeta {k}'] = rel(dbet, g64.sum((0, 1)))
        if ch == C:                                                          # gap rows are zeroed by the writers
            for b in (out, dz):
                full = b[:(N * (L + GAP) + GAP) * C].view(-1, C)
                gaps = torch.ones(full.shape[0], dtype=torch.bool)
                for n in range(N):
                    gaps[GAP + n * (L + GAP):GAP + n * (L + GAP) + L] = False
                assert not full[gaps.to(dev)].any()
    # --- layers 1, 2: the forward convolution, the weight gradient and the data gradient
    for l, K in ((1, 11), (2, 9)):
        a_prev, dzl = rn(N, L, C), rn(N, L, C)
        w, b = rn(C, C, K) * (2.0 / (K * C)) ** 0.5, rn(C)
        a64 = a_prev.double().permute(0, 2, 1).contiguous().requires_grad_()
        w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
        z64 = F.conv1d(a64, w64, b64, padding=K // 2)
        (z64 * dzl.double().permute(0, 2, 1)).sum().backward()
        ab, dzb, wd, bdv = e.from_rows(a_prev.to(dev)), e.from_rows(dzl.to(dev)), w.to(dev), b.to(dev)
        names = ['conv.0.low_hz_', 'conv.0.band_hz_', 'conv.1.weight', 'conv.2.weight', 'conv.3.weight']
        p = {'conv.0.low_hz_': torch.ones(C, 1, device=dev) * 1e4, 'conv.0.band_hz_': torch.ones(C, 1, device=dev) * 1e3,
             'conv.1.weight': wd if l == 1 else torch.zeros(C, C, 11, device=dev),
             'conv.2.weight': wd if l == 2 else torch.zeros(C, C, 9, device=dev), 'conv.3.weight': torch.zeros(1, C, 7, device=dev)}
        e._blob = None
        blob = e.packed({k: p[k] for k in names})
        zk = twice(lambda: e.conv(l, ab, N, L, blob, bdv))
        errs[f'conv{l}'] = rel(e.rows(zk, N, L).permute(0, 2, 1), z64)

        def wgrad():
            e._scratch('_sn_wgrad_ws', 16).fill_(0xff)                        # NaN patterns: every partial the reduce reads is written
            dw, db = torch.full((C, C, K), float('nan'), device=dev), torch.full((C,), float('nan'), device=dev)
            e.conv_wgrad(l, ab, dzb, N, L, dw, db)
            return dw, db
        dw, db = twice(wgrad)
        errs[f'dw{l}'], errs[f'db{l}'] = rel(dw, w64.grad), rel(db, b64.grad)
        img = e._dgrad_image(l, wd)
        da = twice(lambda: e.conv_dgrad(l, dzb, N, L, img))
        errs[f'da{l - 1}'] = rel(e.rows(da, N, L).permute(0, 2, 1), a64.grad)
    # --- layer 3 on the vector pipe
    a2, dz3 = rn(N, L, C), rn(N, L)
    w3, b3 = rn(1, C, 7) * (2.0 / (7 * C)) ** 0.5, rn(1)
    a64 = a2.double().permute(0, 2, 1).contiguous().requires_grad_()
    w64, b64 = w3.double().requires_grad_(), b3.double().requires_grad_()
    z64 = F.conv1d(a64, w64, b64, padding=3)
    (z64 * dz3.double().view(N, 1, L)).sum().backward()
    ab, dzb, w3d = e.from_rows(a2.to(dev)), dz3.reshape(-1).to(dev).contiguous(), w3.to(dev)
    e._blob = None
    blob = e.packed({'conv.0.low_hz_': torch.ones(C, 1, device=dev) * 1e4, 'conv.0.band_hz_': torch.ones(C, 1, device=dev) * 1e3,
                     'conv.1.weight': torch.zeros(C, C, 11, device=dev), 'conv.2.weight': torch.zeros(C, C, 9, device=dev),
                     'conv.3.weight': w3d})
    z3 = twice(lambda: e.conv(3, ab, N, L, blob, b3.to(dev)))
    errs['conv3'] = rel(z3.view(N, 1, L), z64)

    def out_wgrad():
        e._scratch('_sn_out_ws', 16).fill_(0xff)
        dw, db = torch.full((1, C, 7), float('nan'), device=dev), torch.full((1,), float('nan'), device=dev)
        e.out_wgrad(ab, dzb, N, L, dw, db)
        return dw, db
    dw, db = twice(out_wgrad)
    errs['dw3'], errs['db3'] = rel(dw, w64.grad), rel(db, b64.grad)
    da2 = twice(lambda: e.out_dgrad(dzb, w3d, N, L))
    errs['da2'] = rel(e.rows(da2, N, L).permute(0, 2, 1), a64.grad)
    # --- layer 0: the forward on the device-synthesised bank, the bank gradient, dx
    sd = ti.weights('pretty-brook', 1e6)
    low, band = torch.from_numpy(sd['conv.0.low_hz_'].copy()), torch.from_numpy(sd['conv.0.band_hz_'].copy())
    x, dz0 = rn(N, L), rn(N, L, C)
    bank64 = ti.synth64(low.double(), band.double(), 1e6).requires_grad_()
    x64 = x.double().view(N, 1, L).requires_grad_()
    z64 = F.conv1d(x64, bank64, padding=511)
    (z64 * dz0.double().permute(0, 2, 1)).sum().backward()
    e._blob = None
    blob = e.packed({'conv.0.low_hz_': low.to(dev), 'conv.0.band_hz_': band.to(dev), 'conv.1.weight': torch.zeros(C, C, 11, device=dev),
                     'conv.2.weight': torch.zeros(C, C, 9, device=dev), 'conv.3.weight': torch.zeros(1, C, 7, device=dev)})
    xd, dzb = x.to(dev).contiguous(), e.from_rows(dz0.to(dev))
    z0 = twice(lambda: e.conv(0, xd, N, L, blob, None))
    errs['conv0'] = rel(e.rows(z0, N, L).permute(0, 2, 1), z64)

    def bank_grad():
        e._scratch('_sn_bank_ws', 16).fill_(0xff)
        return e.bank_grad(xd, dzb, N, L)
    G = twice(bank_grad)
    errs['bank_grad'] = rel(G, bank64.grad.view(C, 1023))

    def in_dgrad():
        dx = torch.full((N, L), float('nan'), device=dev)
        e.in_dgrad(dzb, blob, N, L, dx)
        return dx
    errs['dx'] = rel(twice(in_dgrad), x64.grad.view(N, L))
    e._blob = None
    record(f'kernels_{N}x{L}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, {k: v for k, v in errs.items() if v > KERNEL_BOUND}


def test_statistics_of_a_channel_far_from_zero(dev, engine):
    N, L = 3, 700
    gen = torch.Generator().manual_seed(77)
    z = torch.randn(N, L, C, generator=gen)
    z[..., 5] += 1e3                                                         # mean / std = 1e3
    z[..., 9] = z[..., 9] * 1e-3 + 1.0
    ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    stat, _, _ = engine.stats(engine.from_rows(z.to(dev)), N, L, C, ones, zeros, zeros, ones)
    z64 = z.numpy().astype(np.float64).reshape(-1, C)
    mean, var = z64.mean(0), z64.var(0)
    got_mean, got_var = stat[0].cpu().numpy(), 1.0 / stat[1].cpu().numpy() ** 2 - 1e-5
    assert np.abs(got_mean / mean - 1).max() <= 1e-6 or np.abs(got_mean - mean).max() <= 1e-6 * np.abs(z64).max()
    assert np.abs(got_mean[[5, 9]] / mean[[5, 9]] - 1).max() <= 1e-6
    assert np.abs(got_var / var - 1).max() <= 1e-6, np.abs(got_var / var - 1).max()


@pytest.mark.parametrize('wkey,fs', [('pretty-brook', 1e6), ('pretty-brook', 2e5), ('noble-monkey', 1.25e9), ('init', 1e6)])
def test_device_bank_and_band_gradient_against_the_host(dev, wkey, fs):
    from stofnet_amd import _lib
    from stofnet_amd.sincnet import filter_bank
    from stofnet_amd.sincnet_training import SincNetTrainEngine
    e = SincNetTrainEngine(dev, fs)
    sd = ti.weights(wkey, fs)
    low, band = sd['conv.0.low_hz_'].astype(np.float32), sd['conv.0.band_hz_'].astype(np.float32)
    host = filter_bank(fs, low, band).view(C, 1023)
    p = {'conv.0.low_hz_': torch.from_numpy(low.copy()).to(dev), 'conv.0.band_hz_': torch.from_numpy(band.copy()).to(dev),
         'conv.1.weight': torch.zeros(C, C, 11, device=dev), 'conv.2.weight': torch.zeros(C, C, 9, device=dev),
         'conv.3.weight': torch.zeros(1, C, 7, device=dev)}
    blob = e.packed(p).view(torch.float32)
    bank_t = blob[e.blob_layout['bank_t']:e.blob_layout['bank_t'] + 1024 * C].view(1024, C).cpu()
    assert not bank_t[1023].any()
    ulp = float(np.spacing(np.float32(host.abs().max())))
    assert float((bank_t[:1023].T - host).abs().max()) <= ulp
    # the fragment image holds the same floats: lane l = 32 h + i, element e of group q of tile nt is W[32 nt + i][8 q + 4 h + e]
    frag = blob[e.blob_layout['frag0']:e.blob_layout['frag0'] + C * 1024].view(4, 128, 2, 32, 4).cpu()
    assert torch.equal(frag.permute(0, 3, 1, 2, 4).reshape(C, 1024), bank_t.T.contiguous())
    # the band gradient on the device against the host entry (double)
    G = torch.from_numpy(np.random.default_rng(5).standard_normal((C, 1023)).astype(np.float32))
    dlow, dband = torch.full((C,), float('nan'), device=dev), torch.full((C,), float('nan'), device=dev)
    e.band_grad(p['conv.0.low_hz_'], p['conv.0.band_hz_'], G.to(dev), dlow, dband)
    desc = _lib.SincNetDesc(float(fs), 1e-5, 0, 0)
    hl, hb = np.zeros(C), np.zeros(C)
    lc, bc, Gn = np.ascontiguousarray(low.reshape(-1)), np.ascontiguousarray(band.reshape(-1)), G.numpy()
    _lib.check(_lib.lib().stof_sincnet_band_grad(ctypes.byref(desc), lc.ctypes.data, bc.ctypes.data, Gn.ctypes.data, hl.ctypes.data,
                                                 hb.ctypes.data), 'stof_sincnet_band_grad')
    assert np.abs(dlow.cpu().numpy() - hl).max() <= KERNEL_BOUND * np.abs(hl).max()
    assert np.abs(dband.cpu().numpy() - hb).max() <= KERNEL_BOUND * np.abs(hb).max()
    assert not dband.cpu().numpy()[hb == 0].any()


# ------------------------------------------------------------------------------------------------ the cases of the fixture
def route_run(name, dev):
    if name in _runs:
        return _runs[name]
    _, wkey, fs, n, L, seed = ti.case(name)
    m = make_net(ti.weights(wkey, fs), fs, L, 'kernels', dev)
    x, t = torch.from_numpy(ti.frames(n, L, seed)).to(dev), torch.from_numpy(ti.cotangent(n, L, seed)).to(dev)
    keep = {}
    y, dx, grads = step(m, x, t, keep=keep)
    eng = next(iter(m._train_engines.values()))
    dec = [(eng.rows(a, n, L) > 0).permute(0, 2, 1).cpu().numpy() for a in keep['saved'].a]
    _runs[name] = dict(y=y.cpu().numpy(), dx=dx.cpu().numpy(), grads={k: v.cpu().numpy() for k, v in grads.items()}, dec=dec,
                       rm=[b.running_mean.cpu().numpy() for b in m.bn], rv=[b.running_var.cpu().numpy() for b in m.bn],
                       nbt=[int(b.num_batches_tracked) for b in m.bn])
    return _runs[name]


@pytest.mark.parametrize('name', ti.IDS)
def test_kernel_route_on_fixture_case(dev, g, name):
    r = route_run(name, dev)
    errs = {}
    own, _ = check_step(name, g, r['y'], r['dx'], r['grads'], r['rm'], r['rv'], r['dec'], errs)
    assert r['nbt'] == [int(g[f'{name}.nbt'])] * 4
    same = all(np.array_equal(a, b) for a, b in zip(r['dec'], own['decisions']))
    record(name, {**errs, 'decisions_equal_float64': float(same)})
    if name in ti.GRAD_IDS:
        _direct.append((name, same))
        if same:
            check_against_reference_fp32(name, g, r['dx'], r['grads'])


def test_direct_comparison_covers_the_fixture(dev, g):
    for name in ti.GRAD_IDS:                                                 # (run alone: the cases have not been through yet)
        if name not in [d[0] for d in _direct]:
            test_kernel_route_on_fixture_case(dev, g, name)
    dropped = sorted({n for n, same in _direct if not same})
    assert len(dropped) <= 2, dropped                                        # at most two cases may drop out of the direct comparison


# ----------------------------------------------------------------------------------------------- behaviour of the boundary
CASE = 'brook_3x129'


@pytest.fixture(scope='module')
def case_inputs(dev):
    _, wkey, fs, n, L, seed = ti.case(CASE)
    return (ti.weights(wkey, fs), fs, L, torch.from_numpy(ti.frames(n, L, seed)).to(dev),
            torch.from_numpy(ti.cotangent(n, L, seed)).to(dev))


def test_two_runs_are_bitwise_equal(dev, case_inputs):
    sd, fs, L, x, t = case_inputs
    a = step(make_net(sd, fs, L, 'kernels', dev), x, t)
    b = step(make_net(sd, fs, L, 'kernels', dev), x, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_aten_route_agrees(dev, g, case_inputs):
    sd, fs, L, x, t = case_inputs
    mk, ma = make_net(sd, fs, L, 'kernels', dev), make_net(sd, fs, L, 'aten', dev)
    yk, dxk, gk = step(mk, x, t, 'kernels')
    ya, dxa, ga = step(ma, x, t, 'aten')
    check_rule(CASE, 'y', yk.cpu().numpy(), ya.cpu().numpy(), g, Y_BOUND)
    check_rule(CASE, 'dx', dxk.cpu().numpy(), dxa.cpu().numpy(), g, GRAD_BOUND)
    for p in ti.PARAMS:
        check_rule(CASE, f'grad.{p}', gk[p].cpu().numpy(), ga[p].cpu().numpy(), g, GRAD_BOUND)
    for i in range(4):
        check_rule(CASE, f'run_mean.{i}', mk.bn[i].running_mean.cpu().numpy(), ma.bn[i].running_mean.cpu().numpy(), g, Y_BOUND)
        check_rule(CASE, f'run_var.{i}', mk.bn[i].running_var.cpu().numpy(), ma.bn[i].running_var.cpu().numpy(), g, Y_BOUND)


def test_eval_mode_after_training_sees_the_new_parameters(dev, case_inputs):
    """The stale-blob trap: after two AdamW steps over ALL parameters, eval mode must see the new parameters and statistics."""
    sd, fs, L, x, t = case_inputs
    m = make_net(sd, fs, L, 'kernels', dev)
    m.eval()
    with torch.no_grad():
        before = m(x)                                                        # packs the eval-mode blob: the trap is its staleness
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    for _ in range(2):
        step(m, x, t, 'kernels', want_dx=False)
        opt.step()
    m.eval()
    with torch.no_grad():
        after = m(x)
        fresh = make_net({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, fs, L, None, dev).eval()
        assert torch.equal(after, fresh(x)) and not torch.equal(after, before)
    assert [int(b.num_batches_tracked) for b in m.bn] == [int(sd['bn.0.num_batches_tracked']) + 2] * 4


def test_running_statistics_after_two_steps_agree_with_the_aten_route(dev, g, case_inputs):
    """Both routes through two AdamW steps.  The conv biases stay out of THIS optimizer: their gradient is analytically 0 under
    train-mode BatchNorm, and AdamW's g / (|g| + eps) turns each route's own rounding noise there into a step of +-lr, which
    moves the next batch mean by more than any rounding (measured 9.7e-5 on run_mean.2 against a bound of 3.5e-5)."""
    sd, fs, L, x, t = case_inputs
    mk, ma = make_net(sd, fs, L, 'kernels', dev), make_net(sd, fs, L, 'aten', dev)
    for m, route in ((mk, 'kernels'), (ma, 'aten')):
        opt = torch.optim.AdamW([p for k, p in m.named_parameters() if not (k.startswith('conv') and k.endswith('bias'))], lr=1e-3)
        for _ in range(2):
            step(m, x, t, route, want_dx=False)
            opt.step()
    assert [int(b.num_batches_tracked) for b in mk.bn] == [int(b.num_batches_tracked) for b in ma.bn]
    for i in range(4):
        check_rule(CASE, f'run_mean.{i}', mk.bn[i].running_mean.cpu().numpy(), ma.bn[i].running_mean.cpu().numpy(), g, Y_BOUND)
        check_rule(CASE, f'run_var.{i}', mk.bn[i].running_var.cpu().numpy(), ma.bn[i].running_var.cpu().numpy(), g, Y_BOUND)


@pytest.mark.parametrize('wkey,fs', [('pretty-brook', 1e6), ('pretty-brook', 2e5), ('noble-monkey', 1.25e9), ('init', 1e6)])
def test_device_packed_blob_gives_the_host_packers_eval_output(dev, wkey, fs):
    from stofnet_amd.sincnet import device_pack_weights, pack_weights
    sd = ti.weights(wkey, fs)
    L = 300
    m = make_net(sd, fs, L, None, dev).eval()
    x = torch.from_numpy(si.frames((3, 1, L), 41)).to(dev)
    with torch.no_grad():
        y_host = m(x)                                                        # train_route None: the host packer
        host_blob = m.packed_weights(dev).clone()
        m.train_route = 'kernels'                                            # a training route: eval packs on the device
        m.invalidate_packed()
        y_dev = m(x)
        dev_blob = m.packed_weights(dev)
    params = [p.detach() for p in m._kernel_params()]
    assert torch.equal(dev_blob, device_pack_weights(fs, 1e-5, params))
    assert torch.equal(host_blob.cpu(), pack_weights(fs, [p.cpu().numpy() for p in params], 1e-5))
    differing = int((dev_blob.view(torch.float32) != host_blob.view(torch.float32)).sum())
    print(wkey, fs, 'floats of the device blob that differ from the host blob:', differing)
    assert torch.equal(y_dev, y_host)                                        # bitwise the same eval-mode output
    assert differing == 0


# the shapes at which a chunk outgrows its minimum: more than 64 x 64 rows (conv weight gradient) and more than 64 tiles of 128
# samples (bank gradient: a work-group walks several tiles and re-stages its LDS image); more than 256 x 256 rows (layer 3's
# weight gradient); more than 1024 x 256 rows (the statistics kernels)
def test_grown_chunks_conv_and_bank_gradients(dev, engine):
    e, N, L = engine, 5, 1700                                                # 8500 rows, 70 tiles
    gen = torch.Generator().manual_seed(515)
    rn = lambda *s: torch.randn(*s, generator=gen)                            # noqa: E731
    errs = {}
    for l, K in ((1, 11), (2, 9)):
        a_prev, dzl = rn(N, L, C), rn(N, L, C)
        a64 = a_prev.to(dev).double().permute(0, 2, 1).contiguous()
        w64 = torch.zeros(C, C, K, dtype=torch.float64, device=dev, requires_grad=True)
        b64 = torch.zeros(C, dtype=torch.float64, device=dev, requires_grad=True)
        (F.conv1d(a64, w64, b64, padding=K // 2) * dzl.to(dev).double().permute(0, 2, 1)).sum().backward()
        ab, dzb = e.from_rows(a_prev.to(dev)), e.from_rows(dzl.to(dev))

        def wgrad():
            e._scratch('_sn_wgrad_ws', 16).fill_(0xff)
            dw, db = torch.full((C, C, K), float('nan'), device=dev), torch.full((C,), float('nan'), device=dev)
            e.conv_wgrad(l, ab, dzb, N, L, dw, db)
            return dw, db
        dw, db = twice(wgrad)
        errs[f'dw{l}'], errs[f'db{l}'] = rel(dw, w64.grad), rel(db, b64.grad)
    x, dz0 = rn(N, L), rn(N, L, C)
    bank64 = torch.zeros(C, 1, 1023, dtype=torch.float64, device=dev, requires_grad=True)
    (F.conv1d(x.to(dev).double().view(N, 1, L), bank64, padding=511) * dz0.to(dev).double().permute(0, 2, 1)).sum().backward()
    xd, dzb = x.to(dev).contiguous(), e.from_rows(dz0.to(dev))

    def bank_grad():
        e._scratch('_sn_bank_ws', 16).fill_(0xff)
        return e.bank_grad(xd, dzb, N, L)
    errs['bank_grad'] = rel(twice(bank_grad), bank64.grad.view(C, 1023))
    record(f'grown_chunks_{N}x{L}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


def test_grown_chunks_layer3_weight_gradient(dev, engine):
    e, N, L = engine, 33, 2000                                               # 66000 rows > 256 x 256
    gen = torch.Generator().manual_seed(516)
    a2, dz3 = torch.randn(N, L, C, generator=gen).to(dev), torch.randn(N, L, generator=gen).to(dev)
    w64 = torch.zeros(1, C, 7, dtype=torch.float64, device=dev, requires_grad=True)
    b64 = torch.zeros(1, dtype=torch.float64, device=dev, requires_grad=True)
    (F.conv1d(a2.double().permute(0, 2, 1), w64, b64, padding=3) * dz3.double().view(N, 1, L)).sum().backward()
    ab, dzb = e.from_rows(a2), dz3.reshape(-1).contiguous()

    def out_wgrad():
        e._scratch('_sn_out_ws', 16).fill_(0xff)
        dw, db = torch.full((1, C, 7), float('nan'), device=dev), torch.full((1,), float('nan'), device=dev)
        e.out_wgrad(ab, dzb, N, L, dw, db)
        return dw, db
    dw, db = twice(out_wgrad)
    errs = {'dw3': rel(dw, w64.grad), 'db3': rel(db, b64.grad)}
    record(f'grown_chunks_{N}x{L}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


@pytest.mark.parametrize('ch', [C, 1])
def test_grown_chunks_statistics_and_batchnorm_backward(dev, engine, ch):
    e, N, L = engine, 132, 2000                                              # 264000 rows > 1024 x 256
    M = N * L
    gen = torch.Generator(device=dev).manual_seed(517 + ch)
    rn = lambda *s: torch.randn(*s, generator=gen, device=dev)                # noqa: E731
    z, a_dec, da = rn(N, L, ch) * 2 + rn(ch), rn(N, L, ch), rn(N, L, ch)
    gamma, beta, rmean, rvar = rn(ch), rn(ch), rn(ch), rn(ch).abs() + 0.5
    z64 = z.double()
    mean, var = z64.mean((0, 1)), z64.var((0, 1), unbiased=False)
    xh = (z64 - mean) / torch.sqrt(var + 1e-5)
    v = xh * gamma.double() + beta.double()
    out64 = torch.where(v > 0, v, 0.2 * v) if ch == C else v
    g64 = da.double() * (torch.where(a_dec > 0, 1.0, 0.2).double() if ch == C else 1.0)
    dz64 = gamma.double() / torch.sqrt(var + 1e-5) * (g64 - g64.mean((0, 1)) - xh * (g64 * xh).mean((0, 1)))
    to_buf = (lambda t: e.from_rows(t)) if ch == C else (lambda t: t.reshape(-1).contiguous())
    of_buf = (lambda b: e.rows(b, N, L)) if ch == C else (lambda b: b.view(N, L, 1))
    zb, ab, dab = to_buf(z), to_buf(a_dec), to_buf(da)
    stat, nm, nv = twice(lambda: e.stats(zb, N, L, ch, gamma, beta, rmean, rvar))
    out = e.apply(zb, N, L, ch, stat)
    dgam, dbet = torch.full((ch,), float('nan'), device=dev), torch.full((ch,), float('nan'), device=dev)
    dz = e.bn_bwd(dab, ab if ch == C else None, zb, stat, gamma, N, L, ch, dgam, dbet)
    errs = {'mean': rel(stat[0], mean), 'var': rel(1.0 / stat[1] ** 2 - 1e-5, var), 'apply': rel(of_buf(out), out64),
            'run_mean': rel(nm, 0.95 * rmean.double() + 0.05 * mean), 'run_var': rel(nv, 0.95 * rvar.double() + 0.05 * var * M / (M - 1)),
            'dz': rel(of_buf(dz), dz64), 'dgamma': rel(dgam, (g64 * xh).sum((0, 1))), 'dbeta': rel(dbet, g64.sum((0, 1)))}
    record(f'grown_chunks_stats_{N}x{L}_c{ch}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


def test_graph_and_error_behaviour(dev, case_inputs):
    sd, fs, L, x, t = case_inputs
    m = make_net(sd, fs, L, 'kernels', dev)
    y, dx, grads = step(m, x, t, want_dx=False)
    assert dx is None and y.shape == x.shape and len(grads) == 16 and all(v is not None for v in grads.values())
    yy = m(x)
    assert type(yy.grad_fn).__name__.startswith('SincNetFunction')
    loss = yy.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()
    for pname in ('conv.0.low_hz_', 'conv.2.weight', 'bn.1.weight'):
        loss = m(x).sum()
        with torch.no_grad():
            dict(m.named_parameters())[pname].mul_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            loss.backward()
    m(x).sum().backward()                                                    # the next step is fine
    nbt = int(m.bn[0].num_batches_tracked)
    with torch.no_grad():                                                    # train mode under no_grad: batch statistics, buffers move
        assert m(x).grad_fn is None and int(m.bn[0].num_batches_tracked) == nbt + 1
    m.eval()
    with torch.no_grad():
        assert m(x).grad_fn is None and int(m.bn[0].num_batches_tracked) == nbt + 1
    with pytest.raises(NotImplementedError, match="train_route='aten'"):
        m(x.clone().requires_grad_(True))
    m.train()
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        m(torch.zeros(1, 1, 1, device=dev))
    with pytest.raises(TypeError):
        m(x.double())


# ------------------------------------------------------------------------------------------------------------ main.py
def run_main_training(tmp_path, run):
    ck = tmp_path / run
    code = ('import sys, json; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[2:]); print(json.dumps(s))')
    log = os.path.join(ROOT, f'{run}_unit.jsonl')
    try:
        res = subprocess.run([sys.executable, '-c', code, ROOT, 'model=sincnet', 'evaluate=False', 'train_route=kernels', 'fs=1e5',
                              f'ckpt_dir={ck}', f'run_name={run}', 'logging=unit', 'epochs=2', 'batch_size=4',
                              'data_dir=./datasets/stof_chirp101_dataset', 'num_waveforms=16', 'num_samples=256', 'seed=5'],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stdout + res.stderr
    finally:
        if os.path.exists(log):
            os.remove(log)
    return json.loads(res.stdout.strip().splitlines()[-1]), sorted(ck.iterdir())


def test_main_entry_point_trains_sincnet_reproducibly(dev, tmp_path):
    from stofnet_amd import SincNet
    sds, hists = [], []
    for k in range(2):
        run = f'sincnettest{os.getpid()}r{k}'
        summary, paths = run_main_training(tmp_path, run)
        hist = summary['train_history']
        assert summary['model'] == 'sincnet' and summary['train_route'] == 'kernels' and len(hist) == 2
        assert all(np.isfinite(h['train_loss']) and np.isfinite(h['val_loss']) for h in hist)
        assert len(paths) == 1 and paths[0].name.endswith('_epoch_2.pth')
        sd = torch.load(str(paths[0]), map_location='cpu', weights_only=True)
        SincNet(si.options(1e5 * 10, 256)).load_state_dict(sd, strict=True)
        assert int(sd['bn.0.num_batches_tracked']) > 0
        sds.append(sd)
        hists.append([(h['train_loss'], h['val_loss']) for h in hist])
    assert hists[0] == hists[1] and all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])

"""WaveUnet training on the gfx950 kernels (`train_route = 'kernels'`, stofnet_amd/waveunet_training.py, csrc/waveunet_train.hip):

  * every new kernel alone on Gaussian operands against float64 torch, 2e-6 x max|ref| (the project's per-kernel bound), run twice
    for equal bits: statistics, apply, BatchNorm backward, every weight-gradient variant (plain / decimated / interpolated +
    concatenated source; Cin <= 192 and > 192), the forward convolution with its training epilogue and the data gradient on the
    same variants, the interpolation transpose (M = 1, 2, 3, a tile edge), the skip sum, the head and its backward, encoder 0's
    convolution, weight and data gradient; and every bounded reduction inside its grown-chunk regime (shapes from CHUNKS x
    MAX_PARTIALS).  The interpolated source of the float64 references is built from the kernels' own fp32 coordinates
    (`interp_table`), which tests/test_waveunet_training_cpu.py pins to ATen's;
  * every case of tests/golden/f30_waveunet_training.npz through the route under the tolerance rule of
    tests/test_waveunet_training_cpu.py (float64 autograd with the route's decisions; where those are float64's, also the
    reference's own fp32 results);
  * bitwise repeatability, train mode under no_grad, the 'aten' route within the same bounds, the route and error contract, the
    eval-mode blob after an optimizer step, and main.py model=unet evaluate=False on both routes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
import waveunet_training_inputs as ti
from test_waveunet_training_cpu import (GRAD_BOUND, Y_BOUND, bn_layers, check_against_reference_fp32, check_rule, check_step, make_net)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'waveunet_training.jsonl')
KERNEL_BOUND = 2e-6
DECIMATED, DECODER, PLAIN = 0, 1, 2
_errors, _runs, _direct = {}, {}, []


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f30_waveunet_training')


@pytest.fixture(scope='module')
def engine(dev):
    from stofnet_amd.waveunet_training import WaveUnetTrainEngine
    return WaveUnetTrainEngine(dev, 2)


def rel(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(a).all()
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def record(name, errs):
    """print the achieved errors and keep them in profiles/waveunet_training.jsonl (one `parity` line, rewritten as cases come in)"""
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


def twice(fn):
    a, b = fn(), fn()
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    return a if len(a) > 1 else a[0]


def randn(dev, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


# ------------------------------------------------------------------------------------------------- the kernels alone
def interp_matrix(M, dev):
    """[2 M, M] float64: the forward's interpolation with the kernels' fp32 coordinates"""
    from stofnet_amd.waveunet_training import interp_table
    i0, i1, l0, l1, _, _ = interp_table(M)
    A = np.zeros((2 * M, M))
    np.add.at(A, (np.arange(2 * M), i0), l0.astype(np.float64))
    np.add.at(A, (np.arange(2 * M), i1), l1.astype(np.float64))
    return torch.from_numpy(A).to(dev)


def virtual64(mode, src, low, dev):
    """the virtual input of a convolution in float64, [N, Cin, Lout]"""
    if mode == DECIMATED:
        return src.double()[:, ::2].permute(0, 2, 1).contiguous()
    if mode == PLAIN:
        return src.double().permute(0, 2, 1).contiguous()
    up = torch.einsum('um,nmc->nuc', interp_matrix(int(low.shape[1]), dev), low.double())
    return torch.cat([up, src.double()], -1).permute(0, 2, 1).contiguous()


def conv_operands(dev, seed, mode, N, Lout, cin, cu, cout, taps):
    if mode == DECIMATED:
        src, low = randn(dev, seed, N, 2 * Lout, cin), None
    elif mode == PLAIN:
        src, low = randn(dev, seed, N, Lout, cin), None
    else:
        src, low = randn(dev, seed, N, Lout, cin - cu), randn(dev, seed + 1, N, Lout // 2, cu)
    w = randn(dev, seed + 2, cout, cin, taps) / (cin * taps) ** 0.5
    return src, low, w, randn(dev, seed + 3, cout), randn(dev, seed + 4, N, Lout, cout)


# (mode, cin, cu, cout, taps): decimated / plain / decoder sources, one and two 192-channel passes, 1 .. 4 and 3 N tiles per wave
CONV_VARIANTS = [(DECIMATED, 16, 0, 32, 15), (DECIMATED, 96, 0, 112, 15), (PLAIN, 48, 0, 16, 15), (PLAIN, 32, 0, 48, 5),
                 (DECODER, 32, 16, 16, 5), (DECODER, 48, 32, 16, 5), (DECODER, 224, 112, 112, 5), (DECODER, 208, 112, 96, 5)]
# (N, Lout): the minimum, odd batches, a tile edge (64 positions) below / on / above, more than one tile with a ragged end
CONV_SHAPES = [(2, 2), (3, 6), (1, 62), (2, 64), (1, 66), (3, 150)]


@pytest.mark.parametrize('mode,cin,cu,cout,taps', CONV_VARIANTS)
def test_conv_forward_weight_and_data_gradient_vs_torch(dev, engine, mode, cin, cu, cout, taps):
    e, errs = engine, {}
    for k, (N, Lout) in enumerate(CONV_SHAPES if cin < 192 else CONV_SHAPES[1::2]):
        src, low, w, b, dz = conv_operands(dev, 100 * cin + 10 * k + mode, mode, N, Lout, cin, cu, cout, taps)
        vin = virtual64(mode, src, low, dev).requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        z64 = F.conv1d(vin, w64, b64, padding=taps // 2)
        (z64 * dz.double().permute(0, 2, 1)).sum().backward()
        z = twice(lambda: e.conv(src, low, N, Lout, cin, cu, cout, taps, mode, e.pack_frag(w, 0), b))
        errs[f'z_{N}x{Lout}'] = rel(z.permute(0, 2, 1), z64)

        def wgrad():
            e._scratch('_wu_wgrad_ws', 16).fill_(0xff)
            dw, db = torch.full((cout, cin, taps), float('nan'), device=dev), torch.full((cout,), float('nan'), device=dev)
            e.conv_wgrad(src, low, dz, N, Lout, cin, cu, cout, taps, mode, dw, db)
            return dw, db
        dw, db = twice(wgrad)
        errs[f'dw_{N}x{Lout}'], errs[f'db_{N}x{Lout}'] = rel(dw, w64.grad), rel(db, b64.grad)
        gin = twice(lambda: e.conv_dgrad(dz, N, Lout, cin, cout, taps, e.pack_frag(w, 1)))
        errs[f'dgrad_{N}x{Lout}'] = rel(gin.permute(0, 2, 1), vin.grad)
    record(f'conv_mode{mode}_{cin}_{cu}_{cout}_k{taps}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


def bn_reference(z, a_dec, da, gamma, beta, eps):
    z64 = z.double()
    mean, var = z64.mean((0, 1)), z64.var((0, 1), unbiased=False)
    xh = (z64 - mean) / torch.sqrt(var + eps)
    v = xh * gamma.double() + beta.double()
    g64 = da.double() * torch.where(a_dec > 0, 1.0, 0.1).double()
    dz64 = gamma.double() / torch.sqrt(var + eps) * (g64 - g64.mean((0, 1)) - xh * (g64 * xh).mean((0, 1)))
    return mean, var, torch.where(v > 0, v, 0.1 * v), dz64, (g64 * xh).sum((0, 1)), g64.sum((0, 1))


def bn_shapes():
    from stofnet_amd.waveunet_training import CHUNKS, MAX_PARTIALS
    c, grown = CHUNKS['stats'], CHUNKS['stats'] * MAX_PARTIALS['stats']
    return ([(2, 1, 16), (3, 7, 48), (1, c - 1, 16), (1, c, 192), (1, c + 1, 80), (2, c + 3, 192)] +
            [(1, grown + 2, 16), (3, grown // 3 + 5, 80)])           # inside the grown-chunk regime: more rows than partials x rows


def test_statistics_apply_and_batchnorm_backward_vs_torch(dev, engine):
    e = engine
    for k, (N, L, ch) in enumerate(bn_shapes()):
        M, eps, mom = N * L, 1e-5, 0.1
        z = randn(dev, 300 + k, N, L, ch) * 2 + randn(dev, 301 + k, ch)
        a_dec, da = randn(dev, 302 + k, N, L, ch), randn(dev, 303 + k, N, L, ch)
        gamma, beta, rmean, rvar = randn(dev, 304 + k, ch), randn(dev, 305 + k, ch), randn(dev, 306 + k, ch), randn(dev, 307 + k, ch).abs() + 0.5
        mean, var, out64, dz64, dg64, db64 = bn_reference(z, a_dec, da, gamma, beta, eps)
        stat, nm, nv = twice(lambda: e.stats(z, gamma, beta, rmean, rvar, eps, mom))
        out = twice(lambda: e.apply(z, stat))

        def bwd():
            dgam, dbet = torch.full((ch,), float('nan'), device=dev), torch.full((ch,), float('nan'), device=dev)
            return e.bn_bwd(da, a_dec, z, stat, dgam, dbet), dgam, dbet
        dz, dgam, dbet = twice(bwd)
        errs = {'mean': rel(stat[0], mean), 'var': rel(1.0 / stat[1] ** 2 - eps, var), 'apply': rel(out, out64),
                'run_mean': rel(nm, (1 - mom) * rmean.double() + mom * mean), 'run_var': rel(nv, (1 - mom) * rvar.double() + mom * var * M / (M - 1)),
                'dz': rel(dz, dz64), 'dgamma': rel(dgam, dg64), 'dbeta': rel(dbet, db64)}
        record(f'bn_{N}x{L}_c{ch}', errs)
        assert max(errs.values()) <= KERNEL_BOUND, errs


def head_shapes():
    from stofnet_amd.waveunet_training import CHUNKS, MAX_PARTIALS
    c = CHUNKS['head_wgrad']
    return [(2, 2), (3, 43), (1, c - 2), (1, c), (1, c + 2), (1, c * MAX_PARTIALS['head_wgrad'] + 2)]


def test_head_and_its_backward_vs_torch(dev, engine):
    e = engine
    for k, (N, L) in enumerate(head_shapes()):
        o, x, dy = randn(dev, 400 + k, N, L, 16), randn(dev, 401 + k, N, L), randn(dev, 402 + k, N, L)
        w, b = randn(dev, 403 + k, 1, 17, 1) * 0.3, randn(dev, 404 + k, 1) * 0.1
        o64, x64 = o.double().requires_grad_(True), x.double().requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        y64 = torch.tanh(F.conv1d(torch.cat([o64.permute(0, 2, 1), x64.view(N, 1, L)], 1), w64, b64)).view(N, L)
        (y64 * dy.double()).sum().backward()
        y = twice(lambda: e.head(o, x, w, b))

        def bwd(want):
            e._scratch('_wu_head_ws', 16).fill_(0xff)
            dw, db = torch.full((1, 17, 1), float('nan'), device=dev), torch.full((1,), float('nan'), device=dev)
            do, dxh = e.head_bwd(dy, y, o, x, w, dw, db, want)
            return (do, dxh, dw, db) if want else (do, dw, db)
        do, dxh, dw, db = twice(lambda: bwd(True))
        assert torch.equal(bwd(False)[0], do)
        errs = {'y': rel(y, y64), 'do': rel(do, o64.grad), 'dxh': rel(dxh, x64.grad), 'dw': rel(dw, w64.grad), 'db': rel(db, b64.grad)}
        record(f'head_{N}x{L}', errs)
        assert max(errs.values()) <= KERNEL_BOUND, errs


def in_shapes():
    from stofnet_amd.waveunet_training import CHUNKS, MAX_PARTIALS
    c = CHUNKS['in_wgrad']
    return [(2, 2), (3, 7), (3, 43), (1, c - 2), (1, c), (1, c + 2), (2, c + 1), (1, c * MAX_PARTIALS['in_wgrad'] + 2)]


def test_encoder0_conv_weight_and_data_gradient_vs_torch(dev, engine):
    e = engine
    for k, (N, L) in enumerate(in_shapes()):
        x, dz, dxh = randn(dev, 500 + k, N, L), randn(dev, 501 + k, N, L, 16), randn(dev, 502 + k, N, L)
        w, b = randn(dev, 503 + k, 16, 1, 15) / 15 ** 0.5, randn(dev, 504 + k, 16)
        x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
        z64 = F.conv1d(x64.view(N, 1, L), w64, b64, padding=7)
        (z64 * dz.double().permute(0, 2, 1)).sum().backward()
        z = twice(lambda: e.in_conv(x, e.pack_in(w, b)))

        def wgrad():
            e._scratch('_wu_in_ws', 16).fill_(0xff)
            dw, db = torch.full((16, 1, 15), float('nan'), device=dev), torch.full((16,), float('nan'), device=dev)
            e.in_wgrad(x, dz, dw, db)
            return dw, db
        dw, db = twice(wgrad)

        def dgrad(head):
            dx = torch.full((N, L), float('nan'), device=dev)
            e.in_dgrad(dz, w, head, dx)
            return dx
        errs = {'z': rel(z.permute(0, 2, 1), z64), 'dw': rel(dw, w64.grad), 'db': rel(db, b64.grad),
                'dx': rel(twice(lambda: dgrad(None)), x64.grad), 'dx_with_head': rel(dgrad(dxh), x64.grad + dxh.double())}
        record(f'enc0_{N}x{L}', errs)
        assert max(errs.values()) <= KERNEL_BOUND, errs


@pytest.mark.parametrize('M', [1, 2, 3, 31, 32, 33, 200])
def test_interpolation_transpose_vs_torch(dev, engine, M):
    N, cg, cu = 3, 48, 32
    gfull = randn(dev, 600 + M, N, 2 * M, cg)
    A = interp_matrix(M, dev)
    ref = torch.einsum('um,nuc->nmc', A, gfull.double()[..., :cu])
    dlow = twice(lambda: engine.interp_t(gfull, N, M, cu))
    errs = {'dlow': rel(dlow, ref)}
    record(f'interp_t_M{M}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


def test_skip_sum_is_decoder_part_then_encoder_part(dev, engine):
    for N, L, cu, cs in ((2, 2, 16, 16), (3, 66, 48, 32), (1, 130, 192, 192)):
        gdec, genc = randn(dev, 700 + L, N, L, cu + cs), randn(dev, 701 + L, N, L // 2, cs)
        ref = gdec[..., cu:].clone()
        ref[:, ::2] = ref[:, ::2] + genc                                    # fp32: one addition per element, so bits are equal
        out = twice(lambda: engine.skip_sum(gdec, genc, N, L, cu, cs))
        assert torch.equal(out, ref)


def test_grown_chunks_conv_weight_gradient(dev, engine):
    """more 64-position tiles than partials: a work-group walks several tiles and stages its LDS windows again"""
    from stofnet_amd.waveunet_training import CHUNKS, MAX_PARTIALS
    e, errs = engine, {}
    rows = CHUNKS['conv_wgrad'] * MAX_PARTIALS['conv_wgrad']
    for mode, N, Lout, cin, cu, cout, taps in ((PLAIN, 1, rows + 2, 16, 0, 16, 15), (DECODER, 3, rows // 2 + 6, 32, 16, 16, 5),
                                               (DECIMATED, 2, rows // 2 + 65, 16, 0, 32, 15)):
        src, low, w, b, dz = conv_operands(dev, 800 + mode, mode, N, Lout, cin, cu, cout, taps)
        vin = virtual64(mode, src, low, dev)
        w64, b64 = torch.zeros_like(w).double().requires_grad_(True), torch.zeros_like(b).double().requires_grad_(True)
        (F.conv1d(vin, w64, b64, padding=taps // 2) * dz.double().permute(0, 2, 1)).sum().backward()

        def wgrad():
            e._scratch('_wu_wgrad_ws', 16).fill_(0xff)
            dw, db = torch.full((cout, cin, taps), float('nan'), device=dev), torch.full((cout,), float('nan'), device=dev)
            e.conv_wgrad(src, low, dz, N, Lout, cin, cu, cout, taps, mode, dw, db)
            return dw, db
        dw, db = twice(wgrad)
        errs[f'dw_mode{mode}'], errs[f'db_mode{mode}'] = rel(dw, w64.grad), rel(db, b64.grad)
    record('grown_chunks_conv_wgrad', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


# ------------------------------------------------------------------------------------------------ the cases of the fixture
def route_run(name, dev):
    if name in _runs:
        return _runs[name]
    _, nl, wseed, n, L, seed = ti.case(name)
    m = make_net(ti.weights(nl, wseed), nl, 'kernels', dev)
    x, t = torch.from_numpy(ti.frames(n, L, seed)).to(dev), torch.from_numpy(ti.cotangent(n, L, seed)).to(dev)
    keep = {}
    y, dx, grads = step(m, x, t, keep=keep)
    dec = [(a > 0).permute(0, 2, 1).cpu().numpy() for a in keep['saved'].a]
    bns = bn_layers(m)
    _runs[name] = dict(y=y.cpu().numpy(), dx=dx.cpu().numpy(), grads={k: v.cpu().numpy() for k, v in grads.items()}, dec=dec,
                       rm=[b.running_mean.cpu().numpy() for b in bns], rv=[b.running_var.cpu().numpy() for b in bns],
                       nbt=[int(b.num_batches_tracked) for b in bns])
    return _runs[name]


@pytest.mark.parametrize('name', ti.IDS)
def test_kernel_route_on_fixture_case(dev, g, name):
    r = route_run(name, dev)
    errs = {}
    own, _ = check_step(name, g, r['y'], r['dx'], r['grads'], r['rm'], r['rv'], r['dec'], errs)
    assert r['nbt'] == [int(g[f'{name}.nbt'])] * len(r['nbt'])
    same = all(np.array_equal(a, b) for a, b in zip(r['dec'], own['decisions']))
    # (recorded: the worst of each kind relative to max|ref64|, without the conv bias gradients, whose reference is an analytic zero)
    zero = {f'grad.{p}' for p in ti.zero_grads(ti.case(name)[1])}
    kept = {q: v for q, v in errs.items() if q not in zero}
    worst = {k: max(v for q, v in kept.items() if q.startswith(k)) for k in ('y', 'run_mean', 'run_var', 'dx', 'grad') if any(q.startswith(k) for q in kept)}
    record(name, {**worst, 'decisions_equal_float64': float(same)})
    if name in ti.GRAD_IDS:
        _direct.append((name, same))
        if same and int(g[f'{name}.same']):
            check_against_reference_fp32(name, g, r['dx'], r['grads'])


# ----------------------------------------------------------------------------------------------- behaviour of the boundary
CASE = 'unet_n2_5x132'


@pytest.fixture(scope='module')
def case_inputs(dev):
    _, nl, wseed, n, L, seed = ti.case(CASE)
    return (ti.weights(nl, wseed), nl, torch.from_numpy(ti.frames(n, L, seed)).to(dev), torch.from_numpy(ti.cotangent(n, L, seed)).to(dev))


def buffers(m):
    return [t.clone() for b in bn_layers(m) for t in (b.running_mean, b.running_var, b.num_batches_tracked)]


def test_two_runs_are_bitwise_equal(dev, case_inputs):
    sd, nl, x, t = case_inputs
    ma, mb = make_net(sd, nl, 'kernels', dev), make_net(sd, nl, 'kernels', dev)
    a, b = step(ma, x, t), step(mb, x, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert all(torch.equal(u, v) for u, v in zip(buffers(ma), buffers(mb)))


def test_train_mode_under_no_grad_moves_the_same_statistics(dev, case_inputs):
    sd, nl, x, t = case_inputs
    ma, mb = make_net(sd, nl, 'kernels', dev), make_net(sd, nl, 'kernels', dev)
    ya = ma(x.clone().requires_grad_(True))
    with torch.no_grad():
        yb = mb(x)
    assert ya.grad_fn is not None and yb.grad_fn is None and torch.equal(ya.detach(), yb)
    assert all(torch.equal(u, v) for u, v in zip(buffers(ma), buffers(mb)))
    assert int(mb.middle[1].num_batches_tracked) == 1


def test_aten_route_agrees(dev, g, case_inputs):
    sd, nl, x, t = case_inputs
    mk, ma = make_net(sd, nl, 'kernels', dev), make_net(sd, nl, 'aten', dev)
    yk, dxk, gk = step(mk, x, t, 'kernels')
    ya, dxa, ga = step(ma, x, t, 'aten')
    check_rule(CASE, 'y', yk.cpu().numpy(), ya.cpu().numpy(), g, Y_BOUND)
    check_rule(CASE, 'dx', dxk.cpu().numpy(), dxa.cpu().numpy(), g, GRAD_BOUND)
    for p in ti.params(nl):
        check_rule(CASE, f'grad.{p}', gk[p].cpu().numpy(), ga[p].cpu().numpy(), g, GRAD_BOUND)
    for i, (bk, ba) in enumerate(zip(bn_layers(mk), bn_layers(ma))):
        check_rule(CASE, f'run_mean.{i}', bk.running_mean.cpu().numpy(), ba.running_mean.cpu().numpy(), g, Y_BOUND)
        check_rule(CASE, f'run_var.{i}', bk.running_var.cpu().numpy(), ba.running_var.cpu().numpy(), g, Y_BOUND)
        assert int(bk.num_batches_tracked) == int(ba.num_batches_tracked) == 1


def test_eval_mode_is_unchanged_by_the_route(dev, case_inputs):
    sd, nl, x, t = case_inputs
    ma, mk = make_net(sd, nl, 'aten', dev).eval(), make_net(sd, nl, 'kernels', dev).eval()
    with torch.no_grad():
        ya, yk = ma(x), mk(x)
        assert torch.equal(ya, yk) and torch.equal(ya, ma.forward_kernels(x))              # the inference kernels' bits on either setting
    before = buffers(mk)
    yg = mk(x.clone().requires_grad_(True))                                                 # eval mode with a graph: forward_aten
    assert yg.grad_fn is not None and not type(yg.grad_fn).__name__.startswith('WaveUnetFunction')
    assert rel(yg, mk.forward_aten(x)) <= 1e-6 and all(torch.equal(u, v) for u, v in zip(before, buffers(mk)))


def test_eval_mode_after_training_sees_the_new_parameters(dev, case_inputs):
    """The stale-blob trap: after an AdamW step over ALL parameters and a further train-mode call, eval mode must see the new
    parameters and running statistics."""
    sd, nl, x, t = case_inputs
    m = make_net(sd, nl, 'kernels', dev)
    m.eval()
    with torch.no_grad():
        before = m(x)                                                        # packs the eval-mode blob: the trap is its staleness
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    step(m, x, t, 'kernels', want_dx=False)
    opt.step()
    with torch.no_grad():
        m(x)                                                                 # train mode: the statistics move once more
    m.eval()
    with torch.no_grad():
        after, aten = m(x), m.forward_aten(x)
    assert not torch.equal(after, before) and rel(after, aten) <= 1e-5
    assert [int(b.num_batches_tracked) for b in bn_layers(m)] == [2] * (2 * nl + 1)


def test_graph_and_error_behaviour(dev, case_inputs):
    sd, nl, x, t = case_inputs
    m = make_net(sd, nl, 'kernels', dev)
    eng_calls = []
    y0 = m(x)                                                                # creates the engine
    eng = next(iter(m._train_engines.values()))
    orig = eng.in_dgrad
    eng.in_dgrad = lambda *a, **k: (eng_calls.append(1), orig(*a, **k))[1]
    try:
        y, dx, grads = step(m, x, t, want_dx=False)
        assert dx is None and not eng_calls                                  # no dx wanted: encoder 0's data gradient is not launched
        assert y.shape == x.shape and len(grads) == 4 * (2 * nl + 1) + 2 and all(v is not None for v in grads.values())
        step(m, x, t, want_dx=True)
        assert len(eng_calls) == 1
    finally:
        eng.in_dgrad = orig
    assert type(y0.grad_fn).__name__.startswith('WaveUnetFunction')
    loss = m(x).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()
    for pname in ('encoder.0.main.0.weight', 'middle.1.weight', 'decoder.1.main.0.bias', 'out.0.weight'):
        loss = m(x).sum()
        with torch.no_grad():
            dict(m.named_parameters())[pname].mul_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            loss.backward()
    m(x).sum().backward()                                                    # the next step is fine
    before = buffers(m)
    with pytest.raises(RuntimeError, match='multiple of 2\\^n_layers'):
        m(torch.zeros(2, 1, 6, device=dev))
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        m(torch.zeros(1, 1, 4, device=dev))
    with pytest.raises(TypeError):
        m(x.double())
    with pytest.raises(RuntimeError):
        m(x.cpu())
    assert all(torch.equal(u, v) for u, v in zip(before, buffers(m)))          # none of them touched a buffer


# ------------------------------------------------------------------------------------------------------------ main.py
def run_main_training(tmp_path, run, route):
    ck = tmp_path / run
    code = ('import sys, json; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[2:]); print(json.dumps(s))')
    log = os.path.join(ROOT, f'{run}_unit.jsonl')
    try:
        res = subprocess.run([sys.executable, '-c', code, ROOT, 'model=unet', 'evaluate=False', f'train_route={route}',
                              f'ckpt_dir={ck}', f'run_name={run}', 'logging=unit', 'epochs=2', 'batch_size=4',
                              'data_dir=./datasets/stof_chirp101_dataset', 'num_waveforms=16', 'num_samples=256', 'seed=5'],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stdout + res.stderr
    finally:
        if os.path.exists(log):
            os.remove(log)
    return json.loads(res.stdout.strip().splitlines()[-1]), sorted(ck.iterdir())


def test_main_entry_point_trains_unet_on_both_routes(dev, tmp_path):
    from stofnet_amd import WaveUnet
    sds, hists, summaries = [], [], []
    for k, route in enumerate(('kernels', 'kernels', 'aten')):
        run = f'unettest{os.getpid()}r{k}'
        summary, paths = run_main_training(tmp_path, run, route)
        hist = summary['train_history']
        assert summary['model'] == 'unet' and summary['train_route'] == route and summary['train_precision'] == 'fp32' and len(hist) == 2
        assert all(np.isfinite(h['train_loss']) and np.isfinite(h['val_loss']) for h in hist)
        assert len(paths) == 1 and paths[0].name.endswith('_epoch_2.pth')
        sd = torch.load(str(paths[0]), map_location='cpu', weights_only=True)
        WaveUnet(2, 16).load_state_dict(sd, strict=True)
        assert int(sd['middle.1.num_batches_tracked']) > 0
        sds.append(sd)
        hists.append([(h['train_loss'], h['val_loss']) for h in hist])
        summaries.append(json.dumps({k2: v for k2, v in summary.items() if 'time' not in k2 and 'per_s' not in k2}, sort_keys=True))
    assert hists[0] == hists[1] and all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])
    assert summaries[0] == summaries[1]                                      # everything but the measured times, NaN included

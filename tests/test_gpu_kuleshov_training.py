"""Kuleshov training on the gfx950 kernels (`train_route = 'kernels'`, stofnet_amd/kuleshov_training.py, csrc/kuleshov_train.hip):

  * every new kernel alone on Gaussian operands against float64 torch, run twice for equal bits: the forward convolution with its
    training epilogue on each (Cin, Cout, taps, stride) of the network with an M tail (1e-5 x max|ref|, the bound of the Kuleshov
    inference tests: the same accumulation chain), and within 2e-6 x max|ref| (the project's bound for new backward kernels) the
    weight gradient and the data gradient of the same variants (stride 2 with both input parities, so that positions 0 and last
    and the rows no output reaches are compared), the statistics, the three apply kernels, the shuffle-addressed BatchNorm
    backward, the skip sum, the bottleneck's gradient, the Linear gradients at 1, 33 and 130 rows, final_conv, down_conv0, and
    every bounded reduction inside its grown-chunk regime (shapes from CHUNKS x MAX_PARTIALS; the wide weight gradient on the
    narrowest layer, 128 -> 256, 33 taps);
  * every case of tests/golden/f31_kuleshov_training.npz through the route under the tolerance rule of
    tests/test_kuleshov_training_cpu.py (float64 autograd with the route's decisions and masks; where the decisions are
    float64's, also the reference's own fp32 results, which may be left out on one case at the most);
  * the 'aten' route with the same masks patched in under the same rule, bitwise repeatability, different `dropout_call`s, train
    mode under no_grad, the eval-mode blob after an optimizer step, the default route, the error contract, and main.py
    model=kuleshov kuleshov_train=True evaluate=False twice on both routes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
import kuleshov_training_inputs as ti
from test_kuleshov_training_cpu import aten_step, check_against_reference_fp32, check_step, make_net

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_BOUND, FORWARD_BOUND = 2e-6, 1e-5
# (cin, cout, taps, stride) of the eight wide convolutions (down 3 and the bottleneck share one)
CONV_VARIANTS = [(128, 256, 33, 2), (256, 512, 17, 2), (512, 512, 9, 2), (512, 1024, 9, 1), (512, 1024, 17, 1), (512, 512, 33, 1), (256, 256, 65, 1)]
_errors, _same = {}, {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def g():
    return golden('f31_kuleshov_training')


@pytest.fixture(scope='module')
def engine(dev):
    from stofnet_amd.kuleshov_training import KuleshovTrainEngine
    e = KuleshovTrainEngine(dev, 700, 24)
    e.seed, e.call = ti.DROP_SEED, 1
    return e


def rel(a, ref, what=None):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(a).all() and a.shape == ref.shape, (a.shape, ref.shape)
    err = float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), 1e-300))
    if what is not None:
        _errors[what] = max(err, _errors.get(what, 0.0))
        print(f'{what}: {err:.3e}')
    return err


def gauss(dev, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def twice(fn):
    """fn() twice -> the first result, after asserting equal bits"""
    a, b = fn(), fn()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(u, v)
    return a


def ncl(t):
    """channel-last [N, L, C] device tensor -> float64 CPU [N, C, L]"""
    return t.detach().cpu().double().transpose(1, 2).contiguous()


def drop_of(engine, p=0.5):
    return (engine.seed, engine.call, 0, (p,) * 5)


def site_mask(n, C, T, site, p, engine):
    from stofnet_amd.kuleshov_training import dropout_keep
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    keep = np.stack([dropout_keep(engine.seed, engine.call, 0, site, row, T * C, p).reshape(T, C).T for row in range(n)])
    return torch.from_numpy(keep.astype(np.float64) * float(scale))


# ------------------------------------------------------------------------------------------------------- each kernel alone
@pytest.mark.parametrize('cin,cout,taps,stride', CONV_VARIANTS)
def test_conv_forward_weight_and_data_gradient_vs_torch(dev, engine, cin, cout, taps, stride):
    n, Lout = 2, 37                                             # M = 74: an M tail in every wave tile
    for Lin in ([stride * (Lout - 1) + taps] if stride == 1 else [2 * (Lout - 1) + taps, 2 * Lout + taps - 1]):      # stride 2: both parities
        tag = f'{cin}x{cout}k{taps}s{stride}'
        x, w, b = gauss(dev, 1, n, Lin, cin), gauss(dev, 2, cout, cin, taps) / np.sqrt(cin * taps), gauss(dev, 3, cout)
        dz = gauss(dev, 4, n, Lout, cout)
        x64, w64, b64 = ncl(x).requires_grad_(True), w.cpu().double().requires_grad_(True), b.cpu().double().requires_grad_(True)
        z64 = F.conv1d(x64, w64, b64, stride=stride)
        (z64 * ncl(dz)).sum().backward()
        frag = engine.pack_frag(w, 0)
        z = twice(lambda: engine.conv(x, Lin * cin, n, Lout, cin, cout, taps, stride, frag, b, 0))
        assert rel(ncl(z), z64, f'conv_fwd.{tag}') <= FORWARD_BOUND
        u = twice(lambda: engine.conv(x, Lin * cin, n, Lout, cin, cout, taps, stride, frag, b, 1))
        assert rel(ncl(u), F.leaky_relu(z64, 0.01), f'conv_fwd_slope.{tag}') <= FORWARD_BOUND

        def wgrad():
            dw, db = torch.empty_like(w), torch.empty_like(b)
            engine.conv_wgrad(x, Lin * cin, dz, cin, taps, stride, dw, db)
            return dw, db
        dw, db = twice(wgrad)
        assert rel(dw, w64.grad, f'conv_wgrad.{tag}') <= KERNEL_BOUND and rel(db, b64.grad, f'conv_bgrad.{tag}') <= KERNEL_BOUND
        frags = (engine.pack_frag(w, 1), None) if stride == 1 else (engine.pack_frag(w, 2), engine.pack_frag(w, 3))
        dx = twice(lambda: engine.conv_dgrad(dz, cin, taps, stride, frags[0], frags[1], Lin))
        assert rel(ncl(dx), x64.grad, f'conv_dgrad.{tag}') <= KERNEL_BOUND
        if Lin == 2 * Lout + taps - 1:
            assert not dx[:, -1].any() and dx[:, -2].any()                                  # the row that no output reaches is zero


def test_grown_chunks_conv_weight_gradient(dev, engine):
    """the wide weight gradient one row below, on and above CHUNKS x MAX_PARTIALS rows and inside the grown-chunk regime, on the
    narrowest layer (128 -> 256, 33 taps, stride 2)"""
    from stofnet_amd.kuleshov_training import CHUNKS, MAX_PARTIALS
    full = CHUNKS['conv_wgrad'] * MAX_PARTIALS['conv_wgrad']
    cin, cout, taps = 128, 256, 33
    w64 = torch.zeros(cout, cin, taps, dtype=torch.float64)
    for rows in (full - 1, full, full + 1, full + 401):
        n, Lout = (1, rows) if rows % 3 else (3, rows // 3)
        Lin = 2 * (Lout - 1) + taps
        x, dz = gauss(dev, rows, n, Lin, cin), gauss(dev, rows + 1, n, Lout, cout)
        ref_w, = torch.autograd.grad((F.conv1d(ncl(x), w64.requires_grad_(True), stride=2) * ncl(dz)).sum(), w64)

        def wgrad():
            dw, db = torch.empty(cout, cin, taps, device=dev), torch.empty(cout, device=dev)
            engine.conv_wgrad(x, Lin * cin, dz, cin, taps, 2, dw, db)
            return dw, db
        dw, db = twice(wgrad)
        assert rel(dw, ref_w, f'conv_wgrad.rows{rows}') <= KERNEL_BOUND
        assert rel(db, dz.cpu().double().sum((0, 1)), f'conv_bgrad.rows{rows}') <= KERNEL_BOUND


def test_grown_chunks_conv_bias_gradient(dev, engine):
    """the bias gradient of the wide convolutions (the column sums of dz, cut by the statistics' chunk rule) inside its grown-chunk
    regime, on the narrowest layer: every partial of its workspace region is filled and folded.  dw is checked for equal bits
    (its own regime is the test above)."""
    from stofnet_amd.kuleshov_training import CHUNKS, MAX_PARTIALS
    cin, cout, taps = 128, 256, 33
    rows = CHUNKS['stats'] * MAX_PARTIALS['stats'] + 300
    assert rows % 4 == 0
    n, Lout = 4, rows // 4
    Lin = 2 * (Lout - 1) + taps
    x, dz = gauss(dev, 40, n, Lin, cin), gauss(dev, 41, n, Lout, cout) + 0.25           # an offset: the sums do not cancel

    def wgrad():
        dw, db = torch.empty(cout, cin, taps, device=dev), torch.empty(cout, device=dev)
        engine.conv_wgrad(x, Lin * cin, dz, cin, taps, 2, dw, db)
        return dw, db
    dw, db = twice(wgrad)
    assert rel(db, dz.cpu().double().sum((0, 1)), f'conv_bgrad.rows{rows}') <= KERNEL_BOUND
    assert bool(torch.isfinite(dw).all()) and dw.any()


@pytest.mark.parametrize('rows_kind', ['small', 'grown'])
def test_statistics_apply_and_batchnorm_backward_vs_torch(dev, engine, rows_kind):
    from stofnet_amd.kuleshov_training import CHUNKS, MAX_PARTIALS
    ch = 256
    n, T = (3, 37) if rows_kind == 'small' else (3, (CHUNKS['stats'] * MAX_PARTIALS['stats'] + 300) // 3)
    z, gamma, beta = gauss(dev, 5, n, T, ch) * 1.5 + 0.3, gauss(dev, 6, ch), gauss(dev, 7, ch)
    rm, rv = gauss(dev, 8, ch), gauss(dev, 9, ch).abs() + 0.5
    z64 = ncl(z).requires_grad_(True)
    g64, b64 = gamma.cpu().double().requires_grad_(True), beta.cpu().double().requires_grad_(True)
    mean, var = z64.mean((0, 2), keepdim=True), z64.var((0, 2), unbiased=False, keepdim=True)
    bn64 = (z64 - mean) / torch.sqrt(var + engine.eps) * g64.view(1, -1, 1) + b64.view(1, -1, 1)
    m = n * T
    stat, nm, nv = twice(lambda: engine.stats(z, gamma, beta, rm, rv, 0.1))
    assert rel(nm, 0.9 * rm.cpu().double() + 0.1 * mean.detach().reshape(-1), f'stats_mean.{rows_kind}') <= KERNEL_BOUND
    assert rel(nv, 0.9 * rv.cpu().double() + 0.1 * var.detach().reshape(-1) * m / (m - 1), f'stats_var.{rows_kind}') <= KERNEL_BOUND
    # down: a = leaky0.2(u s + t) into rows 5 .. of a wider buffer
    buf = torch.zeros(n, T + 5, ch, device=dev)
    engine.apply_down(z, stat, buf[:, 5:], buf.stride(0))
    assert rel(ncl(buf[:, 5:]), F.leaky_relu(bn64, 0.2), f'apply_down.{rows_kind}') <= KERNEL_BOUND and not buf[:, :5].any()
    # up: a = (z s + t) keep scale at the shuffled address, in front of 3 skip rows
    mk = site_mask(n, ch, T, 2, 0.5, engine)
    cat = torch.zeros(n, 2 * T + 3, ch // 2, device=dev)
    engine.apply_up(z, stat, drop_of(engine), 2, cat, cat.stride(0))
    shuffled = lambda v: v.view(n, ch // 2, 2, T).transpose(2, 3).reshape(n, ch // 2, 2 * T)      # noqa: E731
    a64 = shuffled(bn64 * mk)
    assert rel(ncl(cat[:, :2 * T]), a64, f'apply_up.{rows_kind}') <= KERNEL_BOUND and not cat[:, 2 * T:].any()
    # the shuffle-addressed BatchNorm backward
    dcat = gauss(dev, 10, n, 2 * T + 3, ch // 2)
    (a64 * ncl(dcat[:, :2 * T])).sum().backward()

    def bwd():
        dg, db = torch.empty(ch, device=dev), torch.empty(ch, device=dev)
        gz = engine.gather_up(dcat, n, T, ch, drop_of(engine), 2)
        return engine.bn_bwd(gz, z, stat, 0, dg, db), dg, db
    dz, dg, db = twice(bwd)
    assert rel(ncl(dz), z64.grad, f'bn_bwd_up_dz.{rows_kind}') <= KERNEL_BOUND
    assert rel(dg, g64.grad, f'bn_bwd_up_dgamma.{rows_kind}') <= KERNEL_BOUND and rel(db, b64.grad, f'bn_bwd_up_dbeta.{rows_kind}') <= KERNEL_BOUND


def test_down_block_backward_skip_sum_then_both_leaky_decisions(dev, engine):
    n, T, ch = 2, 41, 128
    pre, gamma, beta = gauss(dev, 11, n, T, ch), gauss(dev, 12, ch), gauss(dev, 13, ch)
    u = F.leaky_relu(pre, 0.01)
    ones, zeros = torch.ones(ch, device=dev), torch.zeros(ch, device=dev)
    stat, _, _ = engine.stats(u, gamma, beta, zeros, ones, 0.1)
    cat = torch.zeros(n, T + 6, ch, device=dev)
    engine.apply_down(u, stat, cat[:, 6:], cat.stride(0))
    dcat, dnext = gauss(dev, 14, n, T + 6, ch), gauss(dev, 15, n, T, ch)
    p64 = ncl(pre).requires_grad_(True)
    u64 = F.leaky_relu(p64, 0.01)
    mean, var = u64.mean((0, 2), keepdim=True), u64.var((0, 2), unbiased=False, keepdim=True)
    a64 = F.leaky_relu((u64 - mean) / torch.sqrt(var + engine.eps) * gamma.cpu().double().view(1, -1, 1) + beta.cpu().double().view(1, -1, 1), 0.2)
    assert torch.equal(ncl(cat[:, 6:]) > 0, a64 > 0)
    total = dcat[:, 6:] + dnext                                 # the fp32 sum, skip rows' part first
    (a64 * ncl(total)).sum().backward()

    def bwd():
        dg, db = torch.empty(ch, device=dev), torch.empty(ch, device=dev)
        gd = engine.gather_down(dcat[:, 6:], dnext, cat[:, 6:])
        return engine.bn_bwd(gd, u, stat, 1, dg, db), gd
    dz, gd = twice(bwd)
    assert torch.equal(gd, torch.where(cat[:, 6:] > 0, total, (0.2 * total.double()).float()))
    assert rel(ncl(dz), p64.grad, 'bn_bwd_down_dz') <= KERNEL_BOUND
    only = engine.gather_down(dcat[:, 6:], None, cat[:, 6:])
    assert torch.equal(only, torch.where(cat[:, 6:] > 0, dcat[:, 6:], (0.2 * dcat[:, 6:].double()).float()))


def test_bottleneck_dropout_and_its_gradient(dev, engine):
    n, B = 3, 13
    for p in (0.5, 0.1, 0.0):
        z, gr = gauss(dev, 16, n, B, 512), gauss(dev, 17, n, B, 512)
        mk = site_mask(n, 512, B, 0, p, engine)
        z64 = ncl(z).requires_grad_(True)
        a64 = F.leaky_relu(z64 * mk, 0.2)
        (a64 * ncl(gr)).sum().backward()
        a = twice(lambda: engine.apply_bott(z, drop_of(engine, p)))
        assert rel(ncl(a), a64, f'apply_bott.p{p}') <= KERNEL_BOUND
        dz = twice(lambda: engine.gather_bott(gr, z, drop_of(engine, p)))
        assert rel(ncl(dz), z64.grad, f'gather_bott.p{p}') <= KERNEL_BOUND
        assert abs(float((a == 0).float().mean()) - p) < 0.02


@pytest.mark.parametrize('rows', [1, 33, 130])
def test_linear_gradients_vs_torch(dev, rows):
    from stofnet_amd.kuleshov_training import KuleshovTrainEngine
    e = KuleshovTrainEngine(dev, 641, 77)
    K2, kp = e.d['fc_dim'], (e.d['fc_dim'] + 7) // 8 * 8
    assert K2 % 8                                               # the padded tail of flat is live in this shape
    flat = torch.zeros(rows, kp, device=dev)
    flat[:, :K2] = gauss(dev, 18, rows, K2)
    w, dy = gauss(dev, 19, 77, K2) / np.sqrt(K2), gauss(dev, 20, rows, 77)

    def bwd():
        dw, db = torch.empty_like(w), torch.empty(77, device=dev)
        return e.fc_bwd(dy, flat, w, dw, db), dw, db
    dflat, dw, db = twice(bwd)
    d64 = dy.cpu().double()
    assert rel(dflat[:, :K2], d64 @ w.cpu().double(), f'fc_dflat.rows{rows}') <= KERNEL_BOUND and not dflat[:, K2:].any()
    assert rel(dw, d64.t() @ flat[:, :K2].cpu().double(), f'fc_dw.rows{rows}') <= KERNEL_BOUND
    assert rel(db, d64.sum(0), f'fc_db.rows{rows}') <= KERNEL_BOUND
    # the forward tail on the device-packed images: final_conv + output_fc
    cat3 = gauss(dev, 21, rows, e.d['cat'][3], 128)
    wf, bf, bfc = gauss(dev, 22, 2, 128, 9) / 34.0, gauss(dev, 23, 2), gauss(dev, 24, 77)
    fl, y = twice(lambda: e.tail(cat3, e.pack_final(wf), bf, e.pack_fc(w), bfc))
    o64 = F.conv1d(ncl(cat3), wf.cpu().double(), bf.cpu().double())
    f64 = o64.transpose(1, 2).reshape(rows, -1)
    assert rel(fl[:, :K2], f64, f'tail_flat.rows{rows}') <= FORWARD_BOUND and not fl[:, K2:].any()
    assert rel(y, F.linear(f64, w.cpu().double(), bfc.cpu().double()), f'tail_y.rows{rows}') <= FORWARD_BOUND


@pytest.mark.parametrize('n,L', [(2, 641), (3, 700), (1, 0)])
def test_final_conv_and_down0_backward_vs_torch(dev, n, L):
    """(1, 0): the shape that puts both chunked reductions into their grown-chunk regime"""
    from stofnet_amd.kuleshov_training import CHUNKS, MAX_PARTIALS, KuleshovTrainEngine
    if L == 0:
        L = 2 * (CHUNKS['down0_wgrad'] * MAX_PARTIALS['down0_wgrad'] + 100) + 65
    e = KuleshovTrainEngine(dev, L, 8)
    Lc, Fo, kp = e.d['cat'][3], e.d['final'], (e.d['fc_dim'] + 7) // 8 * 8
    tag = f'{n}x{L}'
    cat3, wf = gauss(dev, 25, n, Lc, 128), gauss(dev, 26, 2, 128, 9) / 34.0
    dflat = torch.zeros(n, kp, device=dev)
    dflat[:, :2 * Fo] = gauss(dev, 27, n, 2 * Fo)
    c64, w64, b64 = ncl(cat3).requires_grad_(True), wf.cpu().double().requires_grad_(True), torch.zeros(2, dtype=torch.float64, requires_grad=True)
    o64 = F.conv1d(c64, w64, b64)
    (o64.transpose(1, 2).reshape(n, -1) * dflat[:, :2 * Fo].cpu().double()).sum().backward()

    def fbwd():
        dw, db = torch.empty_like(wf), torch.empty(2, device=dev)
        return e.final_bwd(dflat, cat3, wf, dw, db), dw, db
    dcat, dw, db = twice(fbwd)
    assert rel(ncl(dcat), c64.grad, f'final_dgrad.{tag}') <= KERNEL_BOUND
    assert rel(dw, w64.grad, f'final_wgrad.{tag}') <= KERNEL_BOUND and rel(db, b64.grad, f'final_bgrad.{tag}') <= KERNEL_BOUND
    # down_conv0 on a frame longer than L: forward, weight gradient, dx (zero behind the first L samples is the engine's job)
    x, w0, b0 = gauss(dev, 28, n, L + 3), gauss(dev, 29, 128, 1, 65) / 8.0, gauss(dev, 30, 128)
    D0 = e.d['down'][0]
    dz = gauss(dev, 31, n, D0, 128)
    x64 = x[:, :L].cpu().double().unsqueeze(1).requires_grad_(True)
    w064, b064 = w0.cpu().double().requires_grad_(True), b0.cpu().double().requires_grad_(True)
    z64 = F.conv1d(x64, w064, b064, stride=2)
    (z64 * ncl(dz)).sum().backward()
    u = twice(lambda: e.down0(x, w0, b0))
    assert rel(ncl(u), F.leaky_relu(z64, 0.01), f'down0_fwd.{tag}') <= FORWARD_BOUND

    def dbwd():
        dw, db, dx = torch.empty_like(w0), torch.empty(128, device=dev), torch.full((n, L + 3), 7.0, device=dev)
        e.down0_bwd(x, dz, w0, dw, db, dx)
        return dw, db, dx
    dw, db, dx = twice(dbwd)
    assert rel(dw, w064.grad, f'down0_wgrad.{tag}') <= KERNEL_BOUND and rel(db, b064.grad, f'down0_bgrad.{tag}') <= KERNEL_BOUND
    assert rel(dx[:, :L], x64.grad[:, 0], f'down0_dgrad.{tag}') <= KERNEL_BOUND and bool((dx[:, L:] == 7.0).all())


# --------------------------------------------------------------------------------------------------------- through the route
def route_decisions(y, L):
    sv, d = y.grad_fn.saved, ti.chain_lengths(L)
    return {'u': [(u > 0).transpose(1, 2).cpu().numpy() for u in sv.u],
            'a': [(sv.cat[3 - j][:, 2 * d['up'][3 - j]:, :] > 0).transpose(1, 2).cpu().numpy() for j in range(4)],
            'b': (sv.ab > 0).transpose(1, 2).cpu().numpy()}


def kernel_step(m, x, t, want_dx=True):
    x = x.clone().requires_grad_(want_dx)
    for p in m.parameters():
        p.grad = None
    y = m(x)
    assert type(y.grad_fn).__name__.startswith('KuleshovFunction')
    dec = route_decisions(y, m.input_length)
    (y * t).sum().backward()
    bns = m._batch_norms()
    return (y.detach(), None if x.grad is None else x.grad, {k: p.grad.clone() for k, p in m.named_parameters()},
            [b.running_mean.clone() for b in bns], [b.running_var.clone() for b in bns], dec)


def to_np(step):
    y, dx, grads, rm, rv, dec = step
    return (y.cpu().numpy(), dx.cpu().numpy(), {k: v.cpu().numpy() for k, v in grads.items()}, [v.cpu().numpy() for v in rm],
            [v.cpu().numpy() for v in rv], dec)


def case_tensors(name, dev):
    _, n, L, O, wseed, seed, p, call = ti.case(name)
    return torch.from_numpy(ti.frames(n, L, seed)).to(dev), torch.from_numpy(ti.cotangent(n, O, seed)).to(dev)


@pytest.mark.parametrize('name', ti.IDS)
def test_kernel_route_on_fixture_case(dev, g, name):
    m = make_net(name, 'kernels', dev, patched=False)
    x, t = case_tensors(name, dev)
    y, dx, grads, rm, rv, dec = to_np(kernel_step(m, x, t))
    assert m.dropout_call == ti.case(name)[7] + 1 and all(int(b.num_batches_tracked) == 1 for b in m._batch_norms())
    errs = {}
    _, same = check_step(name, g, y, dx, grads, rm, rv, dec, errs)
    _errors.update({f'route.{name}.{k}': v for k, v in errs.items() if k in ('y', 'dx') or k.endswith('.weight')})
    _same[name] = same
    if same:
        check_against_reference_fp32(name, g, y, dx, grads)


def test_reference_fp32_comparison_is_left_out_on_one_case_at_most(dev, g):
    for name in ti.IDS:                                         # a case the run above did not reach (-k, -x): run it here
        if name not in _same:
            test_kernel_route_on_fixture_case(dev, g, name)
    assert sum(not v for v in _same.values()) <= 1, _same


@pytest.mark.parametrize('name', ['ks_3x800_11', 'ks_2x700_1400'])
def test_aten_route_with_the_same_masks(dev, g, name):
    m = make_net(name, 'aten', dev, patched=True)
    x, t = case_tensors(name, dev)
    y, dx, grads, rm, rv, dec = aten_step(m, x, t)
    check_step(name, g, y, dx, grads, rm, rv, dec)
    assert m.dropout_call == ti.case(name)[7]


def test_two_runs_are_bitwise_equal_and_calls_differ(dev):
    name = 'ks_call3_2x660_16'
    x, t = case_tensors(name, dev)
    a = kernel_step(make_net(name, 'kernels', dev, patched=False), x, t)
    m = make_net(name, 'kernels', dev, patched=False)
    b = kernel_step(m, x, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert all(torch.equal(u, v) for u, v in zip(a[3] + a[4], b[3] + b[4]))
    assert m.dropout_call == 4
    c = kernel_step(m, x, t)                                    # the next call draws other masks
    assert not torch.equal(a[0], c[0])
    m.dropout_call = 3
    m2 = make_net(name, 'kernels', dev, patched=False)
    m2.load_state_dict(m.state_dict())
    d, e = kernel_step(m, x, t), kernel_step(m2, x, t)           # ... and the same (seed, call) the same ones again
    assert torch.equal(d[0], e[0]) and all(torch.equal(d[2][k], e[2][k]) for k in d[2])
    m2.dropout_seed, m2.dropout_call = ti.DROP_SEED + 1, 3
    assert not torch.equal(kernel_step(m2, x, t)[0], e[0])


def test_default_seed_is_torchs_initial_seed(dev):
    name = 'ks_2x641_8'
    x, _ = case_tensors(name, dev)
    m = make_net(name, 'kernels', dev, patched=False)
    m.dropout_seed = None
    torch.manual_seed(4242)
    with torch.no_grad():
        y = m(x)
    assert m.dropout_seed == 4242 and m.dropout_call == 1
    m2 = make_net(name, 'kernels', dev, patched=False)
    m2.dropout_seed = 4242
    with torch.no_grad():
        assert torch.equal(m2(x), y)


def test_train_mode_under_no_grad_moves_the_same_statistics(dev):
    name = 'ks_3x800_11'
    x, t = case_tensors(name, dev)
    ref = kernel_step(make_net(name, 'kernels', dev, patched=False), x, t)
    m = make_net(name, 'kernels', dev, patched=False)
    with torch.no_grad():
        y = m(x)
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, ref[0])
    bns = m._batch_norms()
    assert all(torch.equal(b.running_mean, u) and torch.equal(b.running_var, v) for b, u, v in zip(bns, ref[3], ref[4]))
    assert all(int(b.num_batches_tracked) == 1 for b in bns)


def test_eval_mode_after_an_optimizer_step_is_a_fresh_module(dev):
    """The stale-blob trap: after an AdamW step over all parameters and the new running statistics, eval-mode model(x) equals a
    fresh module loaded from the state_dict, bitwise."""
    from stofnet_amd import Kuleshov
    name = 'ks_2x641_8'
    x, t = case_tensors(name, dev)
    m = make_net(name, 'kernels', dev, patched=False)
    m.eval()
    with torch.no_grad():
        before = m(x)                                           # packs the eval-mode blob
        assert torch.equal(before, m.forward_kernels(x))
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    kernel_step(m, x, t, want_dx=False)
    opt.step()
    m.eval()
    fresh = Kuleshov(m.input_length, m.output_length).to(dev)
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh.eval()
    with torch.no_grad():
        after = m(x)
        assert not torch.equal(after, before) and torch.equal(after, fresh(x))
    assert int(m.down_bn0.num_batches_tracked) == 1 and fresh.train_route == 'aten'


def test_default_route_is_aten_and_errors_raise(dev):
    name = 'ks_2x641_8'
    x, t = case_tensors(name, dev)
    m = make_net(name, 'aten', dev, patched=False)
    y = m(x)
    assert y.grad_fn is not None and not type(y.grad_fn).__name__.startswith('KuleshovFunction') and m.dropout_call == 0
    m.train_route = 'kernels'
    y, dx, grads, *_ = kernel_step(m, x, t, want_dx=False)
    assert dx is None and len(grads) == 38 and all(v is not None for v in grads.values())
    long = torch.cat((x, torch.ones(2, 1, 5, device=dev)), -1)  # rows longer than input_length are cropped; dx is zero behind
    m.dropout_call = 0
    yl, dxl, *_ = kernel_step(m, long, t)
    assert torch.equal(yl, y) and dxl.shape == long.shape and not dxl[:, :, 641:].any() and dxl[:, :, :641].any()
    loss = m(x).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()
    loss = m(x).sum()
    with torch.no_grad():
        m.up_conv2.weight.mul_(1.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        loss.backward()
    before = [b.clone() for b in m.buffers()]
    calls = m.dropout_call
    with pytest.raises(RuntimeError):
        m(x[:, :, :640])
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        m(x[:1])
    with pytest.raises(TypeError):
        m(x.double())
    with pytest.raises(RuntimeError):
        m(x.cpu())
    m.up_do1.p = 1.0
    with pytest.raises(ValueError, match='Dropout p'):
        m(x)
    m.up_do1.p = 0.5
    m.up_bn3.eps = 1e-3
    with pytest.raises(RuntimeError):
        m(x)
    m.up_bn3.eps = 1e-5
    assert m.dropout_call == calls and all(torch.equal(u, v) for u, v in zip(before, m.buffers()))      # none of them touched a thing


# ------------------------------------------------------------------------------------------------------------ main.py
def run_main_training(tmp_path, run, route):
    ck = tmp_path / run
    code = ('import sys, json; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[2:]); print(json.dumps(s))')
    res = subprocess.run([sys.executable, '-c', code, ROOT, 'model=kuleshov', 'kuleshov_train=True', 'evaluate=False', f'train_route={route}',
                          f'ckpt_dir={ck}', f'run_name={run}', 'epochs=1', 'batch_size=2', 'upsample_factor=2', 'num_waveforms=6',
                          'num_samples=700', 'seed=5'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1]), sorted(ck.iterdir())


@pytest.mark.parametrize('route', ['kernels', 'aten'])
def test_main_entry_point_trains_kuleshov_twice_alike(dev, tmp_path, route):
    from stofnet_amd import Kuleshov
    sds, summaries = [], []
    for k in range(2):
        summary, paths = run_main_training(tmp_path, f'kstest{os.getpid()}{route}{k}', route)
        hist = summary['train_history']
        assert summary['model'] == 'kuleshov' and summary['train_route'] == route and summary['train_precision'] == 'fp32' and len(hist) == 1
        assert all(np.isfinite(h['train_loss']) and np.isfinite(h['val_loss']) for h in hist)
        assert len(paths) == 1 and paths[0].name.endswith('_epoch_1.pth')
        sd = torch.load(str(paths[0]), map_location='cpu', weights_only=True)
        Kuleshov(700, 1400).load_state_dict(sd, strict=True)
        assert int(sd['up_bn3.num_batches_tracked']) == 2
        sds.append(sd)
        summaries.append(json.dumps({k2: v for k2, v in summary.items() if 'time' not in k2 and 'per_s' not in k2}, sort_keys=True))
    assert summaries[0] == summaries[1]                         # everything but the measured times
    assert all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])


def test_zz_record_profile(dev):
    """the achieved figures of this run, for profiles/kuleshov_training.jsonl (printed; the file is written by hand from a run)"""
    print(json.dumps({k: float(f'{v:.3e}') for k, v in sorted(_errors.items())}))

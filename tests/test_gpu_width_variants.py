"""StofNet at other widths on the GPU (models/stofnet.py:11: num_features 1..256, in_channels 1..16): the generic-width
conv1 / up-sample-backward kernels alone against float64 torch, then inference, the autograd boundary and StofNetTrainer
on every case of golden `f25_width_variants` (the reference's own output and autograd gradients)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from width_variants import WIDTH_VARIANTS, rel, width_case, width_input
from oracle import train_oracle as to

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def lib():
    from stofnet_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


def _conv1_reference(N, Cin, L, Fw):
    """float64 truth of relu(conv1(x)) and of its gradients for out_scale = 0.25; the pre-activation takes both signs."""
    gen = torch.Generator().manual_seed(1000 * Cin + Fw + L)
    x = torch.randn(N, Cin, L, generator=gen, dtype=torch.float64).float().double().requires_grad_()
    w = (torch.randn(Fw, Cin, 9, generator=gen, dtype=torch.float64) / (3.0 * Cin ** 0.5)).float().double().requires_grad_()
    b = (0.2 * torch.randn(Fw, generator=gen, dtype=torch.float64)).float().double().requires_grad_()
    pre = F.conv1d(x, w, b, padding=4)
    assert (pre > 0).any() and (pre < 0).any()
    y = torch.relu(pre).detach().permute(0, 2, 1).contiguous()                       # [N, L, F]
    saved = y.float()                                                                # what the backward kernels mask with
    g = torch.randn(N, L, Fw, generator=gen, dtype=torch.float64).float()
    gm = (g.double() * (saved > 0)).permute(0, 2, 1)
    dx, dw, db = torch.autograd.grad(pre, [x, w, b], gm)
    return x.detach().float(), w.detach().float(), b.detach().float(), y, saved, g, 0.25 * dx, 0.25 * dw, 0.25 * db


@pytest.mark.parametrize('N,Cin,L,Fw', [(3, 1, 171, 64),        # 513 rows: cross the chunk edges
                                        (2, 2, 5, 24),          # rows shorter than the taps
                                        (1, 3, 130, 96), (2, 16, 70, 16), (1, 5, 64, 256)])
def test_conv1_c_kernels_vs_torch(lib, N, Cin, L, Fw):
    """stof_train_conv1_c / _wgrad / _dgrad alone against float64 torch at the bound of test_conv_kernels_vs_torch."""
    from stofnet_amd import _lib
    st = _lib.stream_ptr(torch.device(DEV))
    x, w, b, y_ref, saved, g, dx_ref, dw_ref, db_ref = _conv1_reference(N, Cin, L, Fw)
    xd, wd, bd, sd, gd = (t.to(DEV).contiguous() for t in (x, w, b, saved, g))
    y = torch.full((N, L, Fw), float('nan'), device=DEV)
    _lib.check(lib.stof_train_conv1_c(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), N, Cin, L, Fw, st), 'conv1_c')
    err = rel(y.cpu().numpy(), y_ref.numpy())
    print('conv1_c', (N, Cin, L, Fw), err)
    assert err < 2e-6
    nbytes = lib.stof_train_conv1_c_wgrad_workspace_bytes(Cin, Fw)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        dw, db = torch.full((Fw, Cin, 9), float('nan'), device=DEV), torch.full((Fw,), float('nan'), device=DEV)
        ws.fill_(0xff)                                      # NaN patterns: a partial that is read must have been written
        _lib.check(lib.stof_train_conv1_c_wgrad(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(sd), _lib.ptr(dw), _lib.ptr(db), N, Cin, L, Fw, 0.25,
                                                _lib.ptr(ws), ws.numel(), st), 'conv1_c_wgrad')
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # no float atomics
    errs = rel(runs[0][0].cpu().numpy(), dw_ref.numpy()), rel(runs[0][1].cpu().numpy(), db_ref.numpy())
    print('conv1_c_wgrad', errs)
    assert errs[0] < 2e-6 and errs[1] < 2e-6
    dx = torch.full((N, Cin, L), float('nan'), device=DEV)
    _lib.check(lib.stof_train_conv1_c_dgrad(_lib.ptr(gd), _lib.ptr(sd), _lib.ptr(wd), _lib.ptr(dx), N, Cin, L, Fw, 0.25, st), 'conv1_c_dgrad')
    err = rel(dx.cpu().numpy(), dx_ref.numpy())
    print('conv1_c_dgrad', err)
    assert err < 2e-6


@pytest.mark.parametrize('N,L,P,S,C,rem_half', [(2, 44, 2, 20, 24, 2), (1, 10, 5, 2, 1, 0), (3, 260, 1, 256, 96, 2), (2, 160, 2, 80, 64, 0)])
def test_upsample_bwd_c_vs_torch(lib, N, L, P, S, C, rem_half):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(torch.device(DEV))
    gen = torch.Generator().manual_seed(L * 7 + C)
    g = torch.randn(N, L, C, generator=gen)
    e = torch.randn(N, P, C, generator=gen)
    ref = g.double()[:, rem_half:rem_half + P * S].reshape(N, P, S, C).sum(2) * torch.where(e > 0, 1.0, 0.01).double()
    ge = torch.full((N, P, C), float('nan'), device=DEV)
    gd, ed = g.to(DEV), e.to(DEV)
    _lib.check(lib.stof_train_upsample_bwd_c(_lib.ptr(gd), _lib.ptr(ed), _lib.ptr(ge), N, L, P, rem_half, S, C, st), 'upsample_bwd_c')
    err = rel(ge.cpu().numpy(), ref.numpy())
    print('upsample_bwd_c', err)
    assert err < 2e-6
    if C == 64:                                             # the 64-channel kernel computes the same map
        ge64 = torch.empty_like(ge)
        _lib.check(lib.stof_train_upsample_bwd(_lib.ptr(gd), _lib.ptr(ed), _lib.ptr(ge64), N, L, P, rem_half, S, st), 'upsample_bwd')
        assert rel(ge64.cpu().numpy(), ref.numpy()) < 2e-6


def test_new_entry_points_validate_their_arguments(lib):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(torch.device(DEV))
    buf = torch.ones(4096, device=DEV)
    p = _lib.ptr(buf)
    BAD, UNS = _lib.STOF_ERR_BAD_ARG, _lib.STOF_ERR_UNSUPPORTED
    assert lib.stof_train_conv1_c(p, p, p, p, 1, 17, 8, 8, st) == BAD and lib.stof_train_conv1_c(p, p, p, p, 1, 1, 8, 257, st) == BAD
    assert lib.stof_train_conv1_c(p, p, p, p, 1, 0, 8, 8, st) == BAD and lib.stof_train_conv1_c(None, p, p, p, 1, 1, 8, 8, st) == BAD
    assert lib.stof_train_conv1_c(None, None, None, None, 0, 2, 8, 8, st) == 0
    assert lib.stof_train_conv1_c(p, p, p, p, 1 << 20, 2, 1 << 12, 8, st) == UNS
    assert lib.stof_train_conv1_c_wgrad_workspace_bytes(17, 8) == 0 and lib.stof_train_conv1_c_wgrad_workspace_bytes(2, 0) == 0
    assert lib.stof_train_conv1_c_wgrad(p, p, p, None, p, 1, 2, 8, 8, 1.0, p, 1 << 30, st) == BAD
    assert lib.stof_train_conv1_c_wgrad(p, p, p, p, p, 1, 2, 8, 8, 1.0, p, 16, st) == _lib.STOF_ERR_WORKSPACE
    assert lib.stof_train_conv1_c_wgrad(p, p, p, p, p, 1 << 20, 2, 1 << 12, 8, 1.0, p, 1 << 30, st) == UNS
    dw, db = torch.ones(8, 2, 9, device=DEV), torch.ones(8, device=DEV)
    assert lib.stof_train_conv1_c_wgrad(None, None, None, _lib.ptr(dw), _lib.ptr(db), 0, 2, 8, 8, 1.0, None, 0, st) == 0
    assert not dw.any() and not db.any()
    assert lib.stof_train_conv1_c_dgrad(p, p, p, None, 1, 2, 8, 8, 1.0, st) == BAD
    assert lib.stof_train_conv1_c_dgrad(p, p, p, p, 1, 2, 8, 300, 1.0, st) == BAD
    assert lib.stof_train_conv1_c_dgrad(None, None, None, None, 0, 2, 8, 8, 1.0, st) == 0
    assert lib.stof_train_conv1_c_dgrad(p, p, p, p, 1 << 20, 2, 1 << 12, 8, 1.0, st) == UNS
    assert lib.stof_train_upsample_bwd_c(p, p, p, 1, 10, 5, 1, 2, 4, st) == BAD            # window past the row
    assert lib.stof_train_upsample_bwd_c(p, p, p, 1, 10, 5, 0, 2, 0, st) == BAD and lib.stof_train_upsample_bwd_c(p, None, p, 1, 10, 5, 0, 2, 4, st) == BAD
    assert lib.stof_train_upsample_bwd_c(None, None, None, 0, 10, 5, 0, 2, 4, st) == 0
    assert lib.stof_train_upsample_bwd_c(p, p, p, 1 << 20, 1 << 12, 5, 0, 2, 4, st) == UNS


def _loaded(name, **kw):
    from stofnet_amd import StofNet
    var, _, params, x, t, y_ref, dx_ref, grads_ref = width_case(name)
    m = StofNet(**var['ctor'], **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return var, m.to(DEV), params, x, t, y_ref, dx_ref, grads_ref


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('name', list(WIDTH_VARIANTS))
def test_gpu_forward_matches_reference(name, precision):
    var, m, params, x, t, y_ref, _, _ = _loaded(name, precision=precision)
    m.eval()
    with torch.no_grad():
        y = m(torch.from_numpy(x).to(DEV))
    assert y.shape == y_ref.shape and y.dtype == torch.float32
    err = rel(y.cpu().numpy(), y_ref)
    print(name, precision, 'y', err)
    assert err < 2e-5
    m.raise_if_overflow()


@pytest.mark.parametrize('tp,tol', [('fp32', 2e-4), ('f16x3', 2e-3)])
@pytest.mark.parametrize('name', list(WIDTH_VARIANTS))
def test_gpu_gradients_match_reference_autograd(name, tp, tol):
    """Train-mode forward + backward through the autograd boundary: d loss / d x [N, in_channels, L] and every kept
    parameter gradient against the reference's autograd."""
    var, m, params, x, t, y_ref, dx_ref, grads_ref = _loaded(name, train_precision=tp)
    m.train()
    xg = torch.from_numpy(x).to(DEV).requires_grad_()
    y = m(xg)
    assert y.grad_fn is not None and y.shape == y_ref.shape
    assert rel(y.detach().cpu().numpy(), y_ref) < 2e-5
    (y * torch.from_numpy(t).to(DEV)).sum().backward()
    m.raise_if_overflow()
    assert xg.grad.shape == xg.shape
    errs = {'dx': rel(xg.grad.cpu().numpy(), dx_ref)}
    named = dict(m.named_parameters())
    assert all(p.grad is not None and p.grad.shape == p.shape for p in named.values())
    assert grads_ref
    for n, gr in grads_ref.items():
        errs[n] = rel(named[n].grad.cpu().numpy(), gr)
    print(name, tp, errs)
    for n, e in errs.items():
        assert e < tol, (n, e)


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-4), ('f16x3', 2e-3)])
@pytest.mark.parametrize('name', ['f32_c1_nb6_k3_sgs20_r4', 'f96_c2_nb5_k5_nosgb_r3'])
def test_trainer_loss_and_all_gradients_vs_autograd(name, precision, tol):
    """StofNetTrainer.forward_backward against torch autograd on the oracle in float64 with main.py's loss."""
    from stofnet_amd.training import StofNetTrainer
    var, m, params, x, _, _, _, _ = _loaded(name)
    c = var['ctor']
    r, n, L = c['upsample_factor'], var['N'], var['L']
    tr = StofNetTrainer(m, lr=5e-4, weight_decay=1e-8, precision=precision)
    assert (tr.F, tr.cin, tr.sweep) == (c['num_features'], c['in_channels'], False)
    rng = np.random.default_rng(5)
    gt = np.stack([np.sort(rng.integers(1, L * r, size=2)) for _ in range(n)])[:, None, :].astype(np.int64)
    gt[1, 0, 1] = 0                                                        # "no echo" placeholder (index 0 is cleared)
    loss_ref, grads_ref, pred_ref = to.loss_and_grads(params, x, gt, r, c['semi_global_scale'])
    loss, pred = tr.forward_backward(torch.from_numpy(x).to(DEV), torch.from_numpy(gt).to(DEV))
    assert rel(pred.cpu().numpy(), pred_ref) < 1e-5
    assert abs(float(loss) - loss_ref) < 1e-5 * abs(loss_ref)
    assert set(grads_ref) == set(tr.g)
    errs = {nm: rel(tr.g[nm].cpu().numpy(), gref) for nm, gref in grads_ref.items()}
    print(name, precision, errs)
    for nm, e in errs.items():
        assert tr.g[nm].shape == grads_ref[nm].shape
        assert e < tol, (nm, e)
    loss2, _ = tr.train_step(torch.from_numpy(x).to(DEV), torch.from_numpy(gt).to(DEV))      # AdamW on the flat buffer
    tr.raise_if_overflow()
    assert abs(float(loss2) - loss_ref) < 1e-5 * abs(loss_ref)
    assert float(tr.loss(pred, torch.from_numpy(gt).to(DEV))) == pytest.approx(loss_ref, rel=1e-5)


def test_sweep_look_alike_with_two_channels_runs_layer_by_layer():
    from stofnet_amd.mask2samples import onset_indices
    var, m, params, x, _, y_ref, _, _ = _loaded('f64_c2_nb13_k7_sgs80_r4', precision='f16x3', train_precision='f16x3')
    assert not m._fused_sweep()
    assert not m._engine(torch.device(DEV), 'f16x3').sweep and not m._engine(torch.device(DEV), 'fp32').sweep
    m.eval()
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        y = m(xd)
        counts, idx = m.forward_onsets(xd)
    assert rel(y.cpu().numpy(), y_ref) < 2e-5
    c_ref, i_ref = onset_indices(y, 20, None)
    assert torch.equal(counts, c_ref) and torch.equal(idx, i_ref)

"""WaveUnet training, the parts that need no GPU:

  * `WaveUnet.forward_aten` on the CPU in train mode against tests/golden/f30_waveunet_training.npz: y, the running statistics
    and num_batches_tracked on every case, dx and every parameter gradient on the cases with N L >= 128; in fp32 under the
    tolerance rule, in float64 to 1e-10 of `waveunet_training_inputs.restate64` (which the generator asserts to be the
    reference's float64 module);
  * the inputs module reproduces the stored seeds and shapes;
  * the route contract of `WaveUnet.train_route` that needs no device;
  * `main.py model=unet evaluate=False` trains (device=cpu, train_route=aten);
  * the interpolation transpose: the window of wu_interp_window (csrc/waveunet_net.h, through the host entry
    stof_waveunet_interp_table) holds every high position that lands on a low one, l0 + l1 == 1 exactly, and the weights a gather
    over the windows collects are, bit for bit, the transposed dense fp32 interpolation matrix.

Tolerance rule: |ours - ref64| <= max(B max|ref64|, 8 dev_T), dev_T the reference's own fp32-vs-float64 deviation of tensor T
(stored); B = 2e-5 for y and the running statistics, 2e-4 for dx and the gradients.  For the conv bias gradients of the blocks
(analytically 0 under train-mode BatchNorm) dev_T is the largest of eight of the reference's own noise samples.  ref64 is float64
autograd of the restated network with the decisions (BatchNorm output > 0) of the run under test."""
import json

import numpy as np
import pytest
import torch

from conftest import golden
import waveunet_training_inputs as ti

Y_BOUND, GRAD_BOUND = 2e-5, 2e-4


@pytest.fixture(scope='module')
def g():
    return golden('f30_waveunet_training')


def bn_layers(m):
    return [b.main[1] for b in m.encoder] + [m.middle[1]] + [b.main[1] for b in m.decoder]


def make_net(sd, n_layers, route='aten', dev='cpu', dtype=torch.float32):
    from stofnet_amd import WaveUnet
    m = WaveUnet(n_layers, 16)
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


_own = {}


def own64(name):
    """float64 autograd of case `name` with its own decisions, computed once"""
    if name not in _own:
        _, nl, wseed, n, L, seed = ti.case(name)
        _own[name] = ti.restate64(ti.weights(nl, wseed), nl, ti.frames(n, L, seed), ti.cotangent(n, L, seed))
    return _own[name]


def check_step(name, g, y, dx, grads, run_mean, run_var, decisions, errs=None):
    """The whole comparison of one step of case `name` (numpy arrays; decisions per block [N, C, L_level]) with float64 autograd
    taken with those decisions.  -> the float64 runs (own decisions, the given ones)."""
    _, nl, wseed, n, L, seed = ti.case(name)
    own = own64(name)
    same = all(np.array_equal(a, b) for a, b in zip(decisions, own['decisions']))
    routed = own if same else ti.restate64(ti.weights(nl, wseed), nl, ti.frames(n, L, seed), ti.cotangent(n, L, seed), decisions)
    # a decision that differs from float64's lies within the stored margin; no more of them than float64 alone counts there
    for b in range(2 * nl + 1):
        differ = decisions[b] != own['decisions'][b]
        assert (np.abs(own['bn_out'][b][differ]) < ti.MARGIN * g[f'{name}.bn_dev'][b]).all(), (name, b)
        assert int(differ.sum()) <= int(g[f'{name}.near'][b]), (name, b, int(differ.sum()))
    check_rule(name, 'y', y, routed['y'], g, Y_BOUND, errs)
    for b in range(2 * nl + 1):
        check_rule(name, f'run_mean.{b}', run_mean[b], routed['run_mean'][b], g, Y_BOUND, errs)
        check_rule(name, f'run_var.{b}', run_var[b], routed['run_var'][b], g, Y_BOUND, errs)
    assert np.isfinite(dx).all() and all(np.isfinite(v).all() for v in grads.values())
    if name in ti.GRAD_IDS:
        check_rule(name, 'dx', dx, routed['dx'], g, GRAD_BOUND, errs)
        for p in ti.params(nl):
            check_rule(name, f'grad.{p}', np.asarray(grads[p]).reshape(routed['grads'][p].shape), routed['grads'][p], g, GRAD_BOUND, errs)
    return own, routed


def check_against_reference_fp32(name, g, dx, grads):
    """where the decisions are float64's: the same rule against the reference's own fp32 results (the fixture)"""
    check_rule(name, 'dx', dx, g[f'{name}.dx'], g, GRAD_BOUND)
    for p in ti.params(ti.case(name)[1]):
        check_rule(name, f'grad.{p}', ti.view_like_stored(grads[p]), ti.stored_grad(g, name, p, np.asarray(grads[p]).shape), g, GRAD_BOUND)


def aten_step(m, x, t):
    outs = {}
    bns = bn_layers(m)
    hooks = [bn.register_forward_hook(lambda mod, a, o, i=i: outs.__setitem__(i, (o.detach() > 0).cpu().numpy())) for i, bn in enumerate(bns)]
    x = x.clone().requires_grad_(True)
    y = m(x)
    (y * t).sum().backward()
    for h in hooks:
        h.remove()
    return (y.detach().cpu().numpy(), x.grad.cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()},
            [b.running_mean.detach().cpu().numpy() for b in bns], [b.running_var.detach().cpu().numpy() for b in bns],
            [outs[i] for i in range(len(bns))])


def test_inputs_module_reproduces_the_stored_seeds(g):
    for name, nl, _, n, L, seed in ti.CASES:
        assert int(g[f'{name}.seed']) == seed
        assert g[f'{name}.y'].shape == (n, 1, L) and g[f'{name}.dx'].shape == (n, 1, L)
        assert g[f'{name}.bn_dev'].shape == (2 * nl + 1,) and g[f'{name}.run_var.{2 * nl}'].shape == (16,)
    assert ti.frames(2, 8, 7001).shape == (2, 1, 8) and ti.cotangent(3, 7, 1).shape == (3, 1, 7)
    shapes = {c[1:2] + c[3:5] for c in ti.CASES}
    assert {(1, 2, 2), (2, 3, 4), (7, 3, 128), (10, 3, 1024), (12, 2, 4096), (2, 2, 2000)} <= shapes
    from stofnet_amd.waveunet_training import CHUNKS
    for c in CHUNKS.values():                                   # a row count below, on and above every kernel's rows per partial
        assert {(1, 1, c - 2), (1, 1, c), (1, 1, c + 2), (1, 1, 2 * c - 2), (1, 1, 2 * c), (1, 1, 2 * c + 2)} <= shapes


@pytest.mark.parametrize('name', ti.IDS)
def test_forward_aten_fp32_on_the_cpu_against_the_fixture(g, name):
    _, nl, wseed, n, L, seed = ti.case(name)
    m = make_net(ti.weights(nl, wseed), nl)
    y, dx, grads, rm, rv, dec = aten_step(m, torch.from_numpy(ti.frames(n, L, seed)), torch.from_numpy(ti.cotangent(n, L, seed)))
    assert y.shape == (n, 1, L) and y.dtype == np.float32
    assert all(int(b.num_batches_tracked) == int(g[f'{name}.nbt']) for b in bn_layers(m))
    own, _ = check_step(name, g, y, dx, grads, rm, rv, dec)
    check_rule(name, 'y', y, g[f'{name}.y'], g, Y_BOUND)                       # ... and the reference's fp32 y itself
    if name in ti.GRAD_IDS and all(np.array_equal(a, b) for a, b in zip(dec, own['decisions'])):
        check_against_reference_fp32(name, g, dx, grads)


@pytest.mark.parametrize('name', ti.IDS)
def test_forward_aten_float64_is_the_restated_network(name):
    _, nl, wseed, n, L, seed = ti.case(name)
    sd, x, t = ti.weights(nl, wseed), ti.frames(n, L, seed), ti.cotangent(n, L, seed)
    m = make_net(sd, nl, dtype=torch.float64)
    y, dx, grads, rm, rv, dec = aten_step(m, torch.from_numpy(x).double(), torch.from_numpy(t).double())
    assert y.dtype == np.float64
    ref = own64(name)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))   # noqa: E731
    assert rel(y, ref['y']) <= 1e-10
    for b in range(2 * nl + 1):
        assert np.abs(rm[b] - ref['run_mean'][b]).max() <= 1e-10 * max(1.0, np.abs(ref['run_mean'][b]).max())
        assert rel(rv[b], ref['run_var'][b]) <= 1e-10
    if name in ti.GRAD_IDS:
        assert rel(dx, ref['dx']) <= 1e-10
        zero = ti.zero_grads(nl)
        for p in ti.params(nl):
            if p in zero:                 # analytically 0 under train-mode BatchNorm: rounding noise on both sides
                bn = ti.blocks(nl)[zero.index(p)][1]
                assert np.abs(grads[p]).max() <= 1e-10 * max(float(np.abs(ref['grads'][bn + '.bias']).max()), 1.0)
            else:
                assert rel(grads[p], ref['grads'][p]) <= 1e-10, p


def test_route_contract_without_a_device():
    from stofnet_amd import WaveUnet
    m = WaveUnet(2, 16)
    assert WaveUnet.train_route == 'aten' and m.train_route == 'aten'
    assert not any('train_route' in k for k in m.state_dict())
    x = torch.zeros(2, 1, 8)
    x[0, 0, 3] = 1.0
    m.train()
    assert m(x).grad_fn is not None and int(m.middle[1].num_batches_tracked) == 1           # 'aten': forward_aten, as ever
    for bad in ('kernel', None, 'ATEN'):
        m.train_route = bad
        with pytest.raises(ValueError, match='train_route'):
            m(x)
        m.eval()
        with pytest.raises(ValueError, match='train_route'):
            m(x)
        m.train()
    m.train_route = 'kernels'
    before = [b.running_mean.clone() for b in bn_layers(m)]
    with pytest.raises(RuntimeError, match='ROCm device'):                                   # a CPU tensor: no silent fall-back
        m(x)
    assert int(m.middle[1].num_batches_tracked) == 1 and all(torch.equal(a, b.running_mean) for a, b in zip(before, bn_layers(m)))
    m.eval()
    with torch.no_grad():
        assert m(x).shape == (2, 1, 8)                                                       # eval mode is unchanged: forward_aten on the CPU
    with pytest.raises(NotImplementedError, match='train mode only'):
        m.forward_train_kernels(x)
    m2 = WaveUnet(2, 16)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert m2.train_route == 'aten'


def test_main_trains_unet_on_the_aten_route(tmp_path, capsys, monkeypatch):
    """main.py's 'unet' branch no longer forces `evaluate`: train() is entered and the summary says so.  The evaluation pass that
    follows (mask2coords, toa_rmse) runs device kernels, so on this CPU run it is replaced by a stub; the GPU test runs it."""
    import main
    seen = []

    def evaluate_stub(model, name, frames, gt, cfg, log=None):
        seen.append((type(model).__name__, model.train_route, model.training))
        return np.zeros((frames.shape[0], 1)), {'model': name, 'inference_time': 0.0}
    monkeypatch.setattr(main, 'evaluate', evaluate_stub)
    args = ['model=unet', 'evaluate=False', 'train_route=aten', 'device=cpu', 'epochs=1', 'batch_size=2', 'num_waveforms=8',
            'num_samples=64', 'data_dir=./datasets/stof_chirp101_dataset', f'ckpt_dir={tmp_path}', 'seed=3']
    _, summary = main.main(args)
    assert seen == [('WaveUnet', 'aten', False)]
    assert summary['train_route'] == 'aten' and summary['train_precision'] == 'fp32'
    hist = summary['train_history']
    assert len(hist) == 1 and np.isfinite(hist[0]['train_loss']) and np.isfinite(hist[0]['val_loss'])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed['train_history'] == hist
    _, summary = main.main(args[:1] + ['evaluate=True'] + args[2:])                          # evaluate=True still evaluates only
    assert 'train_history' not in summary and 'train_route' not in summary


# ------------------------------------------------------------------------------------------- the interpolation transpose
INTERP_M = list(range(1, 4097)) + [5000, 10000, 1 << 20]


def test_interp_window_holds_every_contribution():
    from stofnet_amd.waveunet_training import interp_table
    for M in INTERP_M:
        i0, i1, l0, l1, lo, hi = interp_table(M)
        u = np.arange(2 * M)
        scale = np.float32(np.float32(M - 1) / np.float32(2 * M - 1))
        r = (scale * u.astype(np.float32)).astype(np.float32)                   # the forward's coordinates, restated
        j0 = np.minimum(r.astype(np.int32), M - 1)
        w1 = np.clip((r - j0.astype(np.float32)).astype(np.float32), 0, 1).astype(np.float32)
        assert np.array_equal(i0, j0) and np.array_equal(i1, np.minimum(j0 + 1, M - 1)) and np.array_equal(l1, w1)
        assert np.array_equal(l0, (np.float32(1) - w1).astype(np.float32))
        assert ((l0 + l1) == np.float32(1)).all(), M
        assert ((lo[i0] <= u) & (u <= hi[i0]) & (lo[i1] <= u) & (u <= hi[i1])).all(), M
        assert (lo >= 0).all() and (hi <= 2 * M - 1).all() and ((hi - lo) < 8).all()


@pytest.mark.parametrize('M', [1, 2, 3, 31, 32, 33, 64, 257, 1000])
def test_gathered_weights_are_the_transposed_interpolation_matrix(M):
    from stofnet_amd.waveunet_training import interp_table
    i0, i1, l0, l1, lo, hi = interp_table(M)
    dense = np.zeros((2 * M, M), np.float32)                    # the forward: up[u] = l0 low[i0] + l1 low[i1]
    for u in range(2 * M):
        dense[u, i0[u]] += l0[u]
        dense[u, i1[u]] += l1[u]
    gathered = np.zeros((M, 2 * M), np.float32)                 # what the transpose kernel visits: u ascending in the window of m
    for m in range(M):
        for u in range(lo[m], hi[m] + 1):
            if i0[u] == m:
                gathered[m, u] += l0[u]
            if i1[u] == m:
                gathered[m, u] += l1[u]
    assert np.array_equal(gathered.view(np.uint32), dense.T.copy().view(np.uint32))
    up = torch.nn.functional.interpolate(torch.eye(M).unsqueeze(0), scale_factor=2, mode='linear', align_corners=True)[0].numpy().T
    assert np.array_equal(dense, up)                            # ... and ATen's own fp32 interpolation

"""Zonzini training on the kernels of csrc/zonzini_train.hip, without a GPU: the float64 restatement the GPU tests lean on
against every array of tests/golden/f28_zonzini_training.npz, the fixture's layout and its margin claims, the `train_route`
switch, `main.zonzini_loss` against the reference's all-pairs value in closed form, the argument checks of every new C entry
(all return before any HIP call) and `main.py model=zonzini` argument handling as far as it runs without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import golden
import zonzini_inputs as zi
import zonzini_training_inputs as ti
from stofnet_amd import _lib
from stofnet_amd import build as sbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = 'f28_zonzini_training'
NEW_SYMBOLS = ('stof_zonzini_train_pack', 'stof_zonzini_train_forward', 'stof_zonzini_train_head_bwd', 'stof_zonzini_train_conv_wgrad_workspace_bytes',
               'stof_zonzini_train_conv_wgrad', 'stof_zonzini_train_dgrad_image_floats', 'stof_zonzini_train_dgrad_image',
               'stof_zonzini_train_conv_dgrad', 'stof_zonzini_train_in_wgrad_workspace_bytes', 'stof_zonzini_train_in_wgrad',
               'stof_zonzini_train_in_dgrad')
RESTATE_BOUND = 1e-5


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def grad_errors(name, net, grads, g):
    """{parameter: distance of `grads` from the fixture's gradient of case `name`, as a share of its max |.|}"""
    errs = {}
    for k in ti.param_names(net):
        v = np.asarray(grads[k], np.float64)
        if ti.kept_in_full(net, k):
            errs[k] = rel(v, g[f'{name}.grad.{k}'])
        else:
            gmax = float(g[f'{name}.gmax.{k}'])
            errs[k] = max(float(np.abs(v.reshape(-1)[::ti.STRIDE] - g[f'{name}.grad_stride53.{k}']).max()) / gmax,
                          abs(float(v.sum()) - float(g[f'{name}.gsum.{k}'])) / (gmax * v.size))     # `size` elements within the bound
    return errs


def test_fixture_layout():
    g = golden(FIXTURE)
    want = set()
    for name, net, _, n, L, seed, _ in ti.CASES:
        want |= {f'{name}.seed', f'{name}.y', f'{name}.dx', f'{name}.dev'}
        for k in ti.param_names(net):
            want |= {f'{name}.grad.{k}'} if ti.kept_in_full(net, k) else {f'{name}.gmax.{k}', f'{name}.gsum.{k}', f'{name}.grad_stride53.{k}'}
        assert g[f'{name}.y'].shape == (n, 1) and g[f'{name}.dx'].shape == (n, 1, L)
        assert g[f'{name}.dev'].shape == (len(ti.CHANNELS[net]) + 1,) and g[f'{name}.dev'].dtype == np.float64
        assert int(g[f'{name}.seed']) == seed and L >= ti.MIN_LEN[net]
    assert set(g.files) == want
    shapes = sorted((c[1], c[3], c[4]) for c in ti.CASES)
    for must in (('small', 2, 936), ('small', 3, 937), ('small', 2, 939), ('small', 2, 1537), ('small', 2, 2000), ('large', 1, 3752),
                 ('large', 2, 4001)):
        assert must in shapes
    # the chunk cases: N = 1, the rows of layer 1 / layer 2 one below, on and one above the chunk of its weight gradient
    for k, chunk in enumerate(ti.CHUNKS):
        for d in (-1, 0, 1):
            L = ti.length_for(chunk + d, k)
            assert ('small', 1, L) in shapes
            rows = L
            for _ in range(k + 1):
                rows = ti.pooled_len(rows)
            assert rows == chunk + d
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', FIXTURE + '.npz')) < 1 << 20


@pytest.mark.parametrize('name', ti.IDS)
def test_float64_restatement_reproduces_fixture(name):
    g = golden(FIXTURE)
    _, net, wkey, n, L, seed, safe = ti.case(name)
    r = ti.restate64(ti.weights(wkey, net), zi.echo_frames(n, L, seed), ti.cotangent(n, seed))
    errs = {'y': rel(r['y'], g[f'{name}.y']), 'dx': rel(r['dx'], g[f'{name}.dx']), **grad_errors(name, net, r['grads'], g)}
    inside = ti.margin_count(r, g[f'{name}.dev'])
    print(name, 'inside the margin', inside, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert max(errs.values()) <= RESTATE_BOUND, errs
    assert inside <= 64 and (inside == 0 or not safe)            # a condition on the inputs, from float64 alone


def test_tie_and_zero_conventions_of_the_restatement():
    # z = [1, 1, 2, 2, -1, -1] -> grad [1, 0, 1, 0, 0, 0]: a tie goes to the even conv output, relu' is 0 at 0
    z = torch.tensor([[[1., 1., 2., 2., -1., -1.]]], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.max_pool1d(torch.relu(z), 2).sum().backward()
    assert z.grad.flatten().tolist() == [1, 0, 1, 0, 0, 0]
    e, o = z.detach()[..., 0::2], z.detach()[..., 1::2]
    sel = torch.where(torch.maximum(e, o) > 0, torch.where(o > e, 2, 1), 0)
    assert sel.flatten().tolist() == [1, 1, 0]


def test_train_route_switch():
    from stofnet_amd import ZonziniNetLarge, ZonziniNetSmall
    for cls in (ZonziniNetSmall, ZonziniNetLarge):
        assert cls.train_route is None
        m = cls()
        assert m.train_route is None and 'train_route' not in m.state_dict()
    m = ZonziniNetSmall()
    x = torch.zeros(2, 1, 936)
    for bad in ('kernel', 'ATEN', 1, ''):
        m.train_route = bad
        with pytest.raises(ValueError, match='train_route'):
            m(x)
    m.train_route = 'aten'                                    # the reference's own layers: runs on CPU tensors too
    m.train()
    y = m(x)
    assert y.shape == (2, 1) and y.requires_grad
    m.train_route = 'kernels'
    with pytest.raises(RuntimeError, match='ROCm device'):
        m(x)


def closed_form(pred, targets):
    """sum over n, m of (pred_n - t_m)^2 / N^2 and its gradient 2 (pred_n - mean t) / N, float64 numpy"""
    p, t = np.asarray(pred, np.float64).reshape(-1), np.asarray(targets, np.float64).reshape(-1)
    return float(((p[:, None] - t[None, :]) ** 2).mean()), 2.0 * (p - t.mean()) / p.size


def test_zonzini_loss_is_the_all_pairs_mean_on_the_first_onset():
    import main
    rng = np.random.default_rng(5)
    pred = torch.tensor(rng.standard_normal((5, 1)) * 300 + 700, dtype=torch.float32, requires_grad=True)
    gt = np.array([[812.4, 0.0, 0.0], [0.0, 433.25, 900.0], [np.nan, -3.0, 671.5], [950.0, 120.75, 0.0], [0.0, 0.0, 0.0]], np.float32)
    want_t = np.array([812.4, 433.25, 671.5, 120.75, 0.0], np.float32)          # the smallest non-zero onset; none: slot 0, value 0
    for r in (1, 4, 10):
        loss = main.zonzini_loss(pred, torch.from_numpy(gt.copy()), r)
        value, grad = closed_form(pred.detach().numpy(), want_t)
        assert abs(float(loss.detach()) - value) <= 1e-6 * value
        pred.grad = None
        loss.backward()
        assert np.abs(pred.grad.numpy().reshape(-1) - grad).max() <= 1e-6 * np.abs(grad).max()
    # the row-wise mean would be another number
    assert abs(float(((pred.detach().numpy().reshape(-1) - want_t) ** 2).mean()) - value) > 1e-3 * value
    # one onset per row, as the synthetic echoes have
    one = main.zonzini_loss(pred, torch.from_numpy(want_t[:, None].copy()), 4)
    assert abs(float(one.detach()) - value) <= 1e-6 * value


def test_argument_contract_returns_before_any_launch(lib):
    BAD, POOL, WS, UNS = _lib.STOF_ERR_BAD_ARG, _lib.STOF_ERR_POOL_EMPTY, _lib.STOF_ERR_WORKSPACE, _lib.STOF_ERR_UNSUPPORTED
    buf = np.zeros(64, np.float32)                      # never dereferenced: every call below returns from its checks
    a = ctypes.c_void_p(buf.ctypes.data)
    big = 1 << 40
    for variant, layers, min_len in ((_lib.ZONZINI_SMALL, 4, 936), (_lib.ZONZINI_LARGE, 5, 3752)):
        d, bad = _lib.ZonziniDesc(variant, 0), _lib.ZonziniDesc(7, 0)
        D, B = ctypes.byref(d), ctypes.byref(bad)
        lists = (ctypes.c_void_p * layers)(*[buf.ctypes.data] * layers)
        holes = (ctypes.c_void_p * layers)(*([buf.ctypes.data] * (layers - 1) + [None]))
        assert lib.stof_zonzini_train_in_wgrad_workspace_bytes(D) > 0 and lib.stof_zonzini_train_in_wgrad_workspace_bytes(B) == 0
        for l in range(1, layers):
            assert 0 < lib.stof_zonzini_train_conv_wgrad_workspace_bytes(D, l) <= 64 << 20
            assert lib.stof_zonzini_train_dgrad_image_floats(D, l) > 0
        for l in (0, -1, layers, 9):
            assert lib.stof_zonzini_train_conv_wgrad_workspace_bytes(D, l) == 0 and lib.stof_zonzini_train_dgrad_image_floats(D, l) == 0
        assert lib.stof_zonzini_train_conv_wgrad_workspace_bytes(B, 1) == 0 and lib.stof_zonzini_train_dgrad_image_floats(B, 1) == 0
        # name -> (call(desc, pointers, N, L), number of pointers)
        calls = {
            'forward': (lambda D, q, N, L: lib.stof_zonzini_train_forward(D, q[0], N, L, q[1], lists, lists, q[2], q[3], q[4], None), 5),
            'conv_wgrad': (lambda D, q, N, L: lib.stof_zonzini_train_conv_wgrad(D, 1, q[0], q[1], q[2], q[3], q[4], N, L, q[5], big, None), 6),
            'conv_dgrad': (lambda D, q, N, L: lib.stof_zonzini_train_conv_dgrad(D, 1, q[0], q[1], q[2], q[3], N, L, None), 4),
            'in_wgrad': (lambda D, q, N, L: lib.stof_zonzini_train_in_wgrad(D, q[0], q[1], q[2], q[3], q[4], N, L, q[5], big, None), 6),
            'in_dgrad': (lambda D, q, N, L: lib.stof_zonzini_train_in_dgrad(D, q[0], q[1], q[2], q[3], N, L, None), 4),
        }
        for name, (call, nptr) in calls.items():
            for k in range(nptr):
                q = [a] * nptr
                q[k] = None
                assert call(D, q, 2, min_len) == BAD, (name, k)
            q = [a] * nptr
            assert call(B, q, 2, min_len) == BAD and call(None, q, 2, min_len) == BAD, name
            assert call(D, q, 0, min_len) == BAD and call(D, q, -1, min_len) == BAD, name
            assert call(D, q, 2, min_len - 1) == POOL and call(D, q, 2, 0) == POOL, name
            assert call(D, q, 1 << 20, 1 << 12) == UNS, name                           # N L = 2^32: rows are ints
        assert lib.stof_zonzini_train_forward(D, a, 2, min_len, a, None, lists, a, a, a, None) == BAD
        assert lib.stof_zonzini_train_forward(D, a, 2, min_len, a, lists, holes, a, a, a, None) == BAD
        assert lib.stof_zonzini_train_forward(D, a, 2, min_len, a, holes, lists, a, a, a, None) == BAD
        for l in (0, layers):
            assert lib.stof_zonzini_train_conv_wgrad(D, l, a, a, a, a, a, 2, min_len, a, big, None) == BAD
            assert lib.stof_zonzini_train_conv_dgrad(D, l, a, a, a, a, 2, min_len, None) == BAD
            assert lib.stof_zonzini_train_dgrad_image(D, l, a, a, None) == BAD
        assert lib.stof_zonzini_train_dgrad_image(D, 1, None, a, None) == BAD and lib.stof_zonzini_train_dgrad_image(D, 1, a, None, None) == BAD
        assert lib.stof_zonzini_train_dgrad_image(B, 1, a, a, None) == BAD
        # the device packer: the desc, the pointer list, every pointer in it, the blob and its size
        nparams = 2 * layers + 4
        full = (ctypes.c_void_p * nparams)(*[buf.ctypes.data] * nparams)
        gap = (ctypes.c_void_p * nparams)(*([buf.ctypes.data] * (nparams - 1) + [None]))
        assert lib.stof_zonzini_train_pack(B, full, a, big, None) == BAD and lib.stof_zonzini_train_pack(D, None, a, big, None) == BAD
        assert lib.stof_zonzini_train_pack(D, gap, a, big, None) == BAD and lib.stof_zonzini_train_pack(D, full, None, big, None) == BAD
        assert lib.stof_zonzini_train_pack(D, full, a, lib.stof_zonzini_packed_bytes(D) - 1, None) == WS
        # a workspace that is too small is refused before the launch as well
        assert lib.stof_zonzini_train_conv_wgrad(D, 1, a, a, a, a, a, 2, min_len, a, 16, None) == WS
        assert lib.stof_zonzini_train_in_wgrad(D, a, a, a, a, a, 2, min_len, a, 16, None) == WS
        # the head: ten pointers, N
        for k in range(10):
            q = [a] * 10
            q[k] = None
            assert lib.stof_zonzini_train_head_bwd(D, *q, 2, None) == BAD, k
        assert lib.stof_zonzini_train_head_bwd(B, *([a] * 10), 2, None) == BAD
        assert lib.stof_zonzini_train_head_bwd(D, *([a] * 10), 0, None) == BAD


def test_new_symbols_are_declared_and_exported(lib):
    import re
    with open(os.path.join(ROOT, 'include', 'stofnet_amd.h')) as fh:
        header = fh.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'^(int|size_t) ' + sym + r'\(', header, re.M), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


def test_main_zonzini_argument_handling(monkeypatch):
    """`main.main` with model=zonzini: evaluate=False stays evaluate=False, `train` is reached with the route of the config
    (default 'kernels') and the summary names it; chirp data selects the Small net, anything else the Large one."""
    import main
    calls = {}

    def fake_train(model, frames, gt, cfg, log=None):
        calls['evaluate'], calls['route'], calls['model'] = bool(cfg.evaluate), str(cfg.train_route), type(model).__name__
        model.train_route = str(cfg.train_route)
        return [{'epoch': 0}]

    for cls in (main.ZonziniNetSmall, main.ZonziniNetLarge):
        monkeypatch.setattr(cls, 'to', lambda self, device: self)
    monkeypatch.setattr(main, 'train', fake_train)
    monkeypatch.setattr(main, 'evaluate', lambda *a, **k: ([], {'inference_time': 0.0}))
    base = ['model=zonzini', 'num_waveforms=4', 'device=cpu', 'logging=Null', 'model_file=']
    _, summary = main.main(base + ['evaluate=False', 'data_dir=chirp', 'num_samples=2000'])
    assert calls == {'evaluate': False, 'route': 'kernels', 'model': 'ZonziniNetSmall'}
    assert summary['train_route'] == 'kernels' and summary['train_precision'] == 'fp32' and summary['train_history'] == [{'epoch': 0}]
    _, summary = main.main(base + ['evaluate=False', 'train_route=aten', 'data_dir=pala', 'num_samples=4000'])
    assert calls == {'evaluate': False, 'route': 'aten', 'model': 'ZonziniNetLarge'} and summary['train_route'] == 'aten'
    calls.clear()
    _, summary = main.main(base + ['evaluate=True', 'data_dir=chirp', 'num_samples=2000'])
    assert calls == {} and 'train_route' not in summary                          # evaluate=True still only evaluates

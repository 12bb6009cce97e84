"""Kuleshov training, the parts that need no GPU:

  * the new C entries exist, equal the header's declarations and check their arguments before any device call;
  * the Dropout keep-mask entry against the numpy Philox of test_augment_cpu.py, the counter layout restated, and its keep rate;
  * `kuleshov_training_inputs.restate64` with the host masks is `Kuleshov.forward_aten` in float64 with the same masks patched in
    (1e-12), and is the reference's float64 module on the fixture: max |fixture fp32 - restate64| equals the stored deviation;
  * `forward_aten` in fp32 on the CPU with the patched masks against the fixture under the tolerance rule;
  * the route and error contract of `Kuleshov.train_route` on CPU tensors;
  * main.py parses `kuleshov_train`; without it `train()` is not called.

Tolerance rule (tests/test_waveunet_training_cpu.py): |ours - ref64| <= max(B max|ref64|, 8 dev_T), dev_T the reference's own
fp32-vs-float64 deviation of tensor T (stored); B = 2e-5 for y and the running statistics, 2e-4 for dx and the gradients.  ref64 is
float64 autograd of the restated network with the decisions and masks of the run under test."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import kuleshov_training_inputs as ti
from test_augment_cpu import philox4x32_10
from test_waveunet_training_cpu import GRAD_BOUND, Y_BOUND

from stofnet_amd import _lib
from stofnet_amd import build as sbuild

CHEAP = ['ks_2x641_8', 'ks_p0_2x650_8', 'ks_call3_2x660_16']          # the cases the CPU runs in full


@pytest.fixture(scope='module')
def g():
    return golden('f31_kuleshov_training')


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


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
        _, n, L, O, wseed, seed, p, call = ti.case(name)
        _own[name] = ti.restate64(ti.weights(L, O, wseed), L, ti.frames(n, L, seed), ti.cotangent(n, O, seed), ti.masks(n, L, p, call))
    return _own[name]


def check_step(name, g, y, dx, grads, run_mean, run_var, decisions, errs=None):
    """The whole comparison of one step of case `name` (numpy arrays) with float64 autograd taken with the run's decisions.
    -> (own float64 run, whether the decisions are float64's)"""
    _, n, L, O, wseed, seed, p, call = ti.case(name)
    own = own64(name)
    same = ti.same_decisions(decisions, own['decisions'])
    flips = {k: [int((np.asarray(a) != np.asarray(b)).sum()) for a, b in zip(decisions[k] if k != 'b' else [decisions[k]],
                                                                               own['decisions'][k] if k != 'b' else [own['decisions'][k]])]
             for k in ('u', 'a', 'b')}
    print(f'{name} decisions that differ from float64: {flips}')
    routed = own if same else ti.restate64(ti.weights(L, O, wseed), L, ti.frames(n, L, seed), ti.cotangent(n, O, seed),
                                           ti.masks(n, L, p, call), decisions)
    check_rule(name, 'y', y, routed['y'], g, Y_BOUND, errs)
    for b in range(8):
        check_rule(name, f'run_mean.{b}', run_mean[b], routed['run_mean'][b], g, Y_BOUND, errs)
        check_rule(name, f'run_var.{b}', run_var[b], routed['run_var'][b], g, Y_BOUND, errs)
        if same:                                # ... and the reference's own fp32 statistics, as far as the fixture keeps them
            check_rule(name, f'run_mean.{b}', run_mean[b][::ti.RUN_STRIDE], g[f'{name}.run_mean.{b}'], g, Y_BOUND)
            check_rule(name, f'run_var.{b}', run_var[b][::ti.RUN_STRIDE], g[f'{name}.run_var.{b}'], g, Y_BOUND)
    check_rule(name, 'dx', dx, routed['dx'], g, GRAD_BOUND, errs)
    for k in ti.param_names():
        check_rule(name, f'grad.{k}', ti.view_like_stored(grads[k]), ti.view_like_stored(routed['grads'][k]), g, GRAD_BOUND, errs)
    return own, same


def check_against_reference_fp32(name, g, y, dx, grads):
    """where the decisions are float64's: the same rule against the reference's own fp32 results (the fixture)"""
    check_rule(name, 'y', y, g[f'{name}.y'], g, Y_BOUND)
    check_rule(name, 'dx', dx, g[f'{name}.dx'], g, GRAD_BOUND)
    for k in ti.param_names():
        check_rule(name, f'grad.{k}', ti.view_like_stored(grads[k]), ti.stored_grad(g, name, k), g, GRAD_BOUND)


def make_net(name, route='aten', dev='cpu', dtype=torch.float32, patched=True):
    """the project's module on case `name`'s weights in train mode; patched: the case's masks as MaskDropout modules, else the
    Dropout p, `dropout_seed` and `dropout_call` of the case"""
    from stofnet_amd import Kuleshov
    _, n, L, O, wseed, seed, p, call = ti.case(name)
    m = Kuleshov(L, O)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ti.weights(L, O, wseed).items()}, strict=True)
    m = m.to(device=dev)
    if dtype != torch.float32:
        m = m.to(dtype)
    m.train()
    m.train_route = route
    for site in ti.SITES:
        getattr(m, site).p = p
    m.dropout_seed, m.dropout_call = ti.DROP_SEED, call
    if patched and p > 0:
        ti.patch_dropout(m, ti.masks(n, L, p, call))
    return m


def aten_step(m, x, t):
    """one step of the ATen route -> y, dx, grads, running statistics, decisions (numpy)"""
    outs = {}
    watched = [getattr(m, f'down_conv{j}') for j in range(4)] + [getattr(m, f'down_bn{j}') for j in range(4)] + [m.bottleneck_dropout]
    hooks = [w.register_forward_hook(lambda mod, a, o, i=i: outs.__setitem__(i, (o.detach() > 0).cpu().numpy())) for i, w in enumerate(watched)]
    x = x.clone().requires_grad_(True)
    y = m(x)
    (y * t).sum().backward()
    for h in hooks:
        h.remove()
    bns = m._batch_norms()
    return (y.detach().cpu().numpy(), x.grad.cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()},
            [b.running_mean.detach().cpu().numpy() for b in bns], [b.running_var.detach().cpu().numpy() for b in bns],
            {'u': [outs[j] for j in range(4)], 'a': [outs[4 + j] for j in range(4)], 'b': outs[8]})


# ------------------------------------------------------------------------------------------------------------ the C ABI
NEW = ['stof_kuleshov_dropout_keep', 'stof_kuleshov_train_constants', 'stof_kuleshov_train_frag_floats', 'stof_kuleshov_train_pack_frag',
       'stof_kuleshov_train_pack_final', 'stof_kuleshov_train_fc_frag_floats', 'stof_kuleshov_train_pack_fc', 'stof_kuleshov_train_down0',
       'stof_kuleshov_train_conv', 'stof_kuleshov_train_stats_workspace_bytes', 'stof_kuleshov_train_stats', 'stof_kuleshov_train_apply_down',
       'stof_kuleshov_train_apply_up', 'stof_kuleshov_train_apply_bott', 'stof_kuleshov_train_tail', 'stof_kuleshov_train_fc_bwd',
       'stof_kuleshov_train_final_bwd_workspace_bytes', 'stof_kuleshov_train_final_bwd', 'stof_kuleshov_train_gather_up',
       'stof_kuleshov_train_gather_down', 'stof_kuleshov_train_gather_bott', 'stof_kuleshov_train_bn_bwd',
       'stof_kuleshov_train_wgrad_workspace_bytes', 'stof_kuleshov_train_wgrad', 'stof_kuleshov_train_dgrad_workspace_bytes',
       'stof_kuleshov_train_dgrad', 'stof_kuleshov_train_down0_bwd_workspace_bytes', 'stof_kuleshov_train_down0_bwd']


def test_new_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'stofnet_amd.h')).read()
    declared = set(re.findall(r'^(?:int|int64_t|size_t|const char\*)\s+(stof_kuleshov_[a-z0-9_]+)\s*\(', hdr, flags=re.M))
    mine = {s for s in _lib.EXPORTED_SYMBOLS if s.startswith('stof_kuleshov_')}
    assert mine == declared and set(NEW) <= mine
    for sym in NEW:
        assert hasattr(lib, sym), sym
    from stofnet_amd.kuleshov_training import CHUNKS, MAX_PARTIALS
    assert CHUNKS == {'stats': 256, 'conv_wgrad': 256, 'final_wgrad': 256, 'down0_wgrad': 256}
    assert MAX_PARTIALS == {'stats': 256, 'conv_wgrad': 8, 'final_wgrad': 256, 'down0_wgrad': 256}
    # the weight-gradient workspace is bounded: up_conv1 (1024 x 512 x 17) never takes more than MAX_PARTIALS partials
    one = 1024 * 512 * 17 * 4
    small, big = (int(lib.stof_kuleshov_train_wgrad_workspace_bytes(N, 100, 512, 1024, 17)) for N in (2, 4096))
    assert 0 < small - one < (5 << 20) and 0 < big - MAX_PARTIALS['conv_wgrad'] * one == small - one


def test_argument_checks_come_before_any_device_call(lib):
    """every entry with a bad argument, NULL pointers or a short workspace: a status, no launch (this machine has no GPU)"""
    BAD, WS, OK = _lib.STOF_ERR_BAD_ARG, _lib.STOF_ERR_WORKSPACE, _lib.STOF_OK
    q = ctypes.c_void_p(4096)                                   # a non-NULL pointer that is never followed
    d = ctypes.byref(_lib.KuleshovDesc(700, 1400, 1e-5, 0, 0))
    short = ctypes.byref(_lib.KuleshovDesc(640, 8, 1e-5, 0, 0))
    keep = np.zeros(8, np.uint8)
    kp = ctypes.c_void_p(keep.ctypes.data)
    assert lib.stof_kuleshov_dropout_keep(1, 0, 0, 0, 0, 8, 0.5, kp) == OK
    for args in ((1, 0, 0, 5, 0, 8, 0.5, kp), (1, 0, 0, -1, 0, 8, 0.5, kp), (1, 0, 0, 0, -1, 8, 0.5, kp), (1, 0, 0, 0, 0, -1, 0.5, kp),
                 (1, 0, 0, 0, 0, 8, 1.0, kp), (1, 0, 0, 0, 0, 8, -0.1, kp), (1, 0, 0, 0, 0, 8, float('nan'), kp), (1, 0, 1 << 29, 0, 0, 8, 0.5, kp),
                 (1, 0, 0, 0, 0, 8, 0.5, None)):
        assert lib.stof_kuleshov_dropout_keep(*args) == BAD, args
    assert lib.stof_kuleshov_train_constants(None) == BAD
    assert lib.stof_kuleshov_train_frag_floats(128, 256, 33, 0) == 128 * 256 * 33
    assert lib.stof_kuleshov_train_frag_floats(128, 256, 33, 2) == 128 * 256 * 17 and lib.stof_kuleshov_train_frag_floats(128, 256, 33, 3) == 128 * 256 * 16
    for args in ((64, 256, 33, 0), (128, 2048, 33, 0), (128, 256, 5, 0), (128, 256, 33, 4), (128, 200, 33, 0)):
        assert lib.stof_kuleshov_train_frag_floats(*args) == 0, args
    assert lib.stof_kuleshov_train_pack_frag(q, 128, 256, 33, 4, q, None) == BAD and lib.stof_kuleshov_train_pack_frag(None, 128, 256, 33, 0, q, None) == BAD
    assert lib.stof_kuleshov_train_pack_final(None, q, None) == BAD and lib.stof_kuleshov_train_pack_final(q, None, None) == BAD
    assert lib.stof_kuleshov_train_fc_frag_floats(short) == 0 and lib.stof_kuleshov_train_fc_frag_floats(d) > 0
    assert lib.stof_kuleshov_train_pack_fc(short, q, q, None) == BAD and lib.stof_kuleshov_train_pack_fc(d, None, q, None) == BAD
    assert lib.stof_kuleshov_train_down0(q, 700, 2, 640, q, q, q, None) == BAD and lib.stof_kuleshov_train_down0(q, 600, 2, 700, q, q, q, None) == BAD
    assert lib.stof_kuleshov_train_down0(None, 700, 2, 700, q, q, q, None) == BAD and lib.stof_kuleshov_train_down0(q, 700, 0, 700, q, q, q, None) == BAD
    conv = lambda **k: lib.stof_kuleshov_train_conv(*[{**dict(src=q, ns=1000, N=2, Lout=10, cin=128, cout=256, rows=33, stride=2, frag=q, bias=None,  # noqa: E731
                                                              slope=0, out=q, ons=2560, ots=256, stream=None), **k}[a]
                                                      for a in ('src', 'ns', 'N', 'Lout', 'cin', 'cout', 'rows', 'stride', 'frag', 'bias', 'slope', 'out', 'ons',
                                                                'ots', 'stream')])
    for k in (dict(src=None), dict(frag=None), dict(out=None), dict(N=0), dict(Lout=0), dict(cin=96), dict(cout=1152), dict(rows=0), dict(rows=66),
              dict(stride=3), dict(ots=255), dict(ns=-1)):
        assert conv(**k) == BAD, k
    assert conv(N=1 << 20, Lout=1 << 12) == _lib.STOF_ERR_UNSUPPORTED                      # N Lout leaves 32-bit indexing
    assert lib.stof_kuleshov_train_stats(q, 1 << 31, 128, q, q, q, q, 1e-5, 0.1, q, q, q, q, 1 << 30, None) == BAD
    assert lib.stof_kuleshov_train_wgrad(q, 1000, q, 1 << 20, 1 << 12, 128, 256, 33, 2, q, q, q, 1 << 40, None) == _lib.STOF_ERR_UNSUPPORTED
    assert lib.stof_kuleshov_train_stats_workspace_bytes() > 0
    ws_bytes = int(lib.stof_kuleshov_train_stats_workspace_bytes())
    stats = lambda rows, ch, ws, wsb: lib.stof_kuleshov_train_stats(q, rows, ch, q, q, q, q, 1e-5, 0.1, q, q, q, ws, wsb, None)   # noqa: E731
    assert stats(1, 128, q, ws_bytes) == BAD and stats(4, 100, q, ws_bytes) == BAD and stats(4, 128, None, ws_bytes) == WS and stats(4, 128, q, 8) == WS
    assert lib.stof_kuleshov_train_apply_down(q, 2, 10, 128, q, q, 1279, None) == BAD and lib.stof_kuleshov_train_apply_down(None, 2, 10, 128, q, q, 1280, None) == BAD
    up = lambda site, p, rank=0, ch=256: lib.stof_kuleshov_train_apply_up(q, 2, 10, ch, q, 1, 0, rank, site, p, q, 5120, None)   # noqa: E731
    assert up(0, 0.5) == BAD and up(5, 0.5) == BAD and up(1, 1.0) == BAD and up(1, -0.5) == BAD and up(1, 0.5, 1 << 29) == BAD and up(1, 0.5, 0, 192) == BAD
    assert lib.stof_kuleshov_train_apply_bott(q, 2, 9, 1, 0, 0, 1.5, q, None) == BAD and lib.stof_kuleshov_train_apply_bott(None, 2, 9, 1, 0, 0, 0.5, q, None) == BAD
    assert lib.stof_kuleshov_train_tail(short, q, 2, q, q, q, q, q, q, None) == BAD and lib.stof_kuleshov_train_tail(d, q, 0, q, q, q, q, q, q, None) == BAD
    assert lib.stof_kuleshov_train_tail(d, None, 2, q, q, q, q, q, q, None) == BAD
    assert lib.stof_kuleshov_train_tail(d, q, 1 << 23, q, q, q, q, q, q, None) == _lib.STOF_ERR_UNSUPPORTED
    assert lib.stof_kuleshov_train_fc_bwd(short, q, q, q, 2, q, q, q, None) == BAD and lib.stof_kuleshov_train_fc_bwd(d, q, q, q, 0, q, q, q, None) == BAD
    assert lib.stof_kuleshov_train_fc_bwd(d, q, None, q, 2, q, q, q, None) == BAD
    assert lib.stof_kuleshov_train_fc_bwd(d, q, q, q, 1 << 18, q, q, q, None) == _lib.STOF_ERR_UNSUPPORTED
    gap = _lib.KuleshovDesc(3355801, 8, 1e-5, 0, 0)                      # Kp = 16776968: one k block more than the grid's second dimension takes
    assert lib.stof_kuleshov_train_fc_frag_floats(ctypes.byref(gap)) > 0
    assert lib.stof_kuleshov_train_fc_bwd(ctypes.byref(gap), q, q, q, 2, q, q, q, None) == _lib.STOF_ERR_UNSUPPORTED
    fw = int(lib.stof_kuleshov_train_final_bwd_workspace_bytes())
    assert fw > 0 and lib.stof_kuleshov_train_final_bwd(d, q, q, q, 2, q, q, q, q, fw - 1, None) == WS
    assert lib.stof_kuleshov_train_final_bwd(d, q, q, q, 2, q, q, q, None, fw, None) == WS and lib.stof_kuleshov_train_final_bwd(d, None, q, q, 2, q, q, q, q, fw, None) == BAD
    assert lib.stof_kuleshov_train_final_bwd(d, q, q, q, 1 << 23, q, q, q, q, fw, None) == _lib.STOF_ERR_UNSUPPORTED
    assert lib.stof_kuleshov_train_gather_up(q, 100, 2, 10, 256, 1, 0, 0, 1, 0.5, q, None) == BAD           # the stride is shorter than a row's data
    assert lib.stof_kuleshov_train_gather_up(q, 2560, 2, 10, 256, 1, 0, 0, 0, 0.5, q, None) == BAD and lib.stof_kuleshov_train_gather_up(q, 2560, 2, 10, 256, 1, 0, 0, 1, 0.5, None, None) == BAD
    assert lib.stof_kuleshov_train_gather_down(q, 1279, None, q, 1280, 2, 10, 128, q, None) == BAD and lib.stof_kuleshov_train_gather_down(q, 1280, None, None, 1280, 2, 10, 128, q, None) == BAD
    assert lib.stof_kuleshov_train_gather_bott(q, None, 2, 9, 1, 0, 0, 0.5, q, None) == BAD and lib.stof_kuleshov_train_gather_bott(q, q, 2, 9, 1, 0, 0, 1.0, q, None) == BAD
    bnb = lambda rows, ch, ws, wsb: lib.stof_kuleshov_train_bn_bwd(q, q, q, rows, ch, 1, q, q, q, ws, wsb, None)   # noqa: E731
    assert bnb(1, 128, q, ws_bytes) == BAD and bnb(4, 64, q, ws_bytes) == BAD and bnb(4, 128, q, ws_bytes - 1) == WS and bnb(4, 128, None, ws_bytes) == WS
    assert lib.stof_kuleshov_train_wgrad_workspace_bytes(2, 10, 128, 256, 7) == 0 and lib.stof_kuleshov_train_wgrad_workspace_bytes(0, 10, 128, 256, 33) == 0
    wg = int(lib.stof_kuleshov_train_wgrad_workspace_bytes(2, 10, 128, 256, 33))
    wgrad = lambda stride, ws, wsb, src=q: lib.stof_kuleshov_train_wgrad(src, 1000, q, 2, 10, 128, 256, 33, stride, q, q, ws, wsb, None)   # noqa: E731
    assert wgrad(3, q, wg) == BAD and wgrad(2, q, wg, None) == BAD and wgrad(2, q, wg - 1) == WS and wgrad(2, None, wg) == WS
    assert lib.stof_kuleshov_train_dgrad_workspace_bytes(2, 10, 256, 33, 3) == 0
    dg = int(lib.stof_kuleshov_train_dgrad_workspace_bytes(2, 10, 256, 33, 2))
    assert dg == 2 * (10 + 32) * 256 * 4 and int(lib.stof_kuleshov_train_dgrad_workspace_bytes(2, 10, 256, 33, 1)) == 2 * (10 + 64) * 256 * 4
    dgrad = lambda stride, Lin, f1=q, ws=q, wsb=1 << 30: lib.stof_kuleshov_train_dgrad(q, 2, 10, 128, 256, 33, stride, q, f1, Lin, q, ws, wsb, None)   # noqa: E731
    assert dgrad(1, 41) == BAD and dgrad(1, 43) == BAD and dgrad(2, 50) == BAD and dgrad(2, 53) == BAD and dgrad(2, 51, None) == BAD
    assert dgrad(2, 51, q, q, dg - 1) == WS and dgrad(2, 52, q, None) == WS and dgrad(1, 42, None, q, 8) == WS
    d0 = int(lib.stof_kuleshov_train_down0_bwd_workspace_bytes())
    d0b = lambda L, xs, dx, dxs, ws=q, wsb=d0: lib.stof_kuleshov_train_down0_bwd(q, xs, q, q, 2, L, q, q, dx, dxs, ws, wsb, None)   # noqa: E731
    assert d0b(640, 700, None, 0) == BAD and d0b(700, 699, None, 0) == BAD and d0b(700, 700, q, 699) == BAD
    assert d0b(700, 700, None, 0, q, d0 - 1) == WS and d0b(700, 700, None, 0, None) == WS


# ---------------------------------------------------------------------------------------------------------- the keep-mask
@pytest.mark.parametrize('seed,call,rank,site,n', [(0, 0, 0, 0, 0), (ti.DROP_SEED, 3, 0, 4, 2), ((1 << 64) - 5, (1 << 32) - 1, 7, 2, 1000)])
def test_keep_mask_is_the_numpy_philox(seed, call, rank, site, n):
    from stofnet_amd.kuleshov_training import dropout_keep
    count = 4099
    e = np.arange(count, dtype=np.uint64)
    w = philox4x32_10((e >> np.uint64(2), np.uint64(n), np.uint64(call), np.uint64((rank << 3) | site)), (seed & 0xffffffff, (seed >> 32) & 0xffffffff))
    words = np.choose((e & np.uint64(3)).astype(np.int64), w).astype(np.uint64)
    for p in (0.5, 0.1, 0.0, 0.999):
        thr = np.uint64(int(np.floor(p * 2.0 ** 32)))
        assert np.array_equal(dropout_keep(seed, call, rank, site, n, count, p), words >= thr), p
    assert dropout_keep(seed, call, rank, site, n, 0, 0.5).shape == (0,)
    assert not np.array_equal(dropout_keep(seed, call, rank, site, n, count, 0.5), dropout_keep(seed, call + 1, rank, site, n, count, 0.5))
    assert not np.array_equal(dropout_keep(seed, call, rank, site, n, count, 0.5), dropout_keep(seed, call, rank, (site + 1) % 5, n, count, 0.5))


def test_keep_rate():
    from stofnet_amd.kuleshov_training import dropout_keep
    count = 1 << 20                                             # binomial: sigma = sqrt(p (1 - p) / count) <= 4.9e-4; six sigma
    for p in (0.5, 0.1):
        rate = dropout_keep(ti.DROP_SEED, 0, 0, 1, 0, count, p).mean()
        assert abs(rate - (1 - p)) < 6 * np.sqrt(p * (1 - p) / count), (p, rate)
    mk = ti.masks(2, 641, 0.5, 0)
    assert [m.shape for m in mk] == [(2, 512, 9), (2, 1024, 1), (2, 1024, 11), (2, 512, 47), (2, 256, 159)]
    assert all(set(np.unique(m)) <= {0.0, 2.0} for m in mk) and not np.array_equal(mk[0][0], mk[0][1])


# -------------------------------------------------------------------------------------------------------- the fixture
def test_inputs_module_reproduces_the_stored_seeds(g):
    from stofnet_amd.kuleshov_training import CHUNKS
    for name, n, L, O, wseed, seed, p, call in ti.CASES:
        assert int(g[f'{name}.seed']) == seed and int(g[f'{name}.nbt']) == 1
        assert g[f'{name}.y'].shape == (n, 1, O) and g[f'{name}.dx'].shape == (n, 1, L)
        assert g[f'{name}.run_var.5'].shape == (342,) and g[f'{name}.grad.final_conv.bias'].shape == (2,)
    shapes = {c[1:4] for c in ti.CASES}
    assert {(2, 641, 8), (3, 800, 11), (5, 719, 64), (2, 700, 1400)} <= shapes
    assert any(c[6] == 0.0 for c in ti.CASES) and any(c[7] == 3 for c in ti.CASES)
    c = CHUNKS['conv_wgrad']                                    # a weight-gradient chunk one below, on and one above its edge
    assert c - 1 in ti.edge_rows('ks_edge255_3x865_8') and c in ti.edge_rows('ks_edge256_4x697_8') and c + 1 in ti.edge_rows('ks_edge257_1x1153_8')


@pytest.mark.parametrize('name', CHEAP)
def test_restate64_is_the_reference_float64_module_on_the_fixture(g, name):
    """max |reference fp32 - restate64| equals the stored max |reference fp32 - reference float64| to 1e-12 of the tensor's size
    for y, dx and every gradient kept in full: the restatement with the host masks IS the reference's float64 module."""
    own = own64(name)
    for key, ref in [('y', own['y']), ('dx', own['dx'])] + [(f'grad.{k}', ti.view_like_stored(own['grads'][k])) for k in ti.param_names()]:
        if key[5:] in ti.ZERO_GRADS:
            continue
        dev = float(np.abs(g[f'{name}.{key}'].astype(np.float64).reshape(ref.shape) - ref).max())
        assert abs(dev - float(g[f'{name}.dev.{key}'])) <= 1e-12 * max(float(np.abs(ref).max()), 1.0), (key, dev, float(g[f'{name}.dev.{key}']))


@pytest.mark.parametrize('name', CHEAP)
def test_forward_aten_float64_is_the_restated_network(name):
    _, n, L, O, wseed, seed, p, call = ti.case(name)
    m = make_net(name, dtype=torch.float64)
    y, dx, grads, rm, rv, dec = aten_step(m, torch.from_numpy(ti.frames(n, L, seed)).double(), torch.from_numpy(ti.cotangent(n, O, seed)).double())
    ref = own64(name)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))   # noqa: E731
    assert ti.same_decisions(dec, ref['decisions'])
    assert rel(y, ref['y']) <= 1e-12 and rel(dx, ref['dx']) <= 1e-12
    for b in range(8):
        assert np.abs(rm[b] - ref['run_mean'][b]).max() <= 1e-12 and rel(rv[b], ref['run_var'][b]) <= 1e-12
    for k in ti.param_names():
        if k not in ti.ZERO_GRADS:              # analytically 0 under train-mode BatchNorm: rounding noise on both sides
            assert rel(grads[k], ref['grads'][k]) <= 1e-12, k


@pytest.mark.parametrize('name', CHEAP)
def test_forward_aten_fp32_on_the_cpu_against_the_fixture(g, name):
    _, n, L, O, wseed, seed, p, call = ti.case(name)
    m = make_net(name)
    y, dx, grads, rm, rv, dec = aten_step(m, torch.from_numpy(ti.frames(n, L, seed)), torch.from_numpy(ti.cotangent(n, O, seed)))
    assert y.shape == (n, 1, O) and y.dtype == np.float32 and all(int(b.num_batches_tracked) == 1 for b in m._batch_norms())
    _, same = check_step(name, g, y, dx, grads, rm, rv, dec)
    if same:
        check_against_reference_fp32(name, g, y, dx, grads)


# ------------------------------------------------------------------------------------------------------------ the route
def test_route_contract_without_a_device():
    from stofnet_amd import Kuleshov
    m = Kuleshov(641, 8)
    assert Kuleshov.train_route == 'aten' and m.train_route == 'aten' and m.dropout_seed is None and m.dropout_call == 0
    assert not any(w in k for k in m.state_dict() for w in ('train_route', 'dropout_seed', 'dropout_call'))
    x = torch.randn(2, 1, 641, generator=torch.Generator().manual_seed(1))
    m.train()
    assert m(x).grad_fn is not None and int(m.down_bn0.num_batches_tracked) == 1 and m.dropout_call == 0      # 'aten': forward_aten, as ever
    for bad in ('kernel', None, 'ATEN'):
        m.train_route = bad
        with pytest.raises(ValueError, match='train_route'):
            m(x)
        m.eval()
        with pytest.raises(ValueError, match='train_route'):
            m(x)
        m.train()
    m.train_route = 'kernels'
    before = [b.running_mean.clone() for b in m._batch_norms()]
    with pytest.raises(RuntimeError, match='ROCm device'):                                   # a CPU tensor: no silent fall-back
        m(x)
    with pytest.raises(RuntimeError, match='ROCm device'):
        with torch.no_grad():
            m(x)
    assert int(m.down_bn0.num_batches_tracked) == 1 and m.dropout_call == 0 and m.dropout_seed is None
    assert all(torch.equal(a, b.running_mean) for a, b in zip(before, m._batch_norms()))
    m.eval()
    with torch.no_grad():
        assert m(x).shape == (2, 1, 8)                                                       # eval mode is unchanged: forward_aten on the CPU
    with pytest.raises(NotImplementedError, match='train mode only'):
        m.forward_train_kernels(x)
    m2 = Kuleshov(641, 8)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert m2.train_route == 'aten'


def test_main_parses_kuleshov_train(monkeypatch):
    """`main.main` up to the point where it needs a device: without kuleshov_train, model=kuleshov evaluates only whatever
    `evaluate` says; with kuleshov_train=True evaluate=False it reaches train()."""
    import main
    seen = []

    def evaluate_stub(model, name, frames, gt, cfg, log=None):
        return np.zeros((frames.shape[0], 1)), {'model': name, 'inference_time': 0.0}

    def train_stub(model, frames, gt, cfg, log=None):
        seen.append((type(model).__name__, bool(cfg.kuleshov_train), bool(cfg.evaluate), str(cfg.train_route)))
        return [{'epoch': 0}]
    monkeypatch.setattr(main, 'evaluate', evaluate_stub)
    monkeypatch.setattr(main, 'train', train_stub)
    base = ['model=kuleshov', 'device=cpu', 'num_waveforms=4', 'num_samples=700', 'upsample_factor=2', 'batch_size=2']
    assert main.config_mod.load(str(main.script_path / 'config.yaml')).kuleshov_train is False
    _, summary = main.main(base + ['evaluate=False'])
    assert seen == [] and 'train_history' not in summary and 'train_route' not in summary
    _, summary = main.main(base + ['evaluate=True', 'kuleshov_train=True'])
    assert seen == [] and 'train_history' not in summary
    _, summary = main.main(base + ['evaluate=False', 'kuleshov_train=True', 'train_route=aten'])
    assert seen == [('Kuleshov', True, False, 'aten')]
    assert summary['train_history'] == [{'epoch': 0}] and summary['train_precision'] == 'fp32'
    assert summary['train_route'] == 'aten'                     # the class default: the stub did not set the route

"""EDSR_1D training on the kernels of csrc/edsr_train.hip, without a GPU: the new C symbols, their argument checks (all
return before any HIP call), the `train_route` switch, a float64 torch-CPU restatement of the network with autograd that
reproduces every array of tests/golden/f26_edsr_training.npz (pinning the fixture independently of the reference run that
made it), and `main.py model=edsr` argument handling as far as it runs without a device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, load_weights
import edsr_training_inputs as ei
import riders_inputs as ri
from stofnet_amd import _lib
from stofnet_amd import build as sbuild
from test_riders_cpu import shuffle64

NEW_SYMBOLS = ('stof_train_edsr_in', 'stof_train_edsr_in_wgrad_workspace_bytes', 'stof_train_edsr_in_wgrad', 'stof_train_edsr_in_dgrad',
               'stof_train_edsr_out', 'stof_train_edsr_out_dgrad', 'stof_train_edsr_out_wgrad_workspace_bytes',
               'stof_train_edsr_out_wgrad')
F64_BOUND = 2e-6


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def edsr64_step(sd, num_blocks, r, x, t):
    """`edsr64` of test_riders_cpu.py with autograd: EDSR_1D in float64 on torch CPU, loss = sum(y * t)
    -> (y, d loss / d x, {parameter name: gradient}) as float64 arrays."""
    p = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in sd.items()}
    conv = lambda a, k: F.conv1d(a, p[k + '.weight'], p[k + '.bias'], padding=1)     # noqa: E731
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    first = F.relu(conv(xt, 'conv_input'))
    out = first
    for b in range(num_blocks):
        out = conv(F.relu(conv(out, f'residual_blocks.{b}.conv1')), f'residual_blocks.{b}.conv2') + out
    y = conv(shuffle64(conv(out, 'conv_mid') + first, r), 'conv_output')
    (y * torch.from_numpy(np.asarray(t, np.float64))).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


def test_new_symbols_exist(lib):
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.stof_abi_version() == 3


def test_argument_contract_returns_before_any_launch(lib):
    BAD, UNS = _lib.STOF_ERR_BAD_ARG, _lib.STOF_ERR_UNSUPPORTED
    buf = np.zeros(64, np.float32)                      # never dereferenced: every call below returns from its checks
    a = ctypes.c_void_p(buf.ctypes.data)
    big = 1 << 40
    assert lib.stof_train_edsr_in_wgrad_workspace_bytes() > 0
    for r in (1, 2, 4, 8, 16, 32, 64):
        assert lib.stof_train_edsr_out_wgrad_workspace_bytes(r) > 0
    for r in (0, 3, 128):
        assert lib.stof_train_edsr_out_wgrad_workspace_bytes(r) == 0
    # (call, positions of the pointers that may not be NULL); g2 of the conv_input pair may be
    calls = {
        'in': (lambda q, N, L, r: lib.stof_train_edsr_in(q[0], q[1], q[2], q[3], N, L, None), 4, False),
        'in_wgrad': (lambda q, N, L, r: lib.stof_train_edsr_in_wgrad(q[0], q[1], None, q[2], q[3], q[4], N, L, 1.0, q[5], big, None), 6, False),
        'in_dgrad': (lambda q, N, L, r: lib.stof_train_edsr_in_dgrad(q[0], None, q[1], q[2], q[3], N, L, 1.0, None), 4, False),
        'out': (lambda q, N, L, r: lib.stof_train_edsr_out(q[0], q[1], q[2], q[3], N, L, r, None), 4, True),
        'out_dgrad': (lambda q, N, L, r: lib.stof_train_edsr_out_dgrad(q[0], q[1], q[2], N, L, r, None), 3, True),
        'out_wgrad': (lambda q, N, L, r: lib.stof_train_edsr_out_wgrad(q[0], q[1], q[2], q[3], N, L, r, 1.0, q[4], big, None), 5, True),
    }
    for name, (call, nptr, has_r) in calls.items():
        for k in range(nptr):
            q = [a] * nptr
            q[k] = None
            assert call(q, 2, 10, 4) == BAD, (name, k)
        assert call([a] * nptr, -1, 10, 4) == BAD and call([a] * nptr, 2, -1, 4) == BAD, name
        if has_r:
            for r in (3, 128, 0, -4):
                assert call([a] * nptr, 2, 10, r) == BAD, (name, r)
        assert call([a] * nptr, 1 << 20, 1 << 12, 4) == UNS, name
        assert call([a] * nptr, 1 << 25, 1, 4) == UNS, name                     # N L 64 = 2^31 exactly
    # a workspace that is too small is refused before the launch as well
    assert lib.stof_train_edsr_in_wgrad(a, a, None, a, a, a, 2, 10, 1.0, a, 16, None) == _lib.STOF_ERR_WORKSPACE
    assert lib.stof_train_edsr_out_wgrad(a, a, a, a, 2, 10, 4, 1.0, a, 16, None) == _lib.STOF_ERR_WORKSPACE
    # empty batches of the kernels that write no gradient: STOF_OK without touching a pointer
    for name in ('in', 'in_dgrad', 'out', 'out_dgrad'):
        call, nptr, _ = calls[name]
        assert call([None] * nptr, 0, 10, 4) == _lib.STOF_OK and call([None] * nptr, 3, 0, 4) == _lib.STOF_OK, name


def test_train_route_switch():
    from stofnet_amd import EDSR_1D
    assert EDSR_1D.train_route == 'aten'
    m = EDSR_1D(1, 64, 1, 4)
    assert m.train_route == 'aten' and 'train_route' not in m.state_dict()
    x = torch.zeros(2, 1, 16)
    for bad in ('kernel', 'ATEN', None, 1):
        m.train_route = bad
        with pytest.raises(ValueError, match='train_route'):
            m(x)
    m.train_route = 'kernels'
    with pytest.raises(RuntimeError, match='ROCm device'):           # CPU tensors: the explicit call raises
        m.forward_train_kernels(x)


def test_fixture_layout():
    g = golden('f26_edsr_training')
    want = set()
    for name, _, b, r, n, L, _, last in ei.CASES:
        want |= {f'{name}.seed', f'{name}.y', f'{name}.dx'} | {f'{name}.grad.{k}' for k in ei.kept_grads(b, last)}
        want |= {f'{name}.{what}.{k}' for k in ei.sampled_grads(b, last) for what in ('gmax', 'gsum', 'grad_stride53')}
        assert sorted(ei.kept_grads(b, last) + ei.sampled_grads(b, last)) == sorted(ei.param_names(b))     # every gradient
        assert g[f'{name}.y'].shape == (n, 1, L * r) and g[f'{name}.dx'].shape == (n, 1, L)
        assert int(g[f'{name}.seed']) == ei.case(name)[6]                # CASES lists the seeds the fixture was made with
    assert set(g.files) == want
    shapes = [(c[2], c[3], c[4], c[5]) for c in ei.CASES]
    assert shapes == [(8, 4, 2, 130), (0, 1, 3, 65), (1, 2, 2, 96), (2, 16, 2, 31), (1, 64, 2, 40), (3, 8, 2, 1), (2, 4, 1, 2),
                      (1, 4, 3, 171)]
    assert ei.CASES[0][1] == 'proud-cherry' and all(isinstance(c[1], int) for c in ei.CASES[1:])


@pytest.mark.parametrize('name', ei.IDS)
def test_float64_restatement_reproduces_fixture(name):
    g = golden('f26_edsr_training')
    _, wkey, b, r, n, L, _, last = ei.case(name)
    seed = int(g[f'{name}.seed'])
    sd = ri.weights(wkey, load_weights, b, r)
    assert list(sd) == ei.param_names(b)
    y, dx, grads = edsr64_step(sd, b, r, ri.frames(n, L, seed), ei.cotangent(n, L * r, seed))
    errs = {'y': rel(g[f'{name}.y'], y), 'dx': rel(g[f'{name}.dx'], dx)}
    for k in ei.kept_grads(b, last):
        assert np.abs(grads[k]).max() >= 0.4, k                          # no gradient is compared against noise
        errs[k] = rel(g[f'{name}.grad.{k}'], grads[k])
    for k in ei.sampled_grads(b, last):                                  # max |.|, whole-tensor sum, every 53rd element
        gmax = np.abs(grads[k]).max()
        assert gmax >= 0.4, k
        errs[k + ' (gmax)'] = abs(float(g[f'{name}.gmax.{k}']) - gmax) / gmax
        errs[k + ' (stride)'] = np.abs(g[f'{name}.grad_stride53.{k}'] - grads[k].reshape(-1)[::ei.STRIDE]).max() / gmax
        # a sum of `size` elements that are each within the bound of max|.|
        errs[k + ' (sum)'] = abs(float(g[f'{name}.gsum.{k}']) - grads[k].sum()) / (gmax * grads[k].size)
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert max(errs.values()) <= F64_BOUND, errs


def test_main_edsr_argument_handling(monkeypatch):
    """`main.main` up to the point where it needs a device: model=edsr builds EDSR_1D(1, 64, 8, upsample_factor) and
    evaluate=True stays evaluate=True; the first device use (`model.to`) is where a box without a GPU stops."""
    import main
    seen = {}

    class Stop(Exception):
        pass

    def to(self, device):
        seen['model'], seen['device'] = self, device
        raise Stop

    monkeypatch.setattr(main.EDSR_1D, 'to', to)
    monkeypatch.setattr(main, 'train', lambda *a, **k: seen.setdefault('trained', True))
    with pytest.raises(Stop):
        main.main(['model=edsr', 'evaluate=True', 'upsample_factor=8', 'num_waveforms=4', 'num_samples=64', 'device=cuda'])
    m = seen['model']
    assert isinstance(m, main.EDSR_1D) and len(m.residual_blocks) == 8 and m.upscale.upsample_factor == 8
    assert m.conv_output.in_channels == 8 and m.train_route == 'aten' and 'trained' not in seen
    cfg = main.config_mod.merge(main.config_mod.load(str(main.script_path / 'config.yaml')),
                                main.config_mod.from_cli(['model=edsr', 'train_route=aten']))
    assert cfg.train_route == 'aten'
    assert main.config_mod.load(str(main.script_path / 'config.yaml')).train_route == 'kernels'

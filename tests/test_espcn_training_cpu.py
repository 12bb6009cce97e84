"""ESPCN_1D training on the kernels of csrc/espcn_train.hip, without a GPU: the new C symbols and their declarations, their
argument checks (all return before any HIP call), the `train_route` switch, this repository's `ESPCN_1D.forward_aten` on the
CPU against every array of tests/golden/f27_espcn_training.npz (pinning the fixture to our module tree; SampleShuffle1D runs
on the device only, so its permutation is restated in torch, `shuffle64` of test_riders_cpu.py), and `main.py model=espcn`
argument handling as far as it runs without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden, load_weights
import espcn_training_inputs as pi
import riders_inputs as ri
from stofnet_amd import _lib
from stofnet_amd import build as sbuild
from test_riders_cpu import shuffle64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('stof_train_espcn_repack_floats', 'stof_train_espcn_repack', 'stof_train_espcn_in', 'stof_train_espcn_mid',
               'stof_train_espcn_out', 'stof_train_espcn_out_wgrad_workspace_bytes', 'stof_train_espcn_out_wgrad',
               'stof_train_espcn_out_dgrad', 'stof_train_espcn_in_wgrad_workspace_bytes', 'stof_train_espcn_in_wgrad',
               'stof_train_espcn_in_dgrad')
Y_BOUND, GRAD_BOUND = 2e-5, 2e-4


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


class TorchShuffle(torch.nn.Module):
    """SampleShuffle1D as view / permute (utils/sample_shuffle.py:24-27), for tensors that are not on a ROCm device"""

    def __init__(self, upsample_factor):
        super().__init__()
        self.upsample_factor = upsample_factor

    def forward(self, x):
        return shuffle64(x, self.upsample_factor)


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def test_header_declares_and_lib_lists_the_new_entries():
    with open(os.path.join(ROOT, 'include', 'stofnet_amd.h')) as fh:
        header = fh.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'^(int|size_t) ' + sym + r'\(', header, re.M), sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym


def test_new_symbols_exist(lib):
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym)
    assert lib.stof_abi_version() == 3
    assert lib.stof_train_espcn_repack_floats() == 32 * 64 * 3


def test_argument_contract_returns_before_any_launch(lib):
    BAD, UNS = _lib.STOF_ERR_BAD_ARG, _lib.STOF_ERR_UNSUPPORTED
    buf = np.zeros(64, np.float32)                      # never dereferenced: every call below returns from its checks
    a = ctypes.c_void_p(buf.ctypes.data)
    big = 1 << 40
    assert lib.stof_train_espcn_in_wgrad_workspace_bytes() > 0
    for r in (1, 2, 3, 4, 10, 17, 33, 63, 64):
        assert lib.stof_train_espcn_out_wgrad_workspace_bytes(r) >= 97 * r * 4
    for r in (0, -1, 65, 128):
        assert lib.stof_train_espcn_out_wgrad_workspace_bytes(r) == 0
    calls = {
        'in': (lambda q, N, L, r: lib.stof_train_espcn_in(q[0], q[1], q[2], q[3], N, L, None), 4, False),
        'mid': (lambda q, N, L, r: lib.stof_train_espcn_mid(q[0], q[1], q[2], q[3], N, L, None), 4, False),
        'out': (lambda q, N, L, r: lib.stof_train_espcn_out(q[0], q[1], q[2], q[3], N, L, r, None), 4, True),
        'out_wgrad': (lambda q, N, L, r: lib.stof_train_espcn_out_wgrad(q[0], q[1], q[2], q[3], q[4], N, L, r, 1.0, q[5], big, None), 6, True),
        'out_dgrad': (lambda q, N, L, r: lib.stof_train_espcn_out_dgrad(q[0], q[1], q[2], q[3], q[4], N, L, r, None), 5, True),
        'in_wgrad': (lambda q, N, L, r: lib.stof_train_espcn_in_wgrad(q[0], q[1], q[2], q[3], q[4], N, L, 1.0, q[5], big, None), 6, False),
        'in_dgrad': (lambda q, N, L, r: lib.stof_train_espcn_in_dgrad(q[0], q[1], q[2], q[3], N, L, 1.0, None), 4, False),
    }
    for name, (call, nptr, has_r) in calls.items():
        for k in range(nptr):
            q = [a] * nptr
            q[k] = None
            assert call(q, 2, 10, 4) == BAD, (name, k)
        assert call([a] * nptr, -1, 10, 4) == BAD and call([a] * nptr, 2, -1, 4) == BAD, name
        if has_r:
            for r in (0, -4, 65, 128):
                assert call([a] * nptr, 2, 10, r) == BAD, (name, r)
        assert call([a] * nptr, 1 << 20, 1 << 12, 4) == UNS, name
        assert call([a] * nptr, 1 << 25, 1, 4) == UNS, name                     # N L 64 = 2^31 exactly
    assert lib.stof_train_espcn_repack(None, a, None) == BAD and lib.stof_train_espcn_repack(a, None, None) == BAD
    # a workspace that is too small is refused before the launch as well
    assert lib.stof_train_espcn_in_wgrad(a, a, a, a, a, 2, 10, 1.0, a, 16, None) == _lib.STOF_ERR_WORKSPACE
    assert lib.stof_train_espcn_out_wgrad(a, a, a, a, a, 2, 10, 4, 1.0, a, 16, None) == _lib.STOF_ERR_WORKSPACE
    # empty batches of the kernels that write no gradient: STOF_OK without touching a pointer
    for name in ('in', 'mid', 'out', 'out_dgrad', 'in_dgrad'):
        call, nptr, _ = calls[name]
        assert call([None] * nptr, 0, 10, 4) == _lib.STOF_OK and call([None] * nptr, 3, 0, 4) == _lib.STOF_OK, name


def test_train_route_switch():
    from stofnet_amd import ESPCN_1D
    assert ESPCN_1D.train_route == 'aten'
    m = ESPCN_1D(4)
    assert m.train_route == 'aten' and 'train_route' not in m.state_dict()
    m.sample_shuffle = TorchShuffle(4)
    x = torch.zeros(2, 1, 16)
    assert m(x).shape == (2, 1, 64)                                  # the default on CPU tensors: forward_aten, as before
    for bad in ('kernel', 'ATEN', None, 1):
        m.train_route = bad
        with pytest.raises(ValueError, match='train_route'):
            m(x)
    m.train_route = 'kernels'
    assert torch.equal(m(x), m.forward_aten(x))                      # CPU tensors: `forward` falls back to ATen
    with pytest.raises(RuntimeError, match='ROCm device'):           # ... the explicit call raises
        m.forward_train_kernels(x)


def test_fixture_layout():
    g = golden('f27_espcn_training')
    want = set()
    for name, _, r, n, L, seed in pi.CASES:
        want |= {f'{name}.seed', f'{name}.y', f'{name}.dx'} | {f'{name}.grad.{k}' for k in pi.PARAMS}
        assert g[f'{name}.y'].shape == (n, 1, L * r) and g[f'{name}.dx'].shape == (n, 1, L)
        assert int(g[f'{name}.seed']) == seed                        # CASES lists the seeds the fixture was made with
        assert g[f'{name}.grad.conv3.weight'].shape == (r, 32, 3) and g[f'{name}.grad.conv1.weight'].shape == (64, 1, 5)
    assert set(g.files) == want
    assert [c[1:] for c in pi.CASES[:10]] == [('vital-puddle', 4, 2, 130, 5400), ('wobbly-sponge', 4, 2, 130, 5401), (720, 1, 3, 65, 5402),
                                              (721, 2, 2, 96, 5403), (722, 3, 2, 31, 5404), (723, 10, 2, 40, 5405), (724, 17, 2, 1, 5406),
                                              (725, 33, 1, 2, 5407), (726, 64, 3, 127, 5408), (727, 4, 3, 257, 5409)]
    assert sorted(c[3] * c[4] for c in pi.CASES[10:]) == sorted(t + d for t in pi.TILES for d in (-1, 0, 1))
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'f27_espcn_training.npz')) < 1 << 20


@pytest.mark.parametrize('name', pi.IDS)
def test_forward_aten_on_cpu_reproduces_fixture(name):
    from stofnet_amd import ESPCN_1D
    g = golden('f27_espcn_training')
    _, wkey, r, n, L, _ = pi.case(name)
    seed = int(g[f'{name}.seed'])
    m = ESPCN_1D(r).train()
    m.sample_shuffle = TorchShuffle(r)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ri.weights(wkey, load_weights, r).items()}, strict=True)
    assert [k for k, _ in m.named_parameters()] == pi.PARAMS
    x = torch.from_numpy(ri.frames(n, L, seed)).requires_grad_(True)
    y = m.forward_aten(x)
    (y * torch.from_numpy(pi.cotangent(n, L * r, seed))).sum().backward()
    errs = {'y': rel(y.detach(), g[f'{name}.y']), 'dx': rel(x.grad, g[f'{name}.dx'])}
    for k, p in m.named_parameters():
        assert np.abs(g[f'{name}.grad.{k}']).max() >= 0.1, k         # no gradient is compared against noise
        errs[k] = rel(p.grad, g[f'{name}.grad.{k}'])
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert errs.pop('y') <= Y_BOUND
    assert max(errs.values()) <= GRAD_BOUND, errs


def test_main_espcn_argument_handling(monkeypatch):
    """`main.main` up to the point where it needs a device: model=espcn builds ESPCN_1D(upsample_factor) and evaluate=False
    stays evaluate=False, so that `train` is reached; the first device use (`model.to`) is where a box without a GPU stops."""
    import main
    seen = {}

    class Stop(Exception):
        pass

    def to(self, device):
        seen['model'], seen['device'] = self, device
        raise Stop

    monkeypatch.setattr(main.ESPCN_1D, 'to', to)
    with pytest.raises(Stop):
        main.main(['model=espcn', 'evaluate=False', 'upsample_factor=8', 'num_waveforms=4', 'num_samples=64', 'device=cuda'])
    m = seen['model']
    assert isinstance(m, main.ESPCN_1D) and m.sample_shuffle.upsample_factor == 8 and m.conv3.out_channels == 8
    assert m.train_route == 'aten'

    # past the device: `main` hands the model to `train` with evaluate still False, and the summary names the route
    calls = {}

    def fake_train(model, frames, gt, cfg, log=None):
        calls['evaluate'], calls['route'] = bool(cfg.evaluate), str(cfg.train_route)
        model.train_route = str(cfg.train_route)
        return [{'epoch': 0}]

    monkeypatch.setattr(main.ESPCN_1D, 'to', lambda self, device: self)
    monkeypatch.setattr(main, 'train', fake_train)
    monkeypatch.setattr(main, 'evaluate', lambda *a, **k: ([], {'inference_time': 0.0}))
    _, summary = main.main(['model=espcn', 'evaluate=False', 'train_route=aten', 'num_waveforms=4', 'num_samples=64',
                            'device=cpu', 'logging=Null'])
    assert calls == {'evaluate': False, 'route': 'aten'}                        # train_route=aten reaches the model
    assert summary['train_route'] == 'aten' and summary['train_precision'] == 'fp32' and summary['train_history'] == [{'epoch': 0}]
    calls.clear()
    main.main(['model=espcn', 'evaluate=True', 'num_waveforms=4', 'num_samples=64', 'device=cpu', 'logging=Null'])
    assert calls == {}                                                           # evaluate=True still only evaluates
    assert main.config_mod.load(str(main.script_path / 'config.yaml')).train_route == 'kernels'

"""The SincNet baseline without a GPU: construction, the reference's state_dict layout and default initialisation,
strict loads of both shipped checkpoints, the drop-in import paths, the option checks, a float64 NumPy/torch-CPU
restatement of the network that reproduces tests/golden/f19_sincnet.npz (pinning the fixture independently of the
reference run that made it), the host-side filter synthesis and weight packer, and the C ABI's argument checks, which
all return before any HIP call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden
import sincnet_inputs as si
from stofnet_amd import _lib
from stofnet_amd import build as sbuild

CASE_IDS = [c[0] for c in si.CASES]


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope='module')
def g():
    return golden('f19_sincnet')


def case(name):
    return next(c for c in si.CASES if c[0] == name)


def weights(wkey):
    """float32 state_dict of a case: a shipped checkpoint (sincnet_inputs.checkpoint_weights), or (`init`) the default
    model with seeded convs."""
    if wkey != 'init':
        return si.checkpoint_weights(wkey)
    from stofnet_amd import SincNet
    sd = {k: v.numpy().copy() for k, v in SincNet(si.options(1e6, 2000)).state_dict().items()}
    sd.update(si.seeded_convs(si.INIT_WSEED))
    return sd


def bank64(fs, low_hz, band_hz):
    """SincConv_fast.forward's filter bank (models/sincnet.py:147-188) in float64 -> [128, 1023]."""
    low = 50.0 + np.abs(np.asarray(low_hz, np.float64).reshape(-1, 1))
    high = np.clip(low + 50.0 + np.abs(np.asarray(band_hz, np.float64).reshape(-1, 1)), 50.0, fs / 2)
    band = high - low
    n = 2 * np.pi * np.arange(-511, 0, dtype=np.float64)[None, :] / fs
    win = 0.54 - 0.46 * np.cos(2 * np.pi * np.linspace(0, 1023 / 2 - 1, 511) / 1023)
    left = (np.sin(high * n) - np.sin(low * n)) / (n / 2) * win
    return np.concatenate([left, 2 * band, left[:, ::-1]], 1) / (2 * band)


def forward64(sd, fs, x, eps=1e-5):
    """SincNet.forward in float64 on torch CPU -> (y [N, 1, L], [the act[0..2] outputs])."""
    d = lambda k: torch.from_numpy(np.asarray(sd[k], np.float64))     # noqa: E731
    a = torch.from_numpy(np.asarray(x, np.float64)).reshape(x.shape[0], 1, x.shape[-1])
    acts = []
    for i, k in enumerate((1023, 11, 9, 7)):
        a = F.pad(a, ((k - 1) // 2, (k - 1) // 2))
        if i == 0:
            a = F.conv1d(a, torch.from_numpy(bank64(fs, sd['conv.0.low_hz_'], sd['conv.0.band_hz_']))[:, None, :])
        else:
            a = F.conv1d(a, d(f'conv.{i}.weight'), d(f'conv.{i}.bias'))
        a = F.batch_norm(a, d(f'bn.{i}.running_mean'), d(f'bn.{i}.running_var'), d(f'bn.{i}.weight'), d(f'bn.{i}.bias'),
                         False, 0.0, eps)
        if i < 3:
            a = F.leaky_relu(a, 0.2)
            acts.append(a)
    return a.numpy(), [t.numpy() for t in acts]


def checkpoint_layout(key):
    """names, shapes and dtypes of the shipped checkpoint's state_dict (manifest_sincnet.json)"""
    with open(os.path.join(GOLDEN, 'manifest_sincnet.json')) as fh:
        return json.load(fh)['layout'][key]


def test_construct_state_dict_and_default_init(g):
    from stofnet_amd import SincNet
    m = SincNet(si.options(1e6, 2000))
    sd = m.state_dict()
    assert len(sd) == 28 and sum(v.dtype == torch.int64 for v in sd.values()) == 4
    assert sum(p.numel() for p in m.parameters()) == 329859
    for key in si.CHECKPOINTS:
        assert {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()} == checkpoint_layout(key)
        assert list(sd) == list(checkpoint_layout(key))
    assert np.array_equal(m.conv[0].low_hz_.detach().numpy(), g['init_low_hz'])
    assert np.array_equal(m.conv[0].band_hz_.detach().numpy(), g['init_band_hz'])
    assert [type(a).__name__ for a in m.act] == ['LeakyReLU'] * 4
    assert [a.negative_slope for a in m.act] == [0.2, 0.2, 0.2, 1]
    assert len(m.ln) == 0 and len(m.drop) == 4 and all(b.momentum == 0.05 and b.eps == 1e-5 for b in m.bn)


@pytest.mark.parametrize('key', list(si.CHECKPOINTS))
def test_shipped_checkpoints_load_strict(key):
    from stofnet_amd import SincNet
    m = SincNet(si.options(1e6, 2000))
    sd = si.checkpoint_weights(key)
    assert {k: [list(v.shape), str(torch.from_numpy(np.asarray(v)).dtype)] for k, v in sd.items()} == checkpoint_layout(key)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)


def test_dropin_import_paths():
    import models
    import stofnet_amd
    from models.sincnet import SincNet
    assert models.SincNet is stofnet_amd.SincNet is SincNet
    with pytest.raises(NotImplementedError):
        models.SincNet()


@pytest.mark.parametrize('key,value', [('cnn_N_filt', [64, 128, 128, 1]), ('cnn_len_filt', [251, 11, 9, 7]),
                                       ('cnn_max_pool_len', [3, 1, 1, 1]), ('cnn_use_laynorm_inp', True),
                                       ('cnn_use_batchnorm_inp', True), ('cnn_use_laynorm', [True, False, False, False]),
                                       ('cnn_use_batchnorm', [True, True, True, False]),
                                       ('cnn_act', ['relu', 'leaky_relu', 'leaky_relu', 'linear']), ('use_sinc', False),
                                       ('fs', 0), ('fs', -1.0), ('fs', float('inf')), ('fs', None)])
def test_unsupported_options_raise(key, value):
    from stofnet_amd import SincNet
    opts = si.options(1e6, 2000)
    opts[key] = value
    with pytest.raises(NotImplementedError, match=key):
        SincNet(opts)
    del opts[key]
    with pytest.raises(NotImplementedError, match=key):
        SincNet(opts)


def test_accepted_options_and_training_errors():
    from stofnet_amd import SincNet
    opts = si.options(312.5e6, 1536)
    opts['cnn_drop'] = [0.1, 0.2, 0.0, 0.5]                            # eval makes dropout a no-op
    opts['cnn_len_filt'] = (1023, 11, 9, 7)
    m = SincNet(opts)
    assert [d.p for d in m.drop] == [0.1, 0.2, 0.0, 0.5]
    x = torch.zeros(2, 1, 100)
    with torch.no_grad():                                              # train mode: BatchNorm would use batch statistics
        with pytest.raises(NotImplementedError, match='training'):
            m(x)
    m.eval()
    with pytest.raises(RuntimeError, match='ROCm device'):
        m(x)


def test_main_needs_fs():
    import main
    with pytest.raises(ValueError, match='fs'):
        main.main(['model=sincnet', 'num_waveforms=4', 'num_samples=100'])


@pytest.mark.parametrize('name', CASE_IDS)
def test_float64_restatement_reproduces_fixture(g, name):
    _, wkey, fs, shape, seed, step = case(name)
    x = si.frames(shape, seed)
    assert x.shape == tuple(shape)
    ry = g[f'{name}_y']
    assert ry.shape == (len(range(0, shape[0], step)), 1, shape[-1])
    y, acts = forward64(weights(wkey), fs, x[::step])
    assert np.abs(y - ry).max() <= 1e-5 * np.abs(ry).max()
    if name == si.LAYER_CASE:
        e = si.LAYER_EDGE
        for i in range(3):
            ref = g['layers'][i]
            got = np.concatenate([acts[i][0, :, :e], acts[i][0, :, -e:]], -1)
            assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), i


@pytest.mark.parametrize('name', si.BANK_CASES)
def test_filter_bank(lib, g, name):
    from stofnet_amd.sincnet import filter_bank
    _, wkey, fs, _, _, _ = case(name)
    sd = weights(wkey)
    ref = g[f'{name}_filters'][:, 0]
    got = filter_bank(fs, sd['conv.0.low_hz_'], sd['conv.0.band_hz_']).numpy()[:, 0]
    assert np.array_equal(got[:, 512:], got[:, 510::-1])                   # symmetric around the centre tap
    assert np.abs(got[::si.BANK_STEP, :512] - ref).max() <= 1e-5 * np.abs(ref).max()
    b64 = bank64(fs, sd['conv.0.low_hz_'], sd['conv.0.band_hz_'])
    assert np.array_equal(got, b64.astype(np.float32)) or np.abs(got - b64).max() <= 1e-6 * np.abs(b64).max()
    if name == 'clamp':
        low = 50 + np.abs(sd['conv.0.low_hz_'][:, 0].astype(np.float64))
        assert (low > fs / 2).sum() == 29 and np.isfinite(got).all()


def unpack(blob):
    """Invert the packed layout documented in csrc/sincnet.hip -> (dense conv weights [k order], s/t affines, w3)."""
    f = blob.view(np.float32)
    al = lambda v: (v + 63) // 64 * 64                                   # noqa: E731
    at, out = 0, {}

    def frag(K):
        nonlocal at
        G = K // 8
        fr = f[at:at + 128 * K].reshape(4, G, 64, 4)
        dense = np.zeros((128, K), np.float32)
        lane = np.arange(64)
        for q in range(G):
            for e in range(4):
                dense[32 * np.arange(4)[:, None] + (lane & 31)[None, :], 8 * q + 4 * (lane >> 5)[None, :] + e] = fr[:, q, :, e]
        at = al(at + 128 * K)
        return dense

    def st(n):
        nonlocal at
        v = f[at:at + 2 * n].reshape(2, n)
        at = al(at + 2 * n)
        return v

    out['bank'], out['st0'] = frag(1024), st(128)
    out['w1'], out['st1'] = frag(11 * 128), st(128)
    out['w2'], out['st2'] = frag(9 * 128), st(128)
    out['w3'] = f[at:at + 7 * 128].reshape(7, 128); at = al(at + 7 * 128)
    out['st3'] = st(1)
    assert at * 4 == blob.size
    return out


def test_packer_round_trip(lib):
    from stofnet_amd.sincnet import filter_bank, pack_weights
    sd = si.checkpoint_weights('noble-monkey')
    fs = 1.25e9
    params = [v for k, v in sd.items() if not k.endswith('num_batches_tracked')]
    assert len(params) == 24
    u = unpack(pack_weights(fs, params).numpy())
    bank = filter_bank(fs, sd['conv.0.low_hz_'], sd['conv.0.band_hz_']).numpy()[:, 0]
    assert np.array_equal(u['bank'][:, :1023], bank) and not u['bank'][:, 1023].any()
    for i, (name, k) in enumerate((('w1', 11), ('w2', 9)), start=1):
        w = sd[f'conv.{i}.weight']                                       # [oc][ci][tap] -> k = tap * 128 + ci
        assert np.array_equal(u[name].reshape(128, k, 128), w.transpose(0, 2, 1))
    assert np.array_equal(u['w3'], sd['conv.3.weight'][0].T)
    for i in range(4):
        d = lambda k: sd[f'bn.{i}.{k}'].astype(np.float64)                # noqa: E731
        s = d('weight') / np.sqrt(d('running_var') + 1e-5)
        b = sd[f'conv.{i}.bias'].astype(np.float64) if i else 0.0
        t = (b - d('running_mean')) * s + d('bias')
        assert np.allclose(u[f'st{i}'][0], s, rtol=1e-7, atol=0) and np.allclose(u[f'st{i}'][1], t, rtol=1e-6, atol=1e-7)


def test_abi_argument_checks_without_gpu(lib):
    r = ctypes.byref
    ok = _lib.SincNetDesc(1e6, 1e-5, 0, 0)
    bads = [_lib.SincNetDesc(fs, 1e-5, 0, 0) for fs in (0.0, -1.0, float('inf'), float('nan'))]
    assert lib.stof_sincnet_packed_bytes(r(ok)) > 0 and lib.stof_sincnet_packed_bytes(None) == 0
    for b in bads:
        assert lib.stof_sincnet_packed_bytes(r(b)) == 0 and lib.stof_sincnet_workspace_bytes(r(b), 4, 2000) == 0
    assert lib.stof_sincnet_workspace_bytes(r(ok), 0, 2000) == 0 and lib.stof_sincnet_workspace_bytes(r(ok), 4, 0) == 0
    for N, L in ((1, 2000), (8, 2000), (3, 1), (5, 20001)):           # two buffers of (N (L + 8) + 8) x 128 floats
        assert lib.stof_sincnet_workspace_bytes(r(ok), N, L) == 2 * 512 * (N * (L + 8) + 8)
    # pack: NULL arguments, a too small output buffer, a bad desc
    n = lib.stof_sincnet_packed_bytes(r(ok))
    buf = np.zeros(n, np.uint8)
    arrs = [np.ascontiguousarray(v, np.float32) for k, v in si.checkpoint_weights('pretty-brook').items()
            if not k.endswith('num_batches_tracked')]
    ptrs = (ctypes.c_void_p * 24)(*[a.ctypes.data for a in arrs])
    pack = lib.stof_sincnet_pack_weights
    assert pack(r(ok), ptrs, buf.ctypes.data, n - 4) == _lib.STOF_ERR_WORKSPACE
    assert pack(r(ok), None, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(ok), ptrs, None, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(bads[0]), ptrs, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    holes = (ctypes.c_void_p * 24)(*[a.ctypes.data for a in arrs])
    holes[23] = None
    assert pack(r(ok), holes, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(ok), ptrs, buf.ctypes.data, n) == _lib.STOF_OK
    # forward: every failing check returns before a HIP call (host pointers stand in for device ones)
    h = np.zeros(64, np.float32).ctypes.data
    ws = lib.stof_sincnet_workspace_bytes(r(ok), 4, 2000)
    fwd = lib.stof_sincnet_forward
    assert fwd(r(ok), h, 4, 2000, h, h, h, ws - 1, None) == _lib.STOF_ERR_WORKSPACE
    for N, L in ((0, 2000), (-1, 2000), (4, 0), (4, -5)):
        assert fwd(r(ok), h, N, L, h, h, h, 1 << 40, None) == _lib.STOF_ERR_BAD_ARG
    for b in bads:
        assert fwd(r(b), h, 4, 2000, h, h, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(None, h, 4, 2000, h, h, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(r(_lib.SincNetDesc(1e6, 1e-5, 4, 0)), h, 4, 2000, h, h, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    for i in range(4):                                                   # x, packed, y, workspace
        args = [h, h, h, h]
        args[i] = None
        assert fwd(r(ok), args[0], 4, 2000, args[1], args[2], args[3], ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(r(ok), h, 1 << 20, 1 << 12, h, h, h, 1 << 62, None) == _lib.STOF_ERR_UNSUPPORTED

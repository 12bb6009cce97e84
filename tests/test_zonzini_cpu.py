"""The Zonzini baselines without a GPU: construction, the reference's state_dict layout, the drop-in import paths, a
float64 torch-CPU restatement of the network that reproduces tests/golden/f18_zonzini.npz (pinning the fixture
independently of the reference run that made it), the host-side weight packer, and the C ABI's argument checks, which
all return before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, load_weights
import zonzini_inputs as zi
from stofnet_amd import _lib
from stofnet_amd import build as sbuild

CASES = [('small_chirp', 'small', 256, 2000), ('small_min', 'small', 8, 936), ('small_odd', 'small', 8, 1537),
         ('small_long', 'small', 16, 20000), ('small_one', 'small', 1, 2000), ('large_min', 'large', 4, 3752),
         ('large_odd', 'large', 32, 4001), ('large_long', 'large', 8, 20000), ('large_longest', 'large', 4, 30720)]


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


def weights(net, g):
    if net == 'small':
        return load_weights('graceful-wave')
    return zi.seeded_weights(zi.LARGE_CHANNELS, int(g['large_wseed']))


def forward64(sd, x):
    """models/zonzini.py's forward in float64 on torch CPU -> (y [N, 1], pooled features [N, C])."""
    a = torch.from_numpy(np.asarray(x, np.float64))
    i = 0
    while f'conv_layers.{i}.weight' in sd:
        w = torch.from_numpy(sd[f'conv_layers.{i}.weight'].astype(np.float64))
        b = torch.from_numpy(sd[f'conv_layers.{i}.bias'].astype(np.float64))
        a = F.max_pool1d(F.relu(F.conv1d(a, w, b, stride=2)), 2)
        i += 1
    f = a.mean(-1)
    h = F.relu(f @ torch.from_numpy(sd['fc1.weight'].astype(np.float64)).T + torch.from_numpy(sd['fc1.bias'].astype(np.float64)))
    y = h @ torch.from_numpy(sd['fc2.weight'].astype(np.float64)).T + torch.from_numpy(sd['fc2.bias'].astype(np.float64))
    return y.numpy(), f.numpy()


def test_construct_without_gpu_and_state_dict_layout():
    from stofnet_amd import ZonziniNetLarge, ZonziniNetSmall
    for cls, chans, tensors, count in ((ZonziniNetSmall, zi.SMALL_CHANNELS, 12, 134481),
                                       (ZonziniNetLarge, zi.LARGE_CHANNELS, 14, 1259299)):
        m = cls()
        sd = m.state_dict()
        assert len(sd) == tensors
        assert sum(v.numel() for v in sd.values()) == count
        ref = zi.seeded_weights(chans, 0)
        assert list(sd) == list(ref)
        assert {k: tuple(v.shape) for k, v in sd.items()} == {k: v.shape for k, v in ref.items()}
        assert all(v.dtype == torch.float32 and v.device.type == 'cpu' for v in sd.values())


def test_shipped_checkpoint_loads_strict():
    from stofnet_amd import ZonziniNetSmall
    m = ZonziniNetSmall()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in load_weights('graceful-wave').items()}, strict=True)


def test_dropin_import_paths():
    import models
    import stofnet_amd
    from models.zonzini import ZonziniNetLarge, ZonziniNetSmall
    assert models.ZonziniNetSmall is stofnet_amd.ZonziniNetSmall is ZonziniNetSmall
    assert models.ZonziniNetLarge is stofnet_amd.ZonziniNetLarge is ZonziniNetLarge
    for name in ('SincNet', 'Kuleshov', 'WaveUnet'):
        with pytest.raises(NotImplementedError):
            getattr(models, name)()


@pytest.mark.parametrize('name,net,n,L', CASES)
def test_float64_restatement_reproduces_fixture(name, net, n, L):
    g = golden('f18_zonzini')
    x = zi.echo_frames(n, L, int(g[f'{name}_seed']))
    assert x.shape == (n, 1, L)
    y, f = forward64(weights(net, g), x)
    ry, rf = g[f'{name}_y'], g[f'{name}_feat']
    assert y.shape == ry.shape and f.shape == rf.shape
    assert np.abs(y - ry).max() <= 1e-5 * np.abs(ry).max()
    assert np.abs(f - rf).max() <= 1e-5 * np.abs(rf).max()


def unpack(blob, variant, sd):
    """Invert the packed layout documented in csrc/zonzini.hip -> dict of dense float32 arrays."""
    chans = zi.SMALL_CHANNELS if variant == _lib.ZONZINI_SMALL else zi.LARGE_CHANNELS
    pad = [(c + 3) // 4 * 4 for c in chans]
    al = lambda v: (v + 63) // 64 * 64                                     # noqa: E731
    f = blob.view(np.float32)
    at, out = 0, {}
    out['conv_layers.0.weight'] = f[at:at + chans[0] * 10].reshape(chans[0], 1, 10); at = al(at + pad[0] * 10)
    out['conv_layers.0.bias'] = f[at:at + chans[0]]; at = al(at + pad[0])
    for i in range(1, len(chans)):
        cp, cin, co = pad[i - 1], chans[i - 1], chans[i]
        nt, groups = (co + 31) // 32, 10 * cp // 8
        frag = f[at:at + nt * groups * 256].reshape(nt, groups, 64, 4)
        dense = np.zeros((32 * nt, 10 * cp), np.float32)
        lane = np.arange(64)
        for q in range(groups):
            for s in range(4):
                dense[32 * np.arange(nt)[:, None] + (lane & 31)[None, :], 8 * q + 4 * (lane >> 5)[None, :] + s] = frag[:, q, :, s]
        k = dense.reshape(32 * nt, 10, cp)                                  # [oc][tap][ci]
        assert not k[co:].any() and not k[:, :, cin:].any()                 # padding is zero
        out[f'conv_layers.{i}.weight'] = k[:co, :, :cin].transpose(0, 2, 1)
        at = al(at + nt * groups * 256)
        out[f'conv_layers.{i}.bias'] = f[at:at + co]
        assert not f[at + co:at + 32 * nt].any()
        at = al(at + 32 * nt)
    C = chans[-1]
    out['fc1.weight'] = f[at:at + C * 1024].reshape(C, 1024).T; at = al(at + C * 1024)
    out['fc1.bias'] = f[at:at + 1024]; at = al(at + 1024)
    out['fc2.weight'] = f[at:at + 1024].reshape(1, 1024); at = al(at + 1024)
    out['fc2.bias'] = f[at:at + 1]; at = al(at + 1)
    assert at * 4 == blob.size
    return out


@pytest.mark.parametrize('variant', [_lib.ZONZINI_SMALL, _lib.ZONZINI_LARGE])
def test_packer_round_trip(lib, variant):
    from stofnet_amd.zonzini import pack_weights
    chans = zi.SMALL_CHANNELS if variant == _lib.ZONZINI_SMALL else zi.LARGE_CHANNELS
    sd = zi.seeded_weights(chans, 17 + variant)
    blob = pack_weights(variant, list(sd.values())).numpy()
    back = unpack(blob, variant, sd)
    assert list(back) == list(sd)
    for k in sd:
        assert np.array_equal(back[k], sd[k]), k


def test_abi_argument_checks_without_gpu(lib):
    small, large, bad = (_lib.ZonziniDesc(v, 0) for v in (_lib.ZONZINI_SMALL, _lib.ZONZINI_LARGE, 7))
    r = ctypes.byref
    assert lib.stof_zonzini_packed_bytes(r(bad)) == 0 and lib.stof_zonzini_packed_bytes(None) == 0
    assert lib.stof_zonzini_packed_bytes(r(small)) > 0
    assert lib.stof_zonzini_workspace_bytes(r(small), 4, 935) == 0
    assert lib.stof_zonzini_workspace_bytes(r(small), 0, 2000) == 0
    assert lib.stof_zonzini_workspace_bytes(r(large), 4, 3751) == 0
    assert lib.stof_zonzini_workspace_bytes(r(bad), 4, 4000) == 0
    ws1 = lib.stof_zonzini_workspace_bytes(r(large), 1, 4000)
    assert lib.stof_zonzini_workspace_bytes(r(large), 8, 4000) >= 8 * ws1 - 2 * 256
    # pack: NULL arguments, a too small output buffer
    n = lib.stof_zonzini_packed_bytes(r(small))
    buf = np.zeros(n, np.uint8)
    arrs = list(zi.seeded_weights(zi.SMALL_CHANNELS, 1).values())
    ptrs = (ctypes.c_void_p * 12)(*[a.ctypes.data for a in arrs])
    assert lib.stof_zonzini_pack_weights(r(small), ptrs, buf.ctypes.data, n - 4) == _lib.STOF_ERR_WORKSPACE
    assert lib.stof_zonzini_pack_weights(r(small), None, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert lib.stof_zonzini_pack_weights(r(bad), ptrs, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert lib.stof_zonzini_pack_weights(r(small), ptrs, None, n) == _lib.STOF_ERR_BAD_ARG
    holes = (ctypes.c_void_p * 12)(*[a.ctypes.data for a in arrs])
    holes[5] = None
    assert lib.stof_zonzini_pack_weights(r(small), holes, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    # forward: every failing check returns before a HIP call (host pointers stand in for device ones)
    h = np.zeros(64, np.float32).ctypes.data
    ws = lib.stof_zonzini_workspace_bytes(r(small), 4, 2000)
    fwd = lib.stof_zonzini_forward
    assert fwd(r(small), h, 4, 935, h, h, None, h, 1 << 40, None) == _lib.STOF_ERR_POOL_EMPTY
    assert fwd(r(large), h, 4, 3751, h, h, None, h, 1 << 40, None) == _lib.STOF_ERR_POOL_EMPTY
    assert fwd(r(large), h, 4, 936, h, h, None, h, 1 << 40, None) == _lib.STOF_ERR_POOL_EMPTY
    assert fwd(r(small), h, 4, 2000, h, h, None, h, ws - 1, None) == _lib.STOF_ERR_WORKSPACE
    assert fwd(r(small), h, 0, 2000, h, h, None, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(r(small), h, -1, 2000, h, h, None, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(r(bad), h, 4, 2000, h, h, None, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(None, h, 4, 2000, h, h, None, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    for i in range(4):                                      # x, packed, y, workspace
        args = [h, h, h, h]
        args[i] = None
        assert fwd(r(small), args[0], 4, 2000, args[1], args[2], None, args[3], ws, None) == _lib.STOF_ERR_BAD_ARG

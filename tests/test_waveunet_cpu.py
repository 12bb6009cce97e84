"""WaveUnet without a GPU: construction, names and parameter counts against the reference's (tests/golden/f23_waveunet.npz,
make_golden_waveunet.py); a float64 numpy restatement of the network (`waveunet64`: BatchNorm folded in double, ATen's
fp32 interpolation coordinates) against every fixture case; the host packer inverted by the layout documented at the top
of csrc/waveunet.hip; `forward_aten` on the CPU; the length contract of `forward_aten` and of `main.py model=unet`.

Bounds: the reference's own fp32 result is within 1.6e-6 x max|ref| of `waveunet64` on these shapes, so 1e-5 leaves a
margin of about 6x.  With double coordinates instead of ATen's fp32 ones the (2, 8000) case is off by 1.75e-5 x max with
these seeds (against 9.3e-7 with the fp32 ones): the fixture tells the two apart, which
`test_double_coordinates_do_not_match` pins."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import golden
import waveunet_inputs as wi
from stofnet_amd import _lib
from stofnet_amd import build as sbuild

_f64_cache = {}


@pytest.fixture(scope='module')
def g():
    return golden('f23_waveunet')


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def fold(sd, conv, bn):
    """eval-mode BatchNorm folded into the convolution in double, rounded to fp32 once (what the packer stores)"""
    s = sd[bn + '.weight'].astype(np.float64) / np.sqrt(sd[bn + '.running_var'].astype(np.float64) + 1e-5)
    w = sd[conv + '.weight'].astype(np.float64) * s[:, None, None]
    b = (sd[conv + '.bias'].astype(np.float64) - sd[bn + '.running_mean'].astype(np.float64)) * s + sd[bn + '.bias'].astype(np.float64)
    return w.astype(np.float32), b.astype(np.float32)


def conv64(x, w, b):
    """x [N, Cin, L] float64, w [Cout, Cin, k] (odd k, padding k // 2), b [Cout] -> [N, Cout, L]"""
    k = w.shape[-1]
    xp = np.pad(x, ((0, 0), (0, 0), (k // 2, k // 2)))
    L = x.shape[-1]
    out = np.zeros((x.shape[0], w.shape[0], L))
    w = w.astype(np.float64)
    for j in range(k):
        out += np.einsum('oc,ncl->nol', w[:, :, j], xp[:, :, j:j + L])
    return out + b.astype(np.float64)[None, :, None]


def interp2(o, fp32_coords=True):
    """x2 linear interpolation with align_corners of [N, C, M] -> [N, C, 2 M]; the coordinates are ATen's: everything in
    fp32 (scale = float(M - 1) / float(2 M - 1), r = scale * j, i0 = (int) r, l1 = r - i0, l0 = 1 - l1), or in double."""
    M = o.shape[-1]
    f = np.float32 if fp32_coords else np.float64
    scale = f(M - 1) / f(2 * M - 1)
    r = scale * np.arange(2 * M).astype(f)
    assert r.dtype == f
    i0 = np.minimum(r.astype(np.int64), M - 1)
    i1 = np.minimum(i0 + 1, M - 1)
    l1 = np.clip(r - i0.astype(f), f(0), f(1))
    l0 = f(1) - l1
    assert l0.dtype == f
    return l0.astype(np.float64) * o[:, :, i0] + l1.astype(np.float64) * o[:, :, i1]


def waveunet64(sd, n, x, fp32_coords=True):
    """(y, logits, bottleneck) of WaveUnet(n, 16) in float64 from the folded fp32 weights"""
    leaky = lambda v: np.where(v > 0, v, 0.1 * v)
    blocks = wi.block_names(n)
    x = x.astype(np.float64)
    o, skips = x, []
    for i in range(n):
        o = leaky(conv64(o, *fold(sd, *blocks[i][:2])))
        skips.append(o)
        o = o[:, :, ::2]
    bott = o = leaky(conv64(o, *fold(sd, *blocks[n][:2])))
    for i in range(n):
        o = np.concatenate([interp2(o, fp32_coords), skips[n - 1 - i]], 1)
        o = leaky(conv64(o, *fold(sd, *blocks[n + 1 + i][:2])))
    w, b = sd['out.0.weight'].astype(np.float64), sd['out.0.bias'].astype(np.float64)
    logits = np.einsum('oc,ncl->nol', w[:, :, 0], np.concatenate([o, x], 1)) + b[None, :, None]
    return np.tanh(logits), logits, bott


def case64(g, name):
    """(state dict, x, (y, logits, bottleneck) in float64) of a fixture case, computed once per session"""
    if name not in _f64_cache:
        _, n, wseed, N, L, _ = wi.case(name)
        sd = wi.seeded_waveunet(n, wseed)
        x = wi.frames(N, L, int(g[f'{name}_seed']))
        _f64_cache[name] = (sd, x, waveunet64(sd, n, x))
    return _f64_cache[name]


def make(sd, n):
    from stofnet_amd import WaveUnet
    m = WaveUnet(n, 16)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m


# ------------------------------------------------------------------------------------------- construction and names
@pytest.mark.parametrize('n,count', [(2, 37762), (10, 2700418)])
def test_names_shapes_and_counts(g, n, count):
    from stofnet_amd import WaveUnet
    m = WaveUnet(n, 16)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f'names_n{n}']]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g[f'shapes_n{n}']]
    assert sum(p.numel() for p in m.parameters()) == count
    seeded = wi.seeded_waveunet(n, 1)
    assert list(seeded.keys()) == list(sd.keys())
    make(seeded, n)                                                      # strict load
    assert len(m._kernel_params()) == 6 * (2 * n + 1) + 2


def test_constructor_contract():
    import models
    from models.wave_unet import Model
    from stofnet_amd import WaveUnet
    assert Model is WaveUnet and models.WaveUnet is WaveUnet
    with pytest.raises(NotImplementedError, match='out of scope'):
        WaveUnet()
    with pytest.raises(NotImplementedError, match='channels_interval=16'):
        WaveUnet(2, 24)
    for bad in (0, 13):
        with pytest.raises(ValueError):
            WaveUnet(bad, 16)
    with pytest.raises(NotImplementedError):
        models.Kuleshov()


# --------------------------------------------------------------------------------------------- float64 restatement
@pytest.mark.parametrize('name', wi.IDS)
def test_float64_restatement_matches_fixture(g, name):
    _, n, _, N, L, _ = wi.case(name)
    _, _, (y, logits, bott) = case64(g, name)
    rows = wi.kept_rows(N, L)
    errs = {'y': rel(y[rows], g[f'{name}_y']), 'logits': rel(logits[rows], g[f'{name}_logits']),
            'bott': rel(wi.bott_edges(bott[rows]), g[f'{name}_bott'])}
    print(name, errs)
    assert max(errs.values()) <= 1e-5


def test_double_coordinates_do_not_match(g):
    name = 'unet_n2_2x8000'
    sd, x, _ = case64(g, name)
    y, logits, _ = waveunet64(sd, 2, x, fp32_coords=False)
    err = max(rel(y[[1]], g[f'{name}_y']), rel(logits[[1]], g[f'{name}_logits']))
    print('double coordinates', err)
    assert err > 1e-5


# ------------------------------------------------------------------------------------------------------- the packer
def ntw(tiles):
    return tiles if tiles <= 4 else (4 if (tiles % 4 == 0 or tiles % 3 != 0) else 3)


def unpack(blob, n):
    """Invert the blob layout documented in csrc/waveunet.hip -> (enc0 w [16, 1, 15], enc0 b, [(w [Cout, Cin, taps], b)]
    of the GEMM convolutions in blob order, head [18]); asserts that all padding is zero and the sizes add up."""
    f = np.frombuffer(blob, np.float32)
    up = lambda v: (v + 63) // 64 * 64
    e0 = f[:256].reshape(16, 16)
    at = 256
    convs = []
    for _, _, co, ci, k in wi.block_names(n)[1:]:
        tiles = co // 16
        ntp = -(-tiles // ntw(tiles)) * ntw(tiles)
        G = k * ci // 16
        frag = f[at:at + ntp * G * 256].reshape(ntp, G, 64, 4); at += ntp * G * 256
        bias = f[at:at + 16 * ntp]; at = up(at + 16 * ntp)
        assert not frag[tiles:].any() and not bias[co:].any()
        w = np.zeros((co, ci, k), np.float32)
        lane = np.arange(64)
        j, q = lane & 15, lane >> 4
        gi = 0
        for c0 in range(0, ci, 192):
            cw = min(192, ci - c0)
            for tap in range(k):
                for b in range(cw // 16):
                    for t in range(tiles):
                        for e in range(4):
                            w[16 * t + j, c0 + 16 * b + 4 * q + e, tap] = frag[t, gi, :, e]
                    gi += 1
        assert gi == G
        convs.append((w, bias[:co].copy()))
    head = f[at:at + 18]; at = up(at + 18)
    assert at == f.size
    return e0[:15].T.reshape(16, 1, 15), e0[15], convs, head


@pytest.mark.parametrize('n', [1, 2, 7, 12])
def test_packer_layout(lib, n):
    from stofnet_amd.waveunet import pack_waveunet_weights
    sd = wi.seeded_waveunet(n, 30 + n)
    blob = pack_waveunet_weights(n, wi.kernel_arrays(sd)).numpy().tobytes()
    w0, b0, convs, head = unpack(blob, n)
    blocks = wi.block_names(n)
    w, b = fold(sd, *blocks[0][:2])
    assert np.array_equal(w0, w) and np.array_equal(b0, b)
    for (cw, cb), blk in zip(convs, blocks[1:]):
        w, b = fold(sd, *blk[:2])
        assert np.array_equal(cw, w) and np.array_equal(cb, b)
    assert np.array_equal(head[:17], sd['out.0.weight'].reshape(17)) and head[17] == sd['out.0.bias'][0]


def test_packer_and_sizes_reject_bad_args(lib):
    from stofnet_amd.waveunet import pack_waveunet_weights
    for n, c in ((2, 24), (0, 16), (13, 16), (2, 12)):
        d = _lib.WaveUnetDesc(n, c)
        assert lib.stof_waveunet_packed_bytes(ctypes.byref(d)) == 0
        assert lib.stof_waveunet_workspace_bytes(ctypes.byref(d), 2, 4096) == 0
    d = _lib.WaveUnetDesc(2, 16)
    assert lib.stof_waveunet_workspace_bytes(ctypes.byref(d), 2, 6) == 0          # L % 4 != 0
    assert lib.stof_waveunet_workspace_bytes(ctypes.byref(d), 0, 8) == 0
    assert lib.stof_waveunet_workspace_bytes(ctypes.byref(d), 2, 8) > 0
    need = lib.stof_waveunet_packed_bytes(ctypes.byref(d))
    arrs = wi.kernel_arrays(wi.seeded_waveunet(2, 1))
    assert len(arrs) == 32
    ptrs = (ctypes.c_void_p * 32)(*[a.ctypes.data for a in arrs])
    blob = np.zeros(need, np.uint8)
    assert lib.stof_waveunet_pack_weights(ctypes.byref(d), ptrs, blob.ctypes.data, need - 4) != _lib.STOF_OK   # short buffer
    assert lib.stof_waveunet_pack_weights(ctypes.byref(d), ptrs, blob.ctypes.data, need) == _lib.STOF_OK
    assert lib.stof_waveunet_pack_weights(ctypes.byref(_lib.WaveUnetDesc(2, 24)), ptrs, blob.ctypes.data, need) == _lib.STOF_ERR_BAD_ARG
    # argument checks of the forward come before any HIP call
    fwd = lambda desc, N, L: lib.stof_waveunet_forward(ctypes.byref(desc), None, N, L, None, None, None, None, None, 0, None)
    assert fwd(d, 0, 8) == _lib.STOF_OK                                  # empty batch: no-op
    assert fwd(d, 0, 6) == _lib.STOF_ERR_BAD_ARG and fwd(d, 2, 8) == _lib.STOF_ERR_BAD_ARG and fwd(d, -1, 8) == _lib.STOF_ERR_BAD_ARG
    assert fwd(_lib.WaveUnetDesc(2, 24), 0, 8) == _lib.STOF_ERR_BAD_ARG
    with pytest.raises(ValueError):
        pack_waveunet_weights(2, arrs[:-1])


# ------------------------------------------------------------------------------------------------------ forward_aten
@pytest.mark.parametrize('name', ['unet_n1_2x6', 'unet_n2_3x4', 'unet_n2_5x132', 'unet_n2_2x8000', 'unet_n3_2x40', 'unet_n10_3x1024'])
def test_forward_aten_matches_fixture(g, name):
    _, n, _, N, L, _ = wi.case(name)
    sd, x, _ = case64(g, name)
    m = make(sd, n).eval()
    with torch.no_grad():
        y = m(torch.from_numpy(x)).numpy()                               # CPU tensors: forward is forward_aten
    assert rel(y[wi.kept_rows(N, L)], g[f'{name}_y']) <= 1e-5


def test_train_mode_uses_batch_statistics(g):
    sd, x, _ = case64(g, 'unet_n2_5x132')
    m = make(sd, 2)
    xt = torch.from_numpy(x)
    with torch.no_grad():
        ye = m.eval()(xt)
        mean0 = m.encoder[0].main[1].running_mean.clone()
        yt = m.train()(xt)
    assert not torch.allclose(ye, yt, atol=1e-3)
    assert not torch.equal(m.encoder[0].main[1].running_mean, mean0)
    assert int(m.middle[1].num_batches_tracked) == 1
    m.train()
    y = m(xt)
    assert y.grad_fn is not None                                         # it trains
    y.square().mean().backward()
    assert m.decoder[0].main[0].weight.grad is not None


# --------------------------------------------------------------------------------------------- lengths and main.py
def test_bad_length_raises_like_the_reference():
    m = make(wi.seeded_waveunet(2, 1), 2).eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        m.forward_aten(torch.zeros(2, 1, 6))
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(torch.zeros(2, 1, 6))
    assert not m.kernels_supported(torch.zeros(2, 1, 8))                 # CPU tensor


def test_main_rejects_bad_frame_length():
    import main
    with pytest.raises(ValueError, match='multiple of 4'):
        main.main(['model=unet', 'num_samples=2002', 'num_waveforms=4', 'batch_size=2', 'evaluate=True', 'device=cpu'])
    with pytest.raises(ValueError, match='multiple of 1024'):
        main.main(['model=unet', 'data_dir=./datasets/pala', 'num_samples=2000', 'num_waveforms=4', 'batch_size=2',
                   'evaluate=True', 'device=cpu'])

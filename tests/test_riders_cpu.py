"""EDSR_1D / ESPCN_1D on the kernels of csrc/riders.hip, without a GPU: the new C symbols, their argument checks (all
return before any HIP call), the host-side packers against a NumPy restatement of the layout documented in riders.hip,
strict loads of the four shipped checkpoints, a float64 torch-CPU restatement of both networks that reproduces
tests/golden/f21_riders.npz (pinning the fixture independently of the reference run that made it), and the routing of
CPU tensors: `forward` is `forward_aten`, `forward_kernels` raises."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, load_weights
import riders_inputs as ri
from riders_inputs import edsr64, espcn64, shuffle64      # noqa: F401  (other test modules import them from here)
from stofnet_amd import _lib
from stofnet_amd import build as sbuild

NEW_SYMBOLS = ('stof_edsr_packed_bytes', 'stof_edsr_pack_weights', 'stof_edsr_workspace_bytes', 'stof_edsr_forward',
               'stof_espcn_packed_bytes', 'stof_espcn_pack_weights', 'stof_espcn_forward')
EDSR_IDS = [c[0] for c in ri.EDSR_CASES]
ESPCN_IDS = [c[0] for c in ri.ESPCN_CASES]


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope='module')
def g():
    return golden('f21_riders')


def edsr_case(name):
    return next(c for c in ri.EDSR_CASES if c[0] == name)


def espcn_case(name):
    return next(c for c in ri.ESPCN_CASES if c[0] == name)


def rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def test_new_symbols_exist(lib):
    # the seven functions of the C ABI block (ESPCN needs no workspace, so it has no *_workspace_bytes) and the two descs
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert ctypes.sizeof(_lib.EdsrDesc) == 8 and ctypes.sizeof(_lib.EspcnDesc) == 8
    assert lib.stof_abi_version() == 3


@pytest.mark.parametrize('key', list(ri.CHECKPOINTS))
def test_shipped_checkpoints_load_strict(key):
    from stofnet_amd import EDSR_1D, ESPCN_1D
    m = EDSR_1D(1, 64, 8, 4) if key in ri.EDSR_CKPTS else ESPCN_1D(4)
    sd = load_weights(key)
    assert list(m.state_dict()) == list(sd)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert all(v.dtype == np.float32 for v in sd.values())
    assert sum(p.numel() for p in m.parameters()) == (210289 if key in ri.EDSR_CKPTS else 6948)


@pytest.mark.parametrize('name', EDSR_IDS)
def test_edsr_float64_restatement_reproduces_fixture(g, name):
    _, wkey, b, r, n, L, _ = edsr_case(name)
    x = ri.frames(n, L, int(g[f'{name}_seed']))
    rows = ri.kept_rows(n, L, r)
    y, trunk = edsr64(ri.weights(wkey, load_weights, b, r), b, r, x)
    ry, rt = g[f'{name}_y'], g[f'{name}_trunk']
    assert ry.shape == (len(rows), 1, L * r) and np.abs(ry).max() > 0
    assert rel(y[rows], ry) <= 1e-5
    assert rel(ri.trunk_edges(trunk[rows[-1]]), rt) <= 1e-5


@pytest.mark.parametrize('name', ESPCN_IDS)
def test_espcn_float64_restatement_reproduces_fixture(g, name):
    _, wkey, r, n, L, _ = espcn_case(name)
    x = ri.frames(n, L, int(g[f'{name}_seed']))
    rows = ri.kept_rows(n, L, r)
    y, logits = espcn64(ri.weights(wkey, load_weights, r), r, x)
    ry, rl = g[f'{name}_y'], g[f'{name}_logits']
    assert ry.shape == rl.shape == (len(rows), 1, L * r) and np.abs(ry).max() > 0
    assert rel(y[rows], ry) <= 1e-5
    assert rel(logits[rows], rl) <= 1e-5


def unfrag(fr, nts, K):
    """Invert the fragment order documented in csrc/riders.hip: [nts][K / 8][64 lanes][4] -> dense [32 nts][K]."""
    fr = fr.reshape(nts, K // 8, 64, 4)
    dense = np.zeros((32 * nts, K), np.float32)
    lane = np.arange(64)
    for q in range(K // 8):
        for e in range(4):
            dense[32 * np.arange(nts)[:, None] + (lane & 31)[None, :], 8 * q + 4 * (lane >> 5)[None, :] + e] = fr[:, q, :, e]
    return dense


def al(v):
    return (v + 63) // 64 * 64


@pytest.mark.parametrize('b,r', [(8, 4), (0, 1), (2, 64), (1, 16)])
def test_edsr_packer_layout(lib, b, r):
    from stofnet_amd.baselines import pack_edsr_weights
    sd = load_weights('proud-cherry') if (b, r) == (8, 4) else ri.seeded_edsr(b, r, 9)
    f = pack_edsr_weights(b, r, list(sd.values())).numpy().view(np.float32)
    cq = 64 // r
    assert f.size * 4 == lib.stof_edsr_packed_bytes(ctypes.byref(_lib.EdsrDesc(b, r)))
    assert f.size == 256 + (2 * b + 1) * (64 * 192 + 64) + al(3 * cq + 1)
    cin = f[:256].reshape(4, 64)
    assert np.array_equal(cin[:3], sd['conv_input.weight'][:, 0, :].T) and np.array_equal(cin[3], sd['conv_input.bias'])
    names = [f'residual_blocks.{i}.conv{j}' for i in range(b) for j in (1, 2)] + ['conv_mid']
    at = 256
    for nm in names:
        w = sd[nm + '.weight']                                           # [oc][ci][tap] -> k = tap * 64 + ci
        assert np.array_equal(unfrag(f[at:at + 64 * 192], 2, 192).reshape(64, 3, 64), w.transpose(0, 2, 1))
        assert np.array_equal(f[at + 64 * 192:at + 64 * 192 + 64], sd[nm + '.bias'])
        at += 64 * 192 + 64
    assert np.array_equal(f[at:at + 3 * cq].reshape(3, cq), sd['conv_output.weight'][0].T)
    assert f[at + 3 * cq] == sd['conv_output.bias'][0] and not f[at + 3 * cq + 1:].any()
    assert at + al(3 * cq + 1) == f.size


@pytest.mark.parametrize('r', [4, 1, 17, 32, 33, 64])
def test_espcn_packer_layout(lib, r):
    from stofnet_amd.baselines import pack_espcn_weights
    sd = load_weights('vital-puddle') if r == 4 else ri.seeded_espcn(r, 9)
    f = pack_espcn_weights(r, list(sd.values())).numpy().view(np.float32)
    nt = 1 if r <= 32 else 2
    assert f.size * 4 == lib.stof_espcn_packed_bytes(ctypes.byref(_lib.EspcnDesc(r, 0)))
    assert f.size == 384 + 32 * 192 + 64 + nt * 32 * 96 + 64
    c1 = f[:384].reshape(6, 64)
    assert np.array_equal(c1[:5], sd['conv1.weight'][:, 0, :].T) and np.array_equal(c1[5], sd['conv1.bias'])
    at = 384
    assert np.array_equal(unfrag(f[at:at + 32 * 192], 1, 192).reshape(32, 3, 64), sd['conv2.weight'].transpose(0, 2, 1))
    at += 32 * 192
    assert np.array_equal(f[at:at + 32], sd['conv2.bias']) and not f[at + 32:at + 64].any()
    at += 64
    w3 = unfrag(f[at:at + nt * 32 * 96], nt, 96).reshape(32 * nt, 3, 32)
    assert np.array_equal(w3[:r], sd['conv3.weight'].transpose(0, 2, 1)) and not w3[r:].any()
    at += nt * 32 * 96
    assert np.array_equal(f[at:at + r], sd['conv3.bias']) and not f[at + r:at + 64].any()
    assert at + 64 == f.size


def test_abi_argument_checks_without_gpu(lib):
    r = ctypes.byref
    h = np.zeros(64, np.float32).ctypes.data
    # ---- EDSR
    ok = _lib.EdsrDesc(8, 4)
    bads = [_lib.EdsrDesc(8, 3), _lib.EdsrDesc(8, 0), _lib.EdsrDesc(8, 128), _lib.EdsrDesc(-1, 4), _lib.EdsrDesc(8, -4)]
    assert lib.stof_edsr_packed_bytes(r(ok)) > 0 and lib.stof_edsr_packed_bytes(None) == 0
    for rr in (1, 2, 4, 8, 16, 32, 64):
        assert lib.stof_edsr_packed_bytes(r(_lib.EdsrDesc(0, rr))) > 0
    for b in bads:
        assert lib.stof_edsr_packed_bytes(r(b)) == 0 and lib.stof_edsr_workspace_bytes(r(b), 4, 2000) == 0
    assert lib.stof_edsr_workspace_bytes(r(ok), 0, 2000) == 0 and lib.stof_edsr_workspace_bytes(r(ok), 4, 0) == 0
    for N, L in ((1, 2000), (8, 2000), (3, 1), (5, 20001)):           # three buffers of (N (L + 1) + 1) x 64 floats
        assert lib.stof_edsr_workspace_bytes(r(ok), N, L) == 3 * 256 * (N * (L + 1) + 1)
    n = lib.stof_edsr_packed_bytes(r(ok))
    buf = np.zeros(n, np.uint8)
    arrs = [np.ascontiguousarray(v, np.float32) for v in load_weights('proud-cherry').values()]
    assert len(arrs) == 38
    ptrs = (ctypes.c_void_p * 38)(*[a.ctypes.data for a in arrs])
    pack = lib.stof_edsr_pack_weights
    assert pack(r(ok), ptrs, buf.ctypes.data, n - 4) == _lib.STOF_ERR_WORKSPACE
    assert pack(r(ok), None, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(ok), ptrs, None, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(bads[0]), ptrs, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    holes = (ctypes.c_void_p * 38)(*[a.ctypes.data for a in arrs])
    holes[37] = None
    assert pack(r(ok), holes, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(ok), ptrs, buf.ctypes.data, n) == _lib.STOF_OK
    ws = lib.stof_edsr_workspace_bytes(r(ok), 4, 2000)
    fwd = lib.stof_edsr_forward
    assert fwd(r(ok), h, 4, 2000, h, h, None, h, ws - 1, None) == _lib.STOF_ERR_WORKSPACE
    for N, L in ((0, 2000), (-1, 2000), (4, 0), (4, -5)):
        assert fwd(r(ok), h, N, L, h, h, None, h, 1 << 40, None) == _lib.STOF_ERR_BAD_ARG
    for b in bads:
        assert fwd(r(b), h, 4, 2000, h, h, None, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(None, h, 4, 2000, h, h, None, h, ws, None) == _lib.STOF_ERR_BAD_ARG
    for i in range(4):                                                   # x, packed, y, workspace
        args = [h, h, h, h]
        args[i] = None
        assert fwd(r(ok), args[0], 4, 2000, args[1], args[2], None, args[3], ws, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(r(ok), h, 1 << 20, 1 << 12, h, h, None, h, 1 << 62, None) == _lib.STOF_ERR_UNSUPPORTED
    assert fwd(r(ok), h, 1 << 40, 1 << 40, h, h, None, h, 1 << 62, None) == _lib.STOF_ERR_UNSUPPORTED
    # ---- ESPCN
    ok = _lib.EspcnDesc(4, 0)
    bads = [_lib.EspcnDesc(0, 0), _lib.EspcnDesc(65, 0), _lib.EspcnDesc(-4, 0)]
    assert lib.stof_espcn_packed_bytes(None) == 0
    for rr in range(1, 65):
        assert lib.stof_espcn_packed_bytes(r(_lib.EspcnDesc(rr, 0))) == 4 * (384 + 32 * 192 + 64 + (1 if rr <= 32 else 2) * 32 * 96 + 64)
    for b in bads:
        assert lib.stof_espcn_packed_bytes(r(b)) == 0
    n = lib.stof_espcn_packed_bytes(r(ok))
    buf = np.zeros(n, np.uint8)
    arrs = [np.ascontiguousarray(v, np.float32) for v in load_weights('vital-puddle').values()]
    assert len(arrs) == 6
    ptrs = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in arrs])
    pack = lib.stof_espcn_pack_weights
    assert pack(r(ok), ptrs, buf.ctypes.data, n - 4) == _lib.STOF_ERR_WORKSPACE
    assert pack(r(ok), None, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(ok), ptrs, None, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(bads[0]), ptrs, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    holes = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in arrs])
    holes[5] = None
    assert pack(r(ok), holes, buf.ctypes.data, n) == _lib.STOF_ERR_BAD_ARG
    assert pack(r(ok), ptrs, buf.ctypes.data, n) == _lib.STOF_OK
    fwd = lib.stof_espcn_forward
    for N, L in ((0, 2000), (-1, 2000), (4, 0), (4, -5)):
        assert fwd(r(ok), h, N, L, h, h, None, None) == _lib.STOF_ERR_BAD_ARG
    for b in bads:
        assert fwd(r(b), h, 4, 2000, h, h, None, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(None, h, 4, 2000, h, h, None, None) == _lib.STOF_ERR_BAD_ARG
    for i in range(3):                                                   # x, packed, y
        args = [h, h, h]
        args[i] = None
        assert fwd(r(ok), args[0], 4, 2000, args[1], args[2], None, None) == _lib.STOF_ERR_BAD_ARG
    assert fwd(r(ok), h, 1 << 20, 1 << 12, h, h, None, None) == _lib.STOF_ERR_UNSUPPORTED
    assert fwd(r(ok), h, 1 << 40, 1 << 40, h, h, None, None) == _lib.STOF_ERR_UNSUPPORTED


def models():
    from stofnet_amd import EDSR_1D, ESPCN_1D
    torch.manual_seed(0)
    return [EDSR_1D(1, 64, 2, 4), ESPCN_1D(4)]


def test_cpu_tensors_stay_on_the_aten_route(monkeypatch):
    """On CPU tensors `forward` is `forward_aten` and `forward_kernels` raises.  The package has no CPU shuffle (its
    SampleShuffle1D raises off the ROCm device, tests/test_abi_cpu.py::test_no_cpu_fallback), so as shipped both
    routes end in that same error; with the shuffle step alone restated as the reference's view / permute, the two are
    compared bit for bit."""
    from stofnet_amd.sample_shuffle import SampleShuffle1D
    x = torch.from_numpy(ri.frames(3, 50, 1))
    for m in models():
        for mode in (m.train, m.eval):
            mode()
            for fn in (m, m.forward_aten):
                with pytest.raises(RuntimeError, match='ROCm device only'):
                    fn(x)
        with pytest.raises(RuntimeError, match='ROCm device'):
            m.forward_kernels(x)
        with pytest.raises(RuntimeError, match='ROCm device'):
            getattr(m, 'forward_with_trunk', getattr(m, 'forward_with_logits', None))(x)
        assert m._packed is None                                       # nothing was packed on the way
    monkeypatch.setattr(SampleShuffle1D, 'forward', lambda self, t: shuffle64(t, self.upsample_factor))
    for m in models():
        y = m(x)
        assert y.grad_fn is not None and y.shape == (3, 1, 200)
        assert torch.equal(y, m.forward_aten(x))
        with torch.no_grad():
            assert torch.equal(m(x), y.detach()) and torch.equal(m.eval()(x), m.forward_aten(x))
        with pytest.raises(RuntimeError, match='ROCm device'):
            m.forward_kernels(x)


def test_kernels_supported_is_false_off_the_supported_ground():
    from stofnet_amd import EDSR_1D, ESPCN_1D
    x = torch.zeros(2, 1, 40)
    good = [EDSR_1D(1, 64, 8, 4), EDSR_1D(1, 64, 0, 64), ESPCN_1D(4), ESPCN_1D(64)]
    bad = [EDSR_1D(1, 16, 2, 4), EDSR_1D(2, 64, 1, 4), EDSR_1D(1, 8, 1, 2), ESPCN_1D(65)]
    assert all(m._config_supported() for m in good) and not any(m._config_supported() for m in bad)
    for m in good + bad:
        assert not m.kernels_supported(x)                               # a CPU tensor
        assert not m.kernels_supported(x.double()) and not m.double().kernels_supported(x.double())
        assert not m.kernels_supported(x[:, 0])

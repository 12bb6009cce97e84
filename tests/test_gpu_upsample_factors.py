"""StofNet and SampleShuffle1D across upsample factors on gfx950: every case of golden f20_upsample_factors
(tests/upsample_variants.py) against the reference's forward result and autograd gradients and the fp64 oracle; both body
kernels of the fused sweep and its segment mode at r where the conv_last tile and the shuffle store branch; the standalone
shuffle at any r and element size, bit for bit."""
import numpy as np
import pytest
import torch

from oracle import stofnet_oracle as so
from test_upsample_factors_cpu import rel, upsample_case
from upsample_variants import UPSAMPLE_CASES, variant_input

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-5           # relative to max|y|, against the fp64 oracle (tests/test_gpu_parity.py)
FUSED = [n for n in UPSAMPLE_CASES if n.startswith(('g1_', 'g2_'))]
_ORACLE = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from stofnet_amd import _lib
    _lib.lib()
    return torch.device('cuda:0')


def truth(name, x, key='fixture'):
    """fp64 oracle map of case `name` on input x (cached per case and input)."""
    if (name, key) not in _ORACLE:
        var, params = UPSAMPLE_CASES[name], upsample_case(name)[1]
        c = var['ctor']
        _ORACLE[name, key] = so.stofnet_forward(params, x, c['upsample_factor'], c['semi_global_scale'], torch.float64).numpy()
    return _ORACLE[name, key]


def model(dev, name, precision='fp32', train_precision='f16x3'):
    from stofnet_amd import StofNet
    var, params = UPSAMPLE_CASES[name], upsample_case(name)[1]
    m = StofNet(**var['ctor'], precision=precision, train_precision=train_precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(dev)


@pytest.mark.parametrize('precision', ['fp32', 'f16x3', 'auto'])
@pytest.mark.parametrize('name', list(UPSAMPLE_CASES))
def test_forward_matches_reference_and_fp64(dev, name, precision):
    var, params, x, t, y_ref, _, _ = upsample_case(name)
    m = model(dev, name, precision).eval()
    with torch.no_grad():
        y = m(torch.from_numpy(x).to(dev))
    assert y.shape == y_ref.shape and y.dtype == torch.float32
    y = y.cpu().numpy()
    assert rel(y, y_ref) < 2e-5
    assert rel(y, truth(name, x)) < MAP_TOL
    if precision == 'f16x3':
        m.raise_if_overflow()


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('name', FUSED)
def test_fused_body_kernels_segments_and_batch(dev, name, precision):
    """One segment per waveform pins the body kernel: L = 400 runs the two-pass body_p2 kernel, L = 240 the r3 kernel
    (body_p2_rows_ok: seg_len + 2 halo + gap >= 384).  Forced 1 / 2 / 4 / 8 segments and the automatic choice give
    identical bits, and the fixture rows inside a batch of 64 equal the same rows computed alone."""
    x = upsample_case(name)[2]
    m = model(dev, name, precision).eval()
    seed = int(UPSAMPLE_CASES[name]['ctor']['upsample_factor']) + 7
    for L in (400, 240):
        xl = torch.from_numpy(variant_input(2, L, seed)).to(dev)
        outs = []
        for policy in (1, 2, 3, 4, 0):
            m._seg_policy = policy
            outs.append(m(xl))
        assert rel(outs[0].cpu().numpy(), truth(name, xl.cpu().numpy(), L)) < MAP_TOL, L
        for y in outs[1:]:
            assert torch.equal(outs[0], y), L
    m._seg_policy = 0
    xd = torch.from_numpy(x).to(dev)
    batch = torch.from_numpy(variant_input(64, x.shape[-1], seed)).to(dev)
    rows = [5, 40][:x.shape[0]]
    batch[rows] = xd
    assert torch.equal(m(batch)[rows], m(xd))
    if precision == 'f16x3':
        m.raise_if_overflow()


def oracle_grads(name):
    """fp64 oracle: d loss / d x and every parameter's gradient for loss = sum(y * t) of case `name` (cached)."""
    if (name, 'grads') not in _ORACLE:
        var, params, x, t = upsample_case(name)[:4]
        c = var['ctor']
        p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
        x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        (so.stofnet_forward(p64, x64, c['upsample_factor'], c['semi_global_scale'], torch.float64)
         * torch.from_numpy(t).double()).sum().backward()
        _ORACLE[name, 'grads'] = (x64.grad.numpy(), {k: v.grad.numpy() for k, v in p64.items()})
    return _ORACLE[name, 'grads']


@pytest.mark.parametrize('tp,tol', [('fp32', 2e-4), ('f16x3', 2e-3)])
@pytest.mark.parametrize('name', list(UPSAMPLE_CASES))
def test_gradients_match_reference_autograd(dev, name, tp, tol):
    """Train-mode forward + backward through the autograd boundary at every r: the conv_last data gradient runs its
    dedicated kernel at r = 4 / 10 only, the generic convolution (and, split-fp16, the row conversion) elsewhere.  Against
    the reference's gradients the fixture keeps, and against the fp64 oracle's for every parameter."""
    var, params, x, t, y_ref, dx_ref, grads_ref = upsample_case(name)
    m = model(dev, name, train_precision=tp).train()
    xg = torch.from_numpy(x).to(dev).requires_grad_()
    y = m(xg)
    assert rel(y.detach().cpu().numpy(), y_ref) < 2e-5
    (y * torch.from_numpy(t).to(dev)).sum().backward()
    m.raise_if_overflow()
    assert rel(xg.grad.cpu().numpy(), dx_ref) < tol
    named = dict(m.named_parameters())
    assert all(p.grad is not None for p in named.values())
    for n, gr in grads_ref.items():
        assert rel(named[n].grad.cpu().numpy(), gr) < tol, n
    dx64, g64 = oracle_grads(name)                       # every parameter, including those the fixture does not keep
    assert rel(xg.grad.cpu().numpy(), dx64) < tol
    assert set(g64) == set(named)
    for n, gr in g64.items():
        assert rel(named[n].grad.cpu().numpy(), gr) < tol, n


# ---------------------------------------------------------------- standalone SampleShuffle1D
SHUFFLE_R = [1, 31, 32, 33, 63, 64, 65, 79, 80, 127, 128, 129, 200]


def _ramp(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g).to(dtype)
    if dtype.is_complex:
        return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)).to(dtype)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * 1e3).to(dtype)


@pytest.mark.parametrize('r', SHUFFLE_R)
@pytest.mark.parametrize('dtype', [torch.uint8, torch.float16, torch.float32, torch.float64, torch.complex128])
def test_shuffle_any_factor_and_element_size_bit_exact(dev, dtype, r):
    """Both kernels (the LDS tile while r * 257 * elem_bytes fits in 64 KiB, the gather beyond) against view / permute /
    contiguous (utils/sample_shuffle.py:24-27), at widths around the 256-wide tile."""
    from stofnet_amd import SampleShuffle1D
    for W, (n, c) in zip((1, 255, 256, 257, 513), ((2, 1), (1, 2), (2, 1), (1, 1), (2, 1))):
        x = _ramp((n, r * c, W), dtype, r * 1000 + W)
        out = SampleShuffle1D(r)(x.to(dev)).cpu()
        want = so.sample_shuffle(x, r)
        assert out.dtype == dtype and out.shape == want.shape == (n, c, W * r)
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), (W, n, c)


def test_shuffle_int64_ramp_beyond_fp32_at_r96(dev):
    from stofnet_amd import SampleShuffle1D
    r, n, c, w = 96, 2, 3, 300
    x = torch.arange(n * r * c * w, dtype=torch.int64).reshape(n, r * c, w) * 7919 + 2 ** 40 + 1
    out = SampleShuffle1D(r)(x.to(dev)).cpu()
    assert torch.equal(out.view(torch.uint8), so.sample_shuffle(x, r).view(torch.uint8))

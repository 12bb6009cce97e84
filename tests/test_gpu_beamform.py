"""GPU tests of the delay-and-sum beamformer (csrc/beamform.hip through stofnet_amd/beamform.py): every case and dtype of
tests/beamform_inputs.py against the reference's recorded runs (tests/golden/f32_beamform.npz) and against the library's
host entry, the B-mode kernels, run-to-run and batch independence bit for bit, scattered pixel lists, all-masked
geometries.

Bounds, as in tests/test_beamform_cpu.py: 64-bit dtypes 1e-10 x max|ref64|; 32-bit dtypes max(2e-6 x max|ref64|, 8 x dev)
against the fixture and 2e-6 x max against the host entry (the kernel and the host entry share the delay, mask and weight
arithmetic; what differs is the device's hypot, sine and cosine, a few ulp of the scalar type); B-mode 1e-4 dB."""
import json
import os

import numpy as np
import pytest
import torch

import beamform_inputs as bi
from conftest import golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'beamform.jsonl')
ALL = [(n, k, b) for n, c in bi.CASES.items() for k in c['kinds'] for b in (64, 32)]
_worst = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    g = golden('f32_beamform')
    return {k: g[k] for k in g.files}


def record(key, dtype, value):
    """keep the worst measured distance per dtype in profiles/beamform.jsonl (one `parity` line, rewritten as cases come in)"""
    slot = _worst.setdefault(key, {})
    name = np.dtype(dtype).name
    slot[name] = max(slot.get(name, 0.0), float(f'{value:.3e}'))
    print(key, name, f'{value:.3e}')
    lines = []
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'parity']
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines + [json.dumps({'kind': 'parity', 'worst': _worst})]) + '\n')
    except OSError:
        pass


def check_sum(key, out, ref, dev_ref, bits):
    mx = np.abs(ref).max()
    err = np.abs(out.astype(ref.dtype) - ref)
    record(key, out.dtype, err.max() / mx)
    if bits == 64:
        assert (err <= 1e-10 * mx).all()
    else:
        assert (err <= np.maximum(2e-6 * mx, 8 * dev_ref)).all()


def check_host(out, host, bits):
    mx = np.abs(host).max()
    err = np.abs(out.astype(np.complex128) - host.astype(np.complex128)).max()
    record('device_vs_host_over_max', out.dtype, err / mx)
    assert err <= (1e-10 if bits == 64 else 2e-6) * mx


@pytest.mark.parametrize('name,kind,bits', ALL)
def test_sum_matches_reference_and_host(dev, gold, name, kind, bits):
    from utils.beamform import bf_das
    case = bi.CASES[name]
    p = bi.param(case)
    sig = bi.signal(name, case, kind, bits)
    t = torch.from_numpy(sig).to(dev)
    got = bf_das(t, p, return_iq=True)
    assert got.dtype == t.dtype and got.device == t.device
    out = got.cpu().numpy()
    ref = gold[f'{name}_{kind}_sum64']
    assert out.shape == ref.shape
    assert np.array_equal(out == 0, ref == 0)
    check_sum('device_vs_reference_over_max', out, ref, gold[f'{name}_{kind}_dev'], bits)
    check_host(out, bf_das(sig, p, return_iq=True), bits)
    again = bf_das(t, p, return_iq=True)
    assert torch.equal(got, again)                                      # two runs, bit for bit
    planes = bf_das(t, p, compound_opt=False, return_iq=True).cpu().numpy()
    check_host(planes, bf_das(sig, p, compound_opt=False, return_iq=True), bits)


@pytest.mark.parametrize('name,kind', [(n, k) for n, c in bi.CASES.items() if c['frames'] == 1 for k in c['kinds']])
def test_bmode(dev, gold, name, kind):
    from utils.beamform import bf_das
    case = bi.CASES[name]
    p = bi.param(case)
    modes = [(True, gold[f'{name}_{kind}_bmode1'], gold[f'{name}_{kind}_sum64'])]
    if case['planes']:
        modes.append((False, gold[f'{name}_{kind}_bmode0'], gold[f'{name}_{kind}_planes64']))
    t64 = torch.from_numpy(bi.signal(name, case, kind, 64)).to(dev)
    t32 = torch.from_numpy(bi.signal(name, case, kind, 32)).to(dev)
    for compound, ref, img in modes:
        nz = img != 0
        bm = bf_das(t64, p, compound_opt=compound)
        assert bm.dtype == torch.float64
        bm = bm.cpu().numpy()
        assert bm.shape == ref.shape and np.isfinite(bm).all()
        record('bmode_vs_reference_dB', bm.dtype, np.abs(bm - ref)[nz].max())
        assert np.abs(bm - ref)[nz].max() <= 1e-4
        assert (bm[~nz] == bm.min()).all() and bm.max() == 0
        # 32-bit: against 20 log10 of the route's own image, taken in double
        own = bf_das(t32, p, compound_opt=compound, return_iq=True).cpu().numpy().astype(np.complex128)
        bm32 = bf_das(t32, p, compound_opt=compound)
        assert bm32.dtype == torch.float32
        bm32 = bm32.cpu().numpy()
        nz32 = own != 0
        want = 20 * np.log10(np.abs(own[nz32]))
        record('bmode_vs_own_image_dB', bm32.dtype, np.abs(bm32[nz32] - (want - want.max())).max())
        assert np.abs(bm32[nz32] - (want - want.max())).max() <= 1e-4
        assert (bm32[~nz32] == bm32.min()).all()


@pytest.mark.parametrize('kind', bi.KINDS)
@pytest.mark.parametrize('bits', [64, 32])
def test_each_frame_of_a_batch_equals_the_frame_alone(dev, kind, bits):
    from utils.beamform import bf_das
    case = bi.CASES['batch5']
    p = bi.param(case)
    t = torch.from_numpy(bi.signal('batch5', case, kind, bits)).to(dev)
    for compound in (True, False):
        whole = bf_das(t, p, compound_opt=compound, return_iq=True)
        bm = bf_das(t, p, compound_opt=compound)
        assert whole.shape[0] == 5
        for f in range(5):
            assert torch.equal(whole[f], bf_das(t[f], p, compound_opt=compound, return_iq=True))
            assert torch.equal(bm[f], bf_das(t[f], p, compound_opt=compound))
        pair = bf_das(t[[4, 1]], p, compound_opt=compound, return_iq=True)     # another batch, other places
        assert torch.equal(pair[0], whole[4]) and torch.equal(pair[1], whole[1])
    lead = bf_das(t[:4].reshape(2, 2, *t.shape[1:]), p, return_iq=True)
    assert lead.shape[:2] == (2, 2) and torch.equal(lead.reshape(4, *lead.shape[2:]), bf_das(t[:4], p, return_iq=True))


@pytest.mark.parametrize('kind', bi.KINDS)
@pytest.mark.parametrize('bits', [64, 32])
def test_scattered_pixel_list(dev, gold, kind, bits):
    from utils.beamform import bf_das_rx
    case = bi.CASES[bi.SCATTER_OF]
    p = dict(bi.param(case))
    p['theta'] = p['angles_list'][bi.SCATTER_ANGLE]
    xs, zs, perm = bi.scatter_grids()
    t = torch.from_numpy(bi.signal(bi.SCATTER_OF, case, kind, bits)[bi.SCATTER_ANGLE]).to(dev)
    out = bf_das_rx(t, p, xs, zs)
    assert tuple(out.shape) == xs.shape and out.dtype == t.dtype
    check_sum('device_vs_reference_over_max', out.cpu().numpy(), gold[f'scatter_{kind}_sum64'], gold[f'scatter_{kind}_dev'], bits)
    x2, z2 = np.meshgrid(p['param_x'], p['param_z'])
    raster = bf_das_rx(t, p, x2, z2)
    assert torch.equal(out.T.flatten(), raster.T.flatten()[torch.from_numpy(perm).to(dev)])


@pytest.mark.parametrize('kind', bi.KINDS)
@pytest.mark.parametrize('bits', [64, 32])
def test_large_grid(dev, gold, kind, bits):
    """300 x 300 pixels: several hundred work-groups, the last one partly filled."""
    from utils.beamform import bf_das
    t = torch.from_numpy(bi.signal('big', bi.BIG, kind, bits)).to(dev)
    img = bf_das(t, bi.param(bi.BIG), return_iq=True)
    flat = img.T.flatten().cpu().numpy()
    ref, mx = gold[f'big_{kind}_sum64'], float(gold[f'big_{kind}_max'])
    err = np.abs(flat[::bi.BIG_STEP].astype(ref.dtype) - ref)
    record('device_vs_reference_over_max', flat.dtype, err.max() / mx)
    if bits == 64:
        assert (err <= 1e-10 * mx).all()
        assert abs(flat.sum() - gold[f'big_{kind}_total']) <= 1e-10 * mx * flat.size
    else:
        assert (err <= np.maximum(2e-6 * mx, 8 * gold[f'big_{kind}_dev'])).all()
    bm = bf_das(t, bi.param(bi.BIG))                                    # 90,000 pixels: 88 block partials per frame
    own = img.cpu().numpy().astype(np.complex128)
    nz = own != 0
    want = 20 * np.log10(np.abs(own[nz]))
    bm = bm.cpu().numpy()
    assert np.abs(bm[nz] - (want - want.max())).max() <= 1e-4 and (bm[~nz] == bm.min()).all() and bm.max() == 0


@pytest.mark.parametrize('change', [{'t0': 1.0}, {'t0': -1.0}, {'fs': 0.0}])
def test_all_masked_geometries_give_exact_zeros(dev, change):
    from utils.beamform import bf_das
    case = bi.CASES['c8']
    p = dict(bi.param(case), **change)
    for kind in bi.KINDS:
        for bits in (64, 32):
            t = torch.from_numpy(bi.signal('c8', case, kind, bits)).to(dev)
            for compound in (True, False):
                img = bf_das(t, p, compound_opt=compound, return_iq=True)
                assert img.dtype == t.dtype and not img.cpu().numpy().any()
                bm = bf_das(t, p, compound_opt=compound)
                assert bm.shape == img.shape and not bm.cpu().numpy().any()


def test_complex_typed_real_input_and_real_channels(dev, gold):
    from utils.beamform import bf_das
    case = bi.CASES['c65']
    p = bi.param(case)
    for bits in (64, 32):
        real = torch.from_numpy(bi.signal('c65', case, 'real', bits)).to(dev)
        out_r = bf_das(real, p, return_iq=True)
        out_c = bf_das(real.to(torch.complex128 if bits == 64 else torch.complex64), p, return_iq=True)
        assert torch.equal(out_c.real, out_r) and not out_c.imag.cpu().numpy().any()


def test_non_finite_geometry_raises_before_any_launch(dev):
    from utils.beamform import bf_das
    case = bi.CASES['c8']
    t = torch.from_numpy(bi.signal('c8', case, 'real', 32)).to(dev)
    with pytest.raises(ValueError, match='finite'):
        bf_das(t, dict(bi.param(case), c=float('nan')))
    with pytest.raises(TypeError):
        bf_das(t.to(torch.float16), bi.param(case))

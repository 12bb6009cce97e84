"""CPU checks of the delay-and-sum beamformer (stofnet_amd/beamform.py on the library's host entry, which runs the very
das_core.h text the kernel runs) against the reference's utils/beamform.py, recorded by tests/golden/make_golden_beamform.py.

Bounds.  64-bit dtypes: 1e-10 x max|ref64| -- the transmit distances are the reference's doubles bit for bit, what remains
is double rounding near 1e-14, and a logic error shows at 1e-6 or above.  32-bit dtypes: the project's rule
|ours - ref64| <= max(2e-6 x max|ref64|, 8 x dev), dev = the reference's own 32-bit deviation from its 64-bit result (the
manifest records dev / max between 3e-8 and 1.3e-7).  B-mode: 1e-4 dB; the generator asserts that every non-zero pixel is
at least 1e-4 of the frame's maximum, that every sample index stays 1e-6 samples away from the range mask's edges and every
pixel 1e-12 m away from a cone's edge, so no term can flip between the reference and this code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import beamform_inputs as bi
from conftest import ROOT, golden
from stofnet_amd import _lib
from stofnet_amd import build as sbuild

SRC = os.path.join(ROOT, 'tests', 'cpu_harness', 'das_harness.cpp')
ALL = [(n, k, b) for n, c in bi.CASES.items() for k in c['kinds'] for b in (64, 32)]


@pytest.fixture(scope='module')
def lib():
    sbuild.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope='module')
def gold():
    g = golden('f32_beamform')
    return {k: g[k] for k in g.files}


def within(ours, ref, dev, bits):
    mx = np.abs(ref).max()
    err = np.abs(ours.astype(ref.dtype) - ref)
    print(f'worst |ours - ref64| / max = {err.max() / mx:.3e}')
    if bits == 64:
        return bool((err <= 1e-10 * mx).all())
    return bool((err <= np.maximum(2e-6 * mx, 8 * dev)).all())


def test_reference_import_line_resolves():
    from utils.beamform import bf_das, bf_das_rx
    from stofnet_amd import beamform
    assert bf_das is beamform.bf_das and bf_das_rx is beamform.bf_das_rx


@pytest.mark.parametrize('name', list(bi.CASES) + ['big'])
def test_tx_distance_is_the_numpy_expression_bit_for_bit(lib, name):
    p = bi.param(bi.BIG if name == 'big' else bi.CASES[name])
    x, z = bi.pixel_list(p)
    xe, ang = np.ascontiguousarray(p['xe']), np.ascontiguousarray(p['angles_list'])
    dtx = np.empty((ang.size, x.size))
    assert lib.stof_das_tx_distance(xe.ctypes.data, xe.size, ang.ctypes.data, ang.size, x.ctypes.data, z.ctypes.data, x.size,
                                    dtx.ctypes.data) == 0
    want = np.stack([bi.tx_distance_numpy(xe, t, x, z) for t in ang])
    assert np.array_equal(dtx, want)


@pytest.mark.parametrize('name,kind,bits', ALL)
def test_sum_matches_reference(lib, gold, name, kind, bits):
    from utils.beamform import bf_das
    case = bi.CASES[name]
    sig = bi.signal(name, case, kind, bits)
    out = bf_das(sig, bi.param(case), return_iq=True)
    assert isinstance(out, np.ndarray) and out.dtype == sig.dtype
    ref = gold[f'{name}_{kind}_sum64']
    assert out.shape == ref.shape
    assert np.array_equal(out == 0, ref == 0)                           # the same pixels lie outside every cone and range
    assert within(out, ref, gold[f'{name}_{kind}_dev'], bits)


@pytest.mark.parametrize('kind', bi.KINDS)
@pytest.mark.parametrize('bits', [64, 32])
def test_scattered_pixel_list(lib, gold, kind, bits):
    """bf_das_rx on 2-D arrays in no raster order; the result is also the raster result, permuted, bit for bit."""
    from utils.beamform import bf_das_rx
    case = bi.CASES[bi.SCATTER_OF]
    p = dict(bi.param(case))
    p['theta'] = p['angles_list'][bi.SCATTER_ANGLE]
    xs, zs, perm = bi.scatter_grids()
    sig = bi.signal(bi.SCATTER_OF, case, kind, bits)[bi.SCATTER_ANGLE]
    out = bf_das_rx(sig, p, xs, zs)
    assert out.shape == xs.shape and out.dtype == sig.dtype
    assert within(out, gold[f'scatter_{kind}_sum64'], gold[f'scatter_{kind}_dev'], bits)
    x2, z2 = np.meshgrid(p['param_x'], p['param_z'])
    raster = bf_das_rx(sig, p, x2, z2)
    assert np.array_equal(out.T.flatten(), raster.T.flatten()[perm])


@pytest.mark.parametrize('kind', bi.KINDS)
@pytest.mark.parametrize('bits', [64, 32])
def test_large_grid(lib, gold, kind, bits):
    from utils.beamform import bf_das
    sig = bi.signal('big', bi.BIG, kind, bits)
    flat = bf_das(sig, bi.param(bi.BIG), return_iq=True).T.flatten()
    ref, mx = gold[f'big_{kind}_sum64'], float(gold[f'big_{kind}_max'])
    err = np.abs(flat[::bi.BIG_STEP].astype(ref.dtype) - ref)
    print(f'worst / max = {err.max() / mx:.3e}')
    if bits == 64:
        assert (err <= 1e-10 * mx).all()
        assert abs(flat.sum() - gold[f'big_{kind}_total']) <= 1e-10 * mx * flat.size
    else:
        assert (err <= np.maximum(2e-6 * mx, 8 * gold[f'big_{kind}_dev'])).all()


@pytest.mark.parametrize('name,kind', [(n, k) for n, c in bi.CASES.items() if c['frames'] == 1 for k in c['kinds']])
def test_bmode_matches_reference(lib, gold, name, kind):
    from utils.beamform import bf_das
    case = bi.CASES[name]
    sig = bi.signal(name, case, kind, 64)
    modes = [(True, gold[f'{name}_{kind}_bmode1'], gold[f'{name}_{kind}_sum64'])]
    if case['planes']:
        modes.append((False, gold[f'{name}_{kind}_bmode0'], gold[f'{name}_{kind}_planes64']))
    for compound, ref, img in modes:
        bm = bf_das(sig, bi.param(case), compound_opt=compound)
        nz = img != 0
        assert bm.shape == ref.shape and bm.dtype == np.float64 and np.isfinite(bm).all()
        print(f'worst B-mode distance = {np.abs(bm - ref)[nz].max():.3e} dB')
        assert np.abs(bm - ref)[nz].max() <= 1e-4
        assert (~nz).any() and (bm[~nz] == bm.min()).all() and bm.max() == 0


@pytest.mark.parametrize('name,kind', [(n, k) for n, c in bi.CASES.items() for k in c['kinds']])
def test_bmode_32bit_follows_its_own_image(lib, name, kind):
    from utils.beamform import bf_das
    case = bi.CASES[name]
    sig = bi.signal(name, case, kind, 32)
    p = bi.param(case)
    for compound in (True, False):
        img = bf_das(sig, p, compound_opt=compound, return_iq=True).astype(np.complex128)
        bm = bf_das(sig, p, compound_opt=compound)
        assert bm.dtype == np.float32 and bm.shape == img.shape
        fdims = 2 if compound else 3
        for f_bm, f_img in zip(bm.reshape((-1,) + bm.shape[-fdims:]), img.reshape((-1,) + img.shape[-fdims:])):
            nz = f_img != 0
            want = 20 * np.log10(np.abs(f_img[nz]))
            assert np.abs(f_bm[nz] - (want - want.max())).max() <= 1e-4
            assert (f_bm[~nz] == f_bm.min()).all()


def test_complex_typed_real_input_equals_the_real_path(lib):
    from utils.beamform import bf_das
    case = bi.CASES['c65']
    p = bi.param(case)
    for bits in (64, 32):
        real = bi.signal('c65', case, 'real', bits)
        out_r = bf_das(real, p, return_iq=True)
        out_c = bf_das(real.astype(bi.DTYPES['cplx', bits]), p, return_iq=True)
        assert np.array_equal(out_c.real, out_r) and not out_c.imag.any()
        assert np.array_equal(bf_das(real.astype(bi.DTYPES['cplx', bits]), p), bf_das(real, p))


def test_purely_real_channels_are_not_rotated(lib, gold):
    """`realch` (channels 0..2 real) differs from the same data with every channel rotated."""
    from stofnet_amd import beamform
    case = bi.CASES['realch']
    sig = bi.signal('realch', case, 'cplx', 64)
    p = bi.param(case)
    x, z = bi.pixel_list(p)
    geo = beamform._Geometry(p, p['angles_list'], x, z, bi.FNUMBER)
    s4 = np.ascontiguousarray(sig)[None]
    out = np.zeros((1, x.size), sig.dtype)
    rot = np.ones((1, case['A'], case['Ne']), np.uint8)
    desc = geo.desc(_lib.DAS_C128, True)
    assert lib.stof_das_beamform_host(ctypes.byref(desc), s4.ctypes.data, 1, case['A'], case['S'], case['Ne'], geo.x.ctypes.data,
                                      geo.z.ctypes.data, geo.dtx.ctypes.data, geo.p, geo.xe.ctypes.data, rot.ctypes.data,
                                      out.ctypes.data) == 0
    ref = gold['realch_cplx_sum64'].T.flatten()
    assert np.abs(out[0] - ref).max() > 1e-3 * np.abs(ref).max()


@pytest.mark.parametrize('change', [{'t0': 1.0}, {'t0': -1.0}, {'fs': 0.0}])
def test_all_masked_geometries_give_exact_zeros(lib, change):
    from utils.beamform import bf_das
    case = bi.CASES['c8']
    p = dict(bi.param(case), **change)
    for kind in bi.KINDS:
        for bits in (64, 32):
            sig = bi.signal('c8', case, kind, bits)
            for compound in (True, False):
                img = bf_das(sig, p, compound_opt=compound, return_iq=True)
                assert img.dtype == sig.dtype and not img.any()
                bm = bf_das(sig, p, compound_opt=compound)          # no finite pixel: zeros (the reference raises here)
                assert bm.shape == img.shape and not bm.any()


def test_batch_dimensions_and_attribute_params(lib):
    from utils.beamform import bf_das

    class Attr:
        pass
    case = bi.CASES['batch5']
    p = bi.param(case)
    a = Attr()
    for k, v in p.items():
        setattr(a, k, v)
    sig = bi.signal('batch5', case, 'cplx', 32)
    whole = bf_das(sig, a, return_iq=True)
    assert whole.shape == (5, case['Nz'], case['Nx'])
    for f in range(5):
        assert np.array_equal(whole[f], bf_das(sig[f], p, return_iq=True))
    two = bf_das(sig[:4].reshape(2, 2, *sig.shape[1:]), p, compound_opt=False)
    assert two.shape == (2, 2, case['A'], case['Nz'], case['Nx'])
    assert np.array_equal(two[1, 0], bf_das(sig[2], p, compound_opt=False))
    assert not hasattr(a, 'theta')


def test_bad_inputs_raise(lib):
    import torch
    from utils.beamform import bf_das, bf_das_rx
    case = bi.CASES['c8']
    p = bi.param(case)
    sig = bi.signal('c8', case, 'real', 32)
    for key, bad in [('c', np.nan), ('t0', np.inf), ('fs', -np.inf), ('f0', np.nan)]:
        with pytest.raises(ValueError, match='finite'):
            bf_das(sig, dict(p, **{key: bad}))
    for key in ('param_x', 'param_z', 'xe', 'angles_list'):
        arr = np.array(p[key], dtype=np.float64)
        arr[0] = np.nan
        with pytest.raises(ValueError, match='finite'):
            bf_das(sig, dict(p, **{key: arr}))
    with pytest.raises(ValueError, match='finite'):
        bf_das(sig, p, fnumber=np.inf)
    x2, z2 = np.meshgrid(p['param_x'], p['param_z'])
    zbad = z2.copy()
    zbad[0, 0] = np.inf
    with pytest.raises(ValueError, match='finite'):
        bf_das_rx(sig[0], dict(p, theta=0.0), x2, zbad)
    with pytest.raises(ValueError):
        bf_das(sig[:2], p)                                              # two angles of signal, three in the geometry
    with pytest.raises(TypeError):
        bf_das(sig.astype(np.int16), p)
    with pytest.raises(RuntimeError, match='ROCm device only'):
        bf_das(torch.from_numpy(sig), p)
    with pytest.raises(RuntimeError, match='ROCm device only'):
        bf_das_rx(torch.from_numpy(sig[0]), dict(p, theta=0.0), x2, z2)


def test_host_entry_under_sanitizers(tmp_path):
    """The host entry on all-masked and edge geometries and on i == S - 1 constructed exactly, in a stand-alone program
    built with AddressSanitizer and UBSan; every buffer is a heap block of the exact size."""
    exe = str(tmp_path / 'das_harness')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-x', 'c++', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-static-libasan', '-o', exe, SRC], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith('ok')

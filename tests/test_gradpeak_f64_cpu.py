"""float64 GradPeak without a GPU: a NumPy restatement in double (written here from models/gradpeak.py's semantics, not
taken from the oracle) reproduces tests/golden/f17_gradpeak_f64.npz -- pinning the fixture independently of the
reference run that made it -- and the float64 C ABI entries reject bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

from conftest import golden
import f64_inputs
from stofnet_amd.gradpeak import gaussian_kernel_1d


# ---- NumPy restatement, float64 throughout ------------------------------------------------------------------------
def envelope(x):
    L = x.shape[-1]
    h = np.zeros(L)
    h[1:L // 2] = 2.0
    h[0] = h[L // 2] = 1.0                                     # utils/hilbert.py:12-17
    return np.abs(np.fft.ifft(np.fft.fft(x, axis=-1) * h, axis=-1))


def smoothed_gradient(env, g):
    grad = np.empty_like(env)
    grad[:, 1:-1] = (env[:, 2:] - env[:, :-2]) / (2.0 * g)    # torch.gradient(spacing=g), :14
    grad[:, 0] = (env[:, 1] - env[:, 0]) / g
    grad[:, -1] = (env[:, -1] - env[:, -2]) / g
    k = gaussian_kernel_1d((2 * g - 1) / 6).numpy()           # float64 taps (:89-96 casts them to the data's dtype)
    r = len(k) // 2
    gp = np.pad(grad, ((0, 0), (r, r)))
    out = np.zeros_like(grad)
    for j, kj in enumerate(k):
        out += kj * gp[:, j:j + grad.shape[1]]
    return out


def default_threshold(grad):
    return np.std(grad, ddof=1) ** 16 * 1.2e13               # :18


class Q9(Exception):
    pass


def detect(env, g, th=None, ival=None):
    """grad_peak_detect (:8-68) -> [N, Kmax, 3] float64"""
    grad = smoothed_gradient(env, g)
    th = default_threshold(grad) if th is None else th
    ival = ival if ival is not None else (g // 2, g * 3)
    rows = []
    for r in range(env.shape[0]):
        ap = np.nonzero(np.diff((grad[r] > th).astype(np.int8)) == 1)[0]
        am = np.nonzero(np.diff((grad[r] < -th / 4).astype(np.int8)) == 1)[0]
        if ap.size == 0 or am.size == 0:
            rows.append([])
            continue
        k = np.searchsorted(ap, am, side='right') - 1          # nearest onset <= each falling edge (none: the first, Q8)
        a = ap[np.maximum(k, 0)]
        keep = ((am - a) > ival[0]) & ((am - a) < ival[1])
        if not keep.any():
            raise Q9
        a, m = a[keep], am[keep]
        first = np.ones(a.size, bool)
        first[1:] = a[1:] != a[:-1]                              # first peak per distinct onset
        rows.append([(float(p), float(q), env[r, q]) for p, q in zip(a[first], m[first])])
    kmax = max((len(e) for e in rows), default=0)
    out = np.zeros((env.shape[0], kmax, 3))
    for r, e in enumerate(rows):
        if e:
            out[r, :len(e)] = e
    return out


def toa(x, rf, th=None, echo_max=float('inf')):
    """toa_detect (:99-116)"""
    e = detect(envelope(x), rf // 6 * 5, th, (rf, 50 * rf))
    if e.shape[1] > echo_max:
        k = int(echo_max)
        out = np.empty((e.shape[0], k, 3))
        for r in range(e.shape[0]):
            sel = e[r][np.argsort(-e[r, :, 2], kind='stable')[:k]]
            out[r] = sel[np.argsort(sel[:, 1], kind='stable')]
        e = out
    return e


@pytest.fixture(scope='module')
def g():
    return golden('f17_gradpeak_f64')


def assert_close(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got[..., :2], want[..., :2])
    assert np.max(np.abs(got[..., 2] - want[..., 2]), initial=0.0) <= 1e-12


@pytest.mark.parametrize('rf', [10, 20])
@pytest.mark.parametrize('thn,th', [('th1e-3', 1e-3), ('thdef', None)])
def test_restatement_toa(g, rf, thn, th):
    x = f64_inputs.echo_frames(1024, 2000, int(g[f'toa_rf{rf}_seed']))
    assert_close(toa(x, rf, th), g[f'toa_rf{rf}_{thn}'])
    if th is None:
        want = float(g[f'toa_rf{rf}_thdef_th'])
        got = default_threshold(smoothed_gradient(envelope(x), rf // 6 * 5))
        assert abs(got - want) <= 1e-12 * want


def test_restatement_long_rows_envelope_input_and_discriminating_case(g):
    assert_close(toa(f64_inputs.echo_frames(64, 30720, int(g['long_rf20_seed'])), 20), g['long_rf20_thdef'])
    assert_close(detect(f64_inputs.envelopes(256, 1536, 1703), 2), g['gpd_env'])
    assert_close(toa(f64_inputs.echo_frames(16, 2000, 1705), 10, float(g['disc_th'])), g['disc'])


def test_restatement_gradpeak_settings(g):
    chirp = toa(f64_inputs.echo_frames(512, 2000, 1704), 10, None, echo_max=1)[..., 0]      # onset column
    assert np.array_equal(chirp, g['chirp'])
    pala = toa(f64_inputs.pala_frames(2, 16, 30720, 1201)[:, 0], 20, 1e-5)[..., 1]          # peak column
    assert np.array_equal(pala, g['pala'])


def test_restatement_q9():
    e = np.zeros(1536)
    e[500:800] = np.linspace(0, 1, 300)
    e[800:1200] = 1
    e[1200:1500] = np.linspace(1, 0, 300)
    with pytest.raises(Q9):
        detect(np.stack([e] * 3), 2, 1e-5)


# ---- C ABI argument checks (no device is touched) -------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from stofnet_amd import _lib
    try:
        return _lib.lib()
    except Exception as exc:                                    # noqa: BLE001
        pytest.skip(f'libstofnet_amd.so not built: {exc}')


FAKE = ctypes.c_void_p(256)                                    # never dereferenced: the checks come first


def test_abi_f64_argument_checks(lib):
    from stofnet_amd import _lib
    BAD, WS = _lib.STOF_ERR_BAD_ARG, _lib.STOF_ERR_WORKSPACE
    need = lib.stof_gradpeak_moments_f64_workspace_bytes(1000)
    assert need == 250 * 16 and lib.stof_gradpeak_moments_f64_workspace_bytes(0) == 0
    assert lib.stof_gradpeak_moments_f64_workspace_bytes(10 ** 6) == 2048 * 16
    mom = lib.stof_gradpeak_moments_f64
    assert mom(None, 1000, 2000, 5, FAKE, 5, FAKE, FAKE, need, None) == BAD
    assert mom(FAKE, -1, 2000, 5, FAKE, 5, FAKE, FAKE, need, None) == BAD
    assert mom(FAKE, 1000, 2000, 0, FAKE, 5, FAKE, FAKE, need, None) == BAD
    assert mom(FAKE, 1000, 2000, 5, FAKE, 5, None, FAKE, need, None) == BAD
    assert mom(FAKE, 1000, 2000, 5, FAKE, 5, FAKE, FAKE, need - 1, None) == WS
    assert mom(FAKE, 1000, 2000, 5, FAKE, 5, FAKE, None, need, None) == WS
    assert lib.stof_gradpeak_threshold_f64(None, FAKE, None) == BAD
    assert lib.stof_gradpeak_threshold_f64(FAKE, None, None) == BAD
    det = lib.stof_grad_peak_detect_f64
    args = [FAKE, 1000, 2000, 5, FAKE, 5, 1e-3, None, 10, 500, 0, FAKE, 32, None, FAKE, FAKE, None]
    for i, bad in ((0, None), (1, -1), (3, 0), (4, None), (14, None), (15, None), (12, -1)):
        a = list(args)
        a[i] = bad
        assert det(*a) == BAD, i
    a = list(args)
    a[10] = 1                                                  # echo_max > 0 needs `reduced`
    assert det(*a) == BAD
    a[13], a[12] = FAKE, 5000                                  # the reduction ranks <= 4096 entries per row
    assert det(*a) == _lib.STOF_ERR_UNSUPPORTED
    a = list(args)
    a[1] = 0                                                   # nothing to do: no HIP call
    assert det(*a) == 0

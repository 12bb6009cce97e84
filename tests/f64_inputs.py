"""Seeded float64 inputs of the float64 GradPeak fixture (tests/golden/f17_gradpeak_f64.npz), shared by its generator
(tests/golden/make_golden_f64.py) and the tests: the inputs are regenerated here rather than stored (1024 x 2000 float64
is 16 MB).  Every frame carries 1e-7 x seeded Gaussian noise on top of a float32 synthetic row, so that it is not
representable in float32 and a float32 detour shows in the results."""
import numpy as np

from stofnet_amd import synth


def _detail(shape, seed):
    return 1e-7 * np.random.default_rng(seed + 7919).standard_normal(shape)


def echo_frames(n, L, seed, noise=0.01):
    """[n, L] float64: synth_echo rows (one echo each, max-abs 1) + 1e-7 noise."""
    x = synth.synth_echo(n, L, seed=seed, noise=noise)[:, 0].astype(np.float64)
    return x + _detail(x.shape, seed)


def pala_frames(B, C, S, seed):
    """[B * C, 1, S] float64: synth.pala_frames flattened as main.py:301 does, + 1e-7 noise."""
    x = np.asarray(synth.pala_frames(B, C, S, seed), dtype=np.float64).reshape(B * C, 1, S)
    return x + _detail(x.shape, seed)


def envelopes(n, L, seed):
    """[n, L] float64 envelope rows for grad_peak_detect: |analytic signal| of echo_frames, formed with NumPy's FFT and
    the reference's bin rule (utils/hilbert.py:12-17: bins 1 .. L//2 - 1 doubled, bins 0 and L//2 kept, the rest zero)."""
    x = echo_frames(n, L, seed)
    h = np.zeros(L)
    h[1:L // 2] = 2.0
    h[0] = h[L // 2] = 1.0
    return np.abs(np.fft.ifft(np.fft.fft(x, axis=-1) * h, axis=-1))

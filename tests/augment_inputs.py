"""Seeded inputs and the case list of the augmentation fixture (tests/golden/f22_augment.npz), shared by its generator
(tests/golden/make_golden_augment.py) and the tests.  Rows are regenerated from their seeds, not stored.  Every row is
rounded to float32 first, and every gt is a multiple of 1/8, so float32 and float64 code see the same inputs and round
the gt alike."""
import numpy as np

SNR_DB = 30

# (L, ratio, gt): NormalizeVol -> CropChannelData(ratio) -> AddNoise(SNR_DB), the chirp chain of main.py:49,54
CROP_CASES = [(2000, .75, g) for g in (700., 10., 1900., 700.5, 701.5, 1997., 1998.)] + [
    (2000, .5, 999.5), (400, .75, 200.25), (20000, .3, 12345.125), (6, .75, 3.), (64, .25, 32.)]
# (L, kind): AddNoise(SNR_DB) alone
NOISE_CASES = [(L, kind) for L in (5, 401, 2000) for kind in ('signed', 'nonneg', 'zero')]
# (L, ratio, gt): the reference raises (randint on an empty range; the size assertion on an odd un-clipped window)
RAISE_CASES = [(2000, .75, 0.), (2000, .75, 1.), (2001, .75, 1000.)]
# (L, ratio, gt): CropChannelData(ratio, resize=True), numpy path only
RESIZE_CASE = (400, .75, 200.25)


def crop_name(i):
    return f'crop{i}'


def noise_name(L, kind):
    return f'noise_{kind}_{L}'


def np_seed(i):
    """Seed of numpy's global generator for case number i (crop cases first, then noise cases, then the others)."""
    return 4200 + i


def row(L, seed, kind='signed'):
    """[L] float64 holding float32 values: a decaying oscillation plus noise, not normalised."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    x = 3.0 * np.sin(0.37 * t + rng.uniform(0, 6.0)) * np.exp(-t / max(L / 2.0, 1.0)) + 0.2 * rng.standard_normal(L)
    if kind == 'nonneg':
        x = np.abs(x)
    elif kind == 'zero':
        x = np.zeros(L)
    return x.astype(np.float32).astype(np.float64)


def window(L, ratio, gt):
    """(start, end, low, high) of CropChannelData before the shift: the window and the half-open range of the shift."""
    width = int(round(L * ratio))
    ref = int(round(gt))
    start, end = max(0, ref - width // 2), min(ref + width // 2, L)
    if end == L:
        start = end - width
    if start == 0:
        end = width
    reach = min(ref - start, end - ref) // 2
    return start, end, -min(start, reach), min(L - end, reach)

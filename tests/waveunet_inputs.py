"""Seeded inputs and weights of the WaveUnet fixture (tests/golden/f23_waveunet.npz), shared by its generator
(tests/golden/make_golden_waveunet.py) and the tests, so that the fixture stores seeds and outputs only.

The whole batch of a case runs; the fixture keeps `kept_rows` of the output and of the logits.  Of the middle block's
output ([N, 16 n, L / 2^n]) it keeps, for every kept row, the first and last BOTT_EDGE samples of every channel
(`bott_edges`): the bottleneck of a long row would outweigh everything else in the file."""
import numpy as np

from stofnet_amd import synth

TILE = 64            # positions per work-group of wu_conv_kernel (encoder and decoder source alike)
BOTT_EDGE = 16

# (n_layers, N, L): the smallest shapes at which each mechanism can break
SHAPES = ([(1, 2, 2), (1, 2, 6),
           (2, 3, 4),                                        # bottom length 1: interpolation scale 0
           (2, 3, 8), (2, 5, 132), (2, 8, 2000),
           (2, 2, 8000), (2, 2, 20000)]                      # the fp32-coordinate cases
          + [(2, 2, L) for L in (TILE - 4, TILE, TILE + 4)]                  # tile edges of the full-resolution level
          + [(2, 2, L) for L in (2 * TILE - 8, 2 * TILE, 2 * TILE + 8)]      # ... and of the half-resolution level
          + [(3, 2, 8), (3, 2, 40),
             (10, 3, 1024),                                  # bottom length 1
             (10, 2, 3072), (12, 2, 4096)])
# name, n_layers, weight seed, N, L, first input seed
CASES = [(f'unet_n{n}_{N}x{L}', n, 800 + n, N, L, 7000 + i) for i, (n, N, L) in enumerate(SHAPES)]
IDS = [c[0] for c in CASES]


def case(name):
    return CASES[IDS.index(name)]


def frames(n, L, seed):
    """[n, 1, L] float32 synthetic echoes (max-abs 1)."""
    return synth.synth_echo(n, L, seed=seed)


def kept_rows(n, L):
    """rows of a case's output that the fixture stores"""
    return sorted({0, n - 1}) if L < 2000 else [n - 1]


def bott_edges(bott):
    """[..., C, Lb] -> the first and last BOTT_EDGE samples of every channel (everything when it is that short)"""
    e = BOTT_EDGE
    return bott if bott.shape[-1] <= 2 * e else np.concatenate([bott[..., :e], bott[..., -e:]], -1)


def block_names(n_layers):
    """prefixes of the Conv1d + BatchNorm1d blocks in module order: (conv prefix, BN prefix, Cout, Cin, taps)"""
    n, c = n_layers, 16
    out = [(f'encoder.{i}.main.0', f'encoder.{i}.main.1', c * (i + 1), 1 if i == 0 else c * i, 15) for i in range(n)]
    out.append(('middle.0', 'middle.1', c * n, c * n, 15))
    out += [(f'decoder.{i}.main.0', f'decoder.{i}.main.1', c * (n - i), 2 * c * n if i == 0 else c * (2 * (n - i) + 1), 5)
            for i in range(n)]
    return out


def seeded_waveunet(n_layers, seed):
    """state_dict (module order, num_batches_tracked included) of WaveUnet(n_layers, 16): He-scaled Gaussian convolution
    weights, biases 0.05 N(0, 1), BatchNorm gamma in U(0.7, 1.4), beta 0.05 N, running mean 0.2 N, running var in
    U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for conv, bn, co, ci, k in block_names(n_layers):
        sd[conv + '.weight'] = (rng.standard_normal((co, ci, k)) * np.sqrt(2.0 / (ci * k))).astype(np.float32)
        sd[conv + '.bias'] = (0.05 * rng.standard_normal(co)).astype(np.float32)
        sd[bn + '.weight'] = rng.uniform(0.7, 1.4, co).astype(np.float32)
        sd[bn + '.bias'] = (0.05 * rng.standard_normal(co)).astype(np.float32)
        sd[bn + '.running_mean'] = (0.2 * rng.standard_normal(co)).astype(np.float32)
        sd[bn + '.running_var'] = rng.uniform(0.5, 2.0, co).astype(np.float32)
        sd[bn + '.num_batches_tracked'] = np.int64(0)
    sd['out.0.weight'] = (rng.standard_normal((1, 17, 1)) * np.sqrt(2.0 / 17)).astype(np.float32)
    sd['out.0.bias'] = (0.05 * rng.standard_normal(1)).astype(np.float32)
    return sd


def kernel_arrays(sd):
    """the arrays stof_waveunet_pack_weights reads: module order without the num_batches_tracked entries"""
    return [np.asarray(v, dtype=np.float32) for k, v in sd.items() if not k.endswith('num_batches_tracked')]

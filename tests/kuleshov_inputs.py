"""Seeded inputs and weights of the Kuleshov fixture (tests/golden/f24_kuleshov.npz), shared by its generator
(tests/golden/make_golden_kuleshov.py) and the tests, so that the fixture stores seeds and outputs only.

The whole batch of a case runs; the fixture keeps `kept_rows` of every tap.  Of the input of final_conv ([N, 128, Lc])
it keeps, for every kept row, `final_in_window`: the first and last EDGE positions of every channel and the 2 EDGE
positions around the seam between the shuffled up_conv3 output and the appended down_conv0 output."""
import functools

import numpy as np

from stofnet_amd import synth
from stofnet_amd.kuleshov import chain_lengths

EDGE = 16
WEIGHT_SEED = 2400
N_FILTERS = (128, 256, 512, 512)
N_FILTERSIZES = (65, 33, 17, 9)

# (N, input_length, output_length, samples per input row): the smallest shapes at which each mechanism can break
SHAPES = [(3, 641, 64, 641),         # every level at its minimum: bottleneck 9, up_conv0 output length 1
          (2, 642, 1, 642),          # a dropped last sample in down_conv0; a single output
          (3, 645, 130, 645),        # mixed parities down the chain; N no tile multiple
          (2, 657, 1314, 657),
          (2, 641, 6410, 641),       # Linear with N much larger than K
          (3, 1000, 2000, 1100),     # rows longer than input_length: the crop
          (2, 2000, 640, 2000),      # the workload's own chain of lengths
          (1, 700, 64, 700)]         # a single row
# name, N, input_length, output_length, row length, first input seed
CASES = [(f'kul_{N}x{L}to{O}', N, L, O, X, 8000 + i) for i, (N, L, O, X) in enumerate(SHAPES)]
IDS = [c[0] for c in CASES]
TAPS = ('y', 'bott', 'fin_in', 'fin')


def case(name):
    return CASES[IDS.index(name)]


def frames(n, length, seed):
    """[n, 1, length] float32 synthetic echoes (max-abs 1)."""
    return synth.synth_echo(n, length, seed=seed)


def kept_rows(n, L):
    """rows of a case's taps that the fixture stores: the first and the last, the last alone from L = 1000 on (the
    bottleneck and final_conv maps of two long rows would outweigh everything else in the file)"""
    return sorted({0, n - 1}) if L < 1000 else [n - 1]


def final_in_window(a, input_length):
    """[..., 128, Lc] -> [..., 128, 4 EDGE]: the first EDGE positions, the 2 EDGE around the seam, the last EDGE"""
    d = chain_lengths(input_length)
    seam = 2 * d['up'][-1]
    assert a.shape[-1] == d['cat'][-1] and EDGE <= seam - EDGE and seam + EDGE <= a.shape[-1] - EDGE
    return np.concatenate([a[..., :EDGE], a[..., seam - EDGE:seam + EDGE], a[..., -EDGE:]], -1)


def block_names():
    """the Conv1d + BatchNorm1d blocks in module order: (conv name, BN name or None, Cout, Cin, taps)"""
    nf, fs = N_FILTERS, N_FILTERSIZES
    out = [(f'down_conv{i}', f'down_bn{i}', nf[i], 1 if i == 0 else nf[i - 1], fs[i]) for i in range(4)]
    out.append(('bottleneck', None, 512, 512, 9))
    out += [(f'up_conv{i}', f'up_bn{i}', 2 * nf[3 - i], 512 if i == 0 else nf[-i], fs[3 - i]) for i in range(4)]
    out.append(('final_conv', None, 2, 128, 9))
    return out


@functools.lru_cache(maxsize=1)
def _seeded_convs(seed):
    rng = np.random.default_rng(seed)
    sd = {}
    for conv, bn, co, ci, k in block_names():
        sd[conv + '.weight'] = (rng.standard_normal((co, ci, k)) * np.sqrt(2.0 / (ci * k))).astype(np.float32)
        sd[conv + '.bias'] = (0.05 * rng.standard_normal(co)).astype(np.float32)
        if bn is not None:
            sd[bn + '.weight'] = rng.uniform(0.7, 1.4, co).astype(np.float32)
            sd[bn + '.bias'] = (0.05 * rng.standard_normal(co)).astype(np.float32)
            sd[bn + '.running_mean'] = (0.2 * rng.standard_normal(co)).astype(np.float32)
            sd[bn + '.running_var'] = rng.uniform(0.5, 2.0, co).astype(np.float32)
            sd[bn + '.num_batches_tracked'] = np.int64(0)
    return sd


def seeded_kuleshov(input_length, output_length, seed=WEIGHT_SEED):
    """state_dict (module order, num_batches_tracked included) of Kuleshov(input_length, output_length): He-scaled
    Gaussian convolution and Linear weights, biases 0.05 N(0, 1), BatchNorm gamma in U(0.7, 1.4), beta 0.05 N, running
    mean 0.2 N, running var in U(0.5, 2).  The convolutions depend on the seed alone, the Linear layer on the lengths too."""
    sd = dict(_seeded_convs(seed))
    fc = chain_lengths(input_length)['fc_dim']
    rng = np.random.default_rng([seed, int(input_length), int(output_length)])
    sd['output_fc.weight'] = (rng.standard_normal((output_length, fc)) * np.sqrt(2.0 / fc)).astype(np.float32)
    sd['output_fc.bias'] = (0.05 * rng.standard_normal(output_length)).astype(np.float32)
    return sd


def kernel_arrays(sd):
    """the arrays stof_kuleshov_pack_weights reads: module order without the num_batches_tracked entries"""
    return [np.asarray(v, dtype=np.float32) for k, v in sd.items() if not k.endswith('num_batches_tracked')]


def forward64(sd, x, input_length, eps=1e-5):
    """The network in float64, restated from its data flow with plain conv1d, indexing and matmul (no module forward).
    x [n, 1, >= input_length] -> dict of the taps y [n, 1, O], bott [n, 512, B], fin_in [n, 128, Lc], fin [n, 2, F]."""
    import torch
    import torch.nn.functional as F
    w = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if not k.endswith('num_batches_tracked')}

    def bn(a, name):
        s = w[name + '.weight'] / torch.sqrt(w[name + '.running_var'] + eps)
        return (a - w[name + '.running_mean'][None, :, None]) * s[None, :, None] + w[name + '.bias'][None, :, None]

    def lrelu(a, slope):
        return torch.where(a > 0, a, slope * a)

    a = torch.from_numpy(np.asarray(x)).double()[:, :, :input_length]
    downs = []
    for i in range(4):
        a = F.conv1d(a, w[f'down_conv{i}.weight'], w[f'down_conv{i}.bias'], stride=2)
        a = lrelu(bn(lrelu(a, 0.01), f'down_bn{i}'), 0.2)
        downs.append(a)
    a = lrelu(F.conv1d(a, w['bottleneck.weight'], w['bottleneck.bias'], stride=2), 0.2)
    out = {'bott': a}
    for i in range(4):
        a = bn(F.conv1d(a, w[f'up_conv{i}.weight'], w[f'up_conv{i}.bias']), f'up_bn{i}')
        n, c, p = a.shape
        sh = torch.empty((n, c // 2, 2 * p), dtype=a.dtype)
        sh[:, :, 0::2] = a[:, 0::2]                      # out[ch >> 1, 2 p + (ch & 1)] = in[ch, p]
        sh[:, :, 1::2] = a[:, 1::2]
        a = torch.cat([sh, downs[3 - i]], -1)
    out['fin_in'] = a
    a = F.conv1d(a, w['final_conv.weight'], w['final_conv.bias'])
    out['fin'] = a
    flat = a.permute(0, 2, 1).reshape(a.shape[0], -1)    # flat[n, 2 pos + ch]
    out['y'] = (flat @ w['output_fc.weight'].T + w['output_fc.bias'])[:, None, :]
    return {k: v.numpy() for k, v in out.items()}

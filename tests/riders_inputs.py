"""Seeded inputs and weights of the EDSR_1D / ESPCN_1D fixture (tests/golden/f21_riders.npz), shared by its generator
(tests/golden/make_golden_riders.py) and the tests, so that the fixture stores seeds and outputs only.

The whole batch of a case runs; the fixture keeps `kept_rows` of its outputs (rows are independent).  Of EDSR's hooked
intermediate (the input of `upscale`, [N, 64, L]) it keeps, for the last kept row, the first and last TRUNK_EDGE samples
of every channel (`trunk_edges`)."""
import numpy as np
import torch
import torch.nn.functional as F

from stofnet_amd import synth

CHECKPOINTS = {'proud-cherry': 'proud-cherry-1441_rf-scale10_epoch_22.pth',      # EDSR_1D(1, 64, 8, 4)
               'snowy-dragon': 'snowy-dragon-1551_rf-scale20_epoch_35.pth',
               'vital-puddle': 'vital-puddle-1443_rf-scale10_epoch_65.pth',      # ESPCN_1D(4)
               'wobbly-sponge': 'wobbly-sponge-1552_rf-scale20_epoch_75.pth'}
EDSR_CKPTS = ('proud-cherry', 'snowy-dragon')
ESPCN_CKPTS = ('vital-puddle', 'wobbly-sponge')

ED_TILE = 128        # outputs per work-group of ed_conv_kernel (the waveforms are flattened: a tile spans rows)
ES_TILE = 126        # samples per work-group of es_kernel
SHAPES = [(8, 2000), (3, 33), (2, 1), (1, 2), (5, 129), (2, 4001)]
TRUNK_EDGE = 16

# name, weights (a checkpoint key, or an int = the seed of seeded weights), num_blocks, r, N, L, first input seed
EDSR_CASES = ([(f'edsr_cherry_{n}x{L}', 'proud-cherry', 8, 4, n, L, 5100 + i) for i, (n, L) in enumerate(SHAPES)]
              + [('edsr_dragon_4x2000', 'snowy-dragon', 8, 4, 4, 2000, 5110)]
              + [(f'edsr_cherry_tile{L}', 'proud-cherry', 8, 4, 2, L, 5120 + i)
                 for i, L in enumerate((ED_TILE - 1, ED_TILE, ED_TILE + 1))]
              + [(f'edsr_seeded_b{b}_r{r}', 610 + i, b, r, n, L, 5130 + i)
                 for i, (b, r, n, L) in enumerate([(0, 1, 3, 65), (1, 2, 2, 96), (3, 8, 2, 100), (2, 16, 2, 31), (1, 32, 3, 64),
                                                   (1, 64, 2, 40)])])
# name, weights, r, N, L, first input seed
ESPCN_CASES = ([(f'espcn_puddle_{n}x{L}', 'vital-puddle', 4, n, L, 5200 + i) for i, (n, L) in enumerate(SHAPES)]
               + [('espcn_sponge_4x2000', 'wobbly-sponge', 4, 4, 2000, 5210)]
               + [(f'espcn_puddle_tile{L}', 'vital-puddle', 4, 2, L, 5220 + i)
                  for i, L in enumerate((ES_TILE - 1, ES_TILE, ES_TILE + 1))]
               + [(f'espcn_seeded_r{r}', 710 + i, r, 3, 130, 5230 + i) for i, r in enumerate((1, 2, 3, 10, 16, 17, 33, 64))])


def frames(n, L, seed):
    """[n, 1, L] float32 synthetic echoes (max-abs 1)."""
    return synth.synth_echo(n, L, seed=seed)


def kept_rows(n, L, r):
    """rows of a case's output that the fixture stores"""
    return sorted({0, n - 1}) if L * r < 2000 else [n - 1]


def trunk_edges(trunk_row):
    """[64, L] -> the first and last TRUNK_EDGE samples of every channel (the whole row when it is that short)"""
    e = TRUNK_EDGE
    return trunk_row if trunk_row.shape[-1] <= 2 * e else np.concatenate([trunk_row[:, :e], trunk_row[:, -e:]], -1)


def _conv(rng, sd, name, co, ci, k, gain=2.0):
    sd[name + '.weight'] = (rng.standard_normal((co, ci, k)) * np.sqrt(gain / (ci * k))).astype(np.float32)
    sd[name + '.bias'] = (0.01 * rng.standard_normal(co)).astype(np.float32)


def seeded_edsr(num_blocks, r, seed):
    """state_dict (float32 arrays, module order) of EDSR_1D(1, 64, num_blocks, r) with He-scaled Gaussian weights"""
    rng = np.random.default_rng(seed)
    sd = {}
    _conv(rng, sd, 'conv_input', 64, 1, 3)
    for b in range(num_blocks):
        _conv(rng, sd, f'residual_blocks.{b}.conv1', 64, 64, 3)
        _conv(rng, sd, f'residual_blocks.{b}.conv2', 64, 64, 3, gain=0.5)
    _conv(rng, sd, 'conv_mid', 64, 64, 3)
    _conv(rng, sd, 'conv_output', 1, 64 // r, 3)
    return sd


def seeded_espcn(r, seed):
    """state_dict of ESPCN_1D(r) with Gaussian weights that leave the logits in the sigmoid's sensitive range"""
    rng = np.random.default_rng(seed)
    sd = {}
    _conv(rng, sd, 'conv1', 64, 1, 5)
    _conv(rng, sd, 'conv2', 32, 64, 3)
    _conv(rng, sd, 'conv3', r, 32, 3, gain=4.0)
    sd['conv3.bias'] = (0.5 * rng.standard_normal(r)).astype(np.float32)
    return sd


def weights(wkey, load, *shape):
    """float32 state_dict of a case: `load(key)` for a shipped checkpoint, seeded weights for an int"""
    if isinstance(wkey, str):
        return load(wkey)
    return seeded_edsr(*shape, wkey) if len(shape) == 2 else seeded_espcn(*shape, wkey)


# float64 torch-CPU restatements of the two networks (tests/test_riders_cpu.py pins them against the fixture)
def shuffle64(x, r):
    """SampleShuffle1D (utils/sample_shuffle.py:24-27): out[n, c, w r + k] = in[n, k C + c, w]"""
    n, cin, w = x.shape
    return x.view(n, r, cin // r, w).permute(0, 2, 3, 1).contiguous().view(n, cin // r, w * r)


def edsr64(sd, num_blocks, r, x):
    """EDSR_1D.forward in float64 on torch CPU -> (y [N, 1, L r], the input of upscale [N, 64, L])"""
    d = lambda k: torch.from_numpy(np.asarray(sd[k], np.float64))     # noqa: E731
    conv = lambda a, k: F.conv1d(a, d(k + '.weight'), d(k + '.bias'), padding=1)     # noqa: E731
    first = F.relu(conv(torch.from_numpy(np.asarray(x, np.float64)), 'conv_input'))
    out = first
    for b in range(num_blocks):
        out = conv(F.relu(conv(out, f'residual_blocks.{b}.conv1')), f'residual_blocks.{b}.conv2') + out
    trunk = conv(out, 'conv_mid') + first
    return conv(shuffle64(trunk, r), 'conv_output').numpy(), trunk.numpy()


def espcn64(sd, r, x):
    """ESPCN_1D.forward in float64 on torch CPU -> (y [N, 1, L r], the logits [N, 1, L r])"""
    d = lambda k: torch.from_numpy(np.asarray(sd[k], np.float64))     # noqa: E731
    a = torch.tanh(F.conv1d(torch.from_numpy(np.asarray(x, np.float64)), d('conv1.weight'), d('conv1.bias'), padding=2))
    a = torch.tanh(F.conv1d(a, d('conv2.weight'), d('conv2.bias'), padding=1))
    logits = shuffle64(F.conv1d(a, d('conv3.weight'), d('conv3.bias'), padding=1), r)
    return torch.sigmoid(logits).numpy(), logits.numpy()

"""Cases of the WaveUnet training fixture (tests/golden/f30_waveunet_training.npz), shared by its generator
(tests/golden/make_golden_waveunet_training.py) and the tests, so that the fixture stores seeds and results only: the weights
come from waveunet_inputs.seeded_waveunet, the frames from waveunet_inputs.frames, the cotangent t of loss = sum(y * t) from
`cotangent`.

Per case `<name>` the fixture holds, all from the reference's Wave-U-Net in .train() on the CPU:
  `<name>.seed`                          the input seed
  `<name>.same`                          1 where the reference's own fp32 LeakyReLU decisions equal its float64 ones
  `<name>.y` [N, 1, L], `<name>.dx`      the fp32 output and d loss / d x
  `<name>.run_mean.<b>`, `.run_var.<b>`  block b's running statistics after the step (blocks in module order: encoder 0 .. n-1,
                                         middle, decoder 0 .. n-1), `<name>.nbt` num_batches_tracked of the first block
  `<name>.grad.<p>`                      d loss / d parameter p in full where p has at most KEEP floats, else
  `<name>.gmax.<p>`, `.gsum.<p>`, `.grad_strided.<p>`   max |.|, float64 sum, every STRIDE-th element
  `<name>.dev.<tensor>`                  max |fp32 - float64| of the reference itself for every tensor above (y, dx, run_mean.b,
                                         run_var.b, grad.p), float64; for the conv bias gradients of the blocks the largest over
                                         NOISE_DRAWS cotangents (see `zero_grads`)
  `<name>.bn_dev` [2 n + 1], `<name>.near` [2 n + 1]   per block: max |fp32 - float64| of the BatchNorm output, and the number of
                                         float64 BatchNorm outputs within MARGIN x that deviation of zero

A LeakyReLU decision that flips under rounding moves a whole term of a gradient sum, so gradients are compared with the float64
network run with the ROUTE's decisions: `restate64(..., decisions)`."""
import numpy as np
import torch
import torch.nn.functional as F

import waveunet_inputs as wi
from stofnet_amd.waveunet_training import CHUNKS

KEEP, STRIDE = 1024, 503
MARGIN = 8.0
EPS, MOMENTUM = 1e-5, 0.1
NOISE_DRAWS = 8
TILE = wi.TILE

# (n_layers, N, L): the smallest shapes at which each mechanism can break
SHAPES = ([(1, 2, 2),                                       # two values per channel in the middle block, the minimum
           (2, 3, 4),                                       # bottom length 1: interpolation scale 0
           (2, 3, 8), (3, 2, 40), (2, 5, 132)]              # odd batches, three levels, rows that are no multiple of any tile
          + [(2, 2, L) for L in (TILE - 4, TILE, TILE + 4)]                  # tile edges of the full-resolution level
          + [(2, 2, L) for L in (2 * TILE - 8, 2 * TILE, 2 * TILE + 8)]      # ... and of the half-resolution level
          # N = 1, n = 1: the rows of level 0 (L, even) two below, on and two above every kernel's rows per partial, and the rows of
          # level 1 (L / 2) one below, on and one above it
          + [(1, 1, L) for L in sorted({c + d for c in set(CHUNKS.values()) for d in (-2, 0, 2)} |
                                       {2 * (c + d) for c in set(CHUNKS.values()) for d in (-1, 0, 1)})]
          + [(7, 3, 128),                                   # the decoders' second 192-channel LDS pass (Cin = 224)
             (10, 3, 1024),                                 # the depth main.py builds for PALA; bottom length 1
             (12, 2, 4096),                                 # the maximum depth
             (2, 2, 2000)])                                 # the chirp workload's own row
# input seeds other than 7300 + index: the generator's --search (the first seed, in steps of 1000, at which the reference's own fp32
# LeakyReLU decisions equal its float64 ones, where one exists within SEARCH_TRIES)
SEARCH_TRIES = 4
SEED_OVERRIDES = {}        # every case but unet_n12_2x4096 holds at its first seed; that one found none (`.same` = 0, 1154 near-zero outputs)
# name, n_layers, weight seed, N, L, input seed
CASES = [(f'unet_n{n}_{N}x{L}', n, 800 + n, N, L, SEED_OVERRIDES.get(f'unet_n{n}_{N}x{L}', 7300 + i)) for i, (n, N, L) in enumerate(SHAPES)]
IDS = [c[0] for c in CASES]
TINY = tuple(c[0] for c in CASES if c[3] * c[4] < 128)          # N L < 128: y, running statistics and finiteness only
GRAD_IDS = [c[0] for c in CASES if c[3] * c[4] >= 128]


def case(name):
    return CASES[IDS.index(name)]


def blocks(n_layers):
    """(conv prefix, BN prefix, Cout, Cin, taps) in module order"""
    return wi.block_names(n_layers)


def params(n_layers):
    """parameter names in module order"""
    out = []
    for conv, bn, *_ in blocks(n_layers):
        out += [conv + '.weight', conv + '.bias', bn + '.weight', bn + '.bias']
    return out + ['out.0.weight', 'out.0.bias']


def zero_grads(n_layers):
    """The conv bias gradients of the blocks are analytically 0 under train-mode BatchNorm (column sums of dz): the reference's
    fp32 deviation there is rounding noise, of which one sample can happen to be ~0.  Their stored `dev` is the largest of
    NOISE_DRAWS samples: the stored gradient's cotangent and NOISE_DRAWS - 1 further ones, cotangent(n, L, seed + 17 k)."""
    return [conv + '.bias' for conv, *_ in blocks(n_layers)]


def weights(n_layers, wseed):
    return wi.seeded_waveunet(n_layers, wseed)


def frames(n, L, seed):
    return wi.frames(n, L, seed)


def cotangent(n, L, seed):
    """t [n, 1, L] float32 of loss = sum(y * t)"""
    return np.random.default_rng(seed + 90000).standard_normal((n, 1, L)).astype(np.float32)


def kept_in_full(shape):
    return int(np.prod(shape)) <= KEEP


def restate64(sd, n_layers, x, t, decisions=None):
    """The network in train mode in float64 torch on the float32 arrays `sd`, x [N, 1, L], t [N, 1, L], loss = sum(y * t).

    decisions: None = its own, else per block a bool array [N, C, L_level] (True: slope 1).
    -> dict: y, dx, grads {name: array}, decisions, bn_out (per block the BatchNorm outputs [N, C, L_level]), run_mean, run_var
       (per block the new running statistics)."""
    n = int(n_layers)
    names = params(n)
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=torch.float64, requires_grad=True) for k in names}
    x = torch.tensor(np.asarray(x), dtype=torch.float64).reshape(x.shape[0], 1, x.shape[-1]).requires_grad_(True)
    decs, bn_out, run_mean, run_var = [], [], [], []

    def block(b, a):
        conv, bn, _, _, k = blocks(n)[b]
        z = F.conv1d(a, p[conv + '.weight'], p[conv + '.bias'], padding=k // 2)
        m = z.shape[0] * z.shape[2]
        mean, var = z.mean((0, 2), keepdim=True), z.var((0, 2), unbiased=False, keepdim=True)
        v = (z - mean) / torch.sqrt(var + EPS) * p[bn + '.weight'].view(1, -1, 1) + p[bn + '.bias'].view(1, -1, 1)
        run_mean.append((1 - MOMENTUM) * np.asarray(sd[bn + '.running_mean'], np.float64) + MOMENTUM * mean.detach().numpy().reshape(-1))
        run_var.append((1 - MOMENTUM) * np.asarray(sd[bn + '.running_var'], np.float64) +
                       MOMENTUM * var.detach().numpy().reshape(-1) * m / (m - 1))
        d = (v > 0) if decisions is None else torch.as_tensor(np.asarray(decisions[b]).astype(bool))
        decs.append(d.numpy())
        bn_out.append(v.detach().numpy())
        return torch.where(d, v, 0.1 * v)

    skips, o = [], x
    for i in range(n):
        o = block(i, o)
        skips.append(o)
        o = o[:, :, ::2]
    o = block(n, o)
    for i in range(n):
        o = F.interpolate(o, scale_factor=2, mode='linear', align_corners=True)
        o = block(n + 1 + i, torch.cat([o, skips[n - 1 - i]], dim=1))
    y = torch.tanh(F.conv1d(torch.cat([o, x], dim=1), p['out.0.weight'], p['out.0.bias']))
    (y * torch.tensor(np.asarray(t), dtype=torch.float64)).sum().backward()
    return {'y': y.detach().numpy(), 'dx': x.grad.numpy(), 'grads': {k: v.grad.numpy() for k, v in p.items()}, 'decisions': decs,
            'bn_out': bn_out, 'run_mean': run_mean, 'run_var': run_var}


def bound(B, ref64, dev):
    """the project's tolerance rule: |ours - ref64| <= max(B max|ref64|, 8 dev)"""
    return max(B * float(np.abs(ref64).max()), 8.0 * float(dev))


def stored_grad(fx, name, p, shape):
    """parameter p's gradient of case `name` as the fixture `fx` stores it"""
    return fx[f'{name}.grad.{p}'] if kept_in_full(shape) else fx[f'{name}.grad_strided.{p}']


def view_like_stored(g):
    """a full gradient array as the fixture stores it"""
    g = np.asarray(g)
    return g if kept_in_full(g.shape) else g.reshape(-1)[::STRIDE]

"""Cases of the SincNet training fixture (tests/golden/f29_sincnet_training.npz), shared by its generator
(tests/golden/make_golden_sincnet_training.py) and the tests, so that the fixture stores seeds and results only: the frames come
from sincnet_inputs.frames, the weights from `weights` (the mel init with sincnet_inputs.seeded_convs, or a shipped checkpoint
through sincnet_inputs.checkpoint_weights), the cotangent t of loss = sum(y * t) from `cotangent`.

Per case `<name>` the fixture holds, all from the reference's SincNet in .train() on the CPU:
  `<name>.seed`                          the input seed
  `<name>.y` [N, 1, L], `<name>.dx`      the fp32 output and d loss / d x
  `<name>.run_mean.<i>`, `.run_var.<i>`  bn.i's running statistics after the step, `<name>.nbt` num_batches_tracked of bn.0
  `<name>.grad.<p>`                      d loss / d parameter p in full where p has at most KEEP floats, else
  `<name>.gmax.<p>`, `.gsum.<p>`, `.grad_stride53.<p>`   max |.|, float64 sum, every 53rd element
  `<name>.dev.<tensor>`                  max |fp32 - float64| of the reference itself for every tensor above (y, dx, run_mean.i,
                                         run_var.i, grad.p), float64; for the conv bias gradients the largest over NOISE_DRAWS
                                         cotangents (see ZERO_GRADS)
  `<name>.bn_dev` [3], `<name>.near` [3] per LeakyReLU layer: max |fp32 - float64| of the BatchNorm output, and the number of
                                         float64 BatchNorm outputs within MARGIN x that deviation of zero

A LeakyReLU decision that flips under rounding moves a whole term of a gradient sum, so gradients are compared with the float64
network run with the ROUTE's decisions: `restate64(..., decisions)`."""
import numpy as np
import torch
import torch.nn.functional as F

import sincnet_inputs as si

KEEP, STRIDE = 6144, 53
MARGIN = 8.0
EPS, MOMENTUM = 1e-5, 0.05
TAPS = (1023, 11, 9, 7)
# rows per partial of the chunked kernels (stofnet_amd/sincnet_training.py CHUNKS)
CHUNKS = {'conv_wgrad': 64, 'out_wgrad': 256, 'bank_grad': 128}

# The conv bias gradients are analytically 0 under train-mode BatchNorm (column sums of dz): the reference's fp32 deviation there
# is rounding noise, of which one sample can happen to be ~0.  Their stored `dev` is the largest of NOISE_DRAWS samples: the
# stored gradient's cotangent and NOISE_DRAWS - 1 further ones, cotangent(n, L, seed + 17 k), k = 1 .. NOISE_DRAWS - 1.
ZERO_GRADS = ['conv.1.bias', 'conv.2.bias', 'conv.3.bias']
NOISE_DRAWS = 8

CHUNK_SEEDS = {129: 8229, 257: 11357}     # input seeds of the N = 1 cases other than 7100 + L

# name, weights ('init' | 'pretty-brook' | 'noble-monkey'), fs, N, L, input seed (the generator's --search: the first seed, in
# steps of 1000, at which the reference's own fp32 LeakyReLU decisions equal its float64 ones)
CASES = ([('init_2x1', 'init', 1e6, 2, 1, 7001),                      # two values per channel, the minimum
          ('init_1x2', 'init', 1e6, 1, 2, 7002),
          ('brook_3x7', 'pretty-brook', 1e6, 3, 7, 7003),             # L below every tap count
          ('brook_3x43', 'pretty-brook', 1e6, 3, 43, 7004),           # 129 rows: a 32-row tile that spans two waveforms
          ('brook_3x127', 'pretty-brook', 1e6, 3, 127, 8005),         # the 128-sample tile of the sinc kernels
          ('brook_3x128', 'pretty-brook', 1e6, 3, 128, 9006),
          ('brook_3x129', 'pretty-brook', 1e6, 3, 129, 8007),
          ('clamp_2x257', 'pretty-brook', 2e5, 2, 257, 11008),        # bands above Nyquist: the clamp gradient is 0
          ('init_2x1025', 'init', 1e6, 2, 1025, 10009),               # the row is longer than the filter
          ('monkey_2x2000', 'noble-monkey', 1.25e9, 2, 2000, 8010)]   # the workload's length
         # N = 1: the flattened row count one below, on and one above a weight-gradient kernel's rows per partial
         + [(f'brook_1x{c + d}', 'pretty-brook', 1e6, 1, c + d, CHUNK_SEEDS.get(c + d, 7100 + c + d))
            for c in sorted(set(CHUNKS.values())) for d in (-1, 0, 1)])
IDS = [c[0] for c in CASES]
TINY = ('init_2x1', 'init_1x2', 'brook_3x7')          # N L < 128: y, running statistics and finiteness only
GRAD_IDS = [c[0] for c in CASES if c[3] * c[4] >= 128]

PARAMS = (['conv.0.low_hz_', 'conv.0.band_hz_'] + [f'conv.{i}.{k}' for i in (1, 2, 3) for k in ('weight', 'bias')] +
          [f'bn.{i}.{k}' for i in range(4) for k in ('weight', 'bias')])
SHAPES = {'conv.0.low_hz_': (128, 1), 'conv.0.band_hz_': (128, 1), 'conv.1.weight': (128, 128, 11), 'conv.1.bias': (128,),
          'conv.2.weight': (128, 128, 9), 'conv.2.bias': (128,), 'conv.3.weight': (1, 128, 7), 'conv.3.bias': (1,),
          **{f'bn.{i}.{k}': ((128,) if i < 3 else (1,)) for i in range(4) for k in ('weight', 'bias')}}


def case(name):
    return next(c for c in CASES if c[0] == name)


def kept_in_full(p):
    return int(np.prod(SHAPES[p])) <= KEEP


def weights(wkey, fs):
    """state_dict of numpy arrays (float32, num_batches_tracked int64)"""
    if wkey != 'init':
        return {k: np.asarray(v) for k, v in si.checkpoint_weights(wkey).items()}
    from stofnet_amd.sincnet import mel_init
    low, band = mel_init(fs)
    sd = {'conv.0.low_hz_': low.numpy(), 'conv.0.band_hz_': band.numpy()}
    sd.update(si.seeded_convs(si.INIT_WSEED))
    for i, c in enumerate((128, 128, 128, 1)):
        sd.update({f'bn.{i}.weight': np.ones(c, np.float32), f'bn.{i}.bias': np.zeros(c, np.float32),
                   f'bn.{i}.running_mean': np.zeros(c, np.float32), f'bn.{i}.running_var': np.ones(c, np.float32),
                   f'bn.{i}.num_batches_tracked': np.zeros((), np.int64)})
    return sd


def frames(n, L, seed):
    """sincnet_inputs.frames [n, 1, L]; one-sample rows, which that normalises to +-1 each (equal rows have batch variance 0:
    BatchNorm would amplify rounding noise alone), get a seeded amplitude in [0.25, 1)"""
    x = si.frames((n, 1, L), seed)
    if L == 1:
        x = x * np.random.default_rng(seed + 50000).uniform(0.25, 1.0, (n, 1, 1)).astype(np.float32)
    return x


def cotangent(n, L, seed):
    """t [n, 1, L] float32 of loss = sum(y * t)"""
    return np.random.default_rng(seed + 90000).standard_normal((n, 1, L)).astype(np.float32)


def synth64(low_p, band_p, fs):
    """the filter synthesis in float64 torch: low_hz_, band_hz_ [128, 1] -> bank [128, 1, 1023]"""
    k = TAPS[0]
    n_lin = torch.linspace(0, k / 2 - 1, steps=k // 2, dtype=torch.float64)
    window = 0.54 - 0.46 * torch.cos(2 * np.pi * n_lin / k)
    n = 2 * np.pi * torch.arange(-(k - 1) / 2, 0, dtype=torch.float64).view(1, -1) / fs
    low = 50 + low_p.abs()
    high = torch.clamp(low + 50 + band_p.abs(), 50, fs / 2)
    band = (high - low)[:, 0]
    left = (torch.sin(high @ n) - torch.sin(low @ n)) / (n / 2) * window
    return (torch.cat([left, 2 * band.view(-1, 1), left.flip(1)], 1) / (2 * band[:, None])).view(128, 1, k)


def restate64(sd, fs, x, t, decisions=None):
    """The network in train mode in float64 torch on the float32 arrays `sd`, x [N, 1, L], t [N, 1, L], loss = sum(y * t).

    decisions: None = its own, else per LeakyReLU layer a bool array [N, 128, L] (True: slope 1).
    -> dict: y, dx, grads {name: array}, decisions (list of bool [N, 128, L]), bn_out (list of [N, 128, L] BatchNorm outputs),
       run_mean, run_var (lists of the new running statistics)."""
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=torch.float64, requires_grad=True) for k in PARAMS}
    x = torch.tensor(np.asarray(x), dtype=torch.float64).reshape(x.shape[0], 1, x.shape[-1]).requires_grad_(True)
    m = x.shape[0] * x.shape[-1]
    a, decs, bn_out, run_mean, run_var = x, [], [], [], []
    for i in range(4):
        k = TAPS[i]
        a = F.pad(a, ((k - 1) // 2, k - 1 - (k - 1) // 2))
        z = F.conv1d(a, synth64(p['conv.0.low_hz_'], p['conv.0.band_hz_'], fs)) if i == 0 else \
            F.conv1d(a, p[f'conv.{i}.weight'], p[f'conv.{i}.bias'])
        mean, var = z.mean((0, 2), keepdim=True), z.var((0, 2), unbiased=False, keepdim=True)
        v = (z - mean) / torch.sqrt(var + EPS) * p[f'bn.{i}.weight'].view(1, -1, 1) + p[f'bn.{i}.bias'].view(1, -1, 1)
        run_mean.append(((1 - MOMENTUM) * np.asarray(sd[f'bn.{i}.running_mean'], np.float64) + MOMENTUM * mean.detach().numpy().reshape(-1)))
        run_var.append(((1 - MOMENTUM) * np.asarray(sd[f'bn.{i}.running_var'], np.float64) +
                        MOMENTUM * var.detach().numpy().reshape(-1) * m / (m - 1)))
        if i == 3:
            a = v
            break
        d = (v > 0) if decisions is None else torch.as_tensor(np.asarray(decisions[i]).astype(bool))
        a = torch.where(d, v, 0.2 * v)
        decs.append(d.numpy())
        bn_out.append(v.detach().numpy())
    (a * torch.tensor(np.asarray(t), dtype=torch.float64)).sum().backward()
    return {'y': a.detach().numpy(), 'dx': x.grad.numpy(), 'grads': {k: v.grad.numpy() for k, v in p.items()}, 'decisions': decs,
            'bn_out': bn_out, 'run_mean': run_mean, 'run_var': run_var}


def bound(B, ref64, dev):
    """the project's tolerance rule: |ours - ref64| <= max(B max|ref64|, 8 dev)"""
    return max(B * float(np.abs(ref64).max()), 8.0 * float(dev))


def stored_grad(fx, name, p):
    """(kind, ...) of parameter p of case `name` in the fixture `fx`"""
    if kept_in_full(p):
        return fx[f'{name}.grad.{p}']
    return fx[f'{name}.grad_stride53.{p}']


def view_like_stored(p, g):
    """a full gradient array as the fixture stores parameter p"""
    g = np.asarray(g)
    return g if kept_in_full(p) else g.reshape(-1)[::STRIDE]

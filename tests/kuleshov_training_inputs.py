"""Cases of the Kuleshov training fixture (tests/golden/f31_kuleshov_training.npz), shared by its generator
(tests/golden/make_golden_kuleshov_training.py) and the tests, so that the fixture stores seeds and results only: the weights are
torch's seeded default initialisation of the module (`weights`), the frames and the cotangent t of loss = sum(y * t) come from
`frames` and `cotangent`, the Dropout keep-masks from the library's host entry (`masks`).

Per case `<name>` the fixture holds, all from the reference's Kuleshov in .train() on the CPU with its five Dropout attributes
replaced by `MaskDropout` (but for the p = 0 case, which runs the unpatched reference):
  `<name>.seed`                          the input seed
  `<name>.y` [N, 1, O], `<name>.dx`      the fp32 output and d loss / d x
  `<name>.run_mean.<b>`, `.run_var.<b>`  every RUN_STRIDE-th running statistic after the step (b: down 0..3, up 0..3), `<name>.nbt`
  `<name>.grad.<p>`                      d loss / d parameter p: every `stride_of`-th element (all of them up to KEEP floats, every
                                         MID_STRIDE-th up to MID floats, else every STRIDE-th), `<name>.gsum.<p>` its float64 sum
  `<name>.dev.<tensor>`                  max |fp32 - float64| of the reference itself for every tensor above, float64 (for a strided
                                         gradient: over the stored elements)
The generator asserts that the reference's fp32 activation decisions equal its float64 ones on every case.

A leaky-ReLU decision that flips under rounding moves a whole term of a gradient sum, so gradients are compared with the float64
network run with the ROUTE's decisions: `restate64(..., decisions)`."""
import numpy as np
import torch
import torch.nn.functional as F

from stofnet_amd.kuleshov import chain_lengths
from stofnet_amd.kuleshov_training import SITES, UP_COUT, dropout_keep, param_names

KEEP, MID, MID_STRIDE, STRIDE = 256, 65536, 7, 8209      # what the fixture keeps of a tensor: see `stride_of`
RUN_STRIDE = 3                                            # ... and of the running statistics
EPS, MOMENTUM = 1e-5, 0.1
DROP_SEED = 0x5EED0F31C0FFEE
# name, N, L, O, weight seed, input seed, Dropout p, dropout_call
CASES = [
    ('ks_2x641_8', 2, 641, 8, 911, 1, 0.5, 0),            # the minimum: up_conv0 has one position, up 0's BatchNorm sees 2 values
    ('ks_3x800_11', 3, 800, 11, 912, 2, 0.5, 0),          # every stride-2 level drops its last sample
    ('ks_5x719_64', 5, 719, 64, 913, 3, 0.5, 0),          # an odd batch, mixed parities
    ('ks_2x700_1400', 2, 700, 1400, 914, 4, 0.5, 0),      # the main.py shape, r = 2
    ('ks_p0_2x650_8', 2, 650, 8, 915, 5, 0.0, 0),         # no dropout: the unpatched reference
    ('ks_call3_2x660_16', 2, 660, 16, 916, 6, 0.5, 3),    # a later draw of the mask
    # a weight-gradient chunk (256 rows) one below, on and one above its edge: N D2 = 255, N D2 = N U2 = 256, D1 = 257 rows
    ('ks_edge255_3x865_8', 3, 865, 8, 917, 7, 0.5, 0),
    ('ks_edge256_4x697_8', 4, 697, 8, 918, 108, 0.5, 0),
    ('ks_edge257_1x1153_8', 1, 1153, 8, 919, 9, 0.5, 0),
]
IDS = [c[0] for c in CASES]
BN_NAMES = [f'down_bn{i}' for i in range(4)] + [f'up_bn{i}' for i in range(4)]
ZERO_GRADS = [f'up_conv{i}.bias' for i in range(4)]       # analytically 0 under train-mode BatchNorm: judged through `dev` alone


def case(name):
    return CASES[IDS.index(name)]


def edge_rows(name):
    """rows (n, t) of the eight wide convolutions of case `name`"""
    _, n, L, *_ = case(name)
    d = chain_lengths(L)
    return [n * v for v in d['down'][1:] + [d['bottleneck']] + d['up']]


def weights(L, O, wseed, module=None):
    """state dict (float32 numpy arrays) of the module's seeded default initialisation; `module`: the class to build (the project's
    by default; the reference's draws the same values)"""
    if module is None:
        from stofnet_amd import Kuleshov as module
    state = torch.random.get_rng_state()
    torch.manual_seed(wseed)
    m = module(input_length=L, output_length=O)
    torch.random.set_rng_state(state)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def frames(n, L, seed):
    return np.random.default_rng(seed + 31000).standard_normal((n, 1, L)).astype(np.float32)


def cotangent(n, O, seed):
    """t [n, 1, O] float32 of loss = sum(y * t)"""
    return np.random.default_rng(seed + 93000).standard_normal((n, 1, O)).astype(np.float32)


def stride_of(shape):
    n = int(np.prod(shape))
    return 1 if n <= KEEP else MID_STRIDE if n <= MID else STRIDE


def site_shapes(L):
    """(channels, positions) of the five Dropout sites"""
    d = chain_lengths(L)
    return [(512, d['bottleneck'])] + [(UP_COUT[i], d['up'][i]) for i in range(4)]


def masks(n, L, p, call, seed=DROP_SEED, rank=0):
    """per Dropout site keep * scale as float32 [n, C, T] in the modules' own layout (element e = t C + c of row n), scale =
    1.0f / (1.0f - p) in float32"""
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    out = []
    for site, (C, T) in enumerate(site_shapes(L)):
        keep = np.stack([dropout_keep(seed, call, rank, site, row, T * C, p).reshape(T, C).T for row in range(n)])
        out.append(keep.astype(np.float32) * scale)
    return out


class MaskDropout(torch.nn.Module):
    """Dropout with a given mask: x * (keep * scale), whatever the mode"""

    def __init__(self, mask):
        super().__init__()
        self.mask = torch.as_tensor(mask)

    def forward(self, x):
        return x * self.mask.to(device=x.device, dtype=x.dtype)


def patch_dropout(model, mask_list):
    """the five Dropout attributes of `model` (the project's or the reference's module), set on the instance"""
    for name, mk in zip(SITES, mask_list):
        setattr(model, name, MaskDropout(mk))
    return model


def restate64(sd, L, x, t, mask_list, decisions=None):
    """The network in train mode in float64 torch on the float32 arrays `sd`, x [N, 1, >= L], t [N, 1, O], loss = sum(y * t).

    mask_list: `masks(...)`.  decisions: None = its own, else a dict 'u' (per down block conv + b > 0), 'a' (per down block
    BatchNorm output > 0), 'b' (the bottleneck behind its Dropout > 0) of bool arrays [N, C, T].
    -> dict: y, dx, grads {name: array}, decisions, run_mean, run_var (down 0..3, up 0..3)."""
    names = param_names()
    p = {k: torch.tensor(np.asarray(sd[k]), dtype=torch.float64, requires_grad=True) for k in names}
    xin = torch.tensor(np.asarray(x), dtype=torch.float64).requires_grad_(True)
    mk = [torch.tensor(np.asarray(m), dtype=torch.float64) for m in mask_list]
    dec = {'u': [], 'a': [], 'b': None}
    run_mean, run_var = [None] * 8, [None] * 8

    def leaky(v, slope, given):
        d = (v > 0) if given is None else torch.as_tensor(np.asarray(given).astype(bool))
        return torch.where(d, v, slope * v), d.numpy()

    def bn(b, z):
        name = BN_NAMES[b]
        m = z.shape[0] * z.shape[2]
        mean, var = z.mean((0, 2), keepdim=True), z.var((0, 2), unbiased=False, keepdim=True)
        run_mean[b] = (1 - MOMENTUM) * np.asarray(sd[name + '.running_mean'], np.float64) + MOMENTUM * mean.detach().numpy().reshape(-1)
        run_var[b] = ((1 - MOMENTUM) * np.asarray(sd[name + '.running_var'], np.float64) +
                      MOMENTUM * var.detach().numpy().reshape(-1) * m / (m - 1))
        return (z - mean) / torch.sqrt(var + EPS) * p[name + '.weight'].view(1, -1, 1) + p[name + '.bias'].view(1, -1, 1)

    o = xin[:, :, :L]
    skips = []
    for j in range(4):
        u, du = leaky(F.conv1d(o, p[f'down_conv{j}.weight'], p[f'down_conv{j}.bias'], stride=2), 0.01,
                      None if decisions is None else decisions['u'][j])
        o, da = leaky(bn(j, u), 0.2, None if decisions is None else decisions['a'][j])
        dec['u'].append(du)
        dec['a'].append(da)
        skips.append(o)
    o, dec['b'] = leaky(F.conv1d(o, p['bottleneck.weight'], p['bottleneck.bias'], stride=2) * mk[0], 0.2,
                        None if decisions is None else decisions['b'])
    for i in range(4):
        z = bn(4 + i, F.conv1d(o, p[f'up_conv{i}.weight'], p[f'up_conv{i}.bias'])) * mk[1 + i]
        n, c, u = z.shape
        z = z.view(n, c // 2, 2, u).transpose(2, 3).reshape(n, c // 2, 2 * u)        # out[ch >> 1][2 pos + (ch & 1)] = in[ch][pos]
        o = torch.cat((z, skips[3 - i]), -1)
    o = F.conv1d(o, p['final_conv.weight'], p['final_conv.bias'])
    flat = o.transpose(1, 2).reshape(o.shape[0], -1)
    y = F.linear(flat, p['output_fc.weight'], p['output_fc.bias']).unsqueeze(1)
    (y * torch.tensor(np.asarray(t), dtype=torch.float64)).sum().backward()
    return {'y': y.detach().numpy(), 'dx': xin.grad.numpy(), 'grads': {k: v.grad.numpy() for k, v in p.items()}, 'decisions': dec,
            'run_mean': run_mean, 'run_var': run_var}


def same_decisions(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a['u'], b['u'])) and all(np.array_equal(x, y) for x, y in zip(a['a'], b['a']))
            and np.array_equal(a['b'], b['b']))


def bound(B, ref64, dev):
    """the project's tolerance rule (tests/test_waveunet_training_cpu.py): |ours - ref64| <= max(B max|ref64|, 8 dev)"""
    return max(B * float(np.abs(ref64).max()), 8.0 * float(dev))


def stored_grad(fx, name, p):
    """parameter p's gradient of case `name` as the fixture `fx` stores it: `view_like_stored` of the full gradient"""
    return fx[f'{name}.grad.{p}']


def view_like_stored(g):
    """a full gradient array as the fixture stores it"""
    g = np.asarray(g)
    return g.reshape(-1)[::stride_of(g.shape)]

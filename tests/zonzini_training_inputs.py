"""Cases of the Zonzini training fixture (tests/golden/f28_zonzini_training.npz), shared by its generator
(tests/golden/make_golden_zonzini_training.py) and the tests, so that the fixture stores seeds and results only: the frames come
from zonzini_inputs.echo_frames, the weights from `weights` (zonzini_inputs.seeded_weights or the shipped graceful-wave
checkpoint), the cotangent t of loss = sum(y * t) from `cotangent`.

Per case the fixture holds `<name>.seed`, `<name>.y` [N, 1], `<name>.dx` [N, 1, L], `<name>.dev` [layers + 1] (the reference's
fp32-vs-float64 deviation of each conv layer's and of fc1's pre-activation as a share of that layer's max |z| in float64) and
per parameter p either `<name>.grad.<p>` (in full, at most KEEP floats) or `<name>.gmax.<p>`, `<name>.gsum.<p>`,
`<name>.grad_stride53.<p>` (max |.|, float64 sum and every 53rd element).

A ReLU or pool decision that flips under rounding moves a whole term of a gradient sum.  `margin_count` counts, in float64
alone, the decisions of a case that lie within MARGIN x dev[l] x max |z_l| of flipping; a case is SAFE when there is none (the
generator asserts it for the cases marked safe), and only safe cases are compared with the reference's own gradients.

`restate64` is the network restated in float64 torch with autograd, either with its own decisions or with given ones (the
route's), which is what the gradient checks of the unsafe cases use."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import zonzini_inputs as zi

KEEP, STRIDE = 6144, 53
MARGIN = 8.0
CHUNKS = (256, 64)      # rows per partial of the weight-gradient kernels: layer 1 (rows = N Lp_1), layers >= 2 (rows = N Lp_l)
CHANNELS = {'small': zi.SMALL_CHANNELS, 'large': zi.LARGE_CHANNELS}
MIN_LEN = {'small': 936, 'large': 3752}


def pooled_len(L):
    return ((L - 10) // 2 + 1) // 2 if L >= 10 else 0


def length_for(rows, layer):
    """the shortest frame whose conv layer `layer` (0-based) has `rows` pooled outputs"""
    L = rows
    for _ in range(layer + 1):
        L = 4 * L + 8
    return L


CHUNK_SEEDS = ((6301, 6301, 6302), (6305, 6307, 6305))      # input seeds of the chunk cases (found safe by the generator's search)

# name, net, weights (a checkpoint key, or an int = the seed of seeded weights), N, L, input seed, safe
CASES = ([('small_2x936', 'small', 740, 2, 936, 6000, True),           # the minimum length: the last pooled length is 1
          ('small_3x937', 'small', 740, 3, 937, 6006, True),           # a dropped sample; row tiles across two waveforms
          ('small_2x939', 'small', 740, 2, 939, 6005, True),           # dropped samples and a dropped conv output
          ('small_2x1537', 'small', 740, 2, 1537, 6000, True),
          ('small_2x2000', 'small', 740, 2, 2000, 6010, True),
          ('wave_2x2000', 'small', 'graceful-wave', 2, 2000, 6117, True)]           # the shipped checkpoint
         # N = 1: the flattened row count of layer 1 (chunk 256) / layer 2 (chunk 64) one below, on and one above the chunk
         + [(f'small_1x{length_for(c + d, k)}', 'small', 740, 1, length_for(c + d, k), seed, True)
            for k, c in enumerate(CHUNKS) for d, seed in zip((-1, 0, 1), CHUNK_SEEDS[k])]
         + [('large_1x3752', 'large', 741, 1, 3752, 6200, False),       # the minimum length
            ('large_2x4001', 'large', 741, 2, 4001, 6201, False)])
IDS = [c[0] for c in CASES]
SAFE_IDS = [c[0] for c in CASES if c[6]]


def case(name):
    return next(c for c in CASES if c[0] == name)


def param_names(net):
    names = []
    for i in range(len(CHANNELS[net])):
        names += [f'conv_layers.{i}.weight', f'conv_layers.{i}.bias']
    return names + ['fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias']


def param_shapes(net):
    shapes, cin = {}, 1
    for i, c in enumerate(CHANNELS[net]):
        shapes[f'conv_layers.{i}.weight'], shapes[f'conv_layers.{i}.bias'] = (c, cin, 10), (c,)
        cin = c
    shapes.update({'fc1.weight': (1024, cin), 'fc1.bias': (1024,), 'fc2.weight': (1, 1024), 'fc2.bias': (1,)})
    return shapes


def kept_in_full(net, k):
    return int(np.prod(param_shapes(net)[k])) <= KEEP


def weights(wkey, net):
    """state_dict of float32 arrays"""
    if isinstance(wkey, int):
        return zi.seeded_weights(CHANNELS[net], wkey)
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', f'weights_{wkey}.npz'))
    return {k: d[k].astype(np.float32) for k in d.files}


def cotangent(n, seed):
    """t [n, 1] float32 of loss = sum(y * t)"""
    return np.random.default_rng(seed + 90000).standard_normal((n, 1)).astype(np.float32)


def restate64(sd, x, t, decisions=None):
    """The network in float64 torch on the float32 arrays `sd`, x [N, 1, L], t [N, 1], with loss = sum(y * t).

    decisions: None = its own, else (sel per conv layer as [N, C, Lp] integer arrays with 0 / 1 / 2, fc1's mask [N, 1024]).
    -> dict: y [N, 1], dx [N, 1, L], grads {name: array}, sel (list, [N, C, Lp] int8), hmask [N, 1024] bool,
       pre (list per conv layer of (even, odd) pre-activations [N, C, Lp]), z1 [N, 1024], zmax (max |z| per layer, fc1 last)."""
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    x = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    layers = sum(1 for k in p if k.startswith('conv_layers') and k.endswith('weight'))
    a, sels, pre, zmax = x, [], [], []
    for l in range(layers):
        z = F.conv1d(a, p[f'conv_layers.{l}.weight'], p[f'conv_layers.{l}.bias'], stride=2)
        lp = z.shape[-1] // 2
        e, o = z[..., 0:2 * lp:2], z[..., 1:2 * lp:2]
        if decisions is None:
            sel = torch.where(torch.maximum(e, o) > 0, torch.where(o > e, 2, 1), 0)
        else:
            sel = torch.as_tensor(np.asarray(decisions[0][l]).astype(np.int64))
        a = torch.where(sel == 1, e, torch.zeros_like(e)) + torch.where(sel == 2, o, torch.zeros_like(o))
        sels.append(sel.numpy().astype(np.int8))
        pre.append((e.detach().numpy(), o.detach().numpy()))
        zmax.append(float(z.detach().abs().max()))
    f = a.mean(-1)
    z1 = f @ p['fc1.weight'].T + p['fc1.bias']
    hmask = (z1 > 0) if decisions is None else torch.as_tensor(np.asarray(decisions[1]).astype(bool))
    h = torch.where(hmask, z1, torch.zeros_like(z1))
    y = h @ p['fc2.weight'].T + p['fc2.bias']
    (y * torch.tensor(np.asarray(t), dtype=torch.float64)).sum().backward()
    zmax.append(float(z1.detach().abs().max()))
    return {'y': y.detach().numpy(), 'dx': x.grad.numpy(), 'grads': {k: v.grad.numpy() for k, v in p.items()}, 'sel': sels,
            'hmask': hmask.numpy(), 'pre': pre, 'z1': z1.detach().numpy(), 'zmax': zmax}


def margin_masks(r64, dev, factor=MARGIN):
    """From float64 alone: per conv layer the [N, C, Lp] mask of decisions within factor x dev[l] x max |z_l| of flipping
    (max(e, o) near 0, or |e - o| of an active pair near 0), and the same for fc1's pre-activations [N, 1024]."""
    masks = []
    for l, (e, o) in enumerate(r64['pre']):
        m = factor * float(dev[l]) * r64['zmax'][l]
        top = np.maximum(e, o)
        masks.append((np.abs(top) < m) | ((top > 0) & (np.abs(e - o) < m)))
    m = factor * float(dev[-1]) * r64['zmax'][-1]
    return masks, np.abs(r64['z1']) < m


def margin_count(r64, dev, factor=MARGIN):
    masks, hm = margin_masks(r64, dev, factor)
    return int(sum(int(m.sum()) for m in masks) + int(hm.sum()))

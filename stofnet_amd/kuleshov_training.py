"""Training Kuleshov on the gfx950 kernels (reference main.py:199-289 with models/kuleshov.py in train mode): a forward that keeps
every stage output in device memory and the full backward pass in exact fp32 on the channel-last layout of the inference
kernels, behind an autograd boundary.

One kernel per stage (csrc/kuleshov_train.hip).  Forward: the inference convolution kernel with its training epilogue on the raw
weights (fragment images packed on the device, cached per parameter version); per down block u = leaky0.01(conv + b), the batch
statistics of u (double sums, fixed fold) and a = leaky0.2(u s + t) in double into the skip rows of the concatenation buffer;
the bottleneck leaky0.2(z keep scale); per up block the statistics of z and a = (z s + t) keep scale at the pixel-shuffled address;
final_conv and output_fc as in inference.  Backward, from the head down: output_fc, final_conv, then per up block the gradient at
the shuffled address times keep scale, the BatchNorm backward, the weight gradient (fp32 MFMA, K over rows, partials bounded by
MAX_PARTIALS) and the data gradient (the forward kernel on the flipped image); per down block the sum `skip rows' part, then the
next convolution's data gradient` in that order, the leaky0.2 decision a > 0, the BatchNorm backward over u, the leaky0.01
decision u > 0, and the stride-2 data gradient as two parity classes.  No MIOpen or rocBLAS call and no float atomic: two runs
give bitwise equal gradients.

Dropout can be replayed: the keep-mask is a pure function of (seed, call, rank, site, row, element) on Philox4x32-10 (the layout
is in csrc/kuleshov_train.hip and DESIGN.md), never stored, and computed again by the backward.  `dropout_keep` returns it on the
host without a GPU.

BatchNorm's running statistics are module buffers: a forward leaves the new ones in `engine.new_running` and
`Kuleshov.forward_train_kernels` copies them into the buffers on the host side.  The kernels never write them.

The training forward is NOT chunked by `max_workspace_bytes`: the batch statistics and the backward need every stage output of
the whole batch."""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._train_boundary import EndsFunction, SavedStepEngine
from .kuleshov import N_FILTERS, N_FILTERSIZES, chain_lengths

UP_CIN, UP_COUT, UP_TAPS = (512, 512, 512, 256), (1024, 1024, 512, 256), (9, 17, 33, 65)
KIND_FWD, KIND_DGRAD, KIND_EVEN, KIND_ODD = 0, 1, 2, 3
SITES = ('bottleneck_dropout', 'up_do0', 'up_do1', 'up_do2', 'up_do3')       # Dropout site 0 .. 4 of the counter

_CONSTANTS = None


def _constants():
    """The chunk constants of csrc/kuleshov_train.hip, read from the library on first use."""
    global _CONSTANTS
    if _CONSTANTS is None:
        v = (ctypes.c_int64 * 8)()
        _lib.call('stof_kuleshov_train_constants', v)
        k = [int(q) for q in v]
        _CONSTANTS = {
            # rows per partial, at the least, of the chunked reductions, and the number of partials at the most: beyond
            # CHUNKS[k] * MAX_PARTIALS[k] rows the rows per partial grow
            'CHUNKS': {'stats': k[0], 'conv_wgrad': k[2], 'final_wgrad': k[4], 'down0_wgrad': k[6]},
            'MAX_PARTIALS': {'stats': k[1], 'conv_wgrad': k[3], 'final_wgrad': k[5], 'down0_wgrad': k[7]},
        }
    return _CONSTANTS


def __getattr__(name):
    """CHUNKS, MAX_PARTIALS: module attributes that come from the built library."""
    if name in ('CHUNKS', 'MAX_PARTIALS'):
        return _constants()[name]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def dropout_keep(seed, call, rank, site, n, count, p):
    """Host only: the keep-mask (bool [count]) of row n at Dropout `site` (0: bottleneck, 1..4: up 0..3); element e = t C + c of the
    layer's unshuffled [position][channel] output."""
    keep = np.zeros(int(count), np.uint8)
    _lib.call('stof_kuleshov_dropout_keep', int(seed) & (2 ** 64 - 1), int(call) & 0xffffffff, int(rank), int(site), int(n), int(count),
              float(p), ctypes.c_void_p(keep.ctypes.data))
    return keep.astype(bool)


def param_names():
    names = []
    for i in range(4):
        names += [f'down_conv{i}.weight', f'down_conv{i}.bias', f'down_bn{i}.weight', f'down_bn{i}.bias']
    names += ['bottleneck.weight', 'bottleneck.bias']
    for i in range(4):
        names += [f'up_conv{i}.weight', f'up_conv{i}.bias', f'up_bn{i}.weight', f'up_bn{i}.bias']
    return names + ['final_conv.weight', 'final_conv.bias', 'output_fc.weight', 'output_fc.bias']


@dataclass
class KuleshovSaved:
    """What one forward keeps for its backward."""
    p: dict                 # name -> parameter tensor of this step
    versions: dict          # name -> its `_version` in the forward: the backward reads the parameters again
    x: torch.Tensor         # [N, Lf] input frame (the first L samples of a row are used)
    u: list                 # per down block leaky0.01(conv + b) [N, D_j, nf_j]
    cat: list               # the four concatenation buffers [N, Lc_i, C_i]: shuffled up output, then the skip
    zb: torch.Tensor        # the bottleneck convolution's output [N, B, 512]
    ab: torch.Tensor        # the bottleneck's output
    z: list                 # per up block conv + b [N, U_i, 2 nf]
    stat: list              # down 0..3, up 0..3: [4, C] float64 mean, rstd, s, t
    flat: torch.Tensor      # [N, Kp] final_conv's output, the Linear layer's input
    drop: tuple             # (seed, call, rank, p of the five sites) of this forward


class KuleshovTrainEngine(SavedStepEngine):
    """Forward with saved stage outputs and backward pass of Kuleshov(input_length, output_length) on explicit parameter /
    gradient dictionaries (the state_dict's names), mirroring `WaveUnetTrainEngine`."""
    label = 'Kuleshov'

    def __init__(self, dev, input_length, output_length, eps=1e-5):
        super().__init__(dev, 1)
        self.L, self.O = int(input_length), int(output_length)
        self.d = chain_lengths(self.L)
        self.eps = float(eps)
        self.momentum = [0.1] * 8
        self.running = None         # per BatchNorm (down 0..3, up 0..3) (running_mean, running_var) to blend into; None: zeros and ones
        self.new_running = None     # the same of the last forward
        self.seed, self.call, self.rank = 0, 0, 0
        self.p = [0.5] * 5          # Dropout p of the five sites
        self.names = param_names()

    def out_shape(self, n, L):
        return (n, 1, self.O)

    def _desc(self):
        return _lib.KuleshovDesc(self.L, self.O, self.eps, 0, 0)

    def _new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def _stats_ws(self):
        return self._scratch('_ks_stats_ws', _lib.call('stof_kuleshov_train_stats_workspace_bytes'))

    # ------------------------------------------------------------------------------------------------ weight images
    def pack_frag(self, w, kind):
        """weight [cout, cin, taps] -> its fragment image: the forward's (0), the stride-1 data gradient's (1), the even / odd tap
        class of the stride-2 data gradient's (2, 3)"""
        cout, cin, taps = (int(v) for v in w.shape)
        img = self._new(int(_lib.call('stof_kuleshov_train_frag_floats', cin, cout, taps, int(kind))))
        _lib.call('stof_kuleshov_train_pack_frag', w, cin, cout, taps, int(kind), img, self._st())
        return img

    def _image(self, name, w, kind):
        return self._cached((name, kind), w, lambda: self.pack_frag(w, kind))

    def pack_final(self, w):
        img = self._new(2 * 9 * 128)
        _lib.call('stof_kuleshov_train_pack_final', w, img, self._st())
        return img

    def pack_fc(self, w):
        desc = self._desc()
        img = self._new(int(_lib.call('stof_kuleshov_train_fc_frag_floats', desc)))
        _lib.call('stof_kuleshov_train_pack_fc', desc, w, img, self._st())
        return img

    # -------------------------------------------------------------------------------------------- one kernel stage each
    def down0(self, x, w, b):
        n = int(x.shape[0])
        u = self._new(n, self.d['down'][0], 128)
        _lib.call('stof_kuleshov_train_down0', x, int(x.shape[1]), n, self.L, w, b, u, self._st())
        return u

    def conv(self, src, src_n_stride, n, Lout, cin, cout, rows, stride, frag, bias, slope01, out=None, out_n_stride=None, out_t_stride=None):
        """-> [n, Lout, cout] (or into `out`): the convolution of `rows` x cin floats per output with the image `frag`"""
        if out is None:
            out, out_n_stride, out_t_stride = self._new(n, Lout, cout), Lout * cout, cout
        _lib.call('stof_kuleshov_train_conv', src, int(src_n_stride), n, Lout, cin, cout, rows, stride, frag, bias, int(slope01), out,
                  int(out_n_stride), int(out_t_stride), self._st())
        return out

    def stats(self, z, gamma, beta, run_mean, run_var, momentum):
        """z [.., ch] -> (stat [4, ch] float64, new running_mean, new running_var)"""
        ch = int(z.shape[-1])
        ws = self._stats_ws()
        stat = torch.empty((4, ch), dtype=torch.float64, device=self.dev)
        new_mean, new_var = self._new(ch), self._new(ch)
        _lib.call('stof_kuleshov_train_stats', z, z.numel() // ch, ch, gamma, beta, run_mean, run_var, self.eps, float(momentum), stat, new_mean,
                  new_var, ws, ws.numel(), self._st())
        return stat, new_mean, new_var

    def apply_down(self, u, stat, out, out_n_stride):
        n, D, ch = (int(v) for v in u.shape)
        _lib.call('stof_kuleshov_train_apply_down', u, n, D, ch, stat, out, int(out_n_stride), self._st())

    def apply_up(self, z, stat, drop, site, out, out_n_stride):
        n, U, ch = (int(v) for v in z.shape)
        seed, call, rank, p = drop
        _lib.call('stof_kuleshov_train_apply_up', z, n, U, ch, stat, seed, call, rank, site, p[site], out, int(out_n_stride), self._st())

    def apply_bott(self, z, drop):
        n, B, _ = (int(v) for v in z.shape)
        seed, call, rank, p = drop
        out = torch.empty_like(z)
        _lib.call('stof_kuleshov_train_apply_bott', z, n, B, seed, call, rank, p[0], out, self._st())
        return out

    def tail(self, cat3, final_image, final_bias, fc_frag, fc_bias):
        n = int(cat3.shape[0])
        kp = (self.d['fc_dim'] + 7) // 8 * 8
        flat, y = self._new(n, kp), self._new(n, self.O)
        _lib.call('stof_kuleshov_train_tail', self._desc(), cat3, n, final_image, final_bias, fc_frag, fc_bias, flat, y, self._st())
        return flat, y

    def fc_bwd(self, dy, flat, w, dw, db):
        dflat = torch.empty_like(flat)
        _lib.call('stof_kuleshov_train_fc_bwd', self._desc(), dy, flat, w, int(dy.shape[0]), dflat, dw, db, self._st())
        return dflat

    def final_bwd(self, dflat, cat3, w, dw, db):
        ws = self._scratch('_ks_final_ws', _lib.call('stof_kuleshov_train_final_bwd_workspace_bytes'))
        dcat = torch.empty_like(cat3)
        _lib.call('stof_kuleshov_train_final_bwd', self._desc(), dflat, cat3, w, int(cat3.shape[0]), dcat, dw, db, ws, ws.numel(), self._st())
        return dcat

    def gather_up(self, dcat, n, U, ch, drop, site):
        seed, call, rank, p = drop
        g = self._new(n, U, ch)
        _lib.call('stof_kuleshov_train_gather_up', dcat, int(dcat.stride(0)), n, U, ch, seed, call, rank, site, p[site], g, self._st())
        return g

    def gather_down(self, dskip, dnext, a):
        n, D, ch = (int(v) for v in a.shape)
        g = self._new(n, D, ch)
        _lib.call('stof_kuleshov_train_gather_down', dskip, int(dskip.stride(0)), dnext, a, int(a.stride(0)), n, D, ch, g, self._st())
        return g

    def gather_bott(self, g, z, drop):
        n, B, _ = (int(v) for v in z.shape)
        seed, call, rank, p = drop
        dz = torch.empty_like(z)
        _lib.call('stof_kuleshov_train_gather_bott', g, z, n, B, seed, call, rank, p[0], dz, self._st())
        return dz

    def bn_bwd(self, g, zu, stat, slope01, dgamma, dbeta):
        """-> dz; dgamma, dbeta are written in place"""
        ch = int(zu.shape[-1])
        ws = self._stats_ws()
        dz = torch.empty_like(zu)
        _lib.call('stof_kuleshov_train_bn_bwd', g, zu, stat, zu.numel() // ch, ch, int(slope01), dgamma, dbeta, dz, ws, ws.numel(), self._st())
        return dz

    def conv_wgrad(self, src, src_n_stride, dz, cin, taps, stride, dw, db):
        n, Lout, cout = (int(v) for v in dz.shape)
        ws = self._scratch('_ks_wgrad_ws', _lib.call('stof_kuleshov_train_wgrad_workspace_bytes', n, Lout, cin, cout, taps))
        _lib.call('stof_kuleshov_train_wgrad', src, int(src_n_stride), dz, n, Lout, cin, cout, taps, stride, dw, db, ws, ws.numel(), self._st())

    def conv_dgrad(self, dz, cin, taps, stride, frag0, frag1, Lin):
        """dz [n, Lout, cout] -> the gradient of the convolution's input [n, Lin, cin]"""
        n, Lout, cout = (int(v) for v in dz.shape)
        ws = self._scratch('_ks_dgrad_ws', _lib.call('stof_kuleshov_train_dgrad_workspace_bytes', n, Lout, cout, taps, stride))
        out = self._new(n, Lin, cin)
        _lib.call('stof_kuleshov_train_dgrad', dz, n, Lout, cin, cout, taps, stride, frag0, frag1, Lin, out, ws, ws.numel(), self._st())
        return out

    def down0_bwd(self, x, dz, w, dw, db, dx):
        ws = self._scratch('_ks_down0_ws', _lib.call('stof_kuleshov_train_down0_bwd_workspace_bytes'))
        _lib.call('stof_kuleshov_train_down0_bwd', x, int(x.shape[1]), dz, w, int(x.shape[0]), self.L, dw, db, dx,
                  0 if dx is None else int(dx.shape[1]), ws, ws.numel(), self._st())

    # ------------------------------------------------------------------------------------------------------- the step
    def _skip(self, cat, j):
        """where down block j's output lives: the rows behind the shuffled up output of concatenation 3 - j"""
        i = 3 - j
        return cat[i][:, 2 * self.d['up'][i]:, :]

    def _running(self, b, ch):
        if self.running is None:
            return torch.zeros(ch, device=self.dev), torch.ones(ch, device=self.dev)
        return self.running[b]

    def _forward_saved(self, p, frame):
        """models/kuleshov.py forward in train mode -> (y [N, O], KuleshovSaved); the new running statistics go to
        `self.new_running`."""
        x = self._flat_frame(frame)
        N, Lf = (int(v) for v in x.shape)
        d = self.d
        if Lf < self.L:
            raise RuntimeError(f'Kuleshov: the gfx950 kernels need rows of at least input_length = {self.L} samples (got {Lf})')
        if N * d['up'][0] < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size([N, 1024, d["up"][0]])}')
        p = {k: v.contiguous() for k, v in p.items()}
        drop = (int(self.seed) & (2 ** 64 - 1), int(self.call) & 0xffffffff, int(self.rank), tuple(float(v) for v in self.p))
        cat = [self._new(N, d['cat'][i], UP_COUT[i] // 2) for i in range(4)]
        us, stats, new_running = [], [None] * 8, [None] * 8
        for j in range(4):
            conv, bn, ch = f'down_conv{j}', f'down_bn{j}', N_FILTERS[j]
            w, bias = p[conv + '.weight'], p[conv + '.bias']
            if j == 0:
                u = self.down0(x, w, bias)
            else:
                src = self._skip(cat, j - 1)
                u = self.conv(src, src.stride(0), N, d['down'][j], N_FILTERS[j - 1], ch, N_FILTERSIZES[j], 2, self._image(conv, w, KIND_FWD), bias, 1)
            rm, rv = self._running(j, ch)
            stats[j], *new_running[j] = self.stats(u, p[bn + '.weight'], p[bn + '.bias'], rm, rv, self.momentum[j])
            dst = self._skip(cat, j)
            self.apply_down(u, stats[j], dst, dst.stride(0))
            us.append(u)
        src = self._skip(cat, 3)
        zb = self.conv(src, src.stride(0), N, d['bottleneck'], 512, 512, 9, 2, self._image('bottleneck', p['bottleneck.weight'], KIND_FWD),
                       p['bottleneck.bias'], 0)
        ab = self.apply_bott(zb, drop)
        zs = []
        for i in range(4):
            conv, bn, ch = f'up_conv{i}', f'up_bn{i}', UP_COUT[i]
            w = p[conv + '.weight']
            src = ab if i == 0 else cat[i - 1]
            z = self.conv(src, src.stride(0), N, d['up'][i], UP_CIN[i], ch, UP_TAPS[i], 1, self._image(conv, w, KIND_FWD), p[conv + '.bias'], 0)
            rm, rv = self._running(4 + i, ch)
            stats[4 + i], *new_running[4 + i] = self.stats(z, p[bn + '.weight'], p[bn + '.bias'], rm, rv, self.momentum[4 + i])
            self.apply_up(z, stats[4 + i], drop, i + 1, cat[i], cat[i].stride(0))
            zs.append(z)
        wf, wfc = p['final_conv.weight'], p['output_fc.weight']
        flat, y = self.tail(cat[3], self._cached('final', wf, lambda: self.pack_final(wf)), p['final_conv.bias'],
                            self._cached('fc', wfc, lambda: self.pack_fc(wfc)), p['output_fc.bias'])
        self.new_running = [tuple(v) for v in new_running]
        return y, KuleshovSaved(p=p, versions={k: v._version for k, v in p.items()}, x=x, u=us, cat=cat, zb=zb, ab=ab, z=zs, stat=stats,
                                flat=flat, drop=drop)

    def _backward_saved(self, saved, dy, g, dx=None):
        """From dy [N, O] = dloss/dy: every parameter gradient into the tensors of `g` (name -> tensor of the parameter's shape) and,
        if `dx` [N, Lf] is given, the gradient with respect to the input frame into it (zero behind the first L samples)."""
        p, d, cat = saved.p, self.d, saved.cat
        N = int(saved.x.shape[0])
        self._check_versions(saved)
        dflat = self.fc_bwd(dy, saved.flat, p['output_fc.weight'], g['output_fc.weight'], g['output_fc.bias'])
        dcat = self.final_bwd(dflat, cat[3], p['final_conv.weight'], g['final_conv.weight'], g['final_conv.bias'])
        dcats = [None] * 4
        for i in reversed(range(4)):
            conv, bn, ch, taps = f'up_conv{i}', f'up_bn{i}', UP_COUT[i], UP_TAPS[i]
            w, U = p[conv + '.weight'], d['up'][i]
            gz = self.gather_up(dcat, N, U, ch, saved.drop, i + 1)
            dz = self.bn_bwd(gz, saved.z[i], saved.stat[4 + i], 0, g[bn + '.weight'], g[bn + '.bias'])
            src = saved.ab if i == 0 else cat[i - 1]
            self.conv_wgrad(src, src.stride(0), dz, UP_CIN[i], taps, 1, g[conv + '.weight'], g[conv + '.bias'])
            dcats[i] = dcat
            dcat = self.conv_dgrad(dz, UP_CIN[i], taps, 1, self._image(conv, w, KIND_DGRAD), None, U + taps - 1)
        w = p['bottleneck.weight']
        dzb = self.gather_bott(dcat, saved.zb, saved.drop)
        src = self._skip(cat, 3)
        self.conv_wgrad(src, src.stride(0), dzb, 512, 9, 2, g['bottleneck.weight'], g['bottleneck.bias'])
        dnext = self.conv_dgrad(dzb, 512, 9, 2, self._image('bottleneck', w, KIND_EVEN), self._image('bottleneck', w, KIND_ODD), d['down'][3])
        for j in reversed(range(4)):
            conv, bn, taps = f'down_conv{j}', f'down_bn{j}', N_FILTERSIZES[j]
            w = p[conv + '.weight']
            gd = self.gather_down(self._skip(dcats, j), dnext, self._skip(cat, j))
            dz = self.bn_bwd(gd, saved.u[j], saved.stat[j], 1, g[bn + '.weight'], g[bn + '.bias'])
            if j == 0:
                if dx is not None and int(dx.shape[-1]) > self.L:
                    dx.zero_()
                self.down0_bwd(saved.x, dz, w, g[conv + '.weight'], g[conv + '.bias'], dx)
                break
            src = self._skip(cat, j - 1)
            self.conv_wgrad(src, src.stride(0), dz, N_FILTERS[j - 1], taps, 2, g[conv + '.weight'], g[conv + '.bias'])
            dnext = self.conv_dgrad(dz, N_FILTERS[j - 1], taps, 2, self._image(conv, w, KIND_EVEN), self._image(conv, w, KIND_ODD), d['down'][j - 1])


class KuleshovFunction(EndsFunction):
    """Autograd boundary of Kuleshov with `train_route = 'kernels'`: returns y [N, 1, output_length]."""

"""Training Wave-U-Net on the gfx950 kernels (reference main.py:199-289 with models/wave_unet.py in train mode): a forward that
keeps, per Conv + BatchNorm + LeakyReLU block, the raw convolution output z and the activation a, and the full backward pass in
exact fp32 on the channel-last layout of the inference kernels, behind an autograd boundary.

One kernel per stage (csrc/waveunet_train.hip).  Forward, per block: the inference convolution kernels with their training
epilogue (z = conv + bias on the raw weights, whose fragment images are packed on the device and cached per parameter version),
the batch statistics (double sums, fixed fold), a = leaky(z s + t) in double.  The decimation, the x2 interpolation and the skip
concatenation are built in LDS as in inference.  Backward, from the head down: the head's gradients, then per block the BatchNorm
reductions and dz, the weight gradient (fp32 MFMA, K over rows, on the forward's virtual input; encoder 0 on the vector pipe) and
the data gradient (the forward kernel on the flipped image), which is routed back by gather kernels: the transpose of the
interpolation to the previous block, and per skip ONE sum `decoder part at every position + next encoder's (or the middle's) part
at even positions`, in that order.  No MIOpen or rocBLAS call and no float atomic: two runs give bitwise equal gradients.

The LeakyReLU decision of the backward is `a > 0` on the saved activation.  BatchNorm's running statistics are module buffers:
a forward leaves the new ones in `engine.new_running` and `WaveUnet.forward_train_kernels` copies them into the buffers on the
host side (`copy_`), which bumps their `_version`, so the eval-mode blob is packed again.  The kernels never write them.

The training forward is NOT chunked by `max_workspace_bytes`: it keeps z and a of the whole batch."""
import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._train_boundary import EndsFunction, SavedStepEngine

SRC_DECIMATED, SRC_DECODER, SRC_PLAIN = 0, 1, 2


_CONSTANTS = None


def _constants():
    """The chunk constants of csrc/waveunet_train.hip, read from the library on first use."""
    global _CONSTANTS
    if _CONSTANTS is None:
        v = (ctypes.c_int64 * 10)()
        _lib.call('stof_waveunet_train_constants', v)
        k = [int(q) for q in v]
        _CONSTANTS = {
            # rows per partial, at the least, of the chunked reductions, and the number of partials at the most: beyond
            # CHUNKS[k] * MAX_PARTIALS[k] rows the rows per partial grow.  The convolutions' weight gradient counts whole
            # TILE-position tiles per waveform, so its rows are TILE * (number of tiles).
            'CHUNKS': {'stats': k[0], 'head_wgrad': k[2], 'in_wgrad': k[4], 'conv_wgrad': k[6]},
            'MAX_PARTIALS': {'stats': k[1], 'head_wgrad': k[3], 'in_wgrad': k[5], 'conv_wgrad': k[7]},
            'TILE': k[8],
            'INTERP_MAX_M': k[9],           # the largest low length the interpolation transpose serves
        }
    return _CONSTANTS


def __getattr__(name):
    """CHUNKS, MAX_PARTIALS, TILE, INTERP_MAX_M: module attributes that come from the built library."""
    if name in ('CHUNKS', 'MAX_PARTIALS', 'TILE', 'INTERP_MAX_M'):
        return _constants()[name]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def blocks_of(n_layers):
    """The Conv + BN + LeakyReLU blocks in module order: (conv prefix, BN prefix, cout, cin, taps, cu); cu > 0: a decoder whose
    first cu input channels are the interpolated map."""
    n, c = int(n_layers), 16
    out = [(f'encoder.{i}.main.0', f'encoder.{i}.main.1', c * (i + 1), 1 if i == 0 else c * i, 15, 0) for i in range(n)]
    out.append(('middle.0', 'middle.1', c * n, c * n, 15, 0))
    for i in range(n):
        cu, cs = (c * n if i == 0 else c * (n - i + 1)), c * (n - i)
        out.append((f'decoder.{i}.main.0', f'decoder.{i}.main.1', cs, cu + cs, 5, cu))
    return out


def param_names(n_layers):
    names = []
    for conv, bn, *_ in blocks_of(n_layers):
        names += [conv + '.weight', conv + '.bias', bn + '.weight', bn + '.bias']
    return names + ['out.0.weight', 'out.0.bias']


def interp_table(M):
    """Host only: (i0, i1, l0, l1 [2 M], lo, hi [M]) as numpy arrays: the fp32 coordinates of every high position as the kernels
    compute them, and the window (inclusive) of high positions the transpose visits for every low position."""
    import numpy as np
    M = int(M)
    i0, i1 = np.empty(2 * M, np.int32), np.empty(2 * M, np.int32)
    l0, l1 = np.empty(2 * M, np.float32), np.empty(2 * M, np.float32)
    lo, hi = np.empty(M, np.int32), np.empty(M, np.int32)
    _lib.call('stof_waveunet_interp_table', M, *[ctypes.c_void_p(a.ctypes.data) for a in (i0, i1, l0, l1, lo, hi)])
    return i0, i1, l0, l1, lo, hi


@dataclass
class WaveUnetSaved:
    """What one forward keeps for its backward."""
    p: dict                 # name -> parameter tensor of this step
    versions: dict          # name -> its `_version` in the forward: the backward reads the parameters again
    x: torch.Tensor         # [N, L] input frame
    y: torch.Tensor         # [N, L] output
    z: list                 # per block the raw conv output [N, L_level, cout]
    a: list                 # per block leaky(BN(z)); the LeakyReLU decision is a > 0
    stat: list              # per block [4, cout] float64: mean, rstd, s, t


class WaveUnetTrainEngine(SavedStepEngine):
    """Forward with saved activations and backward pass of WaveUnet(n_layers, 16) on explicit parameter / gradient dictionaries
    (the state_dict's names), mirroring `SincNetTrainEngine`."""
    label = 'WaveUnet'

    def __init__(self, dev, n_layers, eps=None, momentum=None):
        super().__init__(dev, 1)
        self.n = int(n_layers)
        self.blocks = blocks_of(self.n)
        self.names = param_names(self.n)
        nb = len(self.blocks)
        self.eps = [1e-5] * nb if eps is None else [float(e) for e in eps]
        self.momentum = [0.1] * nb if momentum is None else [float(m) for m in momentum]
        self.running = None         # per block (running_mean, running_var) to blend into; None: zeros and ones
        self.new_running = None     # per block (new running_mean, new running_var) of the last forward

    def _new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def _stats_ws(self):
        return self._scratch('_wu_stats_ws', _lib.call('stof_waveunet_train_stats_workspace_bytes'))

    # ------------------------------------------------------------------------------------------------ weight images
    def pack_frag(self, w, flip):
        """weight [cout, cin, taps] -> its fragment image (flip: the data gradient's)"""
        cout, cin, taps = (int(v) for v in w.shape)
        img = self._new(int(_lib.call('stof_waveunet_train_frag_floats', cin, cout, taps, int(flip))))
        _lib.call('stof_waveunet_train_pack_frag', w, cin, cout, taps, int(flip), img, self._st())
        return img

    def pack_in(self, w, b):
        img = self._new(256)
        _lib.call('stof_waveunet_train_pack_in', w, b, img, self._st())
        return img

    def _in_image(self, w, b):
        version = (w.data_ptr(), w._version, b.data_ptr(), b._version)
        hit = self._images.get('in')
        if hit is None or hit[0] != version:
            hit = self._images['in'] = (version, self.pack_in(w, b))
        return hit[1]

    # -------------------------------------------------------------------------------------------- one kernel stage each
    def in_conv(self, x, image):
        n, L = x.shape
        z = self._new(n, L, 16)
        _lib.call('stof_waveunet_train_in_conv', x, n, L, image, z, self._st())
        return z

    def conv(self, src, low, n, Lout, cin, cu, cout, taps, mode, frag, bias):
        """-> [n, Lout, cout]: the convolution of the virtual input (`mode`) with the image `frag` (+ bias)"""
        out = self._new(n, Lout, cout)
        _lib.call('stof_waveunet_train_conv', src, low, n, Lout, cin, cu, cout, taps, mode, frag, bias, out, self._st())
        return out

    def stats(self, z, gamma, beta, run_mean, run_var, eps, momentum):
        """z [.., ch] -> (stat [4, ch] float64, new running_mean, new running_var)"""
        ch = int(z.shape[-1])
        rows, ws = z.numel() // ch, self._stats_ws()
        stat = torch.empty((4, ch), dtype=torch.float64, device=self.dev)
        new_mean, new_var = self._new(ch), self._new(ch)
        _lib.call('stof_waveunet_train_stats', z, rows, ch, gamma, beta, run_mean, run_var, float(eps), float(momentum), stat, new_mean, new_var, ws,
                  ws.numel(), self._st())
        return stat, new_mean, new_var

    def apply(self, z, stat):
        ch = int(z.shape[-1])
        a = torch.empty_like(z)
        _lib.call('stof_waveunet_train_apply', z, z.numel() // ch, ch, stat, a, self._st())
        return a

    def head(self, o, x, w, b):
        n, L = x.shape
        y = self._new(n, L)
        _lib.call('stof_waveunet_train_head', o, x, n, L, w, b, y, self._st())
        return y

    def head_bwd(self, dy, y, o, x, w, dw, db, want_dx):
        """-> (do [N, L, 16], the head's term of dx [N, L] or None); dw [17], db [1] are written in place"""
        n, L = x.shape
        ws = self._scratch('_wu_head_ws', _lib.call('stof_waveunet_train_head_bwd_workspace_bytes'))
        dout = self._new(n, L, 16)
        dxh = self._new(n, L) if want_dx else None
        _lib.call('stof_waveunet_train_head_bwd', dy, y, o, x, n, L, w, dout, dxh, dw, db, ws, ws.numel(), self._st())
        return dout, dxh

    def bn_bwd(self, da, a, z, stat, dgamma, dbeta):
        """-> dz; dgamma, dbeta are written in place"""
        ch = int(z.shape[-1])
        ws = self._stats_ws()
        dz = torch.empty_like(z)
        _lib.call('stof_waveunet_train_bn_bwd', da, a, z, stat, z.numel() // ch, ch, dgamma, dbeta, dz, ws, ws.numel(), self._st())
        return dz

    def conv_wgrad(self, src, low, dz, n, Lout, cin, cu, cout, taps, mode, dw, db):
        ws = self._scratch('_wu_wgrad_ws', _lib.call('stof_waveunet_train_wgrad_workspace_bytes', n, Lout, cin, cout, taps))
        _lib.call('stof_waveunet_train_wgrad', src, low, dz, n, Lout, cin, cu, cout, taps, mode, dw, db, ws, ws.numel(), self._st())

    def in_wgrad(self, x, dz, dw, db):
        n, L = x.shape
        ws = self._scratch('_wu_in_ws', _lib.call('stof_waveunet_train_in_wgrad_workspace_bytes'))
        _lib.call('stof_waveunet_train_in_wgrad', x, dz, n, L, dw, db, ws, ws.numel(), self._st())

    def conv_dgrad(self, dz, n, Lout, cin, cout, taps, image):
        """dz [n, Lout, cout] -> the gradient of the virtual input [n, Lout, cin]: the forward kernel on the flipped image"""
        return self.conv(dz, None, n, Lout, cout, 0, cin, taps, SRC_PLAIN, image, None)

    def interp_t(self, g, n, M, cu):
        """g [n, 2 M, cg] -> [n, M, cu]: the transpose of the x2 interpolation on the first cu channels"""
        dlow = self._new(n, M, cu)
        _lib.call('stof_waveunet_train_interp_t', g, n, M, int(g.shape[-1]), cu, dlow, self._st())
        return dlow

    def skip_sum(self, gdec, genc, n, L, cu, cs):
        """-> [n, L, cs] = gdec[..., cu:] at every position, then + genc [n, L / 2, cs] at even positions"""
        out = self._new(n, L, cs)
        _lib.call('stof_waveunet_train_skip_sum', gdec, genc, n, L, cu, cs, out, self._st())
        return out

    def in_dgrad(self, dz, w, dxh, dx):
        n, L = dx.shape
        _lib.call('stof_waveunet_train_in_dgrad', dz, w, dxh, n, L, dx, self._st())

    # ------------------------------------------------------------------------------------------------------- the step
    def out_shape(self, n, L):
        return (n, 1, L)

    def _forward_saved(self, p, frame):
        """models/wave_unet.py forward in train mode -> (y [N, L], WaveUnetSaved); the new running statistics go to
        `self.new_running`."""
        x = self._flat_frame(frame)
        N, L = (int(v) for v in x.shape)
        n = self.n
        if L % (1 << n):
            raise RuntimeError(f'WaveUnet: the gfx950 kernels need a length that is a multiple of 2^n_layers (got {L})')
        if N * (L >> n) < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size([N, 16 * n, L >> n])}')
        p = {k: v.contiguous() for k, v in p.items()}
        zs, acts, stats, new_running = [], [], [], []
        for b, (conv, bn, cout, cin, taps, cu) in enumerate(self.blocks):
            w, bias = p[conv + '.weight'], p[conv + '.bias']
            if b == 0:
                z = self.in_conv(x, self._in_image(w, bias))
            else:
                frag = self._cached(('fwd', b), w, lambda: self.pack_frag(w, 0))
                if b <= n:                                  # encoder b, or the middle: every second position of skip b - 1
                    z = self.conv(acts[b - 1], None, N, L >> b, cin, 0, cout, taps, SRC_DECIMATED, frag, bias)
                else:                                       # decoder i on (interpolated previous output, skip n - 1 - i)
                    j = n - 1 - (b - n - 1)
                    z = self.conv(acts[j], acts[b - 1], N, L >> j, cin, cu, cout, taps, SRC_DECODER, frag, bias)
            if self.running is None:
                rm, rv = torch.zeros(cout, device=self.dev), torch.ones(cout, device=self.dev)
            else:
                rm, rv = self.running[b]
            stat, nm, nv = self.stats(z, p[bn + '.weight'], p[bn + '.bias'], rm, rv, self.eps[b], self.momentum[b])
            zs.append(z)
            acts.append(self.apply(z, stat))
            stats.append(stat)
            new_running.append((nm, nv))
        y = self.head(acts[-1], x, p['out.0.weight'], p['out.0.bias'])
        self.new_running = new_running
        return y, WaveUnetSaved(p=p, versions={k: v._version for k, v in p.items()}, x=x, y=y, z=zs, a=acts, stat=stats)

    def _block_bn_bwd(self, saved, b, da, g):
        bn = self.blocks[b][1]
        return self.bn_bwd(da, saved.a[b], saved.z[b], saved.stat[b], g[bn + '.weight'], g[bn + '.bias'])

    def _backward_saved(self, saved, dy, g, dx=None):
        """From dy [N, L] = dloss/dy: every parameter gradient into the tensors of `g` (name -> tensor of the parameter's shape)
        and, if `dx` [N, L] is given, the gradient with respect to the input frame into it."""
        p, n = saved.p, self.n
        N, L = (int(v) for v in saved.x.shape)
        self._check_versions(saved)
        da, dxh = self.head_bwd(dy, saved.y, saved.a[-1], saved.x, p['out.0.weight'], g['out.0.weight'], g['out.0.bias'],
                                dx is not None)
        gdec = {}
        for i in reversed(range(n)):                        # decoder i
            b, j = n + 1 + i, n - 1 - i
            conv, _, cout, cin, taps, cu = self.blocks[b]
            w, Lout = p[conv + '.weight'], L >> j
            dz = self._block_bn_bwd(saved, b, da, g)
            self.conv_wgrad(saved.a[j], saved.a[b - 1], dz, N, Lout, cin, cu, cout, taps, SRC_DECODER, g[conv + '.weight'],
                            g[conv + '.bias'])
            gfull = self.conv_dgrad(dz, N, Lout, cin, cout, taps, self._cached(('dgrad', b), w, lambda: self.pack_frag(w, 1)))
            da = self.interp_t(gfull, N, Lout // 2, cu)
            gdec[j] = (gfull, cu, cin - cu)
        genc = None
        for b in reversed(range(n + 1)):                    # the middle, then encoder n - 1 .. 0
            conv, _, cout, cin, taps, _ = self.blocks[b]
            w, Lb = p[conv + '.weight'], L >> b
            if b < n:
                gfull, cu, cs = gdec.pop(b)
                da = self.skip_sum(gfull, genc, N, Lb, cu, cs)
            dz = self._block_bn_bwd(saved, b, da, g)
            if b == 0:
                self.in_wgrad(saved.x, dz, g[conv + '.weight'], g[conv + '.bias'])
                if dx is not None:
                    self.in_dgrad(dz, w, dxh, dx)
                break
            self.conv_wgrad(saved.a[b - 1], None, dz, N, Lb, cin, 0, cout, taps, SRC_DECIMATED, g[conv + '.weight'], g[conv + '.bias'])
            genc = self.conv_dgrad(dz, N, Lb, cin, cout, taps, self._cached(('dgrad', b), w, lambda: self.pack_frag(w, 1)))


class WaveUnetFunction(EndsFunction):
    """Autograd boundary of WaveUnet with `train_route = 'kernels'`: returns y [N, 1, L]."""

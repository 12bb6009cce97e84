"""Training SincNet on the gfx950 kernels (reference main.py:199-289 with models/sincnet.py in train mode): a forward that keeps,
per layer, the raw convolution output z_l and the activation a_l, and the full backward pass in exact fp32 on the GAP layout of
the inference kernels, behind an autograd boundary.

One kernel per stage (csrc/sincnet_train.hip).  Forward, per layer: the inference convolution kernels with their training
epilogue (z_l = conv + bias), the batch statistics (double sums, fixed fold), a_l = leaky(z_l s + t).  Backward, per layer from
the last: the BatchNorm reductions and dz_l, the weight gradient (fp32 MFMA, K over rows; layer 3 on the vector pipe), the data
gradient (the forward kernel on the flipped image; layer 3 on the vector pipe), and for the sinc layer the gradient of the
128 x 1023 filter bank chained to `low_hz_` / `band_hz_` in double.  No MIOpen or rocBLAS call and no float atomic: two runs give
bitwise equal gradients.

BatchNorm's running statistics are module buffers, not parameters: a forward leaves the new ones in `engine.new_running` and
`SincNet.forward_train_kernels` copies them into the buffers on the host side (`copy_`), which bumps their `_version`, so the
eval-mode blob is packed again (on the device, `sincnet.device_pack_weights`, while a training route is set).  The kernels never
write the module's buffers.

The training forward is NOT chunked by `max_workspace_bytes`: it keeps z_l and a_l of the whole batch."""
import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._train_boundary import EndsFunction, SavedStepEngine

C = 128
TAPS = (1023, 11, 9, 7)
GAP = 8
MOMENTUM = 0.05
# rows per partial, at the least, of the chunked reductions (csrc/sincnet_train.hip: SW_CHUNK, OW_CHUNK, ST_CHUNK); the bank
# gradient's chunks are whole 128-sample tiles of one waveform
CHUNKS = {'conv_wgrad': 64, 'out_wgrad': 256, 'stats': 256, 'bank_grad': 128}

NAMES = (['conv.0.low_hz_', 'conv.0.band_hz_'] + [f'conv.{i}.{k}' for i in (1, 2, 3) for k in ('weight', 'bias')] +
         [f'bn.{i}.{k}' for i in range(4) for k in ('weight', 'bias')])
_PACKED = ('conv.0.low_hz_', 'conv.0.band_hz_', 'conv.1.weight', 'conv.2.weight', 'conv.3.weight')


@dataclass
class SincNetSaved:
    """What one forward keeps for its backward."""
    p: dict                 # name -> parameter tensor of this step
    versions: dict          # name -> its `_version` in the forward: the backward reads the parameters again
    x: torch.Tensor         # [N, L] input frame
    z: list                 # per layer the raw conv output: GAP layout (layers 0..2), flat [N L] (layer 3)
    a: list                 # layers 0..2: leaky(BN(z)), GAP layout; the LeakyReLU decision is a > 0
    stat: list              # per layer [4, channels] float64: mean, rstd, s, t


class SincNetTrainEngine(SavedStepEngine):
    """Forward with saved activations and backward pass of SincNet on explicit parameter / gradient dictionaries (the
    state_dict's names), mirroring `ZonziniTrainEngine`."""
    label = 'SincNet'

    def __init__(self, dev, fs, eps=1e-5, momentum=MOMENTUM):
        super().__init__(dev, 1)
        self.fs, self.eps, self.momentum = float(fs), float(eps), float(momentum)
        self.names = list(NAMES)
        self.running = None         # per layer (running_mean, running_var) to blend into; None: zeros and ones
        self.new_running = None     # per layer (new running_mean, new running_var) of the last forward
        lay = (ctypes.c_int64 * 6)()
        _lib.call('stof_sincnet_train_blob_layout', lay)
        self.blob_layout = dict(zip(('frag0', 'bank_t', 'frag1', 'frag2', 'w3', 'total'), (int(v) for v in lay)))

    def _desc(self):
        return _lib.SincNetDesc(self.fs, self.eps, 0, 0)

    def buffer(self, n, L):
        """an uninitialised 128-channel tensor in the GAP layout"""
        return torch.empty(int(_lib.call('stof_sincnet_train_buffer_floats', n, L)), dtype=torch.float32, device=self.dev)

    def rows(self, buf, n, L):
        """the [N, L, 128] view of a GAP-layout buffer"""
        return buf[GAP * C:GAP * C + n * (L + GAP) * C].view(n, L + GAP, C)[:, :L]

    def from_rows(self, t):
        """[N, L, 128] -> a GAP-layout buffer with zero gap rows"""
        n, L = int(t.shape[0]), int(t.shape[1])
        buf = torch.zeros_like(self.buffer(n, L))
        self.rows(buf, n, L).copy_(t)
        return buf

    def packed(self, p):
        """The forward kernels' blob of this step's parameters."""
        return self._packed_blob(p, _PACKED, 4 * self.blob_layout['total'], 'stof_sincnet_train_pack', self._desc())

    def _dgrad_image(self, layer, w):
        img = torch.empty(C * TAPS[layer] * C, dtype=torch.float32, device=self.dev)
        _lib.call('stof_sincnet_train_dgrad_image', layer, w, img, self._st())
        return img

    def _stats_ws(self):
        return self._scratch('_sn_stats_ws', _lib.call('stof_sincnet_train_stats_workspace_bytes'))

    # -------------------------------------------------------------------------------------------- one kernel stage each
    def conv(self, layer, src, n, L, blob, bias):
        out = self.buffer(n, L) if layer < 3 else torch.empty(n * L, dtype=torch.float32, device=self.dev)
        _lib.call('stof_sincnet_train_conv', layer, src, n, L, blob, bias, out, self._st())
        return out

    def stats(self, z, n, L, ch, gamma, beta, run_mean, run_var):
        """-> (stat [4, ch] float64, new running_mean, new running_var)"""
        desc, ws = self._desc(), self._stats_ws()
        stat = torch.empty((4, ch), dtype=torch.float64, device=self.dev)
        new_mean = torch.empty(ch, dtype=torch.float32, device=self.dev)
        new_var = torch.empty(ch, dtype=torch.float32, device=self.dev)
        _lib.call('stof_sincnet_train_stats', desc, z, n, L, ch, gamma, beta, run_mean, run_var, self.momentum, stat, new_mean, new_var, ws,
                  ws.numel(), self._st())
        return stat, new_mean, new_var

    def apply(self, z, n, L, ch, stat):
        out = self.buffer(n, L) if ch == C else torch.empty(n * L, dtype=torch.float32, device=self.dev)
        _lib.call('stof_sincnet_train_apply', z, n, L, ch, stat, out, self._st())
        return out

    def bn_bwd(self, da, a, z, stat, gamma, n, L, ch, dgamma, dbeta):
        """-> dz (GAP layout / flat); dgamma, dbeta are written in place"""
        ws = self._stats_ws()
        dz = self.buffer(n, L) if ch == C else torch.empty(n * L, dtype=torch.float32, device=self.dev)
        _lib.call('stof_sincnet_train_bn_bwd', da, a, z, stat, gamma, n, L, ch, dgamma, dbeta, dz, ws, ws.numel(), self._st())
        return dz

    def conv_wgrad(self, layer, a_prev, dz, n, L, dw, db):
        ws = self._scratch('_sn_wgrad_ws', _lib.call('stof_sincnet_train_conv_wgrad_workspace_bytes', 1))
        _lib.call('stof_sincnet_train_conv_wgrad', layer, a_prev, dz, n, L, dw, db, ws, ws.numel(), self._st())

    def conv_dgrad(self, layer, dz, n, L, image):
        da = self.buffer(n, L)
        _lib.call('stof_sincnet_train_conv_dgrad', layer, dz, n, L, image, da, self._st())
        return da

    def out_wgrad(self, a2, dz3, n, L, dw, db):
        ws = self._scratch('_sn_out_ws', _lib.call('stof_sincnet_train_out_wgrad_workspace_bytes'))
        _lib.call('stof_sincnet_train_out_wgrad', a2, dz3, n, L, dw, db, ws, ws.numel(), self._st())

    def out_dgrad(self, dz3, w3, n, L):
        da = self.buffer(n, L)
        _lib.call('stof_sincnet_train_out_dgrad', dz3, w3, n, L, da, self._st())
        return da

    def bank_grad(self, x, dz0, n, L):
        """-> G [128, 1023] = d loss / d filter bank"""
        ws = self._scratch('_sn_bank_ws', _lib.call('stof_sincnet_train_bank_grad_workspace_bytes'))
        G = torch.empty((C, TAPS[0]), dtype=torch.float32, device=self.dev)
        _lib.call('stof_sincnet_train_bank_grad', x, dz0, n, L, G, ws, ws.numel(), self._st())
        return G

    def band_grad(self, low, band, G, dlow, dband):
        desc = self._desc()
        _lib.call('stof_sincnet_train_band_grad', desc, low, band, G, dlow, dband, self._st())

    def in_dgrad(self, dz0, blob, n, L, dx):
        _lib.call('stof_sincnet_train_in_dgrad', dz0, blob, n, L, dx, self._st())

    # ------------------------------------------------------------------------------------------------------- the step
    def out_shape(self, n, L):
        return (n, 1, L)

    def _forward_saved(self, p, frame):
        """models/sincnet.py forward in train mode -> (y [N, L], SincNetSaved); the new running statistics go to
        `self.new_running`."""
        x = self._flat_frame(frame)
        n, L = x.shape
        if n * L < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size([n, C, L])}')
        p = {k: v.contiguous() for k, v in p.items()}
        blob = self.packed(p)
        zs, acts, stats, new_running = [], [], [], []
        src = x
        for l in range(4):
            ch = C if l < 3 else 1
            z = self.conv(l, src, n, L, blob, p[f'conv.{l}.bias'] if l else None)
            if self.running is None:
                rm, rv = torch.zeros(ch, device=self.dev), torch.ones(ch, device=self.dev)
            else:
                rm, rv = self.running[l]
            stat, nm, nv = self.stats(z, n, L, ch, p[f'bn.{l}.weight'], p[f'bn.{l}.bias'], rm, rv)
            src = self.apply(z, n, L, ch, stat)
            zs.append(z)
            stats.append(stat)
            new_running.append((nm, nv))
            if l < 3:
                acts.append(src)
        self.new_running = new_running
        return src.view(n, L), SincNetSaved(p=p, versions={k: v._version for k, v in p.items()}, x=x, z=zs, a=acts, stat=stats)

    def _backward_saved(self, saved, dy, g, dx=None):
        """From dy [N, L] = dloss/dy: every parameter gradient into the tensors of `g` (name -> tensor of the parameter's shape)
        and, if `dx` [N, L] is given, the gradient with respect to the input frame into it."""
        p = saved.p
        n, L = saved.x.shape
        self._check_versions(saved)
        dz = self.bn_bwd(dy, None, saved.z[3], saved.stat[3], p['bn.3.weight'], n, L, 1, g['bn.3.weight'], g['bn.3.bias'])
        self.out_wgrad(saved.a[2], dz, n, L, g['conv.3.weight'], g['conv.3.bias'])
        da = self.out_dgrad(dz, p['conv.3.weight'], n, L)
        for l in (2, 1, 0):
            dz = self.bn_bwd(da, saved.a[l], saved.z[l], saved.stat[l], p[f'bn.{l}.weight'], n, L, C, g[f'bn.{l}.weight'],
                             g[f'bn.{l}.bias'])
            if l == 0:
                break
            w = p[f'conv.{l}.weight']
            self.conv_wgrad(l, saved.a[l - 1], dz, n, L, g[f'conv.{l}.weight'], g[f'conv.{l}.bias'])
            da = self.conv_dgrad(l, dz, n, L, self._cached(('dgrad', l), w, lambda: self._dgrad_image(l, w)))
        G = self.bank_grad(saved.x, dz, n, L)
        self.band_grad(p['conv.0.low_hz_'], p['conv.0.band_hz_'], G, g['conv.0.low_hz_'], g['conv.0.band_hz_'])
        if dx is not None:
            self.in_dgrad(dz, self.packed(p), n, L, dx)


class SincNetFunction(EndsFunction):
    """Autograd boundary of SincNet with `train_route = 'kernels'`: returns y [N, 1, L]."""

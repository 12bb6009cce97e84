"""Training ZonziniNetSmall / ZonziniNetLarge on the gfx950 kernels (reference main.py:199-289 with models/zonzini.py): a
forward that saves every pooled activation with its ReLU / max-pool decisions and the full backward pass in exact fp32 on the
channel-last buffers of the inference kernels, behind an autograd boundary.

One kernel per stage (csrc/zonzini_train.hip).  Forward: the inference kernels with their training outputs switched on, so y
is bitwise the inference y.  Backward: the head (fc2, fc1 and the gradient of the global mean), then per conv layer from the
last to the second the weight gradient and the data gradient on the fp32 MFMA, then layer 1's weight gradient and, if the
frame asks, its data gradient on the vector pipe.  The pre-pool gradient dz is never stored: every reader forms it from the
pooled gradient and the layer's selector bytes.  No MIOpen call and no float atomic: two runs give bitwise equal gradients.

The training forward is NOT chunked by `max_workspace_bytes`: it must keep every activation of the whole batch."""
import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._train_boundary import EndsFunction, SavedStepEngine

CHANNELS = {_lib.ZONZINI_SMALL: (16, 32, 64, 64), _lib.ZONZINI_LARGE: (50, 100, 150, 200, 250)}


def pooled_len(L):
    """length after Conv1d(k = 10, stride 2) and MaxPool1d(2)"""
    return ((L - 10) // 2 + 1) // 2 if L >= 10 else 0


def param_names(layers):
    """state_dict order of a Zonzini net with `layers` conv layers (also the order of the packer)"""
    names = []
    for i in range(layers):
        names += [f'conv_layers.{i}.weight', f'conv_layers.{i}.bias']
    return names + ['fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias']


@dataclass
class ZonziniSaved:
    """What one forward keeps for its backward."""
    p: dict                 # name -> parameter tensor of this step
    versions: dict          # name -> its `_version` in the forward: the backward reads the parameters again
    x: torch.Tensor         # [N, L] input frame
    acts: list              # per conv layer [N, Lp_l, cpad_l] pooled activation, pad channels 0
    sel: list               # per conv layer [N, Lp_l, cpad_l] uint8: 0 no gradient, 1 conv output 2p won, 2 conv output 2p + 1
    f: torch.Tensor         # [N, C] global mean of the last activation
    h: torch.Tensor         # [N, 1024] relu(fc1)
    y: torch.Tensor         # [N] the output


class ZonziniTrainEngine(SavedStepEngine):
    """Forward with saved activations and backward pass of a Zonzini net on explicit parameter / gradient dictionaries (the
    state_dict's names), mirroring `EspcnTrainEngine`."""

    def __init__(self, dev, variant):
        super().__init__(dev, 1)
        self.variant = int(variant)
        self.channels = CHANNELS[self.variant]
        self.cpad = tuple((c + 3) & ~3 for c in self.channels)
        self.names = param_names(len(self.channels))
        self.label = 'ZonziniNetSmall' if self.variant == _lib.ZONZINI_SMALL else 'ZonziniNetLarge'

    def out_shape(self, n, L):
        return (n, 1)

    def _desc(self):
        return _lib.ZonziniDesc(self.variant, 0)

    def _packed(self, p):
        """The forward kernels' blob of this step's parameters."""
        desc = self._desc()
        return self._packed_blob(p, self.names, int(_lib.call('stof_zonzini_packed_bytes', desc)), 'stof_zonzini_train_pack', desc)

    def _dgrad_image(self, layer, w):
        desc = self._desc()
        img = torch.empty(_lib.call('stof_zonzini_train_dgrad_image_floats', desc, layer), dtype=torch.float32, device=self.dev)
        _lib.call('stof_zonzini_train_dgrad_image', desc, layer, w, img, self._st())
        return img

    def _forward_saved(self, p, frame):
        """models/zonzini.py forward -> (y [N, 1], ZonziniSaved)."""
        st, desc = self._st(), self._desc()
        x = self._flat_frame(frame)
        n, L = x.shape
        p = {k: v.contiguous() for k, v in p.items()}
        blob = self._packed(p)
        acts, sel, lp = [], [], L
        for cp in self.cpad:
            lp = pooled_len(lp)
            acts.append(torch.empty((n, lp, cp), dtype=torch.float32, device=self.dev))
            sel.append(torch.empty((n, lp, cp), dtype=torch.uint8, device=self.dev))
        f = torch.empty((n, self.channels[-1]), dtype=torch.float32, device=self.dev)
        h = torch.empty((n, 1024), dtype=torch.float32, device=self.dev)
        y = torch.empty((n,), dtype=torch.float32, device=self.dev)
        a_ptrs = (ctypes.c_void_p * len(acts))(*[t.data_ptr() for t in acts])
        s_ptrs = (ctypes.c_void_p * len(sel))(*[t.data_ptr() for t in sel])
        _lib.call('stof_zonzini_train_forward', desc, x, n, L, blob, a_ptrs, s_ptrs, f, h, y, st)
        return y.view(n, 1), ZonziniSaved(p=p, versions={k: v._version for k, v in p.items()}, x=x, acts=acts, sel=sel, f=f, h=h, y=y)

    def _backward_saved(self, saved, dy, g, dx=None):
        """From dy [N, 1] = dloss/dy: every parameter gradient into the tensors of `g` (name -> tensor of the parameter's shape)
        and, if `dx` [N, L] is given, the gradient with respect to the input frame into it."""
        st, p, desc = self._st(), saved.p, self._desc()
        n, L = saved.x.shape
        self._check_versions(saved)
        layers = len(self.channels)
        dout = torch.empty((n, self.cpad[-1]), dtype=torch.float32, device=self.dev)       # df: the mean's gradient, times Lp
        _lib.call('stof_zonzini_train_head_bwd', desc, dy, saved.f, saved.h, p['fc1.weight'], p['fc2.weight'], g['fc1.weight'], g['fc1.bias'],
                  g['fc2.weight'], g['fc2.bias'], dout, n, st)
        for l in range(layers - 1, 0, -1):
            w = p[f'conv_layers.{l}.weight']
            ws = self._scratch('_zz_wgrad_ws', _lib.call('stof_zonzini_train_conv_wgrad_workspace_bytes', desc, l))
            _lib.call('stof_zonzini_train_conv_wgrad', desc, l, saved.acts[l - 1], dout, saved.sel[l], g[f'conv_layers.{l}.weight'],
                      g[f'conv_layers.{l}.bias'], n, L, ws, ws.numel(), st)
            img = self._cached(('dgrad', l), w, lambda: self._dgrad_image(l, w))
            din = torch.empty_like(saved.acts[l - 1])           # dloss/d(act l-1): its ReLU / pool is applied by the readers
            _lib.call('stof_zonzini_train_conv_dgrad', desc, l, dout, saved.sel[l], img, din, n, L, st)
            dout = din
        ws = self._scratch('_zz_in_ws', _lib.call('stof_zonzini_train_in_wgrad_workspace_bytes', desc))
        _lib.call('stof_zonzini_train_in_wgrad', desc, saved.x, dout, saved.sel[0], g['conv_layers.0.weight'], g['conv_layers.0.bias'], n, L, ws,
                  ws.numel(), st)
        if dx is not None:
            _lib.call('stof_zonzini_train_in_dgrad', desc, dout, saved.sel[0], p['conv_layers.0.weight'], dx, n, L, st)


class ZonziniFunction(EndsFunction):
    """Autograd boundary of a Zonzini net with `train_route = 'kernels'`: returns y [N, 1]."""

"""Training ESPCN_1D(r), r = 1..64, on the gfx950 kernels (reference main.py:199-289 with models/espcn_1d.py:31-36): a staged
forward that saves its activations and the full backward pass in exact fp32 on channel-last buffers, behind an autograd
boundary.

One kernel per stage (csrc/espcn_train.hip): conv1 + tanh -> h1 [N][L][64], conv2 + tanh on the fp32 MFMA -> h2 [N][L][32],
conv3 + sigmoid -> y [N][L r]; backwards the conv3 weight and data gradient (which applies tanh' of h2), conv2's two gradient
GEMMs on `stof_train_wgrad` / `stof_train_conv` (csrc/train.hip, through `LayerKernels`) and the conv1 weight and data
gradient (which apply tanh' of h1).  In channel-last order z [N][L][r] is its own SampleShuffle1D(r) image, so the shuffle
costs nothing in either direction.  No MIOpen call and no float atomic: two runs give bitwise equal gradients."""
from dataclasses import dataclass

import torch

from . import _lib
from ._train_boundary import EndsFunction, SavedStepEngine


@dataclass
class EspcnSaved:
    """What one forward keeps for its backward."""
    p: dict                 # name -> parameter tensor of this step
    versions: dict          # name -> its `_version` in the forward: the backward reads the parameters again
    x: torch.Tensor         # [N, L] input frame
    h1: torch.Tensor        # [N, L, 64] tanh(conv1)
    h2: torch.Tensor        # [N, L, 32] tanh(conv2)
    y: torch.Tensor         # [N, L r] the output: sigmoid' = y (1 - y)


class EspcnTrainEngine(SavedStepEngine):
    """Forward with saved activations and backward pass of ESPCN_1D on explicit parameter / gradient dictionaries (the
    state_dict's names), mirroring `EdsrTrainEngine`."""
    label = 'ESPCN_1D'

    def _repack_mid(self, w):
        """conv2.weight as the MFMA operand of `stof_train_espcn_mid`"""
        img = torch.empty(_lib.call('stof_train_espcn_repack_floats'), dtype=torch.float32, device=self.dev)
        _lib.call('stof_train_espcn_repack', w, img, self._st())
        return img

    def _forward_saved(self, p, frame):
        """models/espcn_1d.py:31-36 -> (y [N, L r], EspcnSaved)."""
        st, r = self._st(), self.r
        x = self._flat_frame(frame)
        n, L = x.shape
        p = {k: v.contiguous() for k, v in p.items()}
        h1 = torch.empty((n, L, 64), dtype=torch.float32, device=self.dev)
        _lib.call('stof_train_espcn_in', x, p['conv1.weight'], p['conv1.bias'], h1, n, L, st)
        h2 = torch.empty((n, L, 32), dtype=torch.float32, device=self.dev)
        w2 = p['conv2.weight']
        mid = self._cached('mid', w2, lambda: self._repack_mid(w2))
        _lib.call('stof_train_espcn_mid', h1, mid, p['conv2.bias'], h2, n, L, st)
        y = torch.empty((n, L * r), dtype=torch.float32, device=self.dev)
        _lib.call('stof_train_espcn_out', h2, p['conv3.weight'], p['conv3.bias'], y, n, L, r, st)
        return y, EspcnSaved(p=p, versions={k: v._version for k, v in p.items()}, x=x, h1=h1, h2=h2, y=y)

    def _backward_saved(self, saved, dy, g, dx=None):
        """From dy [N, L r] = dloss/dy: every parameter gradient into the tensors of `g` (name -> tensor of the parameter's
        shape) and, if `dx` [N, L] is given, the gradient with respect to the input frame into it."""
        st, p, r = self._st(), saved.p, self.r
        n, L = saved.x.shape
        self._check_versions(saved)
        ws = self._scratch('_espcn_out_ws', _lib.call('stof_train_espcn_out_wgrad_workspace_bytes', r))
        _lib.call('stof_train_espcn_out_wgrad', saved.h2, saved.y, dy, g['conv3.weight'], g['conv3.bias'], n, L, r, 1.0, ws, ws.numel(), st)
        g2 = torch.empty((n, L, 32), dtype=torch.float32, device=self.dev)            # dloss/d(conv2's output), tanh' included
        _lib.call('stof_train_espcn_out_dgrad', saved.y, dy, saved.h2, p['conv3.weight'], g2, n, L, r, st)
        self._wgrad(saved.h1, g2, g['conv2.weight'], g['conv2.bias'], 64, 32, 3)
        w2 = p['conv2.weight']
        flip = self._cached('flip', w2, lambda: self._repack(w2, True))               # the data-gradient operand of `stof_train_conv`
        g1 = self._conv(g2, flip, None, 32, 64, 3)                                    # dloss/dh1: tanh' of h1 is applied by its readers
        ws = self._scratch('_espcn_in_ws', _lib.call('stof_train_espcn_in_wgrad_workspace_bytes'))
        _lib.call('stof_train_espcn_in_wgrad', saved.x, g1, saved.h1, g['conv1.weight'], g['conv1.bias'], n, L, 1.0, ws, ws.numel(), st)
        if dx is not None:
            _lib.call('stof_train_espcn_in_dgrad', g1, saved.h1, p['conv1.weight'], dx, n, L, 1.0, st)


class EspcnFunction(EndsFunction):
    """Autograd boundary of `ESPCN_1D.forward_train_kernels`."""

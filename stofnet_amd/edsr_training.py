"""Training EDSR_1D(1, 64, B, r | 64) on the gfx950 kernels (reference main.py:199-289 with models/edsr_1d.py:22-45): forward with
saved activations and the full backward pass in exact fp32 on channel-last [N][L][64] buffers, behind an autograd boundary.

The 2 B + 1 body convolutions are `stof_train_conv` / `stof_train_wgrad` (csrc/train.hip, through `LayerKernels`); the two
ends -- conv_input + ReLU and the shuffled conv_output, each with its weight and data gradient -- are the vector-pipe
kernels of csrc/edsr_train.hip.  In channel-last order the trunk [N][L][64] read as [N][L r][64 / r] is its
SampleShuffle1D(r) image, so the shuffle costs nothing in either direction.  No MIOpen call and no float atomic: two runs
give bitwise equal gradients."""
from dataclasses import dataclass

import torch

from . import _lib
from ._train_boundary import EndsFunction, SavedStepEngine
from .training import ACT_NONE, ACT_RELU


@dataclass
class EdsrSaved:
    """What one forward keeps for its backward."""
    p: dict                 # name -> parameter tensor of this step
    versions: dict          # name -> its `_version` in the forward: the backward reads the parameters again
    x: torch.Tensor         # [N, L] input frame
    a0: torch.Tensor        # [N, L, 64] relu(conv_input)
    hs: list                # hs[i] = relu(conv1) of block i
    us: list                # us[i] = input of block i (us[0] = a0), us[B] = conv_mid's input
    trunk: torch.Tensor     # [N, L, 64] conv_mid + a0 = the input of `upscale`


class EdsrTrainEngine(SavedStepEngine):
    """Forward with saved activations and backward pass of EDSR_1D on explicit parameter / gradient dictionaries (the
    state_dict's names), mirroring `TrainEngine`."""
    label = 'EDSR_1D'

    def __init__(self, dev, num_blocks, r):
        super().__init__(dev, r)
        self.B = int(num_blocks)

    def body_layers(self):
        return [f'residual_blocks.{i}.conv{j}' for i in range(self.B) for j in (1, 2)] + ['conv_mid']

    def _image(self, p, name, flip):
        """Tap-major image of a 64 -> 64 weight (flip: the data-gradient operand), repacked when the parameter changed."""
        w = p[name + '.weight']
        return self._cached((name, flip), w, lambda: self._repack(w.contiguous(), flip))

    def _forward_saved(self, p, frame):
        """models/edsr_1d.py:38-45 -> (y [N, L r], EdsrSaved)."""
        st = self._st()
        x = self._flat_frame(frame)
        n, L = x.shape
        p = {k: v.contiguous() for k, v in p.items()}
        fwd = {nm: self._image(p, nm, False) for nm in self.body_layers()}
        a0 = torch.empty((n, L, 64), dtype=torch.float32, device=self.dev)
        _lib.call('stof_train_edsr_in', x, p['conv_input.weight'], p['conv_input.bias'], a0, n, L, st)
        u, hs, us = a0, [], [a0]
        for i in range(self.B):
            c1, c2 = f'residual_blocks.{i}.conv1', f'residual_blocks.{i}.conv2'
            h = self._conv(u, fwd[c1], p[c1 + '.bias'], 64, 64, 3, ACT_RELU)
            u = self._conv(h, fwd[c2], p[c2 + '.bias'], 64, 64, 3, ACT_NONE, residual=u)
            hs.append(h)
            us.append(u)
        trunk = self._conv(u, fwd['conv_mid'], p['conv_mid.bias'], 64, 64, 3, ACT_NONE, residual=a0)
        y = torch.empty((n, L * self.r), dtype=torch.float32, device=self.dev)
        _lib.call('stof_train_edsr_out', trunk, p['conv_output.weight'], p['conv_output.bias'], y, n, L, self.r, st)
        return y, EdsrSaved(p=p, versions={k: v._version for k, v in p.items()}, x=x, a0=a0, hs=hs, us=us, trunk=trunk)

    def _backward_saved(self, saved, dy, g, dx=None):
        """From dy [N, L r] = dloss/dy: every parameter gradient into the tensors of `g` (name -> tensor of the parameter's
        shape) and, if `dx` [N, L] is given, the gradient with respect to the input frame into it."""
        st, p, r = self._st(), saved.p, self.r
        n, L = saved.x.shape
        self._check_versions(saved)
        bwd = {nm: self._image(p, nm, True) for nm in self.body_layers()}
        ws = self._scratch('_edsr_out_ws', _lib.call('stof_train_edsr_out_wgrad_workspace_bytes', r))
        _lib.call('stof_train_edsr_out_wgrad', saved.trunk, dy, g['conv_output.weight'], g['conv_output.bias'], n, L, r, 1.0, ws, ws.numel(), st)
        gt = torch.empty((n, L, 64), dtype=torch.float32, device=self.dev)            # dloss/dtrunk: also the long skip's gradient
        _lib.call('stof_train_edsr_out_dgrad', dy, p['conv_output.weight'], gt, n, L, r, st)
        self._wgrad(saved.us[self.B], gt, g['conv_mid.weight'], g['conv_mid.bias'], 64, 64, 3)
        gu = self._conv(gt, bwd['conv_mid'], None, 64, 64, 3)
        for i in range(self.B - 1, -1, -1):                  # gu = dloss/d(output of block i), the identity path included
            c1, c2 = f'residual_blocks.{i}.conv1', f'residual_blocks.{i}.conv2'
            self._wgrad(saved.hs[i], gu, g[c2 + '.weight'], g[c2 + '.bias'], 64, 64, 3)
            gh = self._conv(gu, bwd[c2], None, 64, 64, 3, ACT_RELU, saved=saved.hs[i])
            self._wgrad(saved.us[i], gh, g[c1 + '.weight'], g[c1 + '.bias'], 64, 64, 3)
            gu = self._conv(gh, bwd[c1], None, 64, 64, 3, residual=gu)
        ws = self._scratch('_edsr_in_ws', _lib.call('stof_train_edsr_in_wgrad_workspace_bytes'))
        _lib.call('stof_train_edsr_in_wgrad', saved.x, gu, gt, saved.a0, g['conv_input.weight'], g['conv_input.bias'], n, L, 1.0, ws, ws.numel(), st)
        if dx is not None:
            _lib.call('stof_train_edsr_in_dgrad', gu, gt, saved.a0, p['conv_input.weight'], dx, n, L, 1.0, st)


class EdsrFunction(EndsFunction):
    """Autograd boundary of `EDSR_1D.forward_train_kernels`."""

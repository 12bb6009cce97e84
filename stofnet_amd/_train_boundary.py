"""What the opt-in training routes of the comparison networks (edsr_training.py, espcn_training.py) share on the host side of
their kernels, and `carve_grads`, which StofNet's own boundary (`training.StofNetFunction`) uses too:

  carve_grads      one fresh flat gradient buffer per backward, carved into the parameters' shapes
  SavedStepEngine  the base of an engine with `_forward_saved(p, frame) -> (y [N, out columns], saved)` and
                   `_backward_saved(saved, dy, g, dx)`: the frame flattening, the check that no parameter changed between
                   the two, and the cache of kernel-layout weight images
  EndsFunction     the autograd boundary over such an engine"""
import numpy as np
import torch

from . import _lib
from .training import LayerKernels


def carve_grads(names, shapes, dev):
    """-> (flat zero buffer, name -> its view of a parameter's shape)."""
    sizes = [int(np.prod(sh)) if len(sh) else 1 for sh in shapes]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)    # fresh: torch may keep these views as .grad
    g, off = {}, 0
    for name, sh, k in zip(names, shapes, sizes):
        g[name] = flat[off:off + k].view(sh)
        off += k
    return flat, g


class SavedStepEngine(LayerKernels):
    """Exact fp32 `LayerKernels` of one model (`label`: its name in messages, `r`: its upscale factor) on one device."""
    label = None

    def __init__(self, dev, r):
        super().__init__(dev, _lib.PREC_FP32)
        self.r = int(r)
        self._images = {}           # key -> ((data_ptr, _version) of the weight, its kernel-layout image)

    def out_shape(self, n, L):
        """shape of `model(frame)` for a frame [n, 1, L]: the upsampled row of the SampleShuffle1D nets"""
        return (n, 1, L * self.r)

    def _flat_frame(self, frame):
        """frame [N, 1, L] -> x [N, L] float32, detached"""
        _lib.require_device(frame, 'frame')
        return frame.detach().reshape(frame.shape[0], frame.shape[-1]).contiguous().float()

    def _check_versions(self, saved):
        """The backward reads the parameters again (the data gradients; the flipped images are packed only when a backward
        runs): an in-place edit since the forward would be used silently, where torch's own convolutions raise."""
        for k, v in saved.p.items():
            if v._version != saved.versions[k]:
                raise RuntimeError(f'{self.label}: parameter {k} needed for gradient computation has been modified by an inplace '
                                   f'operation (version {v._version}, expected {saved.versions[k]})')

    def _cached(self, key, w, make):
        """The image `make()` of weight `w` under `key`, made again when the parameter changed."""
        version = (w.data_ptr(), w._version)
        hit = self._images.get(key)
        if hit is None or hit[0] != version:
            hit = self._images[key] = (version, make())
        return hit[1]


class EndsFunction(torch.autograd.Function):
    """Autograd boundary of `forward_train_kernels`, on the pattern of `StofNetFunction`: `y = model(frame)` returns a tensor
    whose `backward()` runs the gfx950 data- and weight-gradient kernels and hands torch the gradient of every parameter (and
    of the frame, when it asks for one), so torch's loss, `optim.AdamW` and scheduler run unchanged.  The models subclass it
    for the name that shows in `grad_fn`."""

    @staticmethod
    def forward(ctx, frame, engine, names, *params):
        n, L = int(frame.shape[0]), int(frame.shape[-1])
        ctx.engine, ctx.names, ctx.shapes, ctx.dims = engine, names, [tuple(v.shape) for v in params], (n, L)
        if n == 0 or L == 0:
            ctx.saved = ()
            return torch.empty(engine.out_shape(n, L), dtype=torch.float32, device=engine.dev)
        with torch.cuda.device(engine.dev):
            y, ctx.saved = engine._forward_saved({k: v.detach() for k, v in zip(names, params)}, frame)
        return y.view(engine.out_shape(n, L))

    @staticmethod
    def backward(ctx, grad_out):
        engine, saved, (n, L) = ctx.engine, ctx.saved, ctx.dims
        if saved is None:
            raise RuntimeError('Trying to backward through the graph a second time: the saved activations of '
                               f'{engine.label}.forward have been freed')
        with torch.cuda.device(engine.dev):
            _, g = carve_grads(ctx.names, ctx.shapes, engine.dev)
            dx = torch.empty((n, L), dtype=torch.float32, device=engine.dev) if ctx.needs_input_grad[0] else None
            if n and L:
                engine._backward_saved(saved, grad_out.detach().reshape(n, -1).contiguous().float(), g, dx)
        ctx.saved = None
        return (None if dx is None else dx.view(n, 1, L), None, None) + tuple(g[name] for name in ctx.names)

"""What the opt-in training routes of the comparison networks (edsr_training.py, espcn_training.py) share on the host side of
their kernels, and `carve_grads`, which StofNet's own boundary (`training.StofNetFunction`) uses too:

  carve_grads      one fresh flat gradient buffer per backward, carved into the parameters' shapes
  SavedStepEngine  the base of an engine with `_forward_saved(p, frame) -> (y [N, out columns], saved)` and
                   `_backward_saved(saved, dy, g, dx)`: the frame flattening, the check that no parameter changed between
                   the two, and the cache of kernel-layout weight images
                   and of the packed blob of all parameters
  EndsFunction     the autograd boundary over such an engine
  fp32_device_params, train_engine, commit_running_stats   what the models' `forward_train_kernels` do around the boundary"""
import ctypes

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


def fp32_device_params(module, label):
    """(names, parameters) of `module`, every parameter checked to be float32 on a ROCm device"""
    names, params = zip(*module.named_parameters())
    for p in params:
        if p.dtype != torch.float32:
            raise TypeError(f'{label}: parameters must be float32 (got {p.dtype}); the gfx950 kernels are fp32 only')
        _lib.require_device(p, 'parameter')
    return names, params


def train_engine(module, key, make):
    """The training engine of `module` under `key` (the device and whatever else an engine is built for), made on first use."""
    engines = module.__dict__.setdefault('_train_engines', {})
    if key not in engines:
        engines[key] = make()
    return engines[key]


def commit_running_stats(bns, new_running):
    """The new running statistics of a train-mode forward into the BatchNorm modules' buffers, on the host side: `copy_` bumps
    the buffers' versions, which are the eval-mode blob's key."""
    with torch.no_grad():
        for bn, (mean, var) in zip(bns, new_running):
            bn.running_mean.copy_(mean)
            bn.running_var.copy_(var)
            bn.num_batches_tracked.add_(1)


class SavedStepEngine(LayerKernels):
    """Exact fp32 `LayerKernels` of one model (`label`: its name in messages, `r`: its upscale factor) on one device."""
    label = None

    def __init__(self, dev, r):
        super().__init__(dev, _lib.PREC_FP32)
        self.r = int(r)
        self._images = {}           # key -> ((data_ptr, _version) of the weight, its kernel-layout image)
        self._blob = None           # ((data_ptr, _version) of every packed parameter, the blob of the forward kernels)

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

    def _packed_blob(self, p, names, nbytes, entry, desc):
        """The forward kernels' blob of this step's parameters `names`, packed on the device by `entry` (into the same buffer)
        again when one of them changed."""
        version = tuple((p[k].data_ptr(), p[k]._version) for k in names)
        if self._blob is None or self._blob[0] != version:
            blob = self._blob[1] if self._blob is not None else torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            ptrs = (ctypes.c_void_p * len(names))(*[p[k].data_ptr() for k in names])
            _lib.call(entry, desc, ptrs, blob, nbytes, self._st())
            self._blob = (version, blob)
        return self._blob[1]


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

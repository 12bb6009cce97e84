"""What the comparison networks (baselines.py, waveunet.py, kuleshov.py, zonzini.py, sincnet.py) share on the host side of
their gfx950 kernels, as two mix-in layers in front of nn.Module:

  _PackedKernels   the packed-weight cache and the chunk loop under `max_workspace_bytes`: all a model needs to run its
                   kernels (the Zonzini nets and SincNet, which have no other route, stop here);
  _KernelRoute     adds the route decision and the error contract of the models that also have `forward_aten`."""
import ctypes

import numpy as np
import torch

from . import _lib


def _pack(packed_bytes, pack_weights, desc, arrs, what, unsupported=None):
    """Host-side packing through one pair of C entry points: float32 arrays in the packer's order -> uint8 CPU blob."""
    n = int(packed_bytes(ctypes.byref(desc)))
    if n == 0:
        raise ValueError(unsupported or f'{what}: unsupported configuration')
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in arrs]
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    blob = torch.zeros(n, dtype=torch.uint8)
    _lib.check(pack_weights(ctypes.byref(desc), ptrs, ctypes.c_void_p(blob.data_ptr()), n), what)
    return blob


class _PackedKernels:
    _packed = None
    _packed_key = None
    _PACKED_ARRAYS = 'parameters'

    def _kernel_params(self):
        """The tensors the packer reads, in its order."""
        return list(self.parameters())

    def _state_arrays(self):
        """`_kernel_params` of a model with BatchNorm: the parameters and running statistics in state-dict order."""
        return [v for k, v in self.state_dict(keep_vars=True).items() if not k.endswith('num_batches_tracked')]

    def _pack_key(self):
        """What the blob depends on besides the arrays (part of the cache key)."""
        return ()

    def _pack(self, host):
        raise NotImplementedError

    def invalidate_packed(self):
        """Drop the packed weights (they are rebuilt on the next forward; parameter edits are also detected on their own)."""
        self._packed = None
        self._packed_key = None

    def packed_weights(self, device):
        params = self._kernel_params()
        for p in params:
            if p.dtype != torch.float32:
                raise TypeError(f'{type(self).__name__}: {self._PACKED_ARRAYS} must be float32 (got {p.dtype}); the '
                                'gfx950 kernels are fp32 only')
        key = (str(device), *self._pack_key()) + tuple((p.data_ptr(), p._version) for p in params)
        if self._packed is None or self._packed_key != key:
            host = [np.ascontiguousarray(p.detach().cpu().numpy(), dtype=np.float32) for p in params]
            self._packed = self._pack(host).to(device)
            self._packed_key = key
        return self._packed

    def _chunked(self, device, N, workspace_bytes, launch, chunked=True):
        """Call `launch(r0, rows, ws, ws_bytes, stream)` for the N rows of a batch in chunks whose workspace
        (`workspace_bytes(rows)` bytes, allocated once) stays under `max_workspace_bytes`, or for all rows at once with
        chunked=False, with `device` current and on its current stream -> (workspace, its size in bytes)."""
        chunk = max(1, min(N, int(self.max_workspace_bytes) // workspace_bytes(1))) if chunked else N
        ws_bytes = workspace_bytes(chunk)
        with torch.cuda.device(device):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            stream = _lib.stream_ptr(device)
            for r0 in range(0, N, chunk):
                launch(r0, min(chunk, N - r0), ws, ws_bytes, stream)
        return ws, ws_bytes


class _KernelRoute(_PackedKernels):
    _EVAL_ONLY = False      # True: in train mode `forward` stays on forward_aten (BatchNorm batch statistics, live Dropout)

    def _config_supported(self):
        return True

    def kernels_supported(self, x):
        """True when `forward_kernels(x)` can run: x float32 [N, 1, L] on the ROCm device, every parameter float32 on
        that device, and a configuration the kernels are built for."""
        if not (isinstance(x, torch.Tensor) and x.device.type == 'cuda' and x.dtype == torch.float32 and x.dim() == 3
                and x.shape[1] == 1 and self._config_supported()):
            return False
        return all(p.dtype == torch.float32 and p.device == x.device for p in self._kernel_params())

    def _takes_kernels(self, x):
        if (self._EVAL_ONLY and self.training) or not self.kernels_supported(x):
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._kernel_params())))

    def _check_kernels(self, x):
        name = type(self).__name__
        _lib.require_device(x, 'x')
        if x.dtype != torch.float32:
            raise TypeError(f'{name}: x must be float32 (got {x.dtype}); the gfx950 kernels are fp32 only')
        for p in self._kernel_params():
            if p.dtype != torch.float32:
                raise TypeError(f'{name}: parameters must be float32 (got {p.dtype}); the gfx950 kernels are fp32 only')
            _lib.require_device(p, 'parameter')
        if not self.kernels_supported(x):
            raise RuntimeError(f'{name}: the gfx950 kernels need x of shape [N, 1, L] on the parameters\' device and '
                               f'{self._KERNEL_CONFIG} (got x {list(x.shape)}); use forward_aten')

    def forward(self, x):
        return self.forward_kernels(x) if self._takes_kernels(x) else self.forward_aten(x)

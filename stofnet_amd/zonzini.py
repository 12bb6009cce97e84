"""The Zonzini baselines of the reference (models/zonzini.py: ZonziniNetSmall, ZonziniNetLarge) on the gfx950 kernels
of csrc/zonzini.hip, inference only.

Constructor (no arguments), module and parameter names (`conv_layers.{i}.*`, `fc1.*`, `fc2.*`), shapes and default
initialisation are the reference's, so its checkpoints load with strict=True.  The layers are parameter holders: the
forward never calls their ATen kernels.  It packs the parameters once per change (their `_version` counters and
storage), splits the batch into chunks whose workspace stays under `max_workspace_bytes`, and launches the HIP
forward on the current stream.  Rows are independent and bitwise independent of the batch they sit in, so the
chunking does not show in the result."""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib


class _ZonziniNet(nn.Module):
    VARIANT = None
    CHANNELS = ()
    MIN_LEN = 0
    max_workspace_bytes = 512 << 20

    def __init__(self):
        super().__init__()
        self.conv_layers = nn.ModuleList()
        cin = 1
        for c in self.CHANNELS:
            self.conv_layers.append(nn.Conv1d(cin, c, kernel_size=10, stride=2))
            cin = c
        # parameter-free modules of the reference, kept so that the module tree matches (the forward does not call them)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool1d(kernel_size=2)
        self.global_avgpool = nn.AdaptiveAvgPool1d(1)
        self.fc1 = nn.Linear(cin, 1024)
        self.fc2 = nn.Linear(1024, 1)
        self._packed = None
        self._packed_key = None

    def _desc(self):
        return _lib.ZonziniDesc(self.VARIANT, 0)

    def _params(self):
        ps = []
        for conv in self.conv_layers:
            ps += [conv.weight, conv.bias]
        return ps + [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]

    def invalidate_packed(self):
        """Drop the packed weights (they are rebuilt on the next forward; parameter edits are also detected on their own)."""
        self._packed = None
        self._packed_key = None

    def packed_weights(self, device):
        params = self._params()
        for p in params:
            if p.dtype != torch.float32:
                raise TypeError(f'{type(self).__name__}: parameters must be float32 (got {p.dtype}); the gfx950 kernels '
                                'are fp32 only')
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
        if self._packed is None or self._packed_key != key:
            host = [np.ascontiguousarray(p.detach().cpu().numpy(), dtype=np.float32) for p in params]
            self._packed = pack_weights(self.VARIANT, host).to(device)
            self._packed_key = key
        return self._packed

    def _check_input(self, x):
        _lib.require_device(x, 'x')
        if x.dtype != torch.float32:
            raise TypeError(f'{type(self).__name__}: x must be float32 (got {x.dtype}); the gfx950 kernels are fp32 only')
        if x.dim() != 3 or x.shape[1] != 1:
            raise RuntimeError(f'{type(self).__name__}: expected x of shape [N, 1, L], got {list(x.shape)}')
        if torch.is_grad_enabled() and (self.training or x.requires_grad):
            raise NotImplementedError(f'{type(self).__name__}: Zonzini training is not implemented on the gfx950 path '
                                      '(inference only: call model.eval() or run under torch.no_grad())')
        L = int(x.shape[-1])
        if L < self.MIN_LEN:
            raise RuntimeError(f'{type(self).__name__}: rows of {L} samples are too short (the reference raises '
                               f'"max_pool1d() Invalid computed output size: 0" below L = {self.MIN_LEN})')

    def forward_with_features(self, x):
        """(y [N, 1], the global average pool's output [N, C_last]), both float32."""
        return self._run(x, True)

    def forward(self, x):
        return self._run(x, False)[0]

    def _run(self, x, want_features):
        self._check_input(x)
        N, L = int(x.shape[0]), int(x.shape[-1])
        c_last = self.CHANNELS[-1]
        y = torch.empty((N, 1), dtype=torch.float32, device=x.device)
        feats = torch.empty((N, c_last), dtype=torch.float32, device=x.device) if want_features else None
        if N == 0:
            return y, feats
        x = x.detach().contiguous()
        packed = self.packed_weights(x.device)
        lib = _lib.lib()
        desc = self._desc()
        per_row = int(lib.stof_zonzini_workspace_bytes(ctypes.byref(desc), 1, L))
        chunk = max(1, min(N, int(self.max_workspace_bytes) // per_row))
        ws_bytes = int(lib.stof_zonzini_workspace_bytes(ctypes.byref(desc), chunk, L))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        stream = _lib.stream_ptr(x.device)
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            _lib.check(lib.stof_zonzini_forward(
                ctypes.byref(desc), ctypes.c_void_p(x[r0].data_ptr()), n, L, _lib.ptr(packed),
                ctypes.c_void_p(y[r0].data_ptr()), None if feats is None else ctypes.c_void_p(feats[r0].data_ptr()),
                _lib.ptr(ws), ws_bytes, stream), 'stof_zonzini_forward')
        return y, feats


class ZonziniNetSmall(_ZonziniNet):
    """models/zonzini.py ZonziniNetSmall: Conv1d 1 -> 16 -> 32 -> 64 -> 64 (k 10, stride 2), each + ReLU + MaxPool1d(2),
    global average pool, fc1 64 -> 1024 + ReLU, fc2 1024 -> 1.  Rows of at least 936 samples."""
    VARIANT = _lib.ZONZINI_SMALL
    CHANNELS = (16, 32, 64, 64)
    MIN_LEN = 936


class ZonziniNetLarge(_ZonziniNet):
    """models/zonzini.py ZonziniNetLarge: Conv1d 1 -> 50 -> 100 -> 150 -> 200 -> 250 (k 10, stride 2), each + ReLU +
    MaxPool1d(2), global average pool, fc1 250 -> 1024 + ReLU, fc2 1024 -> 1.  Rows of at least 3752 samples."""
    VARIANT = _lib.ZONZINI_LARGE
    CHANNELS = (50, 100, 150, 200, 250)
    MIN_LEN = 3752


def pack_weights(variant, params):
    """Host-side packing (stof_zonzini_pack_weights) of the state_dict's float32 arrays in module order -> a uint8 CPU
    tensor holding the blob."""
    lib = _lib.lib()
    desc = _lib.ZonziniDesc(int(variant), 0)
    n = int(lib.stof_zonzini_packed_bytes(ctypes.byref(desc)))
    if n == 0:
        raise ValueError(f'unknown Zonzini variant {variant}')
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in params]
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    blob = torch.zeros(n, dtype=torch.uint8)
    _lib.check(lib.stof_zonzini_pack_weights(ctypes.byref(desc), ptrs, ctypes.c_void_p(blob.data_ptr()), n),
               'stof_zonzini_pack_weights')
    return blob

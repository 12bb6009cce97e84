"""The Zonzini baselines of the reference (models/zonzini.py: ZonziniNetSmall, ZonziniNetLarge) on the gfx950 kernels
of csrc/zonzini.hip (inference) and, opt-in through `train_route`, csrc/zonzini_train.hip (training, zonzini_training.py).

Constructor (no arguments), module and parameter names (`conv_layers.{i}.*`, `fc1.*`, `fc2.*`), shapes and default
initialisation are the reference's, so its checkpoints load with strict=True.  The layers are parameter holders: the
inference forward never calls their ATen kernels (only `train_route = 'aten'` does).  It packs the parameters once per change (their `_version` counters and
storage), splits the batch into chunks whose workspace stays under `max_workspace_bytes`, and launches the HIP
forward on the current stream.  Rows are independent and bitwise independent of the batch they sit in, so the
chunking does not show in the result."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._kernel_route import _PackedKernels, _pack


class _ZonziniNet(_PackedKernels, nn.Module):
    VARIANT = None
    CHANNELS = ()
    MIN_LEN = 0
    max_workspace_bytes = 512 << 20
    # None | 'kernels' | 'aten': what `forward` does where an autograd graph would be recorded (grad enabled and the module
    # in train mode or x asking for a gradient).  None raises NotImplementedError; 'kernels' goes through the autograd
    # boundary of zonzini_training.py (gfx950 kernels, exact fp32); 'aten' runs the module's own Conv1d / MaxPool1d / Linear
    # layers as the reference's forward does.  Every other call stays on the inference kernels.
    train_route = None

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

    def _desc(self):
        return _lib.ZonziniDesc(self.VARIANT, 0)

    def _kernel_params(self):
        ps = []
        for conv in self.conv_layers:
            ps += [conv.weight, conv.bias]
        return ps + [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]

    def _pack(self, host):
        return pack_weights(self.VARIANT, host)

    def _check_input(self, x):
        _lib.require_device(x, 'x')
        if x.dtype != torch.float32:
            raise TypeError(f'{type(self).__name__}: x must be float32 (got {x.dtype}); the gfx950 kernels are fp32 only')
        if x.dim() != 3 or x.shape[1] != 1:
            raise RuntimeError(f'{type(self).__name__}: expected x of shape [N, 1, L], got {list(x.shape)}')
        if self._records_graph(x):
            raise NotImplementedError(f'{type(self).__name__}: Zonzini training is not implemented on the gfx950 path '
                                      '(inference only: call model.eval() or run under torch.no_grad())')
        L = int(x.shape[-1])
        if L < self.MIN_LEN:
            raise RuntimeError(f'{type(self).__name__}: rows of {L} samples are too short (the reference raises '
                               f'"max_pool1d() Invalid computed output size: 0" below L = {self.MIN_LEN})')

    def forward_with_features(self, x):
        """(y [N, 1], the global average pool's output [N, C_last]), both float32."""
        return self._run(x, True)

    def _records_graph(self, x):
        """Where the inference kernels cannot serve: an autograd graph would be recorded."""
        return torch.is_grad_enabled() and (self.training or x.requires_grad)

    def forward_aten(self, x):
        """The reference's forward on the module's own ATen layers (models/zonzini.py:25-37)."""
        for conv in self.conv_layers:
            x = self.maxpool(self.relu(conv(x)))
        x = self.global_avgpool(x)
        x = x.view(x.size(0), -1)
        return self.fc2(self.relu(self.fc1(x)))

    def forward_train_kernels(self, x):
        """y [N, 1] float32 on the gfx950 training kernels (zonzini_training.py), with an autograd graph: its backward fills
        the gradient of every parameter (and of x, if it asks for one) in exact fp32.  Not chunked by `max_workspace_bytes`:
        the backward needs every activation of the whole batch."""
        from ._train_boundary import fp32_device_params, train_engine
        from .zonzini_training import ZonziniFunction, ZonziniTrainEngine
        with torch.no_grad():                                # the checks of an inference call, minus the graph condition
            self._check_input(x)
        names, params = fp32_device_params(self, type(self).__name__)
        engine = train_engine(self, str(x.device), lambda: ZonziniTrainEngine(x.device, self.VARIANT))
        return ZonziniFunction.apply(x, engine, names, *params)

    def forward(self, x):
        if self.train_route not in (None, 'kernels', 'aten'):
            raise ValueError(f"{type(self).__name__}.train_route must be None, 'kernels' or 'aten' (got {self.train_route!r})")
        if self.train_route is not None and self._records_graph(x):
            return self.forward_train_kernels(x) if self.train_route == 'kernels' else self.forward_aten(x)
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

        def launch(r0, n, ws, ws_bytes, stream):
            _lib.check(lib.stof_zonzini_forward(
                ctypes.byref(desc), ctypes.c_void_p(x[r0].data_ptr()), n, L, _lib.ptr(packed),
                ctypes.c_void_p(y[r0].data_ptr()), None if feats is None else ctypes.c_void_p(feats[r0].data_ptr()),
                _lib.ptr(ws), ws_bytes, stream), 'stof_zonzini_forward')

        self._chunked(x.device, N, lambda n: int(lib.stof_zonzini_workspace_bytes(ctypes.byref(desc), n, L)), launch)
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
    return _pack(lib.stof_zonzini_packed_bytes, lib.stof_zonzini_pack_weights, _lib.ZonziniDesc(int(variant), 0), params,
                 'stof_zonzini_pack_weights', f'unknown Zonzini variant {variant}')

"""EDSR_1D and ESPCN_1D, the two comparison networks of the reference that ride on SampleShuffle1D
(models/edsr_1d.py:8-45, models/espcn_1d.py:8-36; selected by main.py:139-142).

Constructor arguments, module tree, parameter names (checkpoints load with strict=True) and initialisation follow the
reference.  Each network has two routes:

  forward_aten(x)     the reference's forward on stock ATen layers (MIOpen on ROCm) with the gfx950 SampleShuffle1D
                      kernel (the inverse permutation as its backward), so that the networks train;
  forward_kernels(x)  inference on the gfx950 kernels of csrc/riders.hip in exact fp32: one implicit-GEMM kernel per
                      64 -> 64 convolution with bias, ReLU and residual in its epilogue and a fused shuffle + output conv
                      for EDSR_1D(1, 64, B, r | 64); the whole network in one launch for ESPCN_1D(r <= 64).

`forward` takes the kernels when `kernels_supported(x)` holds and no autograd graph would be recorded (under
torch.no_grad(), or when neither x nor any parameter requires grad); everything else (CPU tensors, other dtypes,
other widths, training) stays on `forward_aten`.  Packed weights are cached per (device, storage, `_version`) of every
parameter, so parameter edits are picked up on their own; rows are bitwise independent of their batch, so EDSR's
chunking under `max_workspace_bytes` does not show in the result.

EDSR_1D has a third route, opt-in with `train_route = 'kernels'`:

  forward_train_kernels(x)  the same network behind an autograd boundary (edsr_training.py): `loss.backward()` runs the
                            gfx950 training kernels in exact fp32, deterministic and free of MIOpen.

With it `forward` takes the training kernels wherever it took `forward_aten` only because a graph is recorded.  ESPCN_1D
has the same opt-in route (espcn_training.py: one kernel per stage, activations saved in device memory)."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._kernel_route import _KernelRoute, _pack
from ._train_boundary import train_engine
from .edsr_training import EdsrFunction, EdsrTrainEngine
from .espcn_training import EspcnFunction, EspcnTrainEngine
from .sample_shuffle import SampleShuffle1D


def pack_edsr_weights(num_blocks, upscale_factor, params):
    """Host-side packing (stof_edsr_pack_weights) of the state_dict's float32 arrays in module order -> uint8 CPU blob."""
    params = list(params)
    if len(params) != 2 * (2 * int(num_blocks) + 3):
        raise ValueError(f'EDSR_1D with {num_blocks} blocks has {2 * (2 * int(num_blocks) + 3)} parameters, got {len(params)}')
    lib = _lib.lib()
    return _pack(lib.stof_edsr_packed_bytes, lib.stof_edsr_pack_weights, _lib.EdsrDesc(int(num_blocks), int(upscale_factor)),
                 params, 'stof_edsr_pack_weights')


def pack_espcn_weights(upscale_factor, params):
    """Host-side packing (stof_espcn_pack_weights) of the six state_dict arrays -> uint8 CPU blob."""
    params = list(params)
    if len(params) != 6:
        raise ValueError(f'ESPCN_1D has 6 parameters, got {len(params)}')
    lib = _lib.lib()
    return _pack(lib.stof_espcn_packed_bytes, lib.stof_espcn_pack_weights, _lib.EspcnDesc(int(upscale_factor), 0), params,
                 'stof_espcn_pack_weights')


class _TrainRoute(_KernelRoute):
    """`_KernelRoute` of a model that can also train on the gfx950 kernels: `train_route = 'kernels'` makes `forward` take
    `forward_train_kernels` wherever it took `forward_aten` only because an autograd graph is recorded.  A model supplies
    `_train_engine_key()` (what its engine depends on besides the device), `_make_train_engine(dev, key)` and
    `_train_function`, the engine's autograd boundary."""
    train_route = 'aten'            # 'aten' | 'kernels': which route `forward` takes when an autograd graph is recorded

    def forward_train_kernels(self, x):
        """y [N, 1, L r] float32 on the gfx950 training kernels, with an autograd graph: its backward fills the gradient of
        every parameter (and of x, if it asks for one) in exact fp32; raises where the kernels do not apply."""
        self._check_kernels(x)
        key = (str(x.device), *self._train_engine_key())
        engine = train_engine(self, key, lambda: self._make_train_engine(x.device, key[1:]))
        names, params = zip(*self.named_parameters())
        return self._train_function.apply(x, engine, names, *params)

    def forward(self, x):
        if self.train_route not in ('aten', 'kernels'):
            raise ValueError(f"{type(self).__name__}.train_route must be 'aten' or 'kernels' (got {self.train_route!r})")
        if (self.train_route == 'kernels' and self.kernels_supported(x) and torch.is_grad_enabled()
                and (x.requires_grad or any(p.requires_grad for p in self._kernel_params()))):
            return self.forward_train_kernels(x)
        return super().forward(x)


class ResidualBlock(nn.Module):
    """conv3 - ReLU - conv3 plus identity (models/edsr_1d.py:8-19)."""

    def __init__(self, channels):
        super().__init__()
        self.conv1 = nn.Conv1d(channels, channels, kernel_size=3, stride=1, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv1d(channels, channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x))) + x


class EDSR_1D(_TrainRoute, nn.Module):
    """models/edsr_1d.py:22-45: input conv + ReLU, `num_blocks` residual blocks, mid conv with the long skip,
    SampleShuffle1D (C = num_features / upscale_factor channels survive), output conv."""
    max_workspace_bytes = 512 << 20
    _KERNEL_CONFIG = 'num_channels = 1, num_features = 64 and an upscale_factor that divides 64'
    _train_function = EdsrFunction

    def __init__(self, num_channels=1, num_features=64, num_blocks=8, upscale_factor=4):
        super().__init__()
        self.conv_input = nn.Conv1d(num_channels, num_features, kernel_size=3, stride=1, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.residual_blocks = nn.ModuleList([ResidualBlock(num_features) for _ in range(num_blocks)])
        self.conv_mid = nn.Conv1d(num_features, num_features, kernel_size=3, stride=1, padding=1)
        self.upscale = SampleShuffle1D(upscale_factor)
        self.conv_output = nn.Conv1d(num_features // upscale_factor, num_channels, kernel_size=3, stride=1, padding=1)

    def _config_supported(self):
        r = self.upscale.upsample_factor
        return (self.conv_input.in_channels == 1 and self.conv_input.out_channels == 64 and isinstance(r, int)
                and 1 <= r <= 64 and 64 % r == 0)

    def _pack(self, host):
        return pack_edsr_weights(len(self.residual_blocks), self.upscale.upsample_factor, host)

    def forward_kernels(self, x):
        """y [N, 1, L r] float32 on the gfx950 kernels (no autograd graph); raises where they do not apply."""
        return self._run(x, False)[0]

    def forward_with_trunk(self, x):
        """(y [N, 1, L r], the input of `upscale` [N, 64, L] = conv_mid + the long skip), on the gfx950 kernels."""
        y, trunk = self._run(x, True)
        return y, trunk.transpose(1, 2)

    def _run(self, x, want_trunk):
        self._check_kernels(x)
        N, L, r = int(x.shape[0]), int(x.shape[-1]), int(self.upscale.upsample_factor)
        y = torch.empty((N, 1, L * r), dtype=torch.float32, device=x.device)
        trunk = torch.empty((N, L, 64), dtype=torch.float32, device=x.device) if want_trunk else None
        if N == 0 or L == 0:
            return y, trunk
        x = x.detach().contiguous()
        packed = self.packed_weights(x.device)
        lib = _lib.lib()
        desc = _lib.EdsrDesc(len(self.residual_blocks), r)

        def launch(r0, n, ws, ws_bytes, stream):
            _lib.check(lib.stof_edsr_forward(
                ctypes.byref(desc), ctypes.c_void_p(x[r0].data_ptr()), n, L, _lib.ptr(packed),
                ctypes.c_void_p(y[r0].data_ptr()), None if trunk is None else ctypes.c_void_p(trunk[r0].data_ptr()),
                _lib.ptr(ws), ws_bytes, stream), 'stof_edsr_forward')

        self._chunked(x.device, N, lambda n: int(lib.stof_edsr_workspace_bytes(ctypes.byref(desc), n, L)), launch)
        return y, trunk

    def _train_engine_key(self):
        return len(self.residual_blocks), int(self.upscale.upsample_factor)

    def _make_train_engine(self, dev, key):
        return EdsrTrainEngine(dev, *key)

    def forward_aten(self, x):
        first = self.relu(self.conv_input(x))
        out = first
        for block in self.residual_blocks:
            out = block(out)
        out = self.conv_mid(out) + first
        return self.conv_output(self.upscale(out))


class ESPCN_1D(_TrainRoute, nn.Module):
    """models/espcn_1d.py:8-36: conv5 - tanh - conv3 - tanh - conv3 - SampleShuffle1D - sigmoid, with the reference's
    normal initialisation (std 0.001 for the layer fed by 32 channels, He-style otherwise, zero biases)."""
    _KERNEL_CONFIG = 'an upscale_factor of at most 64'
    _train_function = EspcnFunction

    def __init__(self, upscale_factor):
        super().__init__()
        self.conv1 = nn.Conv1d(1, 64, 5, 1, 2)
        self.conv2 = nn.Conv1d(64, 32, 3, 1, 1)
        self.conv3 = nn.Conv1d(32, upscale_factor, 3, 1, 1)
        self.sample_shuffle = SampleShuffle1D(upscale_factor)
        for m in self.modules():
            if isinstance(m, nn.Conv1d):
                std = 0.001 if m.in_channels == 32 else (2.0 / (m.out_channels * m.weight[0][0].numel())) ** 0.5
                nn.init.normal_(m.weight.data, 0.0, std)
                nn.init.zeros_(m.bias.data)

    def _config_supported(self):
        r = self.sample_shuffle.upsample_factor
        return isinstance(r, int) and 1 <= r <= 64

    def _pack(self, host):
        return pack_espcn_weights(self.sample_shuffle.upsample_factor, host)

    def forward_kernels(self, x):
        """y [N, 1, L r] float32 on the gfx950 kernel (no autograd graph); raises where it does not apply."""
        return self._run(x, False)[0]

    def forward_with_logits(self, x):
        """(y [N, 1, L r], the output of `sample_shuffle` [N, 1, L r], i.e. the map before the sigmoid)."""
        return self._run(x, True)

    def _run(self, x, want_logits):
        self._check_kernels(x)
        N, L, r = int(x.shape[0]), int(x.shape[-1]), int(self.sample_shuffle.upsample_factor)
        y = torch.empty((N, 1, L * r), dtype=torch.float32, device=x.device)
        logits = torch.empty_like(y) if want_logits else None
        if N == 0 or L == 0:
            return y, logits
        x = x.detach().contiguous()
        packed = self.packed_weights(x.device)
        desc = _lib.EspcnDesc(r, 0)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().stof_espcn_forward(ctypes.byref(desc), _lib.ptr(x), N, L, _lib.ptr(packed), _lib.ptr(y),
                                                     _lib.ptr(logits), _lib.stream_ptr(x.device)), 'stof_espcn_forward')
        return y, logits

    def _train_engine_key(self):
        return (int(self.sample_shuffle.upsample_factor),)

    def _make_train_engine(self, dev, key):
        return EspcnTrainEngine(dev, *key)

    def forward_aten(self, x):
        x = torch.tanh(self.conv1(x))
        x = torch.tanh(self.conv2(x))
        return torch.sigmoid(self.sample_shuffle(self.conv3(x)))

"""Wave-U-Net, the reference's `unet` baseline (models/wave_unet.py:34-102; selected by main.py:44-46,159-160).

Constructor arguments, module tree and parameter names follow the reference, so its checkpoints load with strict=True
(`encoder.{i}.main.0|1.*`, `middle.0|1.*`, `decoder.{i}.main.0|1.*`, `out.0.*`).  Three routes:

  forward_aten(x)     the reference's forward on stock ATen layers; it trains, and in train mode BatchNorm uses batch
                      statistics and updates its running ones;
  forward_kernels(x)  inference on the gfx950 kernels of csrc/waveunet.hip in exact fp32 with eval-mode BatchNorm folded
                      into the convolutions: one vector kernel for encoder 0, one implicit-GEMM kernel per other
                      convolution (the x2 decimation is a stride of its loads, the x2 linear interpolation and the
                      concatenation with the skip are built in LDS), one vector kernel for the output convolution + tanh;
  forward_train_kernels(x)  a train-mode step on the gfx950 training kernels (waveunet_training.py, csrc/waveunet_train.hip)
                      behind an autograd boundary: batch statistics, running statistics updated, exact fp32 and bitwise
                      repeatable gradients of every parameter (and of x when it asks for one).

`forward` takes the inference kernels in eval mode when `kernels_supported(x)` holds and no autograd graph would be recorded.
`train_route` (class default 'aten'; 'aten' | 'kernels', not part of the state_dict) decides train-mode calls: with 'aten' they
go to `forward_aten` as every other call does, with 'kernels' to `forward_train_kernels`, graph or not, which raises where the
kernels do not apply instead of falling back.  Eval-mode calls are the same under either setting.
Served on the kernels: channels_interval = 16 (what main.py builds), n_layers 1 .. 12, L a multiple of 2^n_layers; another
channels_interval raises NotImplementedError on construction.  The packed weights are cached per (device, storage,
`_version`) of every parameter and of the BatchNorm running statistics; rows are bitwise independent of their batch, so
the chunking under `max_workspace_bytes` does not show in the result."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._kernel_route import _KernelRoute, _pack

MAX_LAYERS = 12


def pack_waveunet_weights(n_layers, params, channels_interval=16):
    """Host-side packing (stof_waveunet_pack_weights): the state dict's float32 arrays in module order without the
    num_batches_tracked entries -> uint8 CPU blob (layout: csrc/waveunet.hip)."""
    params = list(params)
    want = 6 * (2 * int(n_layers) + 1) + 2
    if len(params) != want:
        raise ValueError(f'WaveUnet with {n_layers} layers has {want} parameter and buffer arrays, got {len(params)}')
    lib = _lib.lib()
    return _pack(lib.stof_waveunet_packed_bytes, lib.stof_waveunet_pack_weights,
                 _lib.WaveUnetDesc(int(n_layers), int(channels_interval)), params, 'stof_waveunet_pack_weights')


class _ConvBlock(nn.Module):
    """Conv1d + BatchNorm1d + LeakyReLU(0.1) under the name `main` (models/wave_unet.py:8-32)."""

    def __init__(self, channel_in, channel_out, kernel_size, padding):
        super().__init__()
        self.main = nn.Sequential(nn.Conv1d(channel_in, channel_out, kernel_size=kernel_size, stride=1, padding=padding),
                                  nn.BatchNorm1d(channel_out), nn.LeakyReLU(negative_slope=0.1))

    def forward(self, x):
        return self.main(x)


class WaveUnet(_KernelRoute, nn.Module):
    """models/wave_unet.py:34-102 with channels_interval = 16: n encoder blocks (k 15) that halve the length, a middle
    block, n decoder blocks (k 5) on the x2 linear interpolation concatenated with the matching skip, and a 17 -> 1
    output convolution on (decoder output, input) with tanh."""
    max_workspace_bytes = 512 << 20
    _KERNEL_CONFIG = 'a length that is a multiple of 2^n_layers'
    _EVAL_ONLY = True       # the inference kernels serve eval mode only; train mode is decided by `train_route`
    train_route = 'aten'    # 'aten' | 'kernels': what a train-mode call runs on

    def __init__(self, n_layers=12, channels_interval=24):
        super().__init__()
        if int(channels_interval) != 16:
            raise NotImplementedError(
                f'WaveUnet(channels_interval={channels_interval}) is out of scope: the MI355X-native path serves '
                f'WaveUnet(n_layers = 1 .. {MAX_LAYERS}, channels_interval=16), the configuration main.py builds')
        if not 1 <= int(n_layers) <= MAX_LAYERS:
            raise ValueError(f'WaveUnet: n_layers must be in 1 .. {MAX_LAYERS} (got {n_layers})')
        n, c = int(n_layers), 16
        self.n_layers, self.channels_interval = n, c
        self.encoder = nn.ModuleList([_ConvBlock(1 if i == 0 else c * i, c * (i + 1), 15, 7) for i in range(n)])
        self.middle = nn.Sequential(nn.Conv1d(c * n, c * n, 15, stride=1, padding=7), nn.BatchNorm1d(c * n),
                                    nn.LeakyReLU(negative_slope=0.1))
        self.decoder = nn.ModuleList([_ConvBlock(2 * c * n if i == 0 else c * (2 * (n - i) + 1), c * (n - i), 5, 2)
                                      for i in range(n)])
        self.out = nn.Sequential(nn.Conv1d(1 + c, 1, kernel_size=1, stride=1), nn.Tanh())

    # parameters and the BatchNorm running statistics, in the order the packer reads them
    _kernel_params = _KernelRoute._state_arrays

    def kernels_supported(self, x):
        """True when `forward_kernels(x)` can run: x float32 [N, 1, L] on the ROCm device with L a multiple of
        2^n_layers, every parameter and running statistic float32 on that device."""
        return super().kernels_supported(x) and x.shape[-1] >= 1 and x.shape[-1] % (1 << self.n_layers) == 0

    def _pack(self, host):
        return pack_waveunet_weights(self.n_layers, host)

    def forward_kernels(self, x):
        """y [N, 1, L] float32 on the gfx950 kernels with the running statistics (no autograd graph); raises where they
        do not apply."""
        return self._run(x, False)[0]

    def forward_with_taps(self, x):
        """(y [N, 1, L], the middle block's output [N, 16 n, L / 2^n], the output convolution before the tanh [N, 1, L]),
        on the gfx950 kernels."""
        y, bott, logits = self._run(x, True)
        return y, bott.transpose(1, 2), logits

    def _run(self, x, want_taps):
        self._check_kernels(x)
        n = self.n_layers
        N, L = int(x.shape[0]), int(x.shape[-1])
        y = torch.empty((N, 1, L), dtype=torch.float32, device=x.device)
        bott = torch.empty((N, L >> n, 16 * n), dtype=torch.float32, device=x.device) if want_taps else None
        logits = torch.empty_like(y) if want_taps else None
        if N == 0:
            return y, bott, logits
        x = x.detach().contiguous()
        packed = self.packed_weights(x.device)
        lib = _lib.lib()
        desc = _lib.WaveUnetDesc(n, 16)

        def launch(r0, rows, ws, ws_bytes, stream):
            _lib.check(lib.stof_waveunet_forward(
                ctypes.byref(desc), ctypes.c_void_p(x[r0].data_ptr()), rows, L, _lib.ptr(packed),
                ctypes.c_void_p(y[r0].data_ptr()), None if bott is None else ctypes.c_void_p(bott[r0].data_ptr()),
                None if logits is None else ctypes.c_void_p(logits[r0].data_ptr()), _lib.ptr(ws), ws_bytes, stream),
                'stof_waveunet_forward')

        self._chunked(x.device, N, lambda rows: int(lib.stof_waveunet_workspace_bytes(ctypes.byref(desc), rows, L)), launch)
        return y, bott, logits

    def forward_aten(self, x):
        if self.training:
            self.invalidate_packed()       # BatchNorm is about to move its running statistics
        skips = []
        o = x
        for block in self.encoder:
            o = block(o)
            skips.append(o)
            o = o[:, :, ::2]
        o = self.middle(o)
        for i, block in enumerate(self.decoder):
            o = F.interpolate(o, scale_factor=2, mode='linear', align_corners=True)
            o = block(torch.cat([o, skips[self.n_layers - i - 1]], dim=1))
        return self.out(torch.cat([o, x], dim=1))

    def forward_train_kernels(self, x):
        """y [N, 1, L] float32 of a train-mode call on the gfx950 training kernels (waveunet_training.py), with an autograd
        graph when one is recorded: its backward fills the gradient of every parameter (and of x, if it asks for one) in
        exact fp32.  BatchNorm uses batch statistics and the running statistics are updated, also under no_grad.  Not
        chunked by `max_workspace_bytes`: the batch statistics and the backward need every activation of the whole batch."""
        from ._train_boundary import commit_running_stats, train_engine
        from .waveunet_training import WaveUnetFunction, WaveUnetTrainEngine
        if not self.training:
            raise NotImplementedError("WaveUnet: train_route='kernels' serves train mode only (batch statistics); eval-mode "
                                      'calls take the inference kernels or forward_aten')
        self._check_kernels(x)
        n = self.n_layers
        N, L = int(x.shape[0]), int(x.shape[-1])
        if N * (L >> n) == 1:                               # torch's BatchNorm check, word for word, before anything is touched
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size([N, 16 * n, L >> n])}')
        bns = [blk.main[1] for blk in self.encoder] + [self.middle[1]] + [blk.main[1] for blk in self.decoder]
        engine = train_engine(self, str(x.device), lambda: WaveUnetTrainEngine(x.device, n))
        engine.eps = [float(bn.eps) for bn in bns]
        engine.momentum = [float(bn.momentum) for bn in bns]
        engine.running = [(bn.running_mean, bn.running_var) for bn in bns]
        names, params = zip(*self.named_parameters())
        y = WaveUnetFunction.apply(x, engine, names, *params)
        if N:
            commit_running_stats(bns, engine.new_running)
        return y

    def forward(self, x):
        route = self.train_route
        if route not in ('aten', 'kernels'):
            raise ValueError(f"WaveUnet.train_route must be 'aten' or 'kernels' (got {route!r})")
        if route == 'kernels' and self.training:
            return self.forward_train_kernels(x)
        return super().forward(x)

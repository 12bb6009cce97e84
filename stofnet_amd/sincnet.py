"""The SincNet baseline of the reference (models/sincnet.py: SincNet with the option dict of main.py:145-157) on the
gfx950 kernels of csrc/sincnet.hip (inference, exact fp32) and, opt-in through `train_route`, csrc/sincnet_train.hip
(training with train-mode BatchNorm, sincnet_training.py).

The module tree (`conv`, `bn`, `ln`, `act`, `drop`), parameter names, shapes and default initialisation are the
reference's, so its checkpoints load with strict=True.  The layers are parameter holders: the forward never calls their
ATen kernels.  It packs the parameters (and the BatchNorm running statistics) once per change, synthesising the sinc
filter bank on the host, splits the batch into chunks whose workspace stays under `max_workspace_bytes`, and launches
the HIP forward on the current stream.  Rows are bitwise independent of the batch they sit in, so the chunking does not
show in the result.

Only the configuration the shipped checkpoints were trained with is accelerated (`ACCELERATED_OPTIONS`, any
`input_dim`, any `cnn_drop`, `fs` > 0); any other option dict raises NotImplementedError naming the key."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._kernel_route import _PackedKernels, _pack

N_FILT = 128
SINC_TAPS = 1023
MIN_LOW_HZ = 50.0
MIN_BAND_HZ = 50.0
GAP = 8                                     # zero rows around every waveform in the workspace (csrc/sincnet.hip)

# main.py:145-157 without input_dim, fs and cnn_drop
ACCELERATED_OPTIONS = {
    'cnn_N_filt': [128, 128, 128, 1],
    'cnn_len_filt': [1023, 11, 9, 7],
    'cnn_max_pool_len': [1, 1, 1, 1],
    'cnn_use_laynorm_inp': False,
    'cnn_use_batchnorm_inp': False,
    'cnn_use_laynorm': [False, False, False, False],
    'cnn_use_batchnorm': [True, True, True, True],
    'cnn_act': ['leaky_relu', 'leaky_relu', 'leaky_relu', 'linear'],
    'use_sinc': True,
}


def _same(a, b):
    if isinstance(b, list):
        return isinstance(a, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(b, bool):
        return isinstance(a, (bool, np.bool_)) and bool(a) == b
    if isinstance(b, str):
        return a == b
    return not isinstance(a, (bool, np.bool_)) and isinstance(a, (int, float, np.integer, np.floating)) and a == b


def check_options(options):
    """Raise NotImplementedError naming the first key of `options` outside the accelerated configuration."""
    if not isinstance(options, dict):
        raise NotImplementedError('SincNet needs the option dict of main.py (the gfx950 path accelerates exactly that '
                                  'configuration)')
    for key, want in ACCELERATED_OPTIONS.items():
        if key not in options:
            raise NotImplementedError(f'SincNet: option {key!r} is missing')
        if not _same(options[key], want):
            raise NotImplementedError(f'SincNet: option {key}={options[key]!r} is not supported on the gfx950 path '
                                      f'(supported: {want!r})')
    for key in ('input_dim', 'fs', 'cnn_drop'):
        if key not in options:
            raise NotImplementedError(f'SincNet: option {key!r} is missing')
    try:
        fs = float(options['fs'])
    except (TypeError, ValueError):
        raise NotImplementedError(f"SincNet: option fs={options['fs']!r} is not a sample rate") from None
    if not (math.isfinite(fs) and fs > 0):
        raise NotImplementedError(f'SincNet: option fs={fs!r} is not supported (needs a finite sample rate > 0)')
    drop = options['cnn_drop']
    if not isinstance(drop, (list, tuple)) or len(drop) != 4:
        raise NotImplementedError(f'SincNet: option cnn_drop={drop!r} is not supported (needs 4 dropout rates)')


def mel_init(fs, n_filt=N_FILT):
    """SincConv_fast's default bands for sample rate fs: n_filt + 1 edges equally spaced in mel between 30 Hz and
    fs / 2 - 100 Hz -> (low_hz_, band_hz_) as float32 [n_filt, 1]."""
    to_mel = lambda hz: 2595 * np.log10(1 + hz / 700)            # noqa: E731
    to_hz = lambda mel: 700 * (10 ** (mel / 2595) - 1)           # noqa: E731
    edges = to_hz(np.linspace(to_mel(30), to_mel(fs / 2 - (MIN_LOW_HZ + MIN_BAND_HZ)), n_filt + 1))
    return (torch.tensor(edges[:-1], dtype=torch.float32).view(-1, 1),
            torch.tensor(np.diff(edges), dtype=torch.float32).view(-1, 1))


def filter_bank(fs, low_hz, band_hz):
    """The sinc filter bank of the packer (SincConv_fast.filters, synthesised in double) -> float32 [128, 1, 1023]."""
    lib = _lib.lib()
    desc = _lib.SincNetDesc(float(fs), 1e-5, 0, 0)
    lo = np.ascontiguousarray(np.asarray(low_hz, np.float32).reshape(-1))
    bd = np.ascontiguousarray(np.asarray(band_hz, np.float32).reshape(-1))
    if lo.size != N_FILT or bd.size != N_FILT:
        raise ValueError(f'low_hz / band_hz need {N_FILT} entries')
    bank = np.zeros((N_FILT, SINC_TAPS), np.float32)
    _lib.check(lib.stof_sincnet_filter_bank(ctypes.byref(desc), lo.ctypes.data, bd.ctypes.data, bank.ctypes.data),
               'stof_sincnet_filter_bank')
    return torch.from_numpy(bank).view(N_FILT, 1, SINC_TAPS)


class SincConv(nn.Module):
    """Parameter holder of SincConv_fast (models/sincnet.py:58-188) for 128 filters of 1023 taps: `low_hz_`,
    `band_hz_` [128, 1] with the mel-spaced default for `sample_rate`.  `filters` is the bank the kernels use."""

    def __init__(self, out_channels, kernel_size, sample_rate):
        super().__init__()
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.sample_rate = sample_rate
        self.min_low_hz = MIN_LOW_HZ
        self.min_band_hz = MIN_BAND_HZ
        low, band = mel_init(sample_rate, out_channels)
        self.low_hz_ = nn.Parameter(low)
        self.band_hz_ = nn.Parameter(band)

    @property
    def filters(self):
        return filter_bank(self.sample_rate, self.low_hz_.detach().cpu().numpy(), self.band_hz_.detach().cpu().numpy())


class SincNet(_PackedKernels, nn.Module):
    """models/sincnet.py SincNet(options) for the option dict of main.py:145-157: sinc conv 1 -> 128 (1023 taps), Conv1d
    128 -> 128 (k 11), 128 -> 128 (k 9), 128 -> 1 (k 7), each "same" zero padded, followed by BatchNorm1d (eval) and
    LeakyReLU(0.2) (the last one linear).  x [N, L] or [N, 1, L] float32 -> y [N, 1, L]."""
    max_workspace_bytes = 512 << 20
    _PACKED_ARRAYS = 'parameters and BatchNorm statistics'
    # None | 'kernels' | 'aten'.  None: every call behaves as an inference-only module (train mode and recorded graphs raise).
    # Otherwise a train-mode call takes the training route whether or not a graph is recorded (train-mode BatchNorm uses batch
    # statistics and updates the running ones under no_grad too): 'kernels' goes through the autograd boundary of
    # sincnet_training.py (gfx950 kernels, exact fp32), 'aten' runs `forward_aten`.  Eval-mode calls that record no graph stay
    # on the inference kernels; one that would record a graph runs `forward_aten` under 'aten' and raises under 'kernels'.
    train_route = None

    def __init__(self, options=None):
        super().__init__()
        check_options(options)
        self.cnn_N_filt = list(options['cnn_N_filt'])
        self.cnn_len_filt = list(options['cnn_len_filt'])
        self.cnn_max_pool_len = list(options['cnn_max_pool_len'])
        self.cnn_act = list(options['cnn_act'])
        self.cnn_drop = list(options['cnn_drop'])
        self.cnn_use_laynorm = list(options['cnn_use_laynorm'])
        self.cnn_use_batchnorm = list(options['cnn_use_batchnorm'])
        self.cnn_use_laynorm_inp = options['cnn_use_laynorm_inp']
        self.cnn_use_batchnorm_inp = options['cnn_use_batchnorm_inp']
        self.input_dim = int(options['input_dim'])
        self.fs = options['fs']
        self.use_sinc = options['use_sinc']
        self.N_cnn_lay = 4
        self.conv = nn.ModuleList()
        self.bn = nn.ModuleList()
        self.ln = nn.ModuleList()                # empty, as in the reference (no layer norm in this configuration)
        self.act = nn.ModuleList()
        self.drop = nn.ModuleList()
        cur = self.input_dim
        for i in range(4):                        # the reference's construction order (torch's RNG draws match)
            self.drop.append(nn.Dropout(p=self.cnn_drop[i]))
            self.act.append(nn.LeakyReLU(0.2) if self.cnn_act[i] == 'leaky_relu' else nn.LeakyReLU(1))
            self.bn.append(nn.BatchNorm1d(self.cnn_N_filt[i], momentum=0.05))
            if i == 0:
                self.conv.append(SincConv(self.cnn_N_filt[0], self.cnn_len_filt[0], self.fs))
            else:
                self.conv.append(nn.Conv1d(self.cnn_N_filt[i - 1], self.cnn_N_filt[i], self.cnn_len_filt[i]))
            cur = int((cur - self.cnn_len_filt[i] + 1) / self.cnn_max_pool_len[i])
        self.out_dim = cur * self.cnn_N_filt[-1]

    def _desc(self, stop_after=0):
        eps = {float(b.eps) for b in self.bn}
        if len(eps) != 1:
            raise NotImplementedError('SincNet: the BatchNorm layers must share one eps on the gfx950 path')
        return _lib.SincNetDesc(float(self.fs), eps.pop(), int(stop_after), 0)

    def _kernel_params(self):
        ps = [self.conv[0].low_hz_, self.conv[0].band_hz_]
        for conv in self.conv[1:]:
            ps += [conv.weight, conv.bias]
        for bn in self.bn:
            ps += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return ps

    def _pack_key(self):
        desc = self._desc()
        return (desc.fs, desc.bn_eps)

    def _pack(self, host):
        fs, bn_eps = self._pack_key()
        return pack_weights(fs, host, bn_eps)

    def packed_weights(self, device):
        """The inference blob.  With a training route set and every array on `device` it is packed there
        (`device_pack_weights`: no device-to-host copy when a validation pass follows an optimizer step), else on the host."""
        params = self._kernel_params()
        if self.train_route is None or any(p.device != torch.device(device) or p.dtype != torch.float32 for p in params):
            return super().packed_weights(device)
        key = ('device', str(device), *self._pack_key()) + tuple((p.data_ptr(), p._version) for p in params)
        if self._packed is None or self._packed_key != key:
            self._packed = device_pack_weights(*self._pack_key(), [p.detach() for p in params])
            self._packed_key = key
        return self._packed

    def _check_frame(self, x):
        _lib.require_device(x, 'x')
        if x.dtype != torch.float32:
            raise TypeError(f'SincNet: x must be float32 (got {x.dtype}); the gfx950 kernels are fp32 only')
        if not (x.dim() == 2 or (x.dim() == 3 and x.shape[1] == 1)):
            raise RuntimeError(f'SincNet: expected x of shape [N, L] or [N, 1, L], got {list(x.shape)}')

    def _check_input(self, x):
        if self.training:
            raise NotImplementedError('SincNet: training is not implemented on the gfx950 path (in train mode the '
                                      "reference's BatchNorm uses batch statistics, also under no_grad; call model.eval())")
        self._check_frame(x)
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError('SincNet: backward is not implemented on the gfx950 path (inference only: run '
                                      'under torch.no_grad() or detach the input)')
        if int(x.shape[-1]) < 1:
            raise RuntimeError('SincNet: rows must hold at least one sample')

    def _check_train_options(self):
        if self.training and any(float(d) != 0.0 for d in self.cnn_drop):
            raise NotImplementedError(f'SincNet: option cnn_drop={self.cnn_drop!r} is not supported on the training routes (live '
                                      'dropout is not implemented; main.py uses 0.0)')

    def sinc_filters(self):
        """SincConv_fast's filter synthesis (models/sincnet.py:147-184) restated in torch on `low_hz_` / `band_hz_`, in their
        dtype and on their device, with an autograd graph -> [128, 1, 1023]."""
        sinc = self.conv[0]
        low_p, band_p = sinc.low_hz_, sinc.band_hz_
        dt, dev = low_p.dtype, low_p.device
        k, fs = SINC_TAPS, sinc.sample_rate
        n_lin = torch.linspace(0, (k / 2) - 1, steps=int(k / 2), dtype=dt, device=dev)
        window = 0.54 - 0.46 * torch.cos(2 * math.pi * n_lin / k)
        n = 2 * math.pi * torch.arange(-(k - 1) / 2.0, 0, dtype=dt, device=dev).view(1, -1) / fs
        low = sinc.min_low_hz + torch.abs(low_p)
        high = torch.clamp(low + sinc.min_band_hz + torch.abs(band_p), sinc.min_low_hz, fs / 2)
        band = (high - low)[:, 0]
        left = ((torch.sin(torch.matmul(high, n)) - torch.sin(torch.matmul(low, n))) / (n / 2)) * window
        bank = torch.cat([left, 2 * band.view(-1, 1), torch.flip(left, dims=[1])], dim=1) / (2 * band[:, None])
        return bank.view(N_FILT, 1, k)

    def forward_aten(self, x):
        """The reference's forward (models/sincnet.py:460-497) restated in torch on the module's own parameters: the sinc
        filter synthesis, "same" zero padding, F.conv1d, then the module's `bn[i]`, `act[i]` and `drop[i]`.  Runs in the
        parameters' dtype on their device (also the CPU, also float64), in train or eval mode."""
        self._check_train_options()
        p0 = self.conv[0].low_hz_
        x = x.to(device=p0.device, dtype=p0.dtype)
        n = int(x.shape[0])
        x = x.reshape(n, 1, int(x.shape[-1]))
        for i in range(4):
            k = self.cnn_len_filt[i]
            x = F.pad(x, ((k - 1) // 2, k - 1 - (k - 1) // 2))
            z = F.conv1d(x, self.sinc_filters()) if i == 0 else F.conv1d(x, self.conv[i].weight, self.conv[i].bias)
            x = self.drop[i](self.act[i](self.bn[i](z)))
        return x.view(n, 1, -1)

    def forward_train_kernels(self, x):
        """y [N, 1, L] float32 of a train-mode call on the gfx950 training kernels (sincnet_training.py), with an autograd
        graph when one is recorded: its backward fills the gradient of all 16 parameters (and of x, if it asks for one) in
        exact fp32.  BatchNorm uses batch statistics and the running statistics are updated, also under no_grad.  Not chunked
        by `max_workspace_bytes`: the batch statistics and the backward need every activation of the whole batch."""
        from ._train_boundary import commit_running_stats, fp32_device_params, train_engine
        from .sincnet_training import SincNetFunction, SincNetTrainEngine
        if not self.training:
            raise NotImplementedError("SincNet: train_route='kernels' serves train mode only; an eval-mode backward (running "
                                      "statistics) is not implemented on the kernels (use train_route='aten' or torch.no_grad())")
        self._check_train_options()
        if isinstance(x, torch.Tensor) and x.dim() in (2, 3) and x.numel() == 1:                # torch's BatchNorm check, word for word
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size([1, N_FILT, 1])}')
        self._check_frame(x)
        N, L = int(x.shape[0]), int(x.shape[-1])
        names, params = fp32_device_params(self, 'SincNet')
        desc = self._desc()
        engine = train_engine(self, (str(x.device), desc.fs, desc.bn_eps), lambda: SincNetTrainEngine(x.device, desc.fs, desc.bn_eps))
        engine.momentum = float(self.bn[0].momentum)
        engine.running = [(bn.running_mean, bn.running_var) for bn in self.bn]
        y = SincNetFunction.apply(x.reshape(N, 1, L), engine, names, *params)
        if N and L:
            commit_running_stats(self.bn, engine.new_running)
        return y

    def forward(self, x):
        route = self.train_route
        if route not in (None, 'kernels', 'aten'):
            raise ValueError(f"SincNet.train_route must be None, 'kernels' or 'aten' (got {route!r})")
        if route is not None:
            if self.training:
                return self.forward_train_kernels(x) if route == 'kernels' else self.forward_aten(x)
            if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
                if route == 'aten':
                    return self.forward_aten(x)
                raise NotImplementedError("SincNet: an eval-mode call that records a graph is not implemented on train_route="
                                          "'kernels' (the kernels' backward is the train-mode one, with batch statistics; use "
                                          "train_route='aten', model.train() or torch.no_grad())")
        self._check_input(x)
        N, L = int(x.shape[0]), int(x.shape[-1])
        y = torch.empty((N, 1, L), dtype=torch.float32, device=x.device)
        if N == 0:
            return y
        self._launch(x, y, 0)
        return y

    def forward_layers(self, x):
        """The post-activation outputs of layers 0, 1 and 2 (the reference's `act[i]` outputs), each [N, 128, L]
        float32: three forwards that stop after the layer, read back from the workspace.  Diagnostics only."""
        self._check_input(x)
        N, L = int(x.shape[0]), int(x.shape[-1])
        outs = []
        for k in (1, 2, 3):
            ws, half = self._launch(x, None, k, chunked=False)
            buf = ws[((k - 1) & 1) * half:].view(torch.float32)[GAP * N_FILT:GAP * N_FILT + N * (L + GAP) * N_FILT]
            outs.append(buf.view(N, L + GAP, N_FILT)[:, :L, :].permute(0, 2, 1).contiguous())
        return outs

    def _launch(self, x, y, stop_after, chunked=True):
        N, L = int(x.shape[0]), int(x.shape[-1])
        x = x.detach().reshape(N, L).contiguous()
        packed = self.packed_weights(x.device)
        lib = _lib.lib()
        desc = self._desc(stop_after)

        def launch(r0, n, ws, ws_bytes, stream):
            _lib.check(lib.stof_sincnet_forward(
                ctypes.byref(desc), ctypes.c_void_p(x[r0].data_ptr()), n, L, _lib.ptr(packed),
                None if y is None else ctypes.c_void_p(y[r0].data_ptr()), _lib.ptr(ws), ws_bytes, stream),
                'stof_sincnet_forward')

        ws, ws_bytes = self._chunked(x.device, N, lambda n: int(lib.stof_sincnet_workspace_bytes(ctypes.byref(desc), n, L)),
                                     launch, chunked)
        return ws, ws_bytes // 2


def pack_weights(fs, params, bn_eps=1e-5):
    """Host-side packing (stof_sincnet_pack_weights) of the 24 float32 arrays in module order (see the header) -> a
    uint8 CPU tensor holding the blob."""
    lib = _lib.lib()
    desc = _lib.SincNetDesc(float(fs), float(bn_eps), 0, 0)
    if not lib.stof_sincnet_packed_bytes(ctypes.byref(desc)):                # the description first, then the count, as ever
        raise ValueError(f'bad SincNet description (fs={fs!r}, bn_eps={bn_eps!r})')
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in params]
    if len(arrs) != 24:
        raise ValueError(f'SincNet packing needs 24 arrays, got {len(arrs)}')
    return _pack(lib.stof_sincnet_packed_bytes, lib.stof_sincnet_pack_weights, desc, arrs, 'stof_sincnet_pack_weights')


def device_pack_weights(fs, bn_eps, params):
    """`pack_weights` on the device (stof_sincnet_device_pack): the same 24 float32 arrays as tensors on one ROCm device -> the
    blob there, a uint8 tensor.  No device-to-host copy; bitwise the host packer's blob on the tested parameter sets."""
    lib = _lib.lib()
    desc = _lib.SincNetDesc(float(fs), float(bn_eps), 0, 0)
    nbytes = int(lib.stof_sincnet_packed_bytes(ctypes.byref(desc)))
    if not nbytes:
        raise ValueError(f'bad SincNet description (fs={fs!r}, bn_eps={bn_eps!r})')
    if len(params) != 24:
        raise ValueError(f'SincNet packing needs 24 arrays, got {len(params)}')
    params = [_lib.require_device(p, 'parameter').contiguous() for p in params]
    dev = params[0].device
    blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * 24)(*[p.data_ptr() for p in params])
    with torch.cuda.device(dev):
        _lib.check(lib.stof_sincnet_device_pack(ctypes.byref(desc), ptrs, _lib.ptr(blob), nbytes, _lib.stream_ptr(dev)),
                   'stof_sincnet_device_pack')
    return blob

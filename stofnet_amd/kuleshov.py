"""Kuleshov, the reference's audio-super-resolution baseline (models/kuleshov.py:19-147; selected by main.py:137-138).

Constructor arguments, attribute names and construction order follow the reference, so its state dict loads with
strict=True (`down_conv{i}`, `down_bn{i}`, `bottleneck`, `up_conv{i}`, `up_bn{i}`, `final_conv`, `output_fc`) and
`torch.manual_seed(s); Kuleshov(...)` draws the reference's initial weights.  Two routes, as for the other baselines:

  forward_aten(x)     the reference's forward (crop included) on stock ATen layers; it trains, and in train mode the
                      Dropouts are live and BatchNorm uses batch statistics and updates its running ones;
  forward_train_kernels(x)  a train-mode call on the gfx950 training kernels (kuleshov_training.py), taken by `forward` when
                      `train_route = 'kernels'` (the class default is 'aten'): batch statistics, Dropout masks that are a pure
                      function of (`dropout_seed`, `dropout_call`), the full backward pass in exact fp32;
  forward_kernels(x)  inference on the gfx950 kernels of csrc/kuleshov.hip in exact fp32: a vector kernel for down_conv0,
                      one implicit-GEMM kernel for the nine 128 .. 1024-wide convolutions (stride 1 or 2; BatchNorm and
                      both leaky ReLUs in the epilogue; the pixel shuffle is the store address of the up convolutions and
                      the length-wise concatenation two row ranges of one buffer), a vector kernel for final_conv and an
                      MFMA GEMM for output_fc that streams the weight once per 128 rows.

`forward` takes the kernels in eval mode when `kernels_supported(x)` holds and no autograd graph would be recorded.
Served: num_layers = 4 (the only value for which the reference's forward runs) and input_length >= 641, the shortest
row for which every convolution has an output.  The packed weights are cached per (device, storage, `_version`) of every
parameter and of the BatchNorm running statistics; rows are bitwise independent of their batch, so the chunking under
`max_workspace_bytes` does not show in the result.  Rows longer than input_length are cropped by stride, without a copy."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._kernel_route import _KernelRoute, _pack

MIN_INPUT_LENGTH = 641
N_FILTERS = (128, 256, 512, 512)
N_FILTERSIZES = (65, 33, 17, 9)
NUM_ARRAYS = 54


def chain_lengths(input_length):
    """The lengths down the network for rows of `input_length` samples: dict with `down` (4), `bottleneck`, `up` (the
    four up convolutions' outputs), `cat` (the four concatenations), `final` and `fc_dim` (models/kuleshov.py:63-112)."""
    w, down = int(input_length), []
    for fs in N_FILTERSIZES:
        w = (w - fs) // 2 + 1
        down.append(w)
    bott = (w - 9) // 2 + 1
    w, up, cat = bott, [], []
    for fs, d in zip(reversed(N_FILTERSIZES), reversed(down)):
        up.append(w - fs + 1)
        w = 2 * up[-1] + d
        cat.append(w)
    return {'down': down, 'bottleneck': bott, 'up': up, 'cat': cat, 'final': w - 8, 'fc_dim': 2 * (w - 8)}


def pack_kuleshov_weights(input_length, output_length, params, bn_eps=1e-5):
    """Host-side packing (stof_kuleshov_pack_weights): the state dict's float32 arrays in module order without the
    num_batches_tracked entries -> uint8 CPU blob (layout: csrc/kuleshov.hip)."""
    params = list(params)
    if len(params) != NUM_ARRAYS:
        raise ValueError(f'Kuleshov has {NUM_ARRAYS} parameter and buffer arrays, got {len(params)}')
    lib = _lib.lib()
    return _pack(lib.stof_kuleshov_packed_bytes, lib.stof_kuleshov_pack_weights,
                 _lib.KuleshovDesc(int(input_length), int(output_length), float(bn_eps), 0, 0), params,
                 'stof_kuleshov_pack_weights')


class Kuleshov(_KernelRoute, nn.Module):
    """models/kuleshov.py:19-147 with num_layers = 4: four stride-2 down blocks, a stride-2 bottleneck, four up blocks
    (convolution, BatchNorm, x2 pixel shuffle, concatenation along the length with the matching down output), a
    128 -> 2 convolution whose flattened output feeds Linear(fc_dim, output_length)."""
    max_workspace_bytes = 512 << 20
    _KERNEL_CONFIG = 'rows of at least input_length samples with one eps in every BatchNorm'
    _EVAL_ONLY = True       # the inference kernels serve eval mode only; train mode is decided by `train_route`
    train_route = 'aten'    # 'aten' | 'kernels': what a train-mode call runs on
    dropout_seed = None     # seed of the kernel route's Dropout masks; None: torch.initial_seed() at first use
    dropout_call = 0        # counts the kernel route's train-mode forwards: the `call` word of the masks' counter
    tile_variant = 0            # 0: wave tile chosen per layer; 1, 2, 3 pin it (bitwise the same; for tests and timing)

    def __init__(self, input_length=None, output_length=None, num_layers=4):
        super().__init__()
        if input_length is None or output_length is None:
            raise NotImplementedError('Kuleshov needs its lengths: Kuleshov(input_length, output_length) as in the '
                                      'reference (main.py:137-138 passes the frame length and frame length x '
                                      'upsample_factor)')
        if int(num_layers) != 4:
            raise NotImplementedError(f'Kuleshov(num_layers={num_layers}) is out of scope: the reference\'s forward runs '
                                      f'for num_layers = 4 only, and so does the MI355X-native path')
        if int(input_length) < MIN_INPUT_LENGTH:
            raise ValueError(f'Kuleshov: input_length must be at least {MIN_INPUT_LENGTH}, the shortest row for which '
                             f'every convolution has an output (got {input_length})')
        if int(output_length) < 1:
            raise ValueError(f'Kuleshov: output_length must be at least 1 (got {output_length})')
        self.layers = int(num_layers)
        self.input_length = int(input_length)
        self.output_length = int(output_length)
        nf, fs = N_FILTERS, N_FILTERSIZES
        for i in range(4):
            setattr(self, f'down_conv{i}', nn.Conv1d(1 if i == 0 else nf[i - 1], nf[i], fs[i], stride=2))
            setattr(self, f'down_bn{i}', nn.BatchNorm1d(nf[i]))
            setattr(self, f'down_do{i}', nn.LeakyReLU(0.2))
        self.bottleneck = nn.Conv1d(nf[-1], nf[-1], 9, stride=2)
        self.bottleneck_dropout = nn.Dropout(p=0.5)
        self.bottleneck_last = nn.LeakyReLU(0.2)
        for i in range(4):
            setattr(self, f'up_conv{i}', nn.Conv1d(nf[-1] if i == 0 else nf[-i], 2 * nf[3 - i], fs[3 - i]))
            setattr(self, f'up_bn{i}', nn.BatchNorm1d(2 * nf[3 - i]))
            setattr(self, f'up_do{i}', nn.Dropout(p=0.5))
        self.subpixel = nn.PixelShuffle(2)
        self.final_conv = nn.Conv1d(nf[0], 2, 9)
        self.fc_dim = chain_lengths(self.input_length)['fc_dim']
        self.output_fc = nn.Linear(self.fc_dim, self.output_length)

    def _batch_norms(self):
        return [getattr(self, f'{p}_bn{i}') for p in ('down', 'up') for i in range(4)]

    # parameters and the BatchNorm running statistics, in the order the packer reads them
    _kernel_params = _KernelRoute._state_arrays

    def _config_supported(self):
        return len({float(bn.eps) for bn in self._batch_norms()}) == 1

    def kernels_supported(self, x):
        """True when `forward_kernels(x)` can run: x float32 [N, 1, L >= input_length] on the ROCm device, every
        parameter and running statistic float32 on that device, one eps in all BatchNorm layers."""
        return super().kernels_supported(x) and x.shape[-1] >= self.input_length

    def _desc(self):
        return _lib.KuleshovDesc(self.input_length, self.output_length, float(self.down_bn0.eps), int(self.tile_variant), 0)

    def _pack(self, host):
        return pack_kuleshov_weights(self.input_length, self.output_length, host, self.down_bn0.eps)

    def _pack_key(self):
        return (float(self.down_bn0.eps),)

    def forward_kernels(self, x):
        """y [N, 1, output_length] float32 on the gfx950 kernels with the running statistics (no autograd graph);
        raises where they do not apply."""
        return self._run(x, False)[0]

    def forward_with_taps(self, x):
        """(y [N, 1, output_length], the output of bottleneck_last [N, 512, B], the input of final_conv [N, 128, Lc],
        the output of final_conv [N, 2, F]) on the gfx950 kernels."""
        y, bott, fin_in, fin = self._run(x, True)
        return y, bott.transpose(1, 2), fin_in.transpose(1, 2), fin.transpose(1, 2)

    def _run(self, x, want_taps):
        self._check_kernels(x)
        N = int(x.shape[0])
        dims = chain_lengths(self.input_length)

        def tap(*shape):
            return torch.empty((N,) + shape, dtype=torch.float32, device=x.device) if want_taps else None

        y = torch.empty((N, 1, self.output_length), dtype=torch.float32, device=x.device)
        bott, fin_in, fin = tap(dims['bottleneck'], 512), tap(dims['cat'][-1], 128), tap(dims['final'], 2)
        if N == 0:
            return y, bott, fin_in, fin
        x = x.detach()
        if x.stride(-1) != 1 or (N > 1 and x.stride(0) < self.input_length):
            x = x.contiguous()
        row_stride = int(x.stride(0)) if N > 1 else int(x.shape[-1])
        packed = self.packed_weights(x.device)
        lib = _lib.lib()
        desc = self._desc()

        def launch(r0, rows, ws, ws_bytes, stream):
            _lib.check(lib.stof_kuleshov_forward(
                ctypes.byref(desc), ctypes.c_void_p(x[r0].data_ptr()), rows, row_stride, _lib.ptr(packed),
                ctypes.c_void_p(y[r0].data_ptr()), *[None if t is None else ctypes.c_void_p(t[r0].data_ptr())
                                                     for t in (bott, fin_in, fin)],
                _lib.ptr(ws), ws_bytes, stream), 'stof_kuleshov_forward')

        self._chunked(x.device, N, lambda rows: int(lib.stof_kuleshov_workspace_bytes(ctypes.byref(desc), rows)), launch)
        return y, bott, fin_in, fin

    def forward_aten(self, x):
        if self.training:
            self.invalidate_packed()       # BatchNorm is about to move its running statistics
        x = x[:, :, :self.input_length]
        skips = [x]
        for i in range(self.layers):
            x = F.leaky_relu(getattr(self, f'down_conv{i}')(x))
            x = getattr(self, f'down_do{i}')(getattr(self, f'down_bn{i}')(x))
            skips.append(x)
        x = self.bottleneck_last(self.bottleneck_dropout(self.bottleneck(x)))
        for i in range(self.layers):
            x = getattr(self, f'up_do{i}')(getattr(self, f'up_bn{i}')(getattr(self, f'up_conv{i}')(x)))
            x = self.subpixel(x.unsqueeze(2))
            x = x.view(-1, x.size(2) * x.size(1), x.size(3))
            x = torch.cat((x, skips[len(skips) - 1 - i]), -1)
        x = self.final_conv(x)                                   # [N, 2, F]
        x = x.transpose(1, 2).reshape(x.size(0), 2 * x.size(2))  # SubPixel1D + view: flat[n, 2 pos + ch]
        return self.output_fc(x).unsqueeze(1)

    def forward_train_kernels(self, x):
        """y [N, 1, output_length] float32 of a train-mode call on the gfx950 training kernels (kuleshov_training.py), with an
        autograd graph when one is recorded: its backward fills the gradient of every parameter (and of x, if it asks for one)
        in exact fp32.  BatchNorm uses batch statistics and the running statistics are updated, also under no_grad; the
        Dropout masks are a pure function of (`dropout_seed`, `dropout_call`, rank, site, row, element), and `dropout_call`
        moves on by one.  Raises where the kernels do not apply.  Not chunked by `max_workspace_bytes`: the batch statistics
        and the backward need every stage output of the whole batch."""
        from ._train_boundary import commit_running_stats, train_engine
        from .kuleshov_training import SITES, KuleshovFunction, KuleshovTrainEngine
        if not self.training:
            raise NotImplementedError("Kuleshov: train_route='kernels' serves train mode only (batch statistics, Dropout); "
                                      'eval-mode calls take the inference kernels or forward_aten')
        self._check_kernels(x)
        N = int(x.shape[0])
        u0 = chain_lengths(self.input_length)['up'][0]
        if N * u0 == 1:                                     # torch's BatchNorm check, word for word, before anything is touched
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size([N, 1024, u0])}')
        ps = [float(getattr(self, name).p) for name in SITES]
        for name, p in zip(SITES, ps):
            if not 0.0 <= p < 1.0:
                raise ValueError(f'Kuleshov: the gfx950 kernels need a Dropout p in [0, 1) (got {name}.p = {p})')
        bns = self._batch_norms()
        if any(bn.momentum is None or not bn.track_running_stats or not bn.affine for bn in bns):
            raise NotImplementedError('Kuleshov: the gfx950 training kernels need affine BatchNorm layers with a momentum and '
                                      'running statistics')
        if self.dropout_seed is None:
            self.dropout_seed = int(torch.initial_seed())
        engine = train_engine(self, str(x.device), lambda: KuleshovTrainEngine(x.device, self.input_length, self.output_length))
        engine.eps = float(bns[0].eps)
        engine.momentum = [float(bn.momentum) for bn in bns]
        engine.running = [(bn.running_mean, bn.running_var) for bn in bns]
        engine.seed, engine.call, engine.p = int(self.dropout_seed), int(self.dropout_call), ps
        engine.rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        names, params = zip(*self.named_parameters())
        y = KuleshovFunction.apply(x, engine, names, *params)
        if N:
            commit_running_stats(bns, engine.new_running)
        self.dropout_call = int(self.dropout_call) + 1
        return y

    def forward(self, x):
        route = self.train_route
        if route not in ('aten', 'kernels'):
            raise ValueError(f"Kuleshov.train_route must be 'aten' or 'kernels' (got {route!r})")
        if route == 'kernels' and self.training:
            return self.forward_train_kernels(x)
        return super().forward(x)

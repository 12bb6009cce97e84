"""Training augmentation on the device: the reference's NormalizeVol -> CropChannelData -> AddNoise chain
(utils/transforms.py, put in front of every training sample at main.py:49,54,82) for a whole batch of rows in one
launch of csrc/augment.hip.  The reference does this per sample in numpy inside DataLoader workers.

Random numbers come from a counter-based generator (Philox4x32-10, layout in include/stofnet_amd.h): a draw is a
function of (seed, rank, call, stream, row, sample) only, so a run is reproducible and resumable and ranks never share
noise.  `noise=` and `shift=` replace the generator's draws; they are the hooks that make parity with the reference
testable."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib


def crop_width(L: int, crop_ratio) -> int:
    """Width of the crop window (Python's round: half to even); L when the ratio switches the crop off."""
    if crop_ratio is None or not (0 < crop_ratio < 1):
        return int(L)
    return int(round(L * float(crop_ratio)))


def _rows(x: torch.Tensor):
    _lib.require_device(x, 'x')
    if x.dtype != torch.float32:
        raise TypeError(f'x must be float32, got {x.dtype}')
    if x.dim() == 3 and x.shape[1] == 1:
        return x.reshape(x.shape[0], x.shape[2]).contiguous()
    if x.dim() == 2:
        return x.contiguous()
    raise RuntimeError(f'x must be [N, L] or [N, 1, L], got {tuple(x.shape)}')


def augment(x, gt=None, *, snr_db=None, crop_ratio=None, normalize=False, seed=0, rank=0, call=0, noise=None, shift=None):
    """x [N, L] or [N, 1, L] float32 on a ROCm device, gt [N] or [N, G] -> (y like x, gt_out like gt or None, start [N] int32).

    normalize: x / max|x| per row.  crop_ratio in (0, 1): a window of round(L * ratio) samples around gt[:, 0], moved by a
    random shift, zero padded back to L; gt moves with it.  snr_db: uniform noise at that signal-to-noise ratio.  None (or
    a ratio outside (0, 1)) leaves a stage out.  noise [N, L] / [N, 1, L] (uniforms in [0, 1)) and shift [N] int32 replace
    the generator's draws.  An odd window width raises ValueError, as the reference asserts on it."""
    rows = _rows(x)
    n, L = rows.shape
    dev = rows.device
    if snr_db is not None and not math.isfinite(float(snr_db)):
        raise ValueError(f'snr_db must be finite, got {snr_db}')
    crop = crop_ratio is not None and 0 < crop_ratio < 1
    width = crop_width(L, crop_ratio)
    if crop and width % 2:
        raise ValueError(f'CropChannelData: L = {L} with ratio = {crop_ratio} gives an odd window width {width}; '
                         'the reference asserts on every such window')
    g2 = None
    if gt is not None:
        _lib.require_device(gt, 'gt')
        cols = 1 if gt.dim() <= 1 else math.prod(gt.shape[1:])          # (an empty batch cannot infer them)
        g2 = gt.to(torch.float32).reshape(n, cols).contiguous()
    elif crop:
        raise ValueError('a crop needs gt: the window is placed around gt[:, 0]')
    G = 0 if g2 is None else g2.shape[1]
    if noise is not None:
        noise = _rows(noise)
        if noise.shape != rows.shape:
            raise RuntimeError(f'noise must have the shape of x, got {tuple(noise.shape)}')
    if shift is not None:
        shift = _lib.require_device(shift, 'shift').to(torch.int32).reshape(n).contiguous()
    y = torch.empty_like(rows)
    gt_out = torch.empty_like(g2) if g2 is not None else None
    start = torch.zeros(n, dtype=torch.int32, device=dev)
    if rows.numel() == 0:                                               # nothing to launch (empty tensors have no address)
        return y.reshape(x.shape), (gt.clone() if gt is not None else None), start
    desc = _lib.AugmentDesc(int(seed) & (2 ** 64 - 1), float(crop_ratio) if crop else 0.0,
                            float(snr_db) if snr_db is not None else 0.0, 1 if normalize else 0,
                            0 if snr_db is None else 1, int(rank), int(call) & 0xffffffff)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().stof_augment(ctypes.byref(desc), _lib.ptr(rows), _lib.ptr(g2), n, L, G, _lib.ptr(noise),
                                           _lib.ptr(shift), _lib.ptr(y), _lib.ptr(gt_out), _lib.ptr(start),
                                           _lib.stream_ptr(dev)), 'stof_augment')
    return y.reshape(x.shape), (gt_out.reshape(gt.shape) if gt is not None else None), start


def device_uniforms(seed, rank, call, stream_id, N, L, device='cuda'):
    """float32 [N, L]: the uniforms the generator hands to `augment` for (seed, rank, call); stream 0 = noise, stream 1 =
    crop shift (sample 0 of each row carries the word the shift is drawn from)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'device_uniforms runs on a ROCm device only, got {dev}')
    out = torch.empty((int(N), int(L)), dtype=torch.float32, device=dev)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().stof_augment_uniforms(int(seed) & (2 ** 64 - 1), int(rank), int(call) & 0xffffffff, int(stream_id),
                                                    _lib.ptr(out), int(N), int(L), _lib.stream_ptr(out.device)),
                   'stof_augment_uniforms')
    return out


class Augment(torch.nn.Module):
    """The training chain as one module: forward(x, gt=None) -> (y, gt_out, start).  Every call uses the next `call`
    value of the generator, so step k of a run draws the same numbers whenever the run is repeated."""

    def __init__(self, snr_db=None, crop_ratio=None, normalize=False, seed=0, rank=0):
        super().__init__()
        self.snr_db, self.crop_ratio, self.normalize = snr_db, crop_ratio, bool(normalize)
        self.seed, self.rank = int(seed), int(rank)
        self.calls = 0

    def forward(self, x, gt=None):
        out = augment(x, gt, snr_db=self.snr_db, crop_ratio=self.crop_ratio, normalize=self.normalize, seed=self.seed,
                      rank=self.rank, call=self.calls)
        self.calls += 1
        return out

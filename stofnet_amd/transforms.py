"""The reference's `utils/transforms.py` classes (NormalizeVol, AddNoise, CropChannelData) with two routes:

  * a batch of rows on a ROCm device ([N, L] or [N, 1, L] float32) goes to the augmentation kernel (stofnet_amd/augment.py),
    every row treated as the chirp dataset treats its 1-D sample;
  * a numpy array or CPU tensor, one sample at a time, takes a plain numpy path that never touches the GPU (DataLoader
    workers call it).  It draws from `numpy.random` (and `torch.rand` for `ratio=None`) in the reference's order, so a
    seeded run reproduces the reference's numbers and its exceptions.

Constructor and `forward(waveform, *args, **kwargs)` signatures and the return conventions are the reference's: the
transformed sample alone when nothing else was passed, else a tuple with the extra positional arguments and the keyword
NAMES appended (CropChannelData always returns a tuple).  On the device the modules draw from the kernel's generator with
seed = torch.initial_seed(), rank = $RANK and one `call` per forward of the module instance."""
from __future__ import annotations

import os

import numpy as np
import torch

from .augment import augment


def _on_device(t) -> bool:
    return isinstance(t, torch.Tensor) and t.device.type == 'cuda'


def _as_numpy(t):
    """(ndarray, back): CPU tensors are handled as numpy arrays and converted back."""
    if isinstance(t, torch.Tensor):
        return t.detach().numpy(), lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return t, lambda a: a


def _returns(first, args, kwargs):
    if len(args) == 0 and len(kwargs) == 0:
        return first
    return (first, *args, *kwargs)


class _DeviceDraws(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._calls = 0

    def _coords(self):
        call = self._calls
        self._calls += 1
        return {'seed': torch.initial_seed(), 'rank': int(os.environ.get('RANK', '0')), 'call': call}


class NormalizeVol(torch.nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, waveform, *args, **kwargs):
        if _on_device(waveform):
            norm = augment(waveform, normalize=True)[0]
        else:
            norm = waveform / abs(waveform).max()
        return _returns(norm, args, kwargs)


class AddNoise(_DeviceDraws):
    def __init__(self, snr=40):
        super().__init__()
        self.snr = snr

    def forward(self, waveform, *args, **kwargs):
        if _on_device(waveform):
            return _returns(augment(waveform, snr_db=self.snr, **self._coords())[0], args, kwargs)
        w, back = _as_numpy(waveform)
        u = np.random.rand(*w.shape)
        noise = 2 * (u - .5) if (w < 0).any() else u
        # builtin sums, as in the reference: sequential float64 over a 1-D sample
        gain = (10 ** (-self.snr / 10) * (sum(w ** 2) / sum(noise ** 2))) ** .5
        return _returns(back(w + noise * gain), args, kwargs)


class CropChannelData(_DeviceDraws):
    def __init__(self, ratio: float = None, resize: bool = False):
        super().__init__()
        self.ratio = ratio
        self.resize = resize

    @staticmethod
    def upscale_1d(data, rescale_factor):
        """Linear interpolation of `data`, placed on an endpoint-inclusive grid over [0, size], at int(size * factor) points."""
        x = np.linspace(0, data.size, num=data.size, endpoint=True)
        t = np.linspace(0, data.size, num=int(data.size * rescale_factor), endpoint=True)
        return np.interp(t, x, data)

    def forward(self, waveform, gt, *args, **kwargs):
        if self.ratio is None:
            self.ratio = float(torch.rand(1))              # drawn once, then kept (as the reference does)
        if not (0 < self.ratio < 1):
            return (waveform, gt, *args, *kwargs)
        if _on_device(waveform):
            if self.resize:
                raise NotImplementedError('CropChannelData(resize=True) has no device kernel; use the numpy path')
            if not isinstance(gt, torch.Tensor):
                gt = torch.as_tensor(gt, dtype=torch.float32)
            y, gt_out, _ = augment(waveform, gt.to(waveform.device), crop_ratio=self.ratio, **self._coords())
            return (y, gt_out, *args, *kwargs)

        w, back = _as_numpy(waveform)
        size = w.size
        width = int(round(size * self.ratio))
        ref = int(round(gt))
        half = width // 2
        start, end = max(0, ref - half), min(ref + half, size)
        if end == size:
            start = end - width
        if start == 0:
            end = width
        reach = min(ref - start, end - ref) // 2           # the window keeps the reference sample inside
        shift = np.random.randint(-min(start, reach), min(size - end, reach))      # raises on an empty range
        start, end = start + shift, end + shift
        cropped = w[start:end]
        gt = gt - start
        assert cropped.size == width
        if self.resize:
            factor = size / cropped.size
            cropped = self.upscale_1d(cropped, factor)
            gt = gt * factor
        else:
            cropped = np.pad(cropped, (0, size - cropped.size), mode='constant')
        assert cropped.size == size
        return (back(cropped), gt, *args, *kwargs)

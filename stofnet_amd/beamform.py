"""Plane-wave delay-and-sum beamforming, the reference's `utils/beamform.py` (bf_das, bf_das_rx), on two routes:

  * torch tensors on a ROCm device, `[..., A, S, Ne]` (`bf_das`) or `[..., S, Ne]` (`bf_das_rx`) with any leading batch
    dimensions, go to the kernels of csrc/beamform.hip: one launch beamforms the whole batch, two more make the B-mode;
  * numpy arrays go to the library's host entry (the same arithmetic, plain loops) and never touch a GPU.

A CPU torch tensor raises: this package has no torch fallback.  float32, float64, complex64 and complex128 are served; the
result has the input's dtype (the B-mode its real type).

Semantics are the reference's, stated in include/stofnet_amd.h.  Deliberate differences:
  * zero-magnitude pixels (outside every receive cone or sample range) take the smallest finite B-mode value of their
    frame; the reference leaves them uninitialised (`np.log10(..., where=)` without `out=`) and means this value;
  * a frame without any finite non-zero pixel gives a B-mode of zeros; the reference raises on its empty minimum;
  * `compound_opt=False` returns one plane per angle for any number of angles; the reference hard-codes 3;
  * a term at sample index exactly S - 1 is kept with the weight 0 on row S, which is not read; the reference indexes out
    of range there;
  * the IQ phase rotation is decided per (frame, angle, channel): the channel is rotated iff its column of `sig` has a
    non-zero imaginary part anywhere.  The reference decides on the values it gathered, so a complex-typed array holding
    real data gives exactly the real-input result on both; the two differ only for a column whose imaginary parts sit
    solely at samples that no pixel addresses (the reference would not rotate it).
`param` is any mapping or attribute object (keys are read by item access, then by attribute); it is not modified."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

_NP_DTYPES = {np.dtype(np.float32): _lib.DAS_F32, np.dtype(np.float64): _lib.DAS_F64,
              np.dtype(np.complex64): _lib.DAS_C64, np.dtype(np.complex128): _lib.DAS_C128}
_TORCH_DTYPES = {torch.float32: _lib.DAS_F32, torch.float64: _lib.DAS_F64, torch.complex64: _lib.DAS_C64,
                 torch.complex128: _lib.DAS_C128}
_REAL_OF = {torch.float32: torch.float32, torch.float64: torch.float64, torch.complex64: torch.float32,
            torch.complex128: torch.float64}


def _get(param, key):
    try:
        return param[key]
    except (KeyError, TypeError, IndexError):
        return getattr(param, key)


def _f64(a, name):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if not np.isfinite(a).all():
        raise ValueError(f'{name} must be finite')
    return a


def _scalar(param, key):
    v = float(_get(param, key))
    if not math.isfinite(v):
        raise ValueError(f'param.{key} must be finite, got {v}')
    return v


def _dptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class _Geometry:
    """Everything that does not depend on the signal: the pixel list, the elements, the transmit distances."""

    def __init__(self, param, angles, xflat, zflat, fnumber):
        fnumber = float(fnumber)
        if not math.isfinite(fnumber):
            raise ValueError(f'fnumber must be finite, got {fnumber}')
        xe_all = _f64(_get(param, 'xe'), 'param.xe').reshape(-1)
        self.ne = int(_get(param, 'Nelements'))
        if not 1 <= self.ne <= xe_all.size:
            raise ValueError(f'param.Nelements = {self.ne} with {xe_all.size} element positions')
        self.xe = np.ascontiguousarray(xe_all[:self.ne])
        self.angles = _f64(angles, 'the transmit angles').reshape(-1)
        self.x, self.z = _f64(xflat, 'x'), _f64(zflat, 'z')
        self.p = self.x.size
        self.consts = [_scalar(param, k) for k in ('c', 't0', 'fs', 'f0')] + [fnumber]
        self.dtx = np.empty((self.angles.size, self.p), np.float64)
        if self.dtx.size:
            _lib.check(_lib.lib().stof_das_tx_distance(_dptr(xe_all), xe_all.size, _dptr(self.angles), self.angles.size,
                                                       _dptr(self.x), _dptr(self.z), self.p, _dptr(self.dtx)), 'stof_das_tx_distance')
        self._on = {}

    def on(self, dev):
        """x, z, dtx, xe as device tensors (uploaded once per device)."""
        if dev not in self._on:
            self._on[dev] = tuple(torch.from_numpy(a).to(dev) for a in (self.x, self.z, self.dtx, self.xe))
        return self._on[dev]

    def desc(self, dtype_code, compound):
        return _lib.DasDesc(*self.consts, dtype_code, 1 if compound else 0)


def _beamform(sig, geo, compound):
    """sig [..., A, S, Ne'] (Ne' >= Nelements) -> [..., P] (compound) or [..., A, P], same kind of array."""
    if isinstance(sig, torch.Tensor):
        _lib.require_device(sig, 'sig')
        code = _TORCH_DTYPES.get(sig.dtype)
    elif isinstance(sig, np.ndarray):
        code = _NP_DTYPES.get(sig.dtype)
    else:
        raise TypeError(f'sig must be a numpy array or a torch tensor, got {type(sig).__name__}')
    if code is None:
        raise TypeError(f'sig must be float32, float64, complex64 or complex128, got {sig.dtype}')
    if sig.ndim < 3:
        raise ValueError(f'sig must be [..., angles, samples, channels], got {tuple(sig.shape)}')
    lead, (A, S, ne_in) = tuple(sig.shape[:-3]), sig.shape[-3:]
    if A != geo.angles.size:
        raise ValueError(f'sig has {A} angles, the geometry {geo.angles.size}')
    if ne_in < geo.ne:
        raise ValueError(f'sig has {ne_in} channels, param.Nelements = {geo.ne}')
    F = math.prod(lead)
    out_shape = lead + ((geo.p,) if compound else (A, geo.p))
    desc = geo.desc(code, compound)
    cplx = code in (_lib.DAS_C64, _lib.DAS_C128)
    if isinstance(sig, np.ndarray):
        s4 = np.ascontiguousarray(sig[..., :geo.ne]).reshape(F, A, S, geo.ne)
        rot = np.ascontiguousarray((s4.imag != 0).any(axis=2).astype(np.uint8)) if cplx else None
        out = np.zeros(out_shape, sig.dtype)
        if out.size:
            _lib.check(_lib.lib().stof_das_beamform_host(ctypes.byref(desc), _dptr(s4), F, A, S, geo.ne, _dptr(geo.x), _dptr(geo.z),
                                                         _dptr(geo.dtx), geo.p, _dptr(geo.xe), None if rot is None else _dptr(rot),
                                                         _dptr(out)), 'stof_das_beamform_host')
        return out
    dev = sig.device
    s4 = sig[..., :geo.ne].contiguous().reshape(F, A, S, geo.ne)
    rot = (s4.imag != 0).any(dim=2).to(torch.uint8).contiguous() if cplx else None
    out = torch.empty(out_shape, dtype=sig.dtype, device=dev)      # the entry writes every value
    if out.numel():
        x, z, dtx, xe = geo.on(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().stof_das_beamform(ctypes.byref(desc), _lib.ptr(s4), F, A, S, geo.ne, _lib.ptr(x), _lib.ptr(z),
                                                    _lib.ptr(dtx), geo.p, _lib.ptr(xe), _lib.ptr(rot), _lib.ptr(out),
                                                    _lib.stream_ptr(dev)), 'stof_das_beamform')
    return out


def _bmode(img, frame_dims):
    """20 log10 |img|, normalised per frame; the last `frame_dims` dimensions of img form one frame."""
    lead = tuple(img.shape[:img.ndim - frame_dims])
    F, n = math.prod(lead), math.prod(img.shape[img.ndim - frame_dims:])
    if isinstance(img, np.ndarray):
        mag = np.abs(img).reshape(F, n)
        out = np.zeros_like(mag)
        with np.errstate(divide='ignore', invalid='ignore'):
            lg = 20 * np.log10(mag)
        for f in range(F):
            ok = np.isfinite(lg[f])
            if ok.any():
                row = np.where(ok, lg[f], lg[f][ok].min())
                out[f] = row - row.max()
        return out.reshape(img.shape)
    out = torch.zeros(img.shape, dtype=_REAL_OF[img.dtype], device=img.device)
    if out.numel():
        src = img.contiguous()
        nbytes = _lib.lib().stof_das_workspace_bytes(F, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        with torch.cuda.device(img.device):
            _lib.check(_lib.lib().stof_das_bmode(_TORCH_DTYPES[img.dtype], _lib.ptr(src), F, n, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                                 _lib.stream_ptr(img.device)), 'stof_das_bmode')
    return out


def _swap_last(a):
    return a.transpose(-1, -2) if isinstance(a, torch.Tensor) else np.swapaxes(a, -1, -2)


def bf_das(rf_iq, param, compound_opt=True, fnumber=1.9, return_iq=False):
    """rf_iq [..., A, S, Ne] -> B-mode [..., Nz, Nx] (compound_opt) or [..., A, Nz, Nx] in dB, 0 at the frame's maximum.
    return_iq: the summed image before the logarithm, in the input's dtype."""
    px = _f64(_get(param, 'param_x'), 'param.param_x').reshape(-1)
    pz = _f64(_get(param, 'param_z'), 'param.param_z').reshape(-1)
    geo = _Geometry(param, _get(param, 'angles_list'), np.repeat(px, pz.size), np.tile(pz, px.size), fnumber)   # p = ix Nz + iz
    flat = _beamform(rf_iq, geo, bool(compound_opt))
    img = _swap_last(flat.reshape(tuple(flat.shape[:-1]) + (px.size, pz.size)))
    if return_iq:
        return img
    return _bmode(img, 2 if compound_opt else 3)


def bf_das_rx(sig, param, x, z, fnumber=1.9):
    """sig [..., S, Ne] of one transmit angle (param.theta), x and z 2-D arrays of one shape -> the delayed sum, shaped
    like x, in the input's dtype."""
    xa = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    za = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else np.asarray(z)
    if xa.ndim != 2 or xa.shape != za.shape:
        raise ValueError(f'x and z must be 2-D arrays of one shape, got {xa.shape} and {za.shape}')
    geo = _Geometry(param, [float(_get(param, 'theta'))], xa.T.reshape(-1), za.T.reshape(-1), fnumber)
    if sig.ndim < 2:
        raise ValueError(f'sig must be [..., samples, channels], got {tuple(sig.shape)}')
    flat = _beamform(sig[..., None, :, :], geo, True)
    rows, cols = xa.shape
    return _swap_last(flat.reshape(tuple(flat.shape[:-1]) + (cols, rows)))

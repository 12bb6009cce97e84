"""Times of the delay-and-sum beamformer (csrc/beamform.hip through stofnet_amd/beamform.py) next to a restatement of the
same gather in stock torch ops on the same device, one JSON line per shape:

    python tools/time_beamform.py [--out profiles/beamform.jsonl]                  # on the GPU
    STOFNET_REFERENCE=<checkout> python tools/time_beamform.py --reference [--out ...]   # the reference's numpy time, no GPU

Shapes: Ne = 128, A = 3, S = 1024, complex64; one frame on an 84 x 143 grid, the same frame on a grid 8 x finer per axis,
64 frames on the coarse grid.
  kernels_ms / stock_ms   medians of 5 windows of 3 calls between two HIP events, the two routes alternated
                          (tools/_train_timing.py).  Both routes get the geometry prepared: ours the pixel list and the
                          transmit distances on the device (its kernel still derives every delay, mask, weight and phase),
                          the stock route its sample indices, weights, masks and phases as tensors, so that it times the
                          gather, the interpolation, the rotation and the sum alone.
  hbm_fraction            (F A S Ne element bytes + output bytes) / kernels time / 8 TB/s
  max_rel_diff            max |ours - stock| / max |stock| on the timed inputs
  bmode_ms                the two B-mode launches on the summed image
`reference_numpy` lines: the reference's bf_das on one CPU, once per shape (one frame timed, scaled by the frame count).
Lines of other kinds that --out already holds stay."""
import argparse
import importlib.util
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM = 8e12
C, F0, FS, T0 = 1540.0, 5e6, 20e6, 2e-6
NE, A, S = 128, 3, 1024
SHAPES = [('one frame, 84 x 143', 1, 84, 143), ('one frame, 672 x 1144', 1, 672, 1144), ('64 frames, 84 x 143', 64, 84, 143)]


def param(nx, nz):
    lam = C / F0
    xe = (np.arange(NE) - (NE - 1) / 2) * lam
    depth = (T0 + S / FS) * C / 2
    return {'param_x': np.linspace(xe[0], xe[-1], nx), 'param_z': np.linspace(2e-3, 0.95 * depth, nz),
            'angles_list': np.deg2rad(np.linspace(-5.0, 5.0, A)), 'xe': xe, 'Nelements': NE, 'c': C, 't0': T0, 'fs': FS, 'f0': F0}


def signal(frames):
    rng = np.random.default_rng(5)
    shape = (frames, A, S, NE)
    return (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)


def keep_other(out, kind, lines):
    kept = []
    if os.path.exists(out):
        with open(out) as fh:
            kept = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != kind]
    with open(out, 'w') as fh:
        fh.write('\n'.join(kept + [json.dumps(rec) for rec in lines]) + '\n')


def reference_lines():
    class Param(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__
    spec = importlib.util.spec_from_file_location('reference_beamform', os.path.join(os.environ['STOFNET_REFERENCE'], 'utils', 'beamform.py'))
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    sig = signal(1)[0]
    lines = []
    for name, frames, nx, nz in SHAPES:
        tic = time.perf_counter()
        with np.errstate(all='ignore'):
            rb.bf_das(sig, Param(param(nx, nz)))
        sec = time.perf_counter() - tic
        lines.append({'kind': 'reference_numpy', 'shape': name, 'frames': frames, 'grid': [nx, nz], 'dtype': 'complex64',
                      'seconds_per_frame': round(sec, 3), 'seconds': round(sec * frames, 2), 'where': 'host CPU, one process'})
        print(json.dumps(lines[-1]), flush=True)
    return lines


def stock_route(sig, geo, dev):
    """-> fn(): the compounded sum [F, P] in stock torch ops, geometry prepared as tensors"""
    import torch
    x, z, dtx, xe = geo.on(dev)
    c, t0, fs, f0, fnum = geo.consts
    F, P = sig.shape[0], geo.p
    drx = torch.hypot(x[:, None] - xe[None], z[:, None].expand(P, NE))
    cone = (x[:, None] - xe[None]).abs() < (z / fnum / 2)[:, None]
    cols = torch.arange(NE, device=dev)[None]
    prep = []
    for a in range(A):
        tau = (dtx[a][:, None] + drx) / c
        i = (tau - t0) * fs
        ok = (i >= 1) & (i <= S - 1) & cone
        i = torch.where(ok, i, torch.ones_like(i))
        fl = torch.floor(i)
        cyc = f0 * tau
        cyc = cyc - torch.floor(cyc)
        rot = torch.polar(ok.to(torch.float32), (2 * math.pi * cyc).to(torch.float32))        # the masks folded into the phase
        i0 = (fl.long() * NE + cols).reshape(-1)
        i1 = (torch.clamp(fl.long() + 1, max=S - 1) * NE + cols).reshape(-1)
        prep.append((i0, i1, (fl + 1 - i).to(torch.float32), (i - fl).to(torch.float32), rot))

    def fn():
        out = torch.zeros((F, P), dtype=sig.dtype, device=dev)
        for a, (i0, i1, w0, w1, rot) in enumerate(prep):
            flat = sig[:, a].reshape(F, S * NE)
            term = flat[:, i0].reshape(F, P, NE) * w0 + flat[:, i1].reshape(F, P, NE) * w1
            out += (term * rot).sum(-1)
        return out
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reference', action='store_true', help="time the reference's numpy route on the host instead (no GPU)")
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    if a.reference:
        lines = reference_lines()
        if a.out:
            keep_other(a.out, 'reference_numpy', lines)
        return
    import torch
    from _train_timing import alternate, gpu_ms
    from stofnet_amd import beamform as bf
    dev = torch.device('cuda:0')
    lines = []
    for name, frames, nx, nz in SHAPES:
        p = param(nx, nz)
        geo = bf._Geometry(p, p['angles_list'], np.repeat(p['param_x'], nz), np.tile(p['param_z'], nx), 1.9)
        sig = torch.from_numpy(signal(frames)).to(dev)
        ours = lambda: bf._beamform(sig, geo, True)          # noqa: E731
        stock = stock_route(sig, geo, dev)
        img, ref = ours(), stock()
        diff = float((img - ref).abs().max() / ref.abs().max())
        mo, so, ms, ss = alternate(ours, stock, a.iters, a.repeats)
        bm = gpu_ms(lambda: bf._bmode(img.reshape(frames, nx, nz), 2), a.iters * a.repeats)
        nbytes = 8 * (frames * A * S * NE + frames * geo.p)
        rec = {'kind': 'timing', 'shape': name, 'frames': frames, 'grid': [nx, nz], 'Ne': NE, 'A': A, 'S': S, 'dtype': 'complex64',
               'kernels_ms': round(mo, 4), 'kernels_spread': round(so, 3), 'stock_ms': round(ms, 4), 'stock_spread': round(ss, 3),
               'stock_over_kernels': round(ms / mo, 2), 'hbm_fraction': round(nbytes / (mo * 1e-3) / HBM, 5),
               'min_bytes_MB': round(nbytes / 1e6, 2), 'max_rel_diff': float(f'{diff:.3e}'), 'bmode_ms': round(bm, 4),
               'iters': a.iters, 'repeats': a.repeats}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del stock, sig, img, ref
        torch.cuda.empty_cache()
    if a.out:
        keep_other(a.out, 'timing', lines)


if __name__ == '__main__':
    main()

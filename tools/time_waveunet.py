"""Times of WaveUnet(n, 16) on the gfx950 kernels of csrc/waveunet.hip next to the same module's `forward_aten` (stock
ATen / MIOpen convolutions, BatchNorm, interpolate and cat) on the same GPU in one process, one JSON line per shape:

    python tools/time_waveunet.py [--out profiles/waveunet.jsonl] [--iters 3] [--repeats 5]

  ours_ms           forward_kernels, HIP events on the launch stream (packing cached, workspace from the caching
                    allocator); the median of --repeats timings of --iters calls, each alternated with a stock timing
  stock_gpu_ms      forward_aten (eval mode), measured the same way in the same call
  ours_spread / stock_spread   (max - min) / median over the repeats
  waveforms_per_s   rows / ours_ms
  peak_fraction     algorithmic FLOPs (2 x the reference's convolution MACs) / ours_ms / 157.3 TFLOP/s (fp32 MFMA peak)
  max_rel_diff      max |ours - stock_gpu| / max |stock_gpu|
--shape n,N,L restricts the run to one shape.  A `parity` line that tests/test_gpu_waveunet.py left in --out is kept."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import WaveUnet  # noqa: E402
import waveunet_inputs as wi  # noqa: E402

PEAK = 157.3e12
SHAPES = [(2, 4096, 8000), (2, 4, 8000), (10, 256, 8192)]        # (n_layers, N, L)


def macs_per_row(n, L):
    """convolution MACs of one waveform: every block at its own length, plus the 17 -> 1 output convolution"""
    total = 17 * L
    for i, (_, _, co, ci, k) in enumerate(wi.block_names(n)):
        level = i if i < n else (n if i == n else 2 * n - i)             # encoder i | middle | decoder i - n - 1
        total += co * ci * k * (L >> level)
    return total


def gpu_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shape', default=None, help='n,N,L: time this shape only')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    shapes = [tuple(int(v) for v in a.shape.split(','))] if a.shape else SHAPES
    lines = []
    for n, N, L in shapes:
        m = WaveUnet(n, 16)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in wi.seeded_waveunet(n, 800 + n).items()}, strict=True)
        m = m.to(dev).eval()
        x = torch.from_numpy(wi.frames(N, L, 1)).to(dev)
        with torch.no_grad():
            y = m.forward_kernels(x)
            ys = m.forward_aten(x)
            diff = float((y - ys).abs().max() / ys.abs().max())
            del y, ys
            m.forward_kernels(x)                                         # warm-up of both routes (MIOpen picks its solvers)
            m.forward_aten(x)
            torch.cuda.synchronize()
            ours, stock = [], []
            for _ in range(a.repeats):                                   # alternate, so that drift hits both alike
                ours.append(gpu_ms(lambda: m.forward_kernels(x), a.iters))
                stock.append(gpu_ms(lambda: m.forward_aten(x), a.iters))
        t_ours, t_stock = statistics.median(ours), statistics.median(stock)
        fl = 2 * macs_per_row(n, L) * N
        rec = {'kind': 'timing', 'model': 'unet', 'n_layers': n, 'shape': [N, 1, L], 'ours_ms': round(t_ours, 4),
               'stock_gpu_ms': round(t_stock, 4), 'ours_spread': round((max(ours) - min(ours)) / t_ours, 4),
               'stock_spread': round((max(stock) - min(stock)) / t_stock, 4),
               'speedup_vs_stock_gpu': round(t_stock / t_ours, 3), 'waveforms_per_s': round(N / t_ours * 1000.0, 1),
               'tflop': round(fl / 1e12, 4), 'peak_fraction': round(fl / (t_ours * 1e-3) / PEAK, 4), 'max_rel_diff': diff,
               'repeats': a.repeats, 'iters': a.iters}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, m
        torch.cuda.empty_cache()
    if a.out:
        keep = []
        if os.path.exists(a.out):
            with open(a.out) as fh:
                keep = [json.loads(ln) for ln in fh.read().splitlines() if ln.strip()]
            keep = [k for k in keep if k.get('kind') == 'parity']
        with open(a.out, 'w') as fh:
            for rec in lines + keep:
                fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

"""Times of EDSR_1D(1, 64, 8, 4) and ESPCN_1D(4) on the gfx950 kernels of csrc/riders.hip next to the same module's
`forward_aten` (stock ATen / MIOpen convolutions + the SampleShuffle1D kernel: what `forward` ran before the kernels
existed) on the same GPU, one JSON line per (model, shape):

    python tools/time_riders.py [--out profiles/riders.jsonl] [--iters 5] [--repeats 5]

  ours_ms           forward_kernels, HIP events on the launch stream (packing cached, workspace from the caching
                    allocator); the median of --repeats timings of --iters calls, each alternated with a stock timing
  stock_gpu_ms      forward_aten, measured the same way in the same call
  ours_spread / stock_spread   (max - min) / median over the repeats
  waveforms_per_s   rows / ours_ms
  peak_fraction     algorithmic FLOPs (2 x the reference's MACs) / ours_ms / 157.3 TFLOP/s (fp32 MFMA peak)
  max_rel_diff      max |ours - stock_gpu| / max |stock_gpu|
--only edsr|espcn and --shape N,L restrict the run (a rocprofv3 --kernel-trace --stats run of one shape gives the
per-kernel times of profiles/riders_kernels.json).  A `parity` line that tests/test_gpu_riders.py left in --out is kept."""
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
from stofnet_amd import EDSR_1D, ESPCN_1D  # noqa: E402
import riders_inputs as ri  # noqa: E402

PEAK = 157.3e12
SHAPES = [(4096, 2000), (4, 2000), (256, 20000)]
R = 4
MACS_PER_SAMPLE = {'edsr': 64 * 3 + 17 * 64 * 64 * 3 + R * (64 // R) * 3, 'espcn': 64 * 5 + 32 * 64 * 3 + R * 32 * 3}
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def gpu_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def build(which, dev):
    key = 'proud-cherry' if which == 'edsr' else 'vital-puddle'
    sd = np.load(os.path.join(GOLDEN, f'weights_{key}.npz'))
    m = EDSR_1D(1, 64, 8, R) if which == 'edsr' else ESPCN_1D(R)
    m.load_state_dict({k: torch.from_numpy(sd[k]) for k in sd.files}, strict=True)
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', choices=('edsr', 'espcn'), default=None)
    ap.add_argument('--shape', default=None, help='N,L: time this shape only')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    shapes = [tuple(int(v) for v in a.shape.split(','))] if a.shape else SHAPES
    lines = []
    for which in ('edsr', 'espcn'):
        if a.only and which != a.only:
            continue
        m = build(which, dev)
        for n, L in shapes:
            x = torch.from_numpy(ri.frames(n, L, 1)).to(dev)
            with torch.no_grad():
                y = m.forward_kernels(x)
                ys = m.forward_aten(x)
                diff = float((y - ys).abs().max() / ys.abs().max())
                del y, ys
                m.forward_kernels(x)                                     # warm-up of both routes (MIOpen picks its solvers)
                m.forward_aten(x)
                torch.cuda.synchronize()
                ours, stock = [], []
                for _ in range(a.repeats):                               # alternate, so that drift hits both alike
                    ours.append(gpu_ms(lambda: m.forward_kernels(x), a.iters))
                    stock.append(gpu_ms(lambda: m.forward_aten(x), a.iters))
            t_ours, t_stock = statistics.median(ours), statistics.median(stock)
            fl = 2 * MACS_PER_SAMPLE[which] * n * L
            rec = {'kind': 'timing', 'model': which, 'r': R, 'shape': [n, 1, L], 'ours_ms': round(t_ours, 4),
                   'stock_gpu_ms': round(t_stock, 4), 'ours_spread': round((max(ours) - min(ours)) / t_ours, 4),
                   'stock_spread': round((max(stock) - min(stock)) / t_stock, 4),
                   'speedup_vs_stock_gpu': round(t_stock / t_ours, 3), 'waveforms_per_s': round(n / t_ours * 1000.0, 1),
                   'tflop': round(fl / 1e12, 4), 'peak_fraction': round(fl / (t_ours * 1e-3) / PEAK, 4), 'max_rel_diff': diff,
                   'repeats': a.repeats, 'iters': a.iters}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del x
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

"""Times of Kuleshov(L, O) on the gfx950 kernels of csrc/kuleshov.hip next to the same module's `forward_aten` (stock
ATen / MIOpen convolutions, BatchNorm, PixelShuffle, cat and Linear) on the same GPU in one process, one JSON line per shape:

    python tools/time_kuleshov.py [--out profiles/kuleshov.jsonl] [--iters 3] [--repeats 5]

  ours_ms           forward_kernels, HIP events on the launch stream (packing cached, workspace from the caching
                    allocator); the median of --repeats timings of --iters calls, each alternated with a stock timing
  stock_gpu_ms      forward_aten (eval mode), measured the same way in the same call
  ours_spread / stock_spread   (max - min) / median over the repeats
  waveforms_per_s   rows / ours_ms
  peak_fraction     algorithmic FLOPs (2 x the convolutions' and the Linear layer's MACs) / ours_ms / 157.3 TFLOP/s
  fc_ms, fc_weight_fraction_of_8TBs   (batches of at most 32 rows) the Linear layer's share of ours_ms, taken as the
                    difference to the same network with output_length 32 measured the same way, and the rate at which
                    that time streams the O x fc_dim fp32 weight, as a fraction of 8 TB/s
  max_rel_diff      max |ours - stock_gpu| / max |stock_gpu|
--shape N,L,O restricts the run to one shape.  A `parity` line that tests/test_gpu_kuleshov.py left in --out is kept."""
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
from stofnet_amd import Kuleshov  # noqa: E402
from stofnet_amd.kuleshov import chain_lengths  # noqa: E402
import kuleshov_inputs as ki  # noqa: E402

PEAK = 157.3e12
HBM = 8e12
SHAPES = [(256, 2000, 20000), (4, 2000, 20000)]        # (N, input_length, output_length)


def macs_per_row(L, O):
    """MACs of one waveform: every convolution at its own output length, plus the Linear layer"""
    d = chain_lengths(L)
    lengths = d['down'] + [d['bottleneck']] + d['up'] + [d['final']]
    return sum(co * ci * k * n for (_, _, co, ci, k), n in zip(ki.block_names(), lengths)) + d['fc_dim'] * O


def gpu_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def build(L, O, dev):
    """seeded convolutions and BatchNorm statistics; the Linear layer keeps torch's seeded default initialisation"""
    torch.manual_seed(0)
    m = Kuleshov(L, O)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in ki._seeded_convs(ki.WEIGHT_SEED).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert sorted(missing) == ['output_fc.bias', 'output_fc.weight'] and not unexpected
    return m.to(dev).eval()


def ours_ms(m, x, iters, repeats):
    m.forward_kernels(x)
    torch.cuda.synchronize()
    return statistics.median(gpu_ms(lambda: m.forward_kernels(x), iters) for _ in range(repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shape', default=None, help='N,L,O: time this shape only')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    shapes = [tuple(int(v) for v in a.shape.split(','))] if a.shape else SHAPES
    lines = []
    for N, L, O in shapes:
        m = build(L, O, dev)
        x = torch.from_numpy(ki.frames(N, L, 1)).to(dev)
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
        fl = 2 * macs_per_row(L, O) * N
        rec = {'kind': 'timing', 'model': 'kuleshov', 'shape': [N, 1, L], 'output_length': O, 'ours_ms': round(t_ours, 4),
               'stock_gpu_ms': round(t_stock, 4), 'ours_spread': round((max(ours) - min(ours)) / t_ours, 4),
               'stock_spread': round((max(stock) - min(stock)) / t_stock, 4),
               'speedup_vs_stock_gpu': round(t_stock / t_ours, 3), 'waveforms_per_s': round(N / t_ours * 1000.0, 1),
               'tflop': round(fl / 1e12, 4), 'peak_fraction': round(fl / (t_ours * 1e-3) / PEAK, 4), 'max_rel_diff': diff,
               'repeats': a.repeats, 'iters': a.iters}
        del m
        torch.cuda.empty_cache()
        if N <= 32:
            with torch.no_grad():
                t_small = ours_ms(build(L, 32, dev), x, a.iters, a.repeats)
            fc_ms = t_ours - t_small
            rec['fc_ms'] = round(fc_ms, 4)
            rec['fc_weight_fraction_of_8TBs'] = round(4.0 * O * chain_lengths(L)['fc_dim'] / (fc_ms * 1e-3) / HBM, 4) if fc_ms > 0 else None
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

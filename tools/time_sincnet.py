"""Times of the SincNet baseline on the gfx950 kernels next to the same network built from stock torch layers (MIOpen
on the same GPU) and on torch CPU, one JSON line per shape:

    python tools/time_sincnet.py [--out profiles/sincnet.jsonl] [--iters 10] [--cpu-iters 1]

  ours_ms         SincNet.forward, HIP events on the launch stream (packing cached, workspace from the caching allocator)
  stock_gpu_ms    the reference's forward on stock F.pad / F.conv1d (the sinc layer with the packer's filter bank) /
                  Conv1d / BatchNorm1d (eval) / LeakyReLU, same GPU, fp32
  cpu_ms          the same stock module on torch CPU (skipped above --cpu-max-rows rows)
  waveforms_per_s rows / ours_ms
  peak_fraction   algorithmic FLOPs (2 x the reference's MACs) / ours_ms / 157.3 TFLOP/s (fp32 MFMA peak)
  max_rel_diff    max |ours - stock_gpu| / max |stock_gpu|
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (profiles/sincnet_kernels.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import SincNet  # noqa: E402
import sincnet_inputs as si  # noqa: E402

PEAK = 157.3e12
SHAPES = [(4096, 2000, 1e6), (4, 2000, 1e6), (2048, 1536, 1.25e9), (64, 20000, 1e6)]
MACS_PER_SAMPLE = 128 * 1023 + 128 * 128 * 11 + 128 * 128 * 9 + 128 * 7


class Stock(nn.Module):
    """the reference's forward on stock layers (same state_dict names)"""

    def __init__(self, model):
        super().__init__()
        self.register_buffer('filters', model.conv[0].filters.clone())
        self.conv = nn.ModuleList([nn.Identity()] + [nn.Conv1d(128, c, k) for c, k in ((128, 11), (128, 9), (1, 7))])
        self.bn = nn.ModuleList([nn.BatchNorm1d(c, momentum=0.05) for c in (128, 128, 128, 1)])
        for i in range(1, 4):
            self.conv[i].load_state_dict(model.conv[i].state_dict())
        for i in range(4):
            self.bn[i].load_state_dict(model.bn[i].state_dict())

    def forward(self, x):
        x = x.view(x.shape[0], 1, x.shape[-1])
        for i, k in enumerate((1023, 11, 9, 7)):
            x = F.pad(x, ((k - 1) // 2, (k - 1) // 2))
            x = F.conv1d(x, self.filters) if i == 0 else self.conv[i](x)
            x = self.bn[i](x)
            if i < 3:
                x = F.leaky_relu(x, 0.2)
        return x


def gpu_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--cpu-iters', type=int, default=1)
    ap.add_argument('--cpu-max-rows', type=int, default=64)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in si.checkpoint_weights('pretty-brook').items()}
    lines = []
    for n, L, fs in SHAPES:
        ours = SincNet(si.options(fs, L))
        ours.load_state_dict(sd)
        ours = ours.to(dev).eval()
        stock = Stock(ours).eval()
        stock_dev = Stock(ours).to(dev).eval()
        x = torch.from_numpy(si.frames((n, 1, L), 1)).to(dev)
        with torch.no_grad():
            y, ys = ours(x), stock_dev(x)
            t_ours = gpu_ms(lambda: ours(x), a.iters)
            t_stock = gpu_ms(lambda: stock_dev(x), a.iters)
            t_cpu = None
            if not a.no_cpu and n <= a.cpu_max_rows:
                xc = x.cpu()
                stock(xc)
                tic = time.perf_counter()
                for _ in range(a.cpu_iters):
                    stock(xc)
                t_cpu = (time.perf_counter() - tic) * 1000.0 / a.cpu_iters
        fl = 2 * MACS_PER_SAMPLE * n * L
        rec = {'shape': [n, 1, L], 'fs': fs, 'ours_ms': round(t_ours, 4), 'stock_gpu_ms': round(t_stock, 4),
               'cpu_ms': None if t_cpu is None else round(t_cpu, 2), 'speedup_vs_stock_gpu': round(t_stock / t_ours, 3),
               'waveforms_per_s': round(n / t_ours * 1000.0, 1), 'tflop': round(fl / 1e12, 4),
               'peak_fraction': round(fl / (t_ours * 1e-3) / PEAK, 4),
               'max_rel_diff': float((y - ys).abs().max() / ys.abs().max())}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del ours, stock, stock_dev, x, y, ys
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

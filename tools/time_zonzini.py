"""Times of the Zonzini baselines on the gfx950 kernels next to the same network built from stock torch.nn layers
(MIOpen on the same GPU) and on torch CPU, one JSON line per shape:

    python tools/time_zonzini.py [--out profiles/zonzini.jsonl] [--iters 20] [--cpu-iters 2]

  ours_ms         ZonziniNet*.forward, HIP events on the launch stream (packing cached, workspace from the caching allocator)
  stock_gpu_ms    the reference's forward on stock Conv1d / ReLU / MaxPool1d / AdaptiveAvgPool1d / Linear, same GPU, fp32
  cpu_ms          the same stock module on torch CPU
  waveforms_per_s rows / ours_ms
  peak_fraction   algorithmic FLOPs (2 x the reference's MACs) / ours_ms / 157.3 TFLOP/s (fp32 MFMA / packed VALU peak)
  max_rel_diff    max |ours - stock_gpu| / max |stock_gpu|
Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (profiles/zonzini_kernels.json)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
from stofnet_amd import ZonziniNetLarge, ZonziniNetSmall  # noqa: E402
import zonzini_inputs as zi  # noqa: E402

PEAK = 157.3e12
SHAPES = [('small', 4096, 2000), ('small', 1, 2000), ('large', 256, 20000), ('large', 1024, 4000)]


class Stock(nn.Module):
    """the reference's forward on stock layers (same parameter names)"""

    def __init__(self, chans):
        super().__init__()
        self.conv_layers = nn.ModuleList()
        cin = 1
        for c in chans:
            self.conv_layers.append(nn.Conv1d(cin, c, kernel_size=10, stride=2))
            cin = c
        self.relu, self.maxpool, self.global_avgpool = nn.ReLU(), nn.MaxPool1d(2), nn.AdaptiveAvgPool1d(1)
        self.fc1, self.fc2 = nn.Linear(cin, 1024), nn.Linear(1024, 1)

    def forward(self, x):
        for conv in self.conv_layers:
            x = self.maxpool(self.relu(conv(x)))
        x = self.global_avgpool(x).view(x.size(0), -1)
        return self.fc2(self.relu(self.fc1(x)))


def flops(chans, L):
    """2 x MACs per row: convs (cout x cin x 10 per conv output), fc1, fc2"""
    f, cin, lin = 0, 1, L
    for c in chans:
        lc = (lin - 10) // 2 + 1
        f += 2 * lc * c * cin * 10
        lin, cin = lc // 2, c
    return f + 2 * cin * 1024 + 2 * 1024


def gpu_ms(fn, iters, warmup=3):
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
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--cpu-iters', type=int, default=2)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lines = []
    for net, n, L in SHAPES:
        chans = zi.SMALL_CHANNELS if net == 'small' else zi.LARGE_CHANNELS
        sd = {k: torch.from_numpy(v) for k, v in zi.seeded_weights(chans, 7).items()}
        ours = (ZonziniNetSmall() if net == 'small' else ZonziniNetLarge())
        ours.load_state_dict(sd)
        ours = ours.to(dev).eval()
        stock = Stock(chans)
        stock.load_state_dict(sd)
        stock = stock.eval()
        x = torch.from_numpy(zi.echo_frames(n, L, 1)).to(dev)
        stock_dev = Stock(chans).to(dev).eval()
        stock_dev.load_state_dict(sd)
        with torch.no_grad():
            y, ys = ours(x), stock_dev(x)
            t_ours = gpu_ms(lambda: ours(x), a.iters)
            t_stock = gpu_ms(lambda: stock_dev(x), a.iters)
            t_cpu = None
            if not a.no_cpu:
                xc = x.cpu()
                stock(xc)
                tic = time.perf_counter()
                for _ in range(a.cpu_iters):
                    stock(xc)
                t_cpu = (time.perf_counter() - tic) * 1000.0 / a.cpu_iters
        fl = flops(chans, L) * n
        rec = {'net': net, 'shape': [n, 1, L], 'ours_ms': round(t_ours, 4), 'stock_gpu_ms': round(t_stock, 4),
               'cpu_ms': None if t_cpu is None else round(t_cpu, 2), 'speedup_vs_stock_gpu': round(t_stock / t_ours, 3),
               'waveforms_per_s': round(n / t_ours * 1000.0, 1), 'gflop': round(fl / 1e9, 3),
               'peak_fraction': round(fl / (t_ours * 1e-3) / PEAK, 4),
               'max_rel_diff': float((y - ys).abs().max() / ys.abs().max())}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, 'w') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

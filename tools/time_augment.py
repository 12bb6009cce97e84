"""Times of the device augmentation (csrc/augment.hip: crop .75 + 30 dB noise, drawn numbers, one launch per batch) next
to the numpy path of stofnet_amd/transforms.py on the same rows (one sample at a time, as DataLoader workers run it), one
JSON line per shape:

    python tools/time_augment.py [--out profiles/augment.jsonl] [--reps 30] [--warmup 5]

  us            median over --reps single launches, each between two HIP events on the launch stream, after --warmup calls
  spread        (max - min) / median over the reps
  hbm_fraction  8 N L bytes (one read of x, one write of y; the second read of the row is served by L2) / time / 8 TB/s
  numpy_ms      the numpy chain CropChannelData -> AddNoise over the same N rows on one CPU core (rows with an empty shift
                range, where the reference raises, keep their window)
A `parity` line that tests/test_gpu_augment.py left in --out is kept."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stofnet_amd import synth  # noqa: E402
from stofnet_amd.augment import augment  # noqa: E402
from stofnet_amd.transforms import AddNoise, CropChannelData  # noqa: E402

HBM = 8e12
SHAPES = [(256, 2000), (4096, 2000), (256, 20000), (4, 2000)]
RATIO, SNR_DB = .75, 30.


def numpy_ms(x, gt):
    crop, add = CropChannelData(RATIO), AddNoise(SNR_DB)
    np.random.seed(0)
    tic = time.perf_counter()
    for row, g in zip(x, gt):
        try:
            row, g = crop(row, float(g))
        except ValueError:                       # empty shift range
            pass
        add(row)
    return (time.perf_counter() - tic) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--numpy-rows', type=int, default=256, help='rows timed on the numpy path (scaled up to N)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = []
    for n, L in SHAPES:
        x, onsets = synth.synth_echo(n, L, seed=7, return_onsets=True)
        gt = onsets.astype(np.float32)
        xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(gt[:, None]).to(dev)
        for k in range(a.warmup):
            augment(xd, gd, snr_db=SNR_DB, crop_ratio=RATIO, seed=1, call=k)
        torch.cuda.synchronize()
        us = []
        for k in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            augment(xd, gd, snr_db=SNR_DB, crop_ratio=RATIO, seed=1, call=a.warmup + k)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        t = statistics.median(us)
        m = min(n, a.numpy_rows)
        host = numpy_ms(x[:m, 0].astype(np.float64), gt[:m]) * n / m
        rec = {'kind': 'timing', 'shape': [n, 1, L], 'crop_ratio': RATIO, 'snr_db': SNR_DB, 'us': round(t, 2),
               'spread': round((max(us) - min(us)) / t, 3), 'hbm_fraction': round(8 * n * L / (t * 1e-6) / HBM, 4),
               'numpy_ms': round(host, 2), 'numpy_rows_timed': m, 'reps': a.reps, 'warmup': a.warmup}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
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

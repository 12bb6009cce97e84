"""Time of one training pass (forward, loss = sum(y * t), backward) of Kuleshov on its two train routes, on the same module on the
same GPU in one process: `train_route = 'kernels'` (the staged gfx950 training kernels, exact fp32, train-mode BatchNorm with
double sums, Philox Dropout masks computed again by the backward) next to `train_route = 'aten'` (`Kuleshov.forward_aten`: MIOpen
convolutions, ATen BatchNorm and Dropout), one JSON line per shape:

    python tools/time_kuleshov_train.py [--out profiles/kuleshov_training.jsonl] [--iters 3] [--repeats 5]
                                        [--shapes 64x2000:20000,4x2000:20000]              (NxL:O)

  kernels_ms / aten_ms   HIP events on the launch stream; the median of --repeats timings of --iters passes, the two routes
                         alternated so that drift hits both alike, after a warm-up pass of each
  *_spread               (max - min) / median over the repeats
  aten_over_kernels      aten_ms / kernels_ms (> 1: the kernels route is faster)
--out keeps the lines of other kinds that the file already holds (the parity line of tests/test_gpu_kuleshov_training.py).

Every timed pass first touches every parameter in place, as an optimizer step would: the kernels route then packs every fragment
image again on the device (output_fc's alone is 305 MB at O = 20000), which is part of what a training step costs.  dx is not
requested.  The two routes draw different Dropout masks (Philox against torch's generator), so their results are not compared
here: tests/test_gpu_kuleshov_training.py compares both with float64 under the same masks."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _train_timing import alternate, make_step, write_timing  # noqa: E402


def parse(shape):
    rows, O = shape.split(':')
    N, L = (int(v) for v in rows.split('x'))
    return N, L, int(O)


def build(N, L, O, dev):
    from stofnet_amd import Kuleshov
    torch.manual_seed(900 + N)
    m = Kuleshov(L, O).to(dev).train()
    x = torch.randn((N, 1, L), generator=torch.Generator().manual_seed(N + L)).to(dev)
    t = torch.randn((N, 1, O), generator=torch.Generator().manual_seed(N + O)).to(dev)
    plain = make_step(m, x, t)
    params = list(m.parameters())

    def step(route):
        with torch.no_grad():
            torch._foreach_add_(params, 0.0)     # an in-place update of every parameter: the next forward packs its images again
        return plain(route)
    return m, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='64x2000:20000,4x2000:20000')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_kuleshov_train.py needs a ROCm GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for N, L, O in (parse(s) for s in a.shapes.split(',')):
        m, step = build(N, L, O, dev)
        mo, so, ms, ss = alternate(lambda: step('kernels'), lambda: step('aten'), a.iters, a.repeats)
        rec = {'kind': 'timing', 'model': 'kuleshov', 'shape': [N, 1, L], 'output_length': O, 'pass': 'parameter touch + forward + backward',
               'repeats': a.repeats, 'iters': a.iters, 'kernels_ms': round(mo, 4), 'kernels_spread': round(so, 4), 'aten_ms': round(ms, 4),
               'aten_spread': round(ss, 4), 'aten_over_kernels': round(ms / mo, 3)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del m, step
        torch.cuda.empty_cache()
    if a.out:
        write_timing(a.out, lines)


if __name__ == '__main__':
    main()

"""Time of one training pass (forward, loss = sum(y * t), backward) of SincNet on its two train routes, on the same module on
the same GPU in one process: `train_route = 'kernels'` (the staged gfx950 training kernels, exact fp32, train-mode BatchNorm
with double sums) next to `train_route = 'aten'` (`SincNet.forward_aten`: MIOpen and rocBLAS), one JSON line per shape:

    python tools/time_sincnet_train.py [--out profiles/sincnet_training.jsonl] [--iters 3] [--repeats 5] [--shapes 256x2000,4x2000]

  kernels_ms / aten_ms   HIP events on the launch stream; the median of --repeats timings of --iters passes, the two routes
                         alternated so that drift hits both alike, after a warm-up pass of each
  *_spread               (max - min) / median over the repeats
  aten_over_kernels      aten_ms / kernels_ms (> 1: the kernels route is faster)
  max_rel_grad_diff      the largest max |kernels - aten| / max |aten| over y and all parameter gradients of one pass
  kernels_vs_f64 / aten_vs_f64   the same distance of either route from the module in float64 on the ATen route (same GPU)
  *_at                   the tensor (y or a parameter's gradient) that holds that maximum
--out keeps the lines of other kinds that the file already holds (the parity line of tests/test_gpu_sincnet_training.py).

Every timed pass first touches `low_hz_` in place, as an optimizer step would: the kernels route then synthesises the bank and
packs every image again on the device, which is part of what a training step costs.  dx is not requested.  The conv bias
gradients are analytically 0 under train-mode BatchNorm, so a relative distance there compares rounding noise with rounding
noise; at these row counts a LeakyReLU decision within rounding of zero also differs between any two fp32 routes, so
max_rel_grad_diff and *_vs_f64 can show a whole gradient term; the tests compare with the decisions pinned."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import SincNet  # noqa: E402
import sincnet_inputs as si  # noqa: E402
import sincnet_training_inputs as ti  # noqa: E402
from _train_timing import make_step, time_routes, write_timing  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='256x2000,4x2000')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_sincnet_train.py needs a ROCm GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for shape in a.shapes.split(','):
        N, L = (int(v) for v in shape.split('x'))
        m = SincNet(si.options(1e6, L))
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in ti.weights('pretty-brook', 1e6).items()}, strict=True)
        m = m.to(dev).train()
        x = torch.from_numpy(si.frames((N, 1, L), 5)).to(dev)
        t = torch.randn((N, 1, L), generator=torch.Generator().manual_seed(N + L)).to(dev)
        plain = make_step(m, x, t)

        def step(route):
            with torch.no_grad():
                m.conv[0].low_hz_.add_(0.0)          # an in-place parameter update: the next forward packs its images again
            return plain(route)

        rec = {'kind': 'timing', 'model': 'sincnet', 'shape': [N, 1, L], 'pass': 'parameter touch + forward + backward',
               'repeats': a.repeats, 'iters': a.iters, **time_routes(m, step, x, t, a.iters, a.repeats)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, t, m
        torch.cuda.empty_cache()
    if a.out:
        write_timing(a.out, lines)


if __name__ == '__main__':
    main()

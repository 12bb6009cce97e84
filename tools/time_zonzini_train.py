"""Time of one training pass (forward, loss = sum(y * t), backward) of the Zonzini nets on their two train routes, on the same
module on the same GPU in one process: `train_route = 'kernels'` (the staged gfx950 training kernels, exact fp32) next to
`train_route = 'aten'` (the module's own Conv1d / MaxPool1d / Linear layers: MIOpen and rocBLAS), one JSON line per shape:

    python tools/time_zonzini_train.py [--out profiles/zonzini_training.jsonl] [--iters 3] [--repeats 5]
                                       [--shapes small:256x2000,small:4x2000,large:64x4000]

  kernels_ms / aten_ms   HIP events on the launch stream; the median of --repeats timings of --iters passes, the two routes
                         alternated so that drift hits both alike, after a warm-up pass of each
  *_spread               (max - min) / median over the repeats
  aten_over_kernels      aten_ms / kernels_ms (> 1: the kernels route is faster)
  max_rel_grad_diff      the largest max |kernels - aten| / max |aten| over y and all parameter gradients of one pass
  kernels_vs_f64 / aten_vs_f64   the same distance of either route from the module in float64 on the ATen route (same GPU)
  *_at                   the tensor (y or a parameter's gradient) that holds that maximum
--out keeps the lines of other kinds that the file already holds (the parity line of tests/test_gpu_zonzini_training.py).

Every timed pass first touches one parameter in place, as an optimizer step would: the kernels route then packs its weight
images again (the forward blob goes through the host), which is part of what a training step costs.  At these row counts
a ReLU / pool decision within rounding of zero differs between any two fp32 routes, so max_rel_grad_diff and *_vs_f64 can
show a whole gradient term; the tests compare with the decisions pinned."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import ZonziniNetLarge, ZonziniNetSmall  # noqa: E402
import zonzini_inputs as zi  # noqa: E402
from _train_timing import make_step, time_routes, write_timing  # noqa: E402

NETS = {'small': (ZonziniNetSmall, zi.SMALL_CHANNELS, 740), 'large': (ZonziniNetLarge, zi.LARGE_CHANNELS, 741)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='small:256x2000,small:4x2000,large:64x4000')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_zonzini_train.py needs a ROCm GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for spec in a.shapes.split(','):
        net, shape = spec.split(':')
        N, L = (int(v) for v in shape.split('x'))
        cls, channels, wseed = NETS[net]
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in zi.seeded_weights(channels, wseed).items()}, strict=True)
        m = m.to(dev).train()
        x = torch.from_numpy(zi.echo_frames(N, L, 5)).to(dev)
        t = torch.randn((N, 1), generator=torch.Generator().manual_seed(N + L)).to(dev)
        plain = make_step(m, x, t)

        def step(route):
            with torch.no_grad():
                m.fc2.bias.add_(0.0)                 # an in-place parameter update: the next forward packs its images again
            return plain(route)

        rec = {'kind': 'timing', 'model': f'zonzini_{net}', 'shape': [N, 1, L], 'pass': 'parameter touch + forward + backward',
               'repeats': a.repeats, 'iters': a.iters, **time_routes(m, step, x, t, a.iters, a.repeats)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, t, m
        torch.cuda.empty_cache()
    if a.out:
        write_timing(a.out, lines)


if __name__ == '__main__':
    main()

"""Time of one training pass (forward, loss = sum(y * t), backward) of WaveUnet on its two train routes, on the same module on
the same GPU in one process: `train_route = 'kernels'` (the staged gfx950 training kernels, exact fp32, train-mode BatchNorm
with double sums) next to `train_route = 'aten'` (`WaveUnet.forward_aten`: MIOpen convolutions, ATen BatchNorm), one JSON line
per shape:

    python tools/time_waveunet_train.py [--out profiles/waveunet_training.jsonl] [--iters 3] [--repeats 5]
                                        [--shapes 2:256x2000,2:4x2000,10:64x8192]          (n_layers:NxL)

  kernels_ms / aten_ms   HIP events on the launch stream; the median of --repeats timings of --iters passes, the two routes
                         alternated so that drift hits both alike, after a warm-up pass of each
  *_spread               (max - min) / median over the repeats
  aten_over_kernels      aten_ms / kernels_ms (> 1: the kernels route is faster)
  max_rel_grad_diff      the largest max |kernels - aten| / max |aten| over y and all parameter gradients of one pass
  kernels_vs_f64 / aten_vs_f64   the same distance of either route from the module in float64 on the ATen route (same GPU)
  *_at                   the tensor (y or a parameter's gradient) that holds that maximum
--out keeps the lines of other kinds that the file already holds (the parity line of tests/test_gpu_waveunet_training.py).

Every timed pass first touches every parameter in place, as an optimizer step would: the kernels route then packs every fragment
image again on the device, which is part of what a training step costs.  dx is not requested.  The conv bias gradients of the
blocks are analytically 0 under train-mode BatchNorm, so a relative distance there compares rounding noise with rounding noise;
at these row counts a LeakyReLU decision within rounding of zero also differs between any two fp32 routes, so max_rel_grad_diff
and *_vs_f64 can show a whole gradient term; the tests compare with the decisions pinned.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_waveunet_train.py --profile-steps 3 --shapes 2:256x2000
    python tools/time_waveunet_train.py --summarize <dir> --shapes 2:256x2000 --out profiles/waveunet_training_kernels.json

run the kernels route alone for a kernel trace (no counters in the same run) and condense it into dispatch groups."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _train_timing import make_step, summarize, time_routes, write_timing  # noqa: E402


def parse(shape):
    n, rest = shape.split(':')
    N, L = (int(v) for v in rest.split('x'))
    return int(n), N, L


def build(n, N, L, dev):
    from stofnet_amd import WaveUnet
    import waveunet_inputs as wi
    m = WaveUnet(n, 16)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in wi.seeded_waveunet(n, 800 + n).items()}, strict=True)
    m = m.to(dev).train()
    x = torch.from_numpy(wi.frames(N, L, 5)).to(dev)
    t = torch.randn((N, 1, L), generator=torch.Generator().manual_seed(N + L)).to(dev)
    plain = make_step(m, x, t)
    params = list(m.parameters())

    def step(route):
        with torch.no_grad():
            torch._foreach_add_(params, 0.0)     # an in-place update of every parameter: the next forward packs its images again
        return plain(route)
    return m, x, t, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='2:256x2000,2:4x2000,10:64x8192')
    ap.add_argument('--profile-steps', type=int, default=0, help='run this many passes of the kernels route on the first shape and exit')
    ap.add_argument('--summarize', default=None, help='directory of a rocprofv3 kernel trace to condense into --out')
    a = ap.parse_args()
    shapes = [parse(s) for s in a.shapes.split(',')]
    if a.summarize:
        n, N, L = shapes[0]
        summarize(a.summarize, f'{N}x{L}', a.out, f'unet(n_layers={n})', 1, {})
        return
    if not torch.cuda.is_available():
        raise SystemExit('time_waveunet_train.py needs a ROCm GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    if a.profile_steps:
        m, x, t, step = build(*shapes[0], dev)
        for _ in range(a.profile_steps):
            step('kernels')
        torch.cuda.synchronize()
        return
    lines = []
    for n, N, L in shapes:
        m, x, t, step = build(n, N, L, dev)
        rec = {'kind': 'timing', 'model': 'unet', 'n_layers': n, 'shape': [N, 1, L], 'pass': 'parameter touch + forward + backward',
               'repeats': a.repeats, 'iters': a.iters, **time_routes(m, step, x, t, a.iters, a.repeats)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, t, m, step
        torch.cuda.empty_cache()
    if a.out:
        write_timing(a.out, lines)


if __name__ == '__main__':
    main()

"""Time of one training pass (forward, loss = sum(y * t), backward) of EDSR_1D(1, 64, 8, 4) on its two train routes, on the
same module on the same GPU in one process: `train_route = 'kernels'` (the gfx950 training kernels, exact fp32) next to
`train_route = 'aten'` (stock ATen layers, MIOpen convolutions), one JSON line per shape:

    python tools/time_edsr_train.py [--out profiles/edsr_training.jsonl] [--iters 3] [--repeats 5] [--shapes 256x2000,4x2000]

  kernels_ms / aten_ms   HIP events on the launch stream; the median of --repeats timings of --iters passes, the two routes
                         alternated so that drift hits both alike, after a warm-up pass of each
  *_spread               (max - min) / median over the repeats
  aten_over_kernels      aten_ms / kernels_ms (> 1: the kernels route is faster)
  max_rel_grad_diff      the largest max |kernels - aten| / max |aten| over y and all parameter gradients of one pass
  kernels_vs_f64 / aten_vs_f64   the same distance of either route from the module in float64 on the ATen route (same GPU)
  *_at                   the tensor (y or a parameter's gradient) that holds that maximum
--out keeps the lines of other kinds that the file already holds (the parity line of tests/test_gpu_edsr_training.py)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import EDSR_1D  # noqa: E402
import riders_inputs as ri  # noqa: E402
from _train_timing import make_step, time_routes, write_timing  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='256x2000,4x2000')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_edsr_train.py needs a ROCm GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    B, r = 8, 4
    m = EDSR_1D(1, 64, B, r)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ri.seeded_edsr(B, r, 77).items()}, strict=True)
    m = m.to(dev).train()
    lines = []
    for shape in a.shapes.split(','):
        N, L = (int(v) for v in shape.split('x'))
        x = torch.from_numpy(ri.frames(N, L, 5)).to(dev)
        t = torch.randn((N, 1, L * r), generator=torch.Generator().manual_seed(N + L)).to(dev)
        rec = {'kind': 'timing', 'model': 'edsr', 'num_blocks': B, 'r': r, 'shape': [N, 1, L], 'pass': 'forward + backward',
               'repeats': a.repeats, 'iters': a.iters, **time_routes(m, make_step(m, x, t), x, t, a.iters, a.repeats)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, t
        torch.cuda.empty_cache()
    if a.out:
        write_timing(a.out, lines)


if __name__ == '__main__':
    main()

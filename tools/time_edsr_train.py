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
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import EDSR_1D  # noqa: E402
import riders_inputs as ri  # noqa: E402


def gpu_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(ours, stock, iters, repeats):
    """Medians and spreads of two callables timed in turn, so that drift hits both alike."""
    ours(), stock()
    torch.cuda.synchronize()
    to, ts = [], []
    for _ in range(repeats):
        to.append(gpu_ms(ours, iters))
        ts.append(gpu_ms(stock, iters))
    mo, ms = statistics.median(to), statistics.median(ts)
    return mo, (max(to) - min(to)) / mo, ms, (max(ts) - min(ts)) / ms


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

        def step(route):
            m.train_route = route
            for q in m.parameters():
                q.grad = None
            y = m(x)
            (y * t).sum().backward()
            return y

        got = {}
        for route in ('kernels', 'aten'):
            y = step(route)
            got[route] = [y.detach().clone()] + [q.grad.clone() for q in m.parameters()]
        m64 = copy.deepcopy(m).double()
        m64.train_route = 'aten'
        y64 = m64(x.double())
        (y64 * t.double()).sum().backward()
        got['f64'] = [y64.detach()] + [q.grad for q in m64.parameters()]
        names = ['y'] + [k for k, _ in m.named_parameters()]

        def dist(a, b):
            """(largest max |a - b| / max |b| over y and the gradients, the tensor that has it)"""
            return max((float((u - v).abs().max() / v.abs().max()), k) for k, u, v in zip(names, got[a], got[b]))

        (diff, worst), (k64, worst_k), (a64, worst_a) = dist('kernels', 'aten'), dist('kernels', 'f64'), dist('aten', 'f64')
        del got, m64, y64
        torch.cuda.empty_cache()
        mo, so, ms, ss = alternate(lambda: step('kernels'), lambda: step('aten'), a.iters, a.repeats)
        rec = {'kind': 'timing', 'model': 'edsr', 'num_blocks': B, 'r': r, 'shape': [N, 1, L], 'pass': 'forward + backward',
               'repeats': a.repeats, 'iters': a.iters, 'kernels_ms': round(mo, 4), 'kernels_spread': round(so, 4),
               'aten_ms': round(ms, 4), 'aten_spread': round(ss, 4), 'aten_over_kernels': round(ms / mo, 3),
               'max_rel_grad_diff': float(f'{diff:.3e}'), 'max_rel_grad_diff_at': worst,
               'kernels_vs_f64': float(f'{k64:.3e}'), 'kernels_vs_f64_at': worst_k, 'aten_vs_f64': float(f'{a64:.3e}'),
               'aten_vs_f64_at': worst_a}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, t
        torch.cuda.empty_cache()
    if a.out:
        kept = []
        if os.path.exists(a.out):
            with open(a.out) as fh:
                kept = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'timing']
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(kept + [json.dumps(rec) for rec in lines]) + '\n')


if __name__ == '__main__':
    main()

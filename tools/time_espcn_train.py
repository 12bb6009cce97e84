"""Time of one training pass (forward, loss = sum(y * t), backward) of ESPCN_1D(4) on its two train routes, on the same module
on the same GPU in one process: `train_route = 'kernels'` (the staged gfx950 training kernels, exact fp32) next to
`train_route = 'aten'` (stock ATen layers, MIOpen convolutions), one JSON line per shape:

    python tools/time_espcn_train.py [--out profiles/espcn_training.jsonl] [--iters 3] [--repeats 5] [--shapes 256x2000,4x2000]

  kernels_ms / aten_ms   HIP events on the launch stream; the median of --repeats timings of --iters passes, the two routes
                         alternated so that drift hits both alike, after a warm-up pass of each
  *_spread               (max - min) / median over the repeats
  aten_over_kernels      aten_ms / kernels_ms (> 1: the kernels route is faster)
  max_rel_grad_diff      the largest max |kernels - aten| / max |aten| over y and all parameter gradients of one pass
  kernels_vs_f64 / aten_vs_f64   the same distance of either route from the module in float64 on the ATen route (same GPU)
  *_at                   the tensor (y or a parameter's gradient) that holds that maximum
--out keeps the lines of other kinds that the file already holds (the parity line of tests/test_gpu_espcn_training.py).

Per-kernel times come from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_espcn_train.py --passes 6 --shapes 256x2000
    python tools/time_espcn_train.py --summarize DIR --shapes 256x2000 --out profiles/espcn_training_kernels.json

--passes K runs K passes of the kernels route on the first shape and nothing else; --summarize groups the trace's
dispatches by (kernel, work-groups, threads, LDS bytes) and sets each new kernel's mean time against the bytes it has to
read and write once (no GPU needed)."""
import argparse
import copy
import csv
import glob
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import ESPCN_1D  # noqa: E402
import riders_inputs as ri  # noqa: E402

R = 4
# bytes per input sample that a kernel of csrc/espcn_train.hip must read and write once, as (constant, factor of r)
MIN_BYTES = {'ep_in_kernel': (4 + 256, 0), 'ep_mid_kernel': (256 + 128, 0), 'ep_out_kernel': (128, 4),
             'ep_out_wgrad_kernel': (128, 8), 'ep_out_dgrad_kernel': (128 + 128, 8), 'ep_in_wgrad_kernel': (256 + 256 + 4, 0),
             'ep_in_dgrad_kernel': (256 + 256 + 4, 0)}


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


def summarize(trace_dir, shape, out):
    """rocprofv3's *_kernel_trace.csv under `trace_dir` -> one JSON of dispatch groups."""
    N, L = (int(v) for v in shape.split('x'))
    paths = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    if not paths:
        raise SystemExit(f'no *kernel_trace.csv under {trace_dir}')
    groups = {}
    for path in paths:
        with open(path, newline='') as fh:
            for row in csv.DictReader(fh):
                name = re.sub(r'\(.*$', '', row['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '')).strip()
                threads = int(row['Workgroup_Size_X'])
                wgs = int(row['Grid_Size_X']) // max(threads, 1) * int(row['Grid_Size_Y']) * int(row['Grid_Size_Z'])
                lds = int(row.get('LDS_Block_Size', row.get('LDS_Block_Size_v', 0)) or 0)
                us = (int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1000.0
                groups.setdefault((name, wgs, threads, lds), []).append(us)
    rec = {'shape': [N, 1, L], 'r': R, 'model': 'espcn', 'pass': 'forward + backward, kernels route', 'groups': {}}
    for (name, wgs, threads, lds), us in sorted(groups.items()):
        g = {'kernel': name, 'workgroups': wgs, 'threads': threads, 'lds_bytes': lds, 'calls': len(us),
             'mean_us': round(statistics.mean(us), 3), 'min_us': round(min(us), 3), 'max_us': round(max(us), 3)}
        if name in MIN_BYTES:
            c, f = MIN_BYTES[name]
            nbytes = N * L * (c + f * R)
            g['min_bytes_MB'] = round(nbytes / 1e6, 1)
            g['TB_per_s'] = round(nbytes / (g['mean_us'] * 1e-6) / 1e12, 2)
        rec['groups'][f'{name}|{wgs}|{threads}|{lds}'] = g
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps({k: v for k, v in rec['groups'].items() if v['kernel'] in MIN_BYTES}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='256x2000,4x2000')
    ap.add_argument('--passes', type=int, default=0)
    ap.add_argument('--summarize', default=None)
    a = ap.parse_args()
    if a.summarize:
        if not a.out:
            raise SystemExit('--summarize needs --out')
        return summarize(a.summarize, a.shapes.split(',')[0], a.out)
    if not torch.cuda.is_available():
        raise SystemExit('time_espcn_train.py needs a ROCm GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    m = ESPCN_1D(R)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ri.seeded_espcn(R, 77).items()}, strict=True)
    m = m.to(dev).train()
    lines = []
    for shape in a.shapes.split(','):
        N, L = (int(v) for v in shape.split('x'))
        x = torch.from_numpy(ri.frames(N, L, 5)).to(dev)
        t = torch.randn((N, 1, L * R), generator=torch.Generator().manual_seed(N + L)).to(dev)

        def step(route):
            m.train_route = route
            for q in m.parameters():
                q.grad = None
            y = m(x)
            (y * t).sum().backward()
            return y

        if a.passes:
            for _ in range(a.passes):
                step('kernels')
            torch.cuda.synchronize()
            return
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
        rec = {'kind': 'timing', 'model': 'espcn', 'r': R, 'shape': [N, 1, L], 'pass': 'forward + backward',
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

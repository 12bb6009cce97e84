"""What tools/time_edsr_train.py and tools/time_espcn_train.py share: the timing of a model's two train routes in one process,
their distances from float64, the `timing` lines of a profiles/*.jsonl and the summary of a rocprofv3 kernel trace."""
import copy
import csv
import glob
import json
import os
import re
import statistics

import torch


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


def make_step(m, x, t):
    """-> step(route): one training pass (forward, loss = sum(y * t), backward) of `m` on that route, returning y"""
    def step(route):
        m.train_route = route
        for q in m.parameters():
            q.grad = None
        y = m(x)
        (y * t).sum().backward()
        return y
    return step


def time_routes(m, step, x, t, iters, repeats):
    """The fields of a `timing` line from kernels_ms on: both routes' times, and the distances between the routes and from the
    module in float64 on the ATen route over y and all parameter gradients of one pass."""
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
    mo, so, ms, ss = alternate(lambda: step('kernels'), lambda: step('aten'), iters, repeats)
    return {'kernels_ms': round(mo, 4), 'kernels_spread': round(so, 4), 'aten_ms': round(ms, 4), 'aten_spread': round(ss, 4),
            'aten_over_kernels': round(ms / mo, 3), 'max_rel_grad_diff': float(f'{diff:.3e}'), 'max_rel_grad_diff_at': worst,
            'kernels_vs_f64': float(f'{k64:.3e}'), 'kernels_vs_f64_at': worst_k, 'aten_vs_f64': float(f'{a64:.3e}'),
            'aten_vs_f64_at': worst_a}


def write_timing(out, lines):
    """`lines` become the `timing` lines of `out`; the lines of other kinds that the file already holds stay."""
    kept = []
    if os.path.exists(out):
        with open(out) as fh:
            kept = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'timing']
    with open(out, 'w') as fh:
        fh.write('\n'.join(kept + [json.dumps(rec) for rec in lines]) + '\n')


def summarize(trace_dir, shape, out, model, r, min_bytes):
    """rocprofv3's *_kernel_trace.csv under `trace_dir` -> one JSON of dispatch groups.  `min_bytes`: kernel -> the bytes per
    input sample that it must read and write once, as (constant, factor of r)."""
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
    rec = {'shape': [N, 1, L], 'r': r, 'model': model, 'pass': 'forward + backward, kernels route', 'groups': {}}
    for (name, wgs, threads, lds), us in sorted(groups.items()):
        g = {'kernel': name, 'workgroups': wgs, 'threads': threads, 'lds_bytes': lds, 'calls': len(us),
             'mean_us': round(statistics.mean(us), 3), 'min_us': round(min(us), 3), 'max_us': round(max(us), 3)}
        if name in min_bytes:
            c, f = min_bytes[name]
            nbytes = N * L * (c + f * r)
            g['min_bytes_MB'] = round(nbytes / 1e6, 1)
            g['TB_per_s'] = round(nbytes / (g['mean_us'] * 1e-6) / 1e12, 2)
        rec['groups'][f'{name}|{wgs}|{threads}|{lds}'] = g
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps({k: v for k, v in rec['groups'].items() if v['kernel'] in min_bytes}, indent=1))

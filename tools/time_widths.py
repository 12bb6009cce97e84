"""Times of StofNet at other widths (num_features F, in_channels Cin; shipped depth, 7-tap body, SemiGlobalBlock at scale 80,
r = 4) on the gfx950 kernels next to the same network on stock torch-ROCm layers (F.conv1d / leaky_relu / max-pool on device
tensors, fp32: oracle/stofnet_oracle.py:stofnet_forward restated on the device, since the oracle computes on the CPU) on the
same GPU in one process, one JSON line per (F, Cin):

    python tools/time_widths.py [--out profiles/widths.jsonl] [--iters 3] [--repeats 5] [--batch 256] [--length 2000]

  infer_fp32_ms / infer_f16x3_ms   model(x) in eval mode under no_grad, HIP events on the launch stream; the median of
                    --repeats timings of --iters calls, each alternated with a stock timing
  stock_infer_ms    the stock forward, measured the same way in the same loop
  train_f16x3_ms    one autograd training step in train mode (train_precision='f16x3'): forward, sum(y * t) loss, backward
  stock_train_ms    the same step on the stock layers (fp32)
  *_spread          (max - min) / median over the repeats
  max_rel_diff      max |ours fp32 - stock| / max |stock|
--widths F,Cin restricts the run to one pair."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from stofnet_amd import StofNet  # noqa: E402
from ctor_variants import variant_params  # noqa: E402

WIDTHS = [(32, 1), (128, 1), (64, 2), (64, 16)]        # (num_features, in_channels)


def stock_forward(p, x, r, scale, nb):
    """The network on stock torch layers, on whatever device `p` and `x` live on."""
    x = F.relu(F.conv1d(x, p['conv1.weight'], p['conv1.bias'], padding=4))
    if scale != 1:
        L = x.shape[-1]
        P = L // scale
        rem = L - P * scale
        z = F.leaky_relu(F.conv1d(x, p['semi_global_block.contract_conv.weight'], p['semi_global_block.contract_conv.bias'], padding=2), 0.01)
        z = F.max_pool1d(z, scale, scale)
        z = F.leaky_relu(F.conv1d(z, p['semi_global_block.expand_conv.weight'], p['semi_global_block.expand_conv.bias'], padding=2), 0.01)
        x = x + F.pad(z.repeat_interleave(scale, dim=-1), (rem // 2, rem - rem // 2))
    res1 = res = x
    for i in range(2, nb - 1):
        w = p[f'conv{i}.weight']
        y = F.conv1d(x, w, p[f'conv{i}.bias'], padding=w.shape[-1] // 2)
        if i % 2:
            x = res = res + y
        else:
            x = F.leaky_relu(y, 0.01)
    w = p[f'conv{nb - 1}.weight']
    x = res1 + F.conv1d(x, w, p[f'conv{nb - 1}.bias'], padding=w.shape[-1] // 2)
    x = F.conv1d(x, p['conv_last.weight'], p['conv_last.bias'], padding=1)
    n, _, L = x.shape
    return x.permute(0, 2, 1).reshape(n, 1, L * r)          # one output channel: the shuffle interleaves the r maps


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
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--length', type=int, default=2000)
    ap.add_argument('--widths', default=None, help='F,Cin: time this pair only')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    widths = [tuple(int(v) for v in a.widths.split(','))] if a.widths else WIDTHS
    N, L, r, scale, nb = a.batch, a.length, 4, 80, 13
    lines = []
    for Fw, Cin in widths:
        m = StofNet(upsample_factor=r, num_features=Fw, num_blocks=nb, kernel_sizes=[9, 7, 3], in_channels=Cin,
                    semi_global_scale=scale, precision='fp32', train_precision='f16x3')
        params = variant_params({n: tuple(t.shape) for n, t in m.state_dict().items()}, 7 + Fw + Cin)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        m = m.to(dev)
        p = {k: v.detach() for k, v in m.named_parameters()}
        rng = np.random.RandomState(Fw * 100 + Cin)
        x = torch.from_numpy((0.3 * rng.standard_normal((N, Cin, L))).astype(np.float32)).to(dev)
        t = torch.from_numpy(rng.standard_normal((N, 1, L * r)).astype(np.float32)).to(dev)
        rec = {'kind': 'timing', 'model': 'stofnet', 'num_features': Fw, 'in_channels': Cin, 'shape': [N, Cin, L], 'r': r,
               'num_blocks': nb, 'body_kernel': 7, 'semi_global_scale': scale, 'repeats': a.repeats, 'iters': a.iters}
        m.eval()
        with torch.no_grad():
            ys = stock_forward(p, x, r, scale, nb)
            rec['max_rel_diff'] = float((m(x) - ys).abs().max() / ys.abs().max())
            del ys
            for prec in ('fp32', 'f16x3'):
                m.precision = prec
                mo, so, ms, ss = alternate(lambda: m(x), lambda: stock_forward(p, x, r, scale, nb), a.iters, a.repeats)
                rec[f'infer_{prec}_ms'], rec[f'infer_{prec}_spread'] = round(mo, 4), round(so, 4)
                if prec == 'fp32':
                    rec['stock_infer_ms'], rec['stock_infer_spread'] = round(ms, 4), round(ss, 4)
                m.raise_if_overflow()
            rec['speedup_infer_fp32'] = round(rec['stock_infer_ms'] / rec['infer_fp32_ms'], 3)
            rec['speedup_infer_f16x3'] = round(rec['stock_infer_ms'] / rec['infer_f16x3_ms'], 3)
        m.train()
        pg = {k: v.detach().clone().requires_grad_() for k, v in p.items()}

        def ours_step():
            for q in m.parameters():
                q.grad = None
            (m(x) * t).sum().backward()

        def stock_step():
            for q in pg.values():
                q.grad = None
            (stock_forward(pg, x, r, scale, nb) * t).sum().backward()

        mo, so, ms, ss = alternate(ours_step, stock_step, a.iters, a.repeats)
        m.raise_if_overflow()
        rec.update(train_f16x3_ms=round(mo, 4), train_f16x3_spread=round(so, 4), stock_train_ms=round(ms, 4),
                   stock_train_spread=round(ss, 4), speedup_train=round(ms / mo, 3))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del m, p, pg, x, t
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

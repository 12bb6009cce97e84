"""HIP-event times of GradPeak on float64 frames next to the fp32 path, one JSON line per shape and threshold mode:

    python tools/time_gradpeak_f64.py [--out profiles/gradpeak_f64.jsonl] [--fp32-only] [--iters 20]

  f64_env_us      hilbert_envelope (stof_hilbert_f64)
  f64_detect_us   the detection launches on that envelope: stof_grad_peak_detect_f64, preceded by
                  stof_gradpeak_moments_f64 + stof_gradpeak_threshold_f64 for the default threshold
  f64_e2e_us      toa_detect end to end (including its one host read)
  f32_detect_us   the fp32 detection launches on the fp32 envelope (stof_gradpeak_moments + stof_gradpeak_threshold +
                  stof_grad_peak_detect), the same shape and threshold
  f32_e2e_us      fp32 toa_detect end to end
--fp32-only times fp32 toa_detect at [4096, 2000] alone (A/B runs of two builds in alternating processes)."""
import argparse
import json
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (after PYTHONPATH: A/B runs of another tree)
from stofnet_amd import _lib, synth, toa_detect  # noqa: E402
from stofnet_amd.gradpeak import _taps_on  # noqa: E402
from stofnet_amd.hilbert import hilbert_envelope  # noqa: E402

dev = torch.device('cuda:0')


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1000.0 / iters, 1)


def detect_launches(env, rf, th):
    """the detection launches of _detect on a ready envelope (no host read), fp32 or float64 by env's dtype"""
    lib = _lib.lib()
    f64 = env.dtype == torch.float64
    n, L = env.shape
    gs = rf // 6 * 5
    taps = _taps_on(dev, gs, env.dtype)
    rad = (taps.numel() - 1) // 2
    stream = _lib.stream_ptr(dev)
    cap = 32
    echoes = torch.empty((n, cap, 3), dtype=env.dtype, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    stats0 = torch.tensor([0.0, 0.0, float(n * L)], dtype=torch.float64, device=dev)
    stats = torch.empty_like(stats0)
    th_dev = torch.empty(1, dtype=env.dtype, device=dev)
    ws = torch.empty(max(lib.stof_gradpeak_moments_f64_workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
    p = _lib.ptr

    def run():
        thp = None
        if th is None:
            stats.copy_(stats0)
            if f64:
                _lib.check(lib.stof_gradpeak_moments_f64(p(env), n, L, gs, p(taps), rad, p(stats), p(ws), ws.numel(), stream))
                _lib.check(lib.stof_gradpeak_threshold_f64(p(stats), p(th_dev), stream))
            else:
                _lib.check(lib.stof_gradpeak_moments(p(env), n, L, gs, p(taps), rad, p(stats), stream))
                _lib.check(lib.stof_gradpeak_threshold(p(stats), p(th_dev), stream))
            thp = p(th_dev)
        call = lib.stof_grad_peak_detect_f64 if f64 else lib.stof_grad_peak_detect
        _lib.check(call(p(env), n, L, gs, p(taps), rad, th if th is not None else 0.0, thp, rf, 50 * rf, 0, p(echoes), cap,
                        None, p(counts), p(flags), stream))
    return run


def frames(rows, L, dtype):
    return torch.from_numpy(synth.synth_echo(rows, L, seed=11, noise=0.01)[:, 0]).to(dev, dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--fp32-only', action='store_true')
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    lines = []
    if a.fp32_only:
        x32 = frames(4096, 2000, torch.float32)
        for th in (1e-3, None):
            lines.append({'rows': 4096, 'L': 2000, 'rf': 10, 'th': th,
                          'f32_e2e_us': timed(lambda: toa_detect(x32, threshold=th, rescale_factor=10), a.iters)})
    else:
        for rows, L, rf, th in [(4096, 2000, 10, 1e-3), (4096, 2000, 10, None), (1024, 20000, 10, 1e-3), (512, 30720, 20, 1e-5)]:
            x64, x32 = frames(rows, L, torch.float64), frames(rows, L, torch.float32)
            env64, env32 = hilbert_envelope(x64), hilbert_envelope(x32, keep_cached=True)
            r = {'rows': rows, 'L': L, 'rf': rf, 'th': th}
            r['f64_env_us'] = timed(lambda: hilbert_envelope(x64), a.iters)
            r['f64_detect_us'] = timed(detect_launches(env64, rf, th), a.iters)
            r['f64_e2e_us'] = timed(lambda: toa_detect(x64, threshold=th, rescale_factor=rf), a.iters)
            r['f32_detect_us'] = timed(detect_launches(env32, rf, th), a.iters)
            r['f32_e2e_us'] = timed(lambda: toa_detect(x32, threshold=th, rescale_factor=rf), a.iters)
            r['detect_f64_over_f32'] = round(r['f64_detect_us'] / r['f32_detect_us'], 2)
            lines.append(r)
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()

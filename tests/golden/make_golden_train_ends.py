#!/usr/bin/env python3
"""The bits that the entry points of the training ends produce, recorded from the built library on the GPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_ends.py --commit <hash the library was built from>

Data only (expected outputs); the inputs are regenerated from seeds by tests/train_ends_inputs.py.  Unlike the other
fixtures this one has no independent reference: it pins stof_train_{edsr,espcn}_in / _in_wgrad / _in_dgrad,
stof_train_{edsr,espcn}_out_wgrad, stof_train_conv1_wgrad and stof_train_conv1_c_wgrad to what the commit named in the
manifest computed, so that a change to the shared kernels behind them (csrc/train_ends.h, csrc/wgrad_reduce.h) shows as a
changed bit.  Whether those bits are right is the business of the training tests.  Re-record only for a change that is meant
to alter a sum's order, and say so.

  f28_train_ends_bits.npz    `<case>.<output>` for every case of train_ends_inputs.CASES, raw fp32
  manifest_train_ends.json   the commit, and per case: entry, shape, parameters, seed, SHA-256 of the inputs, output shapes
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True

import train_ends_inputs as ti  # noqa: E402

NAME = 'f28_train_ends_bits'
LIMIT = 300 * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the loaded library was built from')
    ap.add_argument('--out-dir', default=HERE)
    a = ap.parse_args()
    from stofnet_amd import _lib
    lib, dev = _lib.lib(), torch.device('cuda', 0)
    out, manifest = {}, {'commit': a.commit, 'torch': torch.__version__, 'numpy': np.__version__, 'out_scale': ti.OUT_SCALE,
                         'cases': {}}
    for c in ti.CASES:
        name, entry, sh, p, seed = c
        got, again = ti.run(lib, dev, c), ti.run(lib, dev, c)
        for k, v in got.items():
            assert np.isfinite(v).all() and np.array_equal(v, again[k]), (name, k)
            out[f'{name}.{k}'] = v
        manifest['cases'][name] = {'entry': entry, 'shape': list(ti.SHAPES[sh]), 'params': p, 'seed': seed,
                                   'inputs_sha256': ti.digest(ti.operands(c)), 'outputs': {k: list(v.shape) for k, v in got.items()}}
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, NAME + '.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    with open(os.path.join(a.out_dir, 'manifest_train_ends.json'), 'w') as fh:
        json.dump(manifest, fh, indent=1)
    print(f'{NAME}: {len(ti.CASES)} cases, {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()

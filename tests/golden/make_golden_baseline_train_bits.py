#!/usr/bin/env python3
"""The bits that the training entry points of the SincNet, Wave-U-Net and Zonzini baselines (and ESPCN's weight repack)
produce, recorded from the built library on the GPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_baseline_train_bits.py --commit <hash the library was built from>

Data only (expected outputs); the inputs are regenerated from seeds by tests/baseline_train_bits_inputs.py.  Like
f28_train_ends_bits this fixture has no independent reference: it pins the entries to what the commit named in the manifest
computed, so that a change to the kernels behind them (csrc/bn_train.h, the chunk rules of csrc/wgrad_reduce.h, the fragment
order of csrc/mfma32_frag.h) shows as a changed bit.  Whether those bits are right is the business of the training tests.
Re-record only for a change that is meant to alter a sum's order or an arithmetic, and say so.

  f31_baseline_train_bits.npz          `<case>.<output>` for every output of at most RAW_BYTES bytes, raw
  manifest_baseline_train_bits.json    the commit, and per case: family, parameters, seed, SHA-256 of the inputs, and per output
                                       its shape and dtype, and for the larger ones the SHA-256 of their bytes
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

import baseline_train_bits_inputs as bi  # noqa: E402

NAME = 'f31_baseline_train_bits'
MANIFEST = 'manifest_baseline_train_bits.json'
LIMIT = 300 * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the loaded library was built from')
    ap.add_argument('--out-dir', default=HERE)
    a = ap.parse_args()
    from stofnet_amd import _lib
    lib, dev = _lib.lib(), torch.device('cuda', 0)
    out, manifest = {}, {'commit': a.commit, 'torch': torch.__version__, 'numpy': np.__version__, 'raw_bytes': bi.RAW_BYTES, 'cases': {}}
    for c in bi.CASES:
        name, family, p, seed = c
        got, again = bi.run(lib, dev, c), bi.run(lib, dev, c)
        outputs = {}
        for k, v in got.items():
            assert v.tobytes() == again[k].tobytes(), (name, k)
            assert v.dtype == np.uint8 or np.isfinite(v).all(), (name, k)
            outputs[k] = {'shape': list(v.shape), 'dtype': str(v.dtype)}
            if bi.stored_raw(v):
                out[f'{name}.{k}'] = v
            else:
                outputs[k]['sha256'] = bi.sha(v)
        manifest['cases'][name] = {'family': family, 'params': p, 'seed': seed, 'inputs_sha256': bi.digest(bi.operands(c)),
                                   'outputs': outputs}
        print(name, 'ok', flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, NAME + '.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    with open(os.path.join(a.out_dir, MANIFEST), 'w') as fh:
        json.dump(manifest, fh, indent=1)
    print(f'{NAME}: {len(bi.CASES)} cases, {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()

"""The entry points behind csrc/train_ends.h and csrc/wgrad_reduce.h, bit for bit against what the commit named in
tests/golden/manifest_train_ends.json computed (tests/train_ends_inputs.py has the cases; the fixture comes from
tests/golden/make_golden_train_ends.py).  Every summation order of these kernels is fixed by the shape alone, so any
difference is a changed order or a changed contraction: it is fixed in the kernel, never by recording again."""
import json
import os

import numpy as np
import pytest
import torch

import train_ends_inputs as ti

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def manifest():
    with open(os.path.join(GOLDEN, 'manifest_train_ends.json')) as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'f28_train_ends_bits.npz')) as z:
        return {k: z[k] for k in z.files}


def test_fixture_matches_its_recipe(manifest, golden):
    """the manifest lists exactly the cases of train_ends_inputs, the operands regenerated from its seeds hash to what the
    recorder saw, and the fixture holds exactly the outputs the manifest lists"""
    assert list(manifest['cases']) == ti.IDS
    assert manifest['out_scale'] == ti.OUT_SCALE
    stored = set()
    for c in ti.CASES:
        name, entry, sh, p, seed = c
        m = manifest['cases'][name]
        assert (m['entry'], tuple(m['shape']), m['params'], m['seed']) == (entry, ti.SHAPES[sh], p, seed), name
        assert ti.digest(ti.operands(c, m['seed'])) == m['inputs_sha256'], name
        for k, shape in m['outputs'].items():
            assert golden[f'{name}.{k}'].shape == tuple(shape) and golden[f'{name}.{k}'].dtype == np.float32, (name, k)
            stored.add(f'{name}.{k}')
    assert stored == set(golden)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ti.IDS)
def test_bits(name, manifest, golden):
    from stofnet_amd import _lib
    assert torch.cuda.is_available()
    m = manifest['cases'][name]
    got = ti.run(_lib.lib(), torch.device('cuda', 0), ti.case(name), m['seed'])
    assert sorted(got) == sorted(m['outputs'])
    for k, v in got.items():
        ref = golden[f'{name}.{k}']
        differ = int((v.view(np.uint32) != ref.view(np.uint32)).sum())
        print(name, k, 'floats', v.size, 'differing', differ)
        assert np.array_equal(v.view(np.uint32), ref.view(np.uint32)), (name, k, differ)

"""The training entry points of the SincNet, Wave-U-Net and Zonzini baselines and ESPCN's weight repack, bit for bit against
what the commit named in tests/golden/manifest_baseline_train_bits.json computed (tests/baseline_train_bits_inputs.py has the
cases; the fixture comes from tests/golden/make_golden_baseline_train_bits.py).  Every summation order of these kernels is fixed
by the shape alone, so any difference is a changed order, a changed chunk rule, a changed rounding or a changed contraction: it
is fixed in the kernel, never by recording again."""
import json
import os

import numpy as np
import pytest
import torch

import baseline_train_bits_inputs as bi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def manifest():
    with open(os.path.join(GOLDEN, 'manifest_baseline_train_bits.json')) as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'f31_baseline_train_bits.npz')) as z:
        return {k: z[k] for k in z.files}


def test_fixture_matches_its_recipe(manifest, golden):
    """the manifest lists exactly the cases of baseline_train_bits_inputs, the operands regenerated from its seeds hash to what
    the recorder saw, and the fixture holds exactly the small outputs the manifest lists, the manifest a hash of every other"""
    assert list(manifest['cases']) == bi.IDS
    assert manifest['raw_bytes'] == bi.RAW_BYTES
    stored = set()
    for c in bi.CASES:
        name, family, p, seed = c
        m = manifest['cases'][name]
        assert (m['family'], m['params'], m['seed']) == (family, p, seed), name
        assert bi.digest(bi.operands(c, m['seed'])) == m['inputs_sha256'], name
        for k, o in m['outputs'].items():
            nbytes = int(np.prod(o['shape'])) * np.dtype(o['dtype']).itemsize
            if nbytes <= bi.RAW_BYTES:
                g = golden[f'{name}.{k}']
                assert g.shape == tuple(o['shape']) and str(g.dtype) == o['dtype'] and 'sha256' not in o, (name, k)
                stored.add(f'{name}.{k}')
            else:
                assert len(o['sha256']) == 64, (name, k)
    assert stored == set(golden)


@pytest.mark.gpu
@pytest.mark.parametrize('name', bi.IDS)
def test_bits(name, manifest, golden):
    from stofnet_amd import _lib
    assert torch.cuda.is_available()
    m = manifest['cases'][name]
    got = bi.run(_lib.lib(), torch.device('cuda', 0), bi.case(name), m['seed'])
    assert sorted(got) == sorted(m['outputs'])
    bad = []
    for k, v in got.items():
        o = m['outputs'][k]
        assert list(v.shape) == o['shape'] and str(v.dtype) == o['dtype'], (name, k)
        if 'sha256' in o:
            same = bi.sha(v) == o['sha256']
            print(name, k, 'words', v.size, 'SHA-256', 'equal' if same else 'DIFFERS')
        else:
            word = {1: np.uint8, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize]
            differ = int((v.view(word) != golden[f'{name}.{k}'].view(word)).sum())
            print(name, k, 'words', v.size, 'differing', differ)
            same = differ == 0
        if not same:
            bad.append(k)
    assert not bad, (name, bad)

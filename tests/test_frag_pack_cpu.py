"""CPU check of pack_frag32 (stofnet_amd/csrc/mfma32_frag.h), the one packer of the A-operand fragment order of
v_mfma_f32_32x32x2_f32 behind every baseline's stof_*_pack_weights: the header is host/device neutral, so a g++-built
harness runs the very code the library runs, against a numpy restatement of the lane map.  One case per combination of
its three guards (output row beyond cout, input channel beyond cin inside cin_pad, k beyond the real K)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'cpu_harness', 'frag_harness.cpp')

# cout, cin, taps, cin_pad, ntiles, groups
CASES = {
    'no_padding': (64, 64, 3, 64, 2, 24),                # an EDSR 64 -> 64 convolution
    'short_cout': (3, 32, 3, 32, 1, 12),                 # ESPCN conv3 with r = 3
    'padded_cin': (50, 16, 10, 32, 2, 40),               # a Zonzini layer: 16 real channels stored 32 wide, 50 of 64 rows
    'linear': (32, 1, 1024, 1, 1, 128),                  # cin = cin_pad = 1, taps = K
    'short_k': (5, 1, 13, 1, 1, 2),                      # k runs past K = 13 inside the second group
}


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('frag') / 'frag_harness.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.frag_pack.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    lib.frag_pack.restype = None
    return lib


def lane_map(w, cin_pad, ntiles, groups):
    """Lane l (i = l & 31, h = l >> 5), element e of K group q of N tile nt holds W[32 nt + i][8 q + 4 h + e], where W is
    w [cout][cin][taps] laid out with k = tap * cin_pad + ci and zero wherever there is no weight."""
    cout, cin, taps = w.shape
    full = np.zeros((32 * ntiles, max(taps, -(-8 * groups // cin_pad)), cin_pad), np.float32)
    full[:cout, :taps, :cin] = w.transpose(0, 2, 1)
    dense = full.reshape(32 * ntiles, -1)[:, :8 * groups]
    nt, q, lane, e = np.ix_(np.arange(ntiles), np.arange(groups), np.arange(64), np.arange(4))
    return dense[32 * nt + (lane & 31), 8 * q + 4 * (lane >> 5) + e]


@pytest.mark.parametrize('name', CASES)
def test_pack_frag32_matches_the_lane_map(harness, name):
    cout, cin, taps, cin_pad, ntiles, groups = CASES[name]
    w = np.random.default_rng(cout * 1000 + taps).standard_normal((cout, cin, taps)).astype(np.float32)
    out = np.full((ntiles, groups, 64, 4), np.nan, np.float32)          # every element must be written
    harness.frag_pack(w.ctypes.data, cout, cin, taps, cin_pad, ntiles, groups, out.ctypes.data)
    want = lane_map(w, cin_pad, ntiles, groups)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(want) == w.size                             # every weight has its place, the rest is zero

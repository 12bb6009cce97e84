"""CPU checks of the training augmentation: the reference's import line, the numpy path of the three transforms against
the reference's recorded runs (tests/golden/f22_augment.npz, written by tests/golden/make_golden_augment.py), the Philox
layout of the device generator restated in numpy, the argument checks of the C ABI and main.py's batch order."""
import ctypes
import json
import os

import numpy as np
import pytest

import augment_inputs as ai
from conftest import GOLDEN, ROOT, golden

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Philox4x32-10 on uint32 arrays: ctr = 4 arrays (broadcastable), key = 2 values -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*ctr)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return [v.astype(np.uint32) for v in c]


def words_np(seed, rank, call, stream_id, N, L):
    """uint32 [N, L]: the generator's word for every (row, sample): key = (seed lo, seed hi), counter = (j >> 2, row, call,
    (rank << 1) | stream), word j & 3."""
    j = np.arange(L, dtype=np.uint64)[None, :]
    row = np.arange(N, dtype=np.uint64)[:, None]
    w = philox4x32_10((j >> np.uint64(2), row, np.uint64(call), np.uint64((rank << 1) | stream_id)),
                      (seed & 0xffffffff, (seed >> 32) & 0xffffffff))
    sel = np.broadcast_to(j & np.uint64(3), (N, L))
    return np.choose(sel.astype(np.int64), w)


def uniforms_np(seed, rank, call, stream_id, N, L):
    return ((words_np(seed, rank, call, stream_id, N, L) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def manifest():
    with open(os.path.join(GOLDEN, 'manifest_augment.json')) as f:
        return json.load(f)


def test_reference_import_line_resolves():
    from utils.transforms import NormalizeVol, CropChannelData, AddNoise      # reference main.py:25
    assert AddNoise().snr == 40
    c = CropChannelData()
    assert c.ratio is None and c.resize is False
    x = np.array([1., -4., 2.])
    assert np.array_equal(NormalizeVol()(x), x / 4)
    out = NormalizeVol()(x, 'a', k=1)
    assert isinstance(out, tuple) and out[1:] == ('a', 'k')                    # extra arguments and keyword names come back


@pytest.mark.parametrize('i', range(len(ai.CROP_CASES)))
def test_numpy_path_reproduces_the_reference_crop_chain(i):
    from stofnet_amd.transforms import AddNoise, CropChannelData, NormalizeVol
    g, rec = golden('f22_augment'), manifest()['crop'][i]
    L, ratio, gt = ai.CROP_CASES[i]
    assert (rec['L'], rec['ratio'], rec['gt']) == (L, ratio, gt)
    np.random.seed(rec['np_seed'])
    cropped, gt_out = CropChannelData(ratio=ratio)(NormalizeVol()(ai.row(L, rec['row_seed'])), gt)
    y = AddNoise(snr=ai.SNR_DB)(cropped)
    name = ai.crop_name(i)
    assert gt - gt_out == int(g[name + '_start']) and gt_out == float(g[name + '_gt'])
    ref = g[name + '_y']
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(name, 'rel err', err)
    assert err <= 1e-12


@pytest.mark.parametrize('L,kind', ai.NOISE_CASES)
def test_numpy_path_reproduces_the_reference_noise(L, kind):
    from stofnet_amd.transforms import AddNoise
    g = golden('f22_augment')
    rec = next(r for r in manifest()['noise'] if r['name'] == ai.noise_name(L, kind))
    np.random.seed(rec['np_seed'])
    y = AddNoise(snr=ai.SNR_DB)(ai.row(L, rec['row_seed'], kind))
    ref = g[rec['name'] + '_y']
    if kind == 'zero':
        assert not ref.any() and not y.any()
    else:
        assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


def test_numpy_path_resize_and_cpu_tensor():
    import torch
    from stofnet_amd.transforms import CropChannelData, NormalizeVol
    g, rec = golden('f22_augment'), manifest()['resize']
    x = NormalizeVol()(ai.row(rec['L'], rec['row_seed']))
    np.random.seed(rec['np_seed'])
    y, gt_out = CropChannelData(ratio=rec['ratio'], resize=True)(x, rec['gt'])
    assert abs(gt_out - float(g['resize_gt'])) <= 1e-12 * abs(float(g['resize_gt']))
    assert np.abs(y - g['resize_y']).max() <= 1e-12 * np.abs(g['resize_y']).max()
    # a CPU tensor takes the same numpy path and comes back as a tensor
    np.random.seed(rec['np_seed'])
    yt, gt_t = CropChannelData(ratio=rec['ratio'])(torch.from_numpy(x), rec['gt'])
    np.random.seed(rec['np_seed'])
    yn, gt_n = CropChannelData(ratio=rec['ratio'])(x, rec['gt'])
    assert isinstance(yt, torch.Tensor) and yt.device.type == 'cpu' and np.array_equal(yt.numpy(), yn) and gt_t == gt_n
    # ratio=None: drawn once from torch.rand, then kept; ratios outside (0, 1) hand the inputs back
    c = CropChannelData()
    torch.manual_seed(5)
    c(x, rec['gt'])
    torch.manual_seed(5)
    assert c.ratio == float(torch.rand(1))
    same = CropChannelData(ratio=1.5)(x, rec['gt'], 'extra')
    assert same[0] is x and same[1:] == (rec['gt'], 'extra')


@pytest.mark.parametrize('j', range(len(ai.RAISE_CASES)))
def test_numpy_path_raises_where_the_reference_does(j):
    from stofnet_amd.transforms import CropChannelData, NormalizeVol
    rec = manifest()['raises'][j]
    L, ratio, gt = ai.RAISE_CASES[j]
    assert (rec['L'], rec['ratio'], rec['gt']) == (L, ratio, gt)
    exc = {'ValueError': ValueError, 'AssertionError': AssertionError}[rec['exception']]
    np.random.seed(rec['np_seed'])
    with pytest.raises(exc):
        CropChannelData(ratio=ratio)(NormalizeVol()(ai.row(L, rec['row_seed'])), gt)


@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(ctr, key)
    assert ' '.join(f'{int(v):08x}' for v in got) == want


def test_philox_layout_of_the_uniforms():
    seed = 0xab12345678
    w = words_np(seed, 3, 7, 1, 2, 9)
    one = philox4x32_10((1, 1, 7, (3 << 1) | 1), (seed & 0xffffffff, seed >> 32))       # row 1, samples 4..7
    assert [int(v) for v in w[1, 4:8]] == [int(v) for v in one]
    u = uniforms_np(seed, 3, 7, 1, 2, 9)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()


def test_stof_augment_argument_errors_need_no_device():
    from stofnet_amd import _lib
    from stofnet_amd import build as sbuild
    sbuild.build(verbose=False)
    lib = _lib.lib()
    P = ctypes.c_void_p
    x, gt, y, go, st = P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000)       # never dereferenced: no launch happens

    def call(desc, x=x, gt=gt, N=4, L=2000, G=1, y=y, go=go, st=st):
        return lib.stof_augment(ctypes.byref(desc) if desc is not None else None, x, gt, N, L, G, None, None, y, go, st, None)

    ok = _lib.AugmentDesc(1, 0.75, 30.0, 1, 1, 0, 0)
    assert lib.stof_augment(None, x, gt, 4, 2000, 1, None, None, y, go, st, None) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, x=None) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, y=None) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, st=None) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, gt=None) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, go=None) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, y=x) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, N=-1) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, gt=None, go=None, G=0) == _lib.STOF_ERR_BAD_ARG              # a crop needs a gt column
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert call(_lib.AugmentDesc(1, 0.75, bad, 1, 1, 0, 0)) == _lib.STOF_ERR_BAD_ARG
    assert call(_lib.AugmentDesc(1, 0.75, 30.0, 1, 1, 1 << 31, 0)) == _lib.STOF_ERR_BAD_ARG
    assert call(ok, L=2001) == _lib.STOF_ERR_UNSUPPORTED                          # width 1501
    assert call(ok, N=0) == _lib.STOF_OK and call(ok, L=0) == _lib.STOF_OK        # nothing to do: no launch
    assert call(ok, N=0, L=2001) == _lib.STOF_ERR_UNSUPPORTED                     # the checks come first
    assert lib.stof_augment_uniforms(1, 0, 0, 0, None, 4, 8, None) == _lib.STOF_ERR_BAD_ARG
    assert lib.stof_augment_uniforms(1, 0, 0, 2, y, 4, 8, None) == _lib.STOF_ERR_BAD_ARG
    assert lib.stof_augment_uniforms(1, 0, 0, 1, y, 0, 8, None) == _lib.STOF_OK


def test_crop_width_rounds_half_to_even():
    from stofnet_amd.augment import crop_width
    assert crop_width(6, .75) == 4 and crop_width(2000, .75) == 1500 and crop_width(2001, .75) == 1501     # half to even
    assert crop_width(2000, None) == 2000 and crop_width(2000, 1.5) == 2000 and crop_width(2000, 0) == 2000


def test_default_batch_order_is_unchanged():
    import main as entry
    from stofnet_amd import config as config_mod
    from stofnet_amd.sharding import rank_batches
    cfg = config_mod.load(os.path.join(ROOT, 'config.yaml'))
    assert cfg.augment is False and cfg.shuffle is False
    for world in (1, 2, 3):
        for rank in range(world):
            for epoch in (0, 5):
                got = entry.epoch_batches(23, 4, epoch, rank, world)
                assert got == [(b, slice(4 * b, 4 * b + 4)) for b in rank_batches(23 // 4, rank, world)]


def test_shuffle_is_one_permutation_for_all_ranks():
    import main as entry
    n, bs = 46, 4

    def epoch_rows(world, epoch, seed=11):
        per_batch = {}
        for rank in range(world):
            for b, rows in entry.epoch_batches(n, bs, epoch, rank, world, True, seed):
                assert b not in per_batch and len(rows) == bs
                per_batch[b] = np.asarray(rows)
        return per_batch

    one, two, four = epoch_rows(1, 0), epoch_rows(2, 0), epoch_rows(4, 0)
    assert sorted(one) == list(range(n // bs))
    for b, rows in two.items():
        assert np.array_equal(rows, one[b])
    for b, rows in four.items():
        assert np.array_equal(rows, one[b])
    flat = np.concatenate([one[b] for b in sorted(one)])
    assert len(set(flat.tolist())) == flat.size and flat.max() < n                  # rows of a permutation: none twice
    assert not np.array_equal(flat, np.arange(flat.size))
    again, other_epoch, other_seed = epoch_rows(1, 0), epoch_rows(1, 1), epoch_rows(1, 0, seed=12)
    assert all(np.array_equal(again[b], one[b]) for b in one)
    assert any(not np.array_equal(other_epoch[b], one[b]) for b in one)
    assert any(not np.array_equal(other_seed[b], one[b]) for b in one)

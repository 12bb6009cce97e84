"""The two-pass training sweeps and the split-row route, stage by stage (tests/split_route_inputs.py has the shapes, the codec
and the float64 references; tests/test_split_route_refs_cpu.py pins them).

On a 256-CU device every other training test lands on the r3 sweep kernel with fp32 dumps: the two-pass kernel needs at least
384 stream rows per (virtual) waveform, and the launch cuts the suite's small batches into short segments.  Here:

  * the small split-row kernels bit for bit (stof_train_to_split_rows, stof_train_add_split / _split2,
    stof_train_conv_last_dgrad_split) and their return codes;
  * stof_train_wgrad_batch_split on both of its kernels (every operand split: conv_wgrad_split_async16_kernel; mixed split
    bits and stof_train_wgrad_batch: the register-staged conv_wgrad_f16x3_batch_kernel) where a work-group takes a second
    tile: dyadic operands bitwise, Gaussian operands at max(2e-6, 4 x e32);
  * stof_train_sweep / _split and stof_train_sweep_bwd / _split through the C ABI with stof_net_desc.seg_policy forcing the
    geometry, every dump tensor against its float64 stage reference computed from the kernel's OWN previous tensor at 2e-6 x
    max|ref|, next to the layer kernel (stof_train_conv, f16x3) on the same operands;
  * the whole step where the engine itself picks the split route, against float64 autograd, and the same step on fp32 dumps.

Figures go to profiles/split_route.jsonl.  The float64 references are matmuls / autograd on the device; they never touch the
kernels under test."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import multi_tile_inputs as mt
import split_route_inputs as sr
from stofnet_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'split_route.jsonl')
BOUND = sr.STAGE_BOUND
OUT_SCALE = 0.25
CANARY_FLOATS = 4096


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib(dev):
    from stofnet_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _nan(shape, dev):
    return torch.full(tuple(shape), float('nan'), device=dev)


def _rounded(v):
    return float(f'{v:.3e}')


def _record(entries):
    """print the cases' figures and keep them in profiles/split_route.jsonl: one line per case; the lines of cases that this
    session did not run stay as they are (test_gpu_multi_tile._record, several cases at once)"""
    lines = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            for ln in fh.read().splitlines():
                if ln.strip():
                    lines[json.loads(ln)['case']] = ln
    for name, entry in entries.items():
        print(name, json.dumps(entry))
        lines[name] = json.dumps({'case': name, **entry})
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines[k] for k in sorted(lines)) + '\n')
    except OSError as exc:
        print(f'{PROFILE} not written: {exc}')


def _off_by_4_bytes(t):
    """the same values 4 bytes off a 16-byte boundary"""
    big = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    out = big[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


# --------------------------------------------------------------------------------------------- the small split-row kernels
def _edge_rows(rows, seed, dev):
    """Gaussian rows with the codec's edge values in front: fp16 subnormals and below, values next to 65504"""
    v = sr.gauss((rows, 64), seed)
    edge = sr.codec_edge_values()[:rows]
    v[:edge.shape[0]] = edge
    return v.to(dev)


@pytest.mark.parametrize('rows', sr.ROW_COUNTS)
def test_to_split_rows_is_the_codec(lib, dev, rows):
    """stof_train_to_split_rows = to_split byte for byte: dyadic operands (lo = 0) and Gaussian ones with values below 2^-14 and
    next to 65504 (the definition is deterministic: hi = fp16(v), lo = fp16(v - hi), round to nearest even)."""
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    for v in (mt.ints((rows, 64), 10 + rows, dev), _edge_rows(rows, 20 + rows, dev)):
        out = _nan((rows + 1, 64), dev)
        _lib.check(lib.stof_train_to_split_rows(_lib.ptr(v), _lib.ptr(out), rows, st), 'stof_train_to_split_rows')
        assert sr.same_bits(out[:rows], sr.to_split(v))
        assert torch.isnan(out[rows]).all()                                                   # nothing behind the last row
    assert float(v.abs().max()) > 65000 and float(v.abs()[v != 0].min()) < 2.0 ** -14
    assert (sr.split_halves(sr.to_split(v))[1] != 0).any()


@pytest.mark.parametrize('rows', sr.ROW_COUNTS)
def test_add_split_kernels(lib, dev, rows):
    """stof_train_add_split: out = (hi + lo) + b, stof_train_add_split2: out = (hi_a + lo_a) + (hi_b + lo_b), each bracket and
    the final sum one fp32 addition (add_split_kernel): bitwise on dyadic and on Gaussian operands."""
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    for a, b in ((mt.ints((rows, 64), 30 + rows, dev), mt.dyadic((rows, 64), -100, 100, 0.25, 31 + rows, dev)),
                 (sr.gauss((rows, 64), 32 + rows, dev), sr.gauss((rows, 64), 33 + rows, dev))):
        a_s, b_s = sr.to_split(a), sr.to_split(b)
        for fn, second, want in ((lib.stof_train_add_split, b, sr.from_split(a_s) + b),
                                 (lib.stof_train_add_split2, b_s, sr.from_split(a_s) + sr.from_split(b_s))):
            out = _nan((rows + 1, 64), dev)
            _lib.check(fn(_lib.ptr(a_s), _lib.ptr(second), _lib.ptr(out), rows, st), 'stof_train_add_split')
            assert sr.same_bits(out[:rows], want) and torch.isnan(out[rows]).all()
    d = mt.ints((rows, 64), 30 + rows, dev)
    assert torch.equal(sr.from_split(sr.to_split(d)), d)                                      # dyadic: from_split(a) IS a


@pytest.mark.parametrize('N,L', sr.CONV_LAST_SHAPES)
@pytest.mark.parametrize('r', [4, 10])
def test_conv_last_dgrad_split(lib, dev, r, N, L):
    """stof_train_conv_last_dgrad_split = to_split of what stof_train_conv_last_dgrad writes, byte for byte, and within
    test_conv_last_data_gradient_kernel's bound (2e-6 x max) of conv_transpose1d in float64."""
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    dz, w = sr.gauss((N, L, r), r * 100 + L, dev), sr.gauss((r, 64, 3), r * 100 + L + 1, dev)
    plain, split = _nan((N, L, 64), dev), _nan((N, L, 64), dev)
    _lib.check(lib.stof_train_conv_last_dgrad(_lib.ptr(dz), _lib.ptr(w), _lib.ptr(plain), N, L, r, st), 'conv_last_dgrad')
    _lib.check(lib.stof_train_conv_last_dgrad_split(_lib.ptr(dz), _lib.ptr(w), _lib.ptr(split), N, L, r, st), 'conv_last_dgrad_split')
    assert not torch.isnan(plain).any()
    assert sr.same_bits(split, sr.to_split(plain))
    ref = sr.conv_t(dz.double(), w.double())
    assert sr.rel(sr.from_split(split, torch.float64), ref) < 2e-6 and sr.rel(plain, ref) < 2e-6
    assert lib.stof_train_conv_last_dgrad_split(_lib.ptr(dz), _lib.ptr(w), _lib.ptr(split), N, L, 20, st) == _lib.STOF_ERR_UNSUPPORTED


def test_small_split_kernels_return_codes(lib, dev):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    a, b = sr.gauss((16, 64), 1, dev), sr.gauss((16, 64), 2, dev)
    a4, out = _off_by_4_bytes(a), _nan((16, 64), dev)
    out4 = _off_by_4_bytes(out)
    BAD, OK = _lib.STOF_ERR_BAD_ARG, _lib.STOF_OK
    assert lib.stof_train_to_split_rows(None, _lib.ptr(out), 16, st) == BAD
    assert lib.stof_train_to_split_rows(_lib.ptr(a), None, 16, st) == BAD
    assert lib.stof_train_to_split_rows(_lib.ptr(a4), _lib.ptr(out), 16, st) == BAD
    assert lib.stof_train_to_split_rows(_lib.ptr(a), _lib.ptr(out4), 16, st) == BAD
    assert lib.stof_train_to_split_rows(_lib.ptr(a), _lib.ptr(out), 0, st) == OK
    for fn in (lib.stof_train_add_split, lib.stof_train_add_split2):
        assert fn(None, _lib.ptr(b), _lib.ptr(out), 16, st) == BAD
        assert fn(_lib.ptr(a), None, _lib.ptr(out), 16, st) == BAD
        assert fn(_lib.ptr(a), _lib.ptr(b), None, 16, st) == BAD
        assert fn(_lib.ptr(a4), _lib.ptr(b), _lib.ptr(out), 16, st) == BAD
        assert fn(_lib.ptr(a), _lib.ptr(a4), _lib.ptr(out), 16, st) == BAD
        assert fn(_lib.ptr(a), _lib.ptr(b), _lib.ptr(out4), 16, st) == BAD
        assert fn(_lib.ptr(a), _lib.ptr(b), _lib.ptr(out), 0, st) == OK
    dz, w = sr.gauss((1, 7, 4), 3, dev), sr.gauss((4, 64, 3), 4, dev)
    o7 = _nan((1, 7, 64), dev)
    assert lib.stof_train_conv_last_dgrad_split(None, _lib.ptr(w), _lib.ptr(o7), 1, 7, 4, st) == BAD
    assert lib.stof_train_conv_last_dgrad_split(_lib.ptr(dz), None, _lib.ptr(o7), 1, 7, 4, st) == BAD
    assert lib.stof_train_conv_last_dgrad_split(_lib.ptr(dz), _lib.ptr(w), None, 1, 7, 4, st) == BAD
    # `out` is written with vector stores and read as 16-byte pieces by the backward sweep and the weight-gradient kernel: 16-byte
    # aligned or STOF_ERR_BAD_ARG, in both entry points; dz and weight are read float by float (any fp32 pointer, see the header)
    o7m = _off_by_4_bytes(o7)
    for fn in (lib.stof_train_conv_last_dgrad_split, lib.stof_train_conv_last_dgrad):
        assert fn(_lib.ptr(dz), _lib.ptr(w), _lib.ptr(o7m), 1, 7, 4, st) == BAD
    assert lib.stof_train_conv_last_dgrad_split(_lib.ptr(dz), _lib.ptr(w), _lib.ptr(o7), 0, 7, 4, st) == OK
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(out4).all() and torch.isnan(o7).all() and torch.isnan(o7m).all()       # nothing written
    dz4, w4 = _off_by_4_bytes(dz), _off_by_4_bytes(w)
    _lib.check(lib.stof_train_conv_last_dgrad_split(_lib.ptr(dz4), _lib.ptr(w4), _lib.ptr(o7), 1, 7, 4, st), 'conv_last_dgrad_split')
    assert sr.rel(sr.from_split(o7, torch.float64), sr.conv_t(dz.double(), w.double())) < 2e-6


# ------------------------------------------------------------------------------------------ stof_train_wgrad_batch_split
def _ptrs(ts):
    from stofnet_amd import _lib
    return (ctypes.c_void_p * len(ts))(*[_lib.ptr(t) for t in ts])


def _batch_groups(lib, count):
    return sr.wgrad_batch_groups(lib.stof_train_wgrad_batch_workspace_bytes(count, 7), count)


_batch_cache = {}


def _batch_case(lib, dev, count, which, mode):
    """operands (fp32 and split rows) and the float64 reference of one (count, shape, kind of operand), shared by the tests"""
    key = (count, which, mode)
    if key not in _batch_cache:
        _batch_cache.clear()
        G = _batch_groups(lib, count)
        N, L = mt.tile_shapes(G, mt.WGRAD_TILE[mt.F16X3])[which]
        tiles = mt.tiles_of(N, L, mt.WGRAD_TILE[mt.F16X3])
        assert tiles > G and sr.in_loop_range(tiles, G), (tiles, G)          # some work-groups take a second tile, others one
        c = dict(N=N, L=L, G=G, x=[], dy=[], xs=[], dys=[], dw=[], db=[], e32=[])
        for i in range(count):
            if mode == 'dyadic':
                x, dy = mt.ints((N, L, 64), 1000 * count + 2 * i, dev), mt.ints((N, L, 64), 1000 * count + 2 * i + 1, dev)
            else:
                x, dy = sr.gauss((N, L, 64), 2000 * count + 2 * i, dev), sr.gauss((N, L, 64), 2000 * count + 2 * i + 1, dev, 0.25)
            xs, dys = sr.to_split(x), sr.to_split(dy)
            if mode == 'dyadic':
                assert not sr.split_halves(xs)[1].any() and not sr.split_halves(dys)[1].any()          # fp16 numbers: lo = 0
                sums, bsum = mt.wgrad_ref(x.double().abs(), dy.double().abs(), 7)
                mt.headroom(max(float(sums.max()), float(bsum.max())), 0)            # (out_scale: a power of two, exact)
            else:
                assert sr.split_halves(xs)[1].any() and sr.split_halves(dys)[1].any()
                x, dy = sr.from_split(xs), sr.from_split(dys)                   # the reference reads the decoded operands
                d32 = mt.wgrad_ref(x, dy, 7)
                c['e32'].append(d32)
            dw, db = mt.wgrad_ref(x.double(), dy.double(), 7)
            for k, v in zip(('x', 'dy', 'xs', 'dys', 'dw', 'db'), (x, dy, xs, dys, dw, db)):
                c[k].append(v)
        _batch_cache[key] = c
    return _batch_cache[key]


def _run_batch(lib, dev, c, count, x_bits, dy_bits, out_scale, entry='split'):
    """one batched weight gradient twice into NaN-prefilled outputs through a 0xff-filled workspace -> ([dw], [db])"""
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    N, L = c['N'], c['L']
    xin = [c['xs'][i] if (x_bits >> i) & 1 else c['x'][i] for i in range(count)]
    dyin = [c['dys'][i] if (dy_bits >> i) & 1 else c['dy'][i] for i in range(count)]
    ws = torch.empty(lib.stof_train_wgrad_batch_workspace_bytes(count, 7), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        dw, db = [_nan((64, 64, 7), dev) for _ in range(count)], [_nan((64,), dev) for _ in range(count)]
        ws.fill_(0xff)
        if entry == 'split':
            code = lib.stof_train_wgrad_batch_split(_ptrs(xin), _ptrs(dyin), _ptrs(dw), _ptrs(db), count, x_bits, dy_bits, N, L, 7,
                                                    out_scale, _lib.ptr(ws), ws.numel(), st)
        else:
            assert x_bits == 0 and dy_bits == 0
            code = lib.stof_train_wgrad_batch(_ptrs(xin), _ptrs(dyin), _ptrs(dw), _ptrs(db), count, N, L, 7, out_scale, _lib.ptr(ws),
                                              ws.numel(), st)
        _lib.check(code, 'stof_train_wgrad_batch' + ('_split' if entry == 'split' else ''))
        runs.append((dw, db))
    for i in range(count):
        assert torch.equal(runs[0][0][i], runs[1][0][i]) and torch.equal(runs[0][1][i], runs[1][1][i]), i      # no float atomics
    return runs[0]


def _assert_exact(c, count, got, out_scale, what):
    for i in range(count):
        assert torch.equal(got[0][i], mt.exact_fp32(out_scale * c['dw'][i])), (what, i, 'dw')
        assert torch.equal(got[1][i], mt.exact_fp32(out_scale * c['db'][i])), (what, i, 'db')


@pytest.mark.parametrize('which', ['short', 'long'])
@pytest.mark.parametrize('count', [11, 3])
def test_wgrad_batch_split_second_tile_exact(lib, dev, count, which):
    """Every operand split, dyadic (lo = 0), K = 7: the one case wgrad_batch_impl (train.hip) sends to
    conv_wgrad_split_async16_kernel.  dw and db of every layer bitwise equal to the float64 reference, at a layer count that
    gives few groups many tiles (11: G = 46 on a 256-CU device) and one that gives many groups few (3: G = 170).  One dropped,
    doubled or stale tile, one wrong swizzle slot or tap offset fails it.
    What this cannot show: WHICH kernel ran.  On dyadic operands the register-staged kernel gives the same bits; that all-split
    operands reach the global_load_lds kernel is read off the dispatch, not observed.  Indirect evidence only: breaking the copy
    of conv_wgrad_split_async16_kernel alone failed exactly these cases."""
    c = _batch_case(lib, dev, count, which, 'dyadic')
    bits = (1 << count) - 1
    _assert_exact(c, count, _run_batch(lib, dev, c, count, bits, bits, OUT_SCALE), OUT_SCALE, (count, which))


@pytest.mark.parametrize('which', ['short', 'long'])
@pytest.mark.parametrize('count', [11, 3])
def test_wgrad_batch_mixed_operands_exact(lib, dev, count, which):
    """conv_wgrad_f16x3_batch_kernel, which every batch with one operand that is not split reaches, and its split staging: x
    split and dy fp32, the reverse, alternating layers; then fp32 operands through both entry points.  The last line is all
    split again (conv_wgrad_split_async16_kernel) at out_scale = 2^-10 (a power of two: still bitwise)."""
    c = _batch_case(lib, dev, count, which, 'dyadic')
    bits = (1 << count) - 1
    alt = 0x555 & bits
    for xb, db_ in ((bits, 0), (0, bits), (alt, bits ^ alt), (0, 0)):
        _assert_exact(c, count, _run_batch(lib, dev, c, count, xb, db_, OUT_SCALE), OUT_SCALE, (count, which, xb, db_))
    _assert_exact(c, count, _run_batch(lib, dev, c, count, 0, 0, OUT_SCALE, entry='fp32'), OUT_SCALE, (count, which, 'fp32'))
    _assert_exact(c, count, _run_batch(lib, dev, c, count, bits, bits, 2.0 ** -10), 2.0 ** -10, (count, which, 'scale'))


@pytest.mark.parametrize('count', [11, 3])
def test_wgrad_batch_split_second_tile_gaussian(lib, dev, count):
    """conv_wgrad_split_async16_kernel (every operand split) on Gaussian operands with a non-zero lo, at the long shape, so that
    the lo halves and the hi*lo / lo*hi products count: rel(dw), rel(db) <= max(2e-6, 4 x e32), e32 the deviation from float64
    of the same gradient evaluated by torch in fp32 (the rule and margin of test_gpu_multi_tile)."""
    c = _batch_case(lib, dev, count, 'long', 'gauss')
    bits = (1 << count) - 1
    dw, db = _run_batch(lib, dev, c, count, bits, bits, OUT_SCALE)
    worst = {}
    for tag, got, k in (('dw', dw, 0), ('db', db, 1)):
        err = max(sr.rel(got[i], OUT_SCALE * c[tag][i]) for i in range(count))
        e32 = max(sr.rel(c['e32'][i][k], c[tag][i]) for i in range(count))
        worst[tag] = (err, max(2e-6, 4 * e32), e32)
    _record({f'wgrad_batch_split count {count}': {
        'rows': c['N'] * c['L'], 'G': c['G'],
        **{t: {'kernel': _rounded(v[0]), 'e32': _rounded(v[2]), 'bound': _rounded(v[1])} for t, v in worst.items()}}})
    for tag, (err, bound, _) in worst.items():
        assert err <= bound, (count, tag, err, bound)


def test_wgrad_batch_split_return_codes(lib, dev):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    count, N, L = 3, 2, 70
    x = [sr.to_split(mt.ints((N, L, 64), 50 + i, dev)) for i in range(count)]
    dy = [sr.to_split(mt.ints((N, L, 64), 60 + i, dev)) for i in range(count)]
    dw, db = [_nan((64, 64, 7), dev) for _ in range(count)], [_nan((64,), dev) for _ in range(count)]
    need = lib.stof_train_wgrad_batch_workspace_bytes(count, 7)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda xs, dys, n, nbytes: lib.stof_train_wgrad_batch_split(_ptrs(xs), _ptrs(dys), _ptrs(dw), _ptrs(db), count, 7, 7, n, L, 7,      # noqa: E731
                                                                       1.0, _lib.ptr(ws), nbytes, st)
    assert call([x[0], _off_by_4_bytes(x[1]), x[2]], dy, N, need) == _lib.STOF_ERR_BAD_ARG
    assert call(x, [dy[0], dy[1], _off_by_4_bytes(dy[2])], N, need) == _lib.STOF_ERR_BAD_ARG
    assert call(x, dy, N, need - 1) == _lib.STOF_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in dw + db)
    assert call(x, dy, 0, need) == _lib.STOF_OK
    assert all(not t.any() for t in dw + db)                                                   # an empty batch: zeros
    _lib.check(call(x, dy, N, need), 'stof_train_wgrad_batch_split')
    ref = [mt.wgrad_ref(sr.from_split(a, torch.float64), sr.from_split(b, torch.float64), 7) for a, b in zip(x, dy)]
    assert all(torch.equal(dw[i], mt.exact_fp32(ref[i][0])) and torch.equal(db[i], mt.exact_fp32(ref[i][1])) for i in range(count))


# ------------------------------------------------------------------------------------- the sweeps, stage by stage (C ABI)
SWEEP_RUNS = [(case, r, scale) for case in sr.CASES for r, scale in ((4, 80), (10, 80), (4, 1), (10, 1))]
CANARY = 12345.5


class _Sweeps:
    """one (case, r, scale): parameters, operands and the packed blobs; runs the four sweep entry points"""

    def __init__(self, lib, dev, cus, case, r, scale):
        from stofnet_amd import _lib
        self.lib, self.dev, self.case, self.r, self.scale = lib, dev, case, r, scale
        self.N, self.L, policy = sr.case_shape(case, cus)
        N, L = self.N, self.L
        self.st = _lib.stream_ptr(dev)
        sd = synth.synth_state_dict(r, seed=500 + r + scale, semi_global_scale=scale)
        self.p = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
        self.p64 = {k: v.double() for k, v in self.p.items()}
        self.x = torch.from_numpy(synth.synth_echo(N, L, seed=7 + L))[:, 0].contiguous().to(dev)
        self.e = sr.gauss((N, L // sr.SGB_SCALE, 64), 11 + L, dev, 0.1) if scale != 1 else None
        self.g6 = sr.gauss((N, L, 64), 13 + L, dev, 0.25)                       # like a loss-scaled gradient: largest entries ~ 1
        self.desc = _lib.NetDesc(r, scale, _lib.PREC_F16X3, policy)
        nbytes = lib.stof_train_sweep_blob_bytes(ctypes.byref(self.desc))
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.blob_bwd = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        names = ['conv1'] + [f'conv{i}' for i in range(2, 13)] + ['conv_last']
        arr = (ctypes.c_void_p * 26)()
        for i, nm in enumerate(names):
            arr[2 * i], arr[2 * i + 1] = _lib.ptr(self.p[nm + '.weight']), _lib.ptr(self.p[nm + '.bias'])
        _lib.check(lib.stof_train_sweep_pack(ctypes.byref(self.desc), arr, _lib.ptr(self.blob), self.st), 'stof_train_sweep_pack')
        _lib.check(lib.stof_train_sweep_bwd_pack(_ptrs([self.p[f'conv{i}.weight'] for i in range(2, 13)]), _lib.ptr(self.blob_bwd),
                                                 self.st), 'stof_train_sweep_bwd_pack')
        self.floats = lib.stof_train_sweep_dump_floats(N, L)
        assert self.floats == 12 * N * L * 64 + 1024

    def buffer(self):
        """NaN-filled dump of exactly stof_train_sweep_dump_floats floats inside a larger buffer whose rest holds a canary"""
        buf = _nan((self.floats + CANARY_FLOATS,), self.dev)
        buf[self.floats:] = CANARY
        assert buf.data_ptr() % 16 == 0
        return buf

    def tensors(self, buf):
        return buf[:12 * self.N * self.L * 64].view(12, self.N, self.L, 64)

    def canary_ok(self, buf):
        return bool((buf[self.floats:] == CANARY).all())

    def forward(self, split, n=None):
        from stofnet_amd import _lib
        buf, y = self.buffer(), _nan((self.N, self.L * self.r), self.dev)
        fn = self.lib.stof_train_sweep_split if split else self.lib.stof_train_sweep
        code = fn(ctypes.byref(self.desc), _lib.ptr(self.blob), _lib.ptr(self.x), _lib.ptr(self.e), _lib.ptr(buf), _lib.ptr(y),
                  self.N if n is None else n, self.L, self.st)
        return code, buf, y

    def backward(self, split, g6, fwd_buf, n=None):
        from stofnet_amd import _lib
        buf = self.buffer()
        fn = self.lib.stof_train_sweep_bwd_split if split else self.lib.stof_train_sweep_bwd
        code = fn(ctypes.byref(self.desc), _lib.ptr(self.blob_bwd), _lib.ptr(g6), _lib.ptr(fwd_buf), _lib.ptr(buf),
                  self.N if n is None else n, self.L, self.st)
        return code, buf

    # ---- the layer kernels the suite already tests, on the same operands
    def image(self, w, flip):
        from stofnet_amd import _lib
        co, ci, K = w.shape
        out = torch.empty(self.lib.stof_train_repack_floats(co, ci, K, flip, mt.F16X3), device=self.dev)
        _lib.check(self.lib.stof_train_repack(_lib.ptr(w), _lib.ptr(out), co, ci, K, flip, mt.F16X3, self.st), 'stof_train_repack')
        return out

    def conv(self, x, name, flip, bias, residual, saved, act, cout=64, K=7):
        from stofnet_amd import _lib
        y = _nan((self.N, self.L, cout), self.dev)
        b = self.p[name + '.bias'] if bias else None
        _lib.check(self.lib.stof_train_conv(_lib.ptr(x.contiguous()), _lib.ptr(self.image(self.p[name + '.weight'], flip)), _lib.ptr(b),
                                            _lib.ptr(residual), _lib.ptr(saved), _lib.ptr(y), self.N, self.L, 64, cout, K, act, mt.F16X3,
                                            self.st), 'stof_train_conv')
        return y

    def layer_forward(self, t32):
        """stage -> output of the layer kernels on the decoded fp32 operands"""
        from stofnet_amd import _lib
        N, L, lib = self.N, self.L, self.lib
        a1 = _nan((N, L, 64), self.dev)
        _lib.check(lib.stof_train_conv1(_lib.ptr(self.x), _lib.ptr(self.p['conv1.weight']), _lib.ptr(self.p['conv1.bias']), _lib.ptr(a1),
                                        N, L, self.st), 'stof_train_conv1')
        out = {0: a1}
        if self.e is not None:
            P = L // sr.SGB_SCALE
            out[0] = _nan((N, L, 64), self.dev)
            _lib.check(lib.stof_train_upsample_add(_lib.ptr(a1), _lib.ptr(self.e), _lib.ptr(out[0]), N, L, P, (L - P * sr.SGB_SCALE) // 2,
                                                   sr.SGB_SCALE, self.st), 'stof_train_upsample_add')
        for k in range(5):
            out[2 * k + 1] = self.conv(t32[2 * k], f'conv{2 * k + 2}', 0, True, None, None, mt.ACT_LRELU)
            out[2 * k + 2] = self.conv(t32[2 * k + 1], f'conv{2 * k + 3}', 0, True, t32[2 * k].contiguous(), None, mt.ACT_NONE)
        out[11] = self.conv(t32[10], 'conv12', 0, True, t32[0].contiguous(), None, mt.ACT_NONE)
        out['y'] = self.conv(t32[11], 'conv_last', 0, True, None, None, mt.ACT_NONE, cout=self.r, K=3).reshape(N, L * self.r)
        return out

    def layer_backward(self, g32, T32, y32):
        out = {1: self.conv(g32, 'conv12', 1, False, None, None, mt.ACT_NONE)}
        for k in range(4, -1, -1):
            out[10 - 2 * k] = self.conv(T32[9 - 2 * k], f'conv{2 * k + 3}', 1, False, None, y32[k].contiguous(), mt.ACT_LRELU)
            out[11 - 2 * k] = self.conv(T32[10 - 2 * k], f'conv{2 * k + 2}', 1, False, T32[9 - 2 * k].contiguous(), None, mt.ACT_NONE)
        return out


def _decode(t, i, split, dtype):
    return sr.from_split(t[i], dtype) if split and i <= 10 else t[i].to(dtype)


def _unwritten(t, idx, split):
    """elements of the tensors `idx` that still hold the NaN prefill (split rows: a NaN fp16 half; no finite half pair reads as an
    fp32 NaN and the prefill's upper half is an fp16 NaN, so either view finds an unwritten element)"""
    n = 0
    for i in idx:
        v = t[i].contiguous()
        n += int(torch.isnan(v.view(torch.float16) if split and i <= 10 else v).sum())
    return n


def _positive(fwd_t, k, split):
    """the route's rule: fp32 dumps -> the fp32 value > 0; split dumps -> the hi half > 0 (|y| < 2^-25 is not positive)"""
    y = fwd_t[2 * k + 1]
    return sr.split_halves(y)[0] > 0 if split else y > 0


def _measure_forward(s, split, fbuf, y):
    """one forward sweep -> (stage errors {0..11, 'y'}, the layer kernels' errors, elements left unwritten, canary intact)"""
    ft = s.tensors(fbuf)
    t64 = [_decode(ft, i, split, torch.float64) for i in range(12)]
    ref, yref = sr.forward_refs(s.p64, s.x.double(), None if s.e is None else s.e.double(), s.r, given=t64)
    errs = {i: sr.rel(t64[i], ref[i]) for i in range(12)}
    errs['y'] = sr.rel(y, yref)
    lay = s.layer_forward([_decode(ft, i, split, torch.float32) for i in range(12)])
    layer = {i: sr.rel(lay[i], yref if i == 'y' else ref[i]) for i in lay}
    return errs, layer, _unwritten(ft, range(12), split) + int(torch.isnan(y).sum()), s.canary_ok(fbuf)


def _measure_backward(s, split, ft, g6s, bbuf):
    """one backward sweep on the forward tensors ft -> (stage errors {1..11}, layer kernels' errors, unwritten, canary, mask fractions)"""
    bt = s.tensors(bbuf)
    g64 = sr.from_split(g6s, torch.float64) if split else s.g6.double()
    T64 = {j: (sr.from_split(bt[j], torch.float64) if split else bt[j].double()) for j in range(1, 12)}
    positive = [_positive(ft, k, split) for k in range(5)]
    bref = sr.backward_refs(s.p64, g64, positive, given=T64)
    errs = {j: sr.rel(T64[j], bref[j]) for j in range(1, 12)}
    T32 = {j: (sr.from_split(bt[j]) if split else bt[j]) for j in range(1, 12)}
    y32 = [_decode(ft, 2 * k + 1, split, torch.float32) for k in range(5)]
    lay = s.layer_backward(sr.from_split(g6s) if split else s.g6, T32, y32)
    layer = {j: sr.rel(lay[j], bref[j]) for j in lay}
    return errs, layer, _unwritten(bt, range(1, 12), split), s.canary_ok(bbuf), [float(q.float().mean()) for q in positive]


def _measure_planted(s, split, fbuf, g6, signs):
    """exact zeros and +-2^-26 planted in a copy of forward tensor 1 (the mask of T[10]), one backward run -> the error of T[10]
    against the reference under the route's own rule (mask read off the planted bytes), under the hi-half rule and under the fp32
    rule, and how many masks the two rules decide differently"""
    from stofnet_amd import _lib
    pbuf = fbuf.clone()
    planted = sr.plant(_decode(s.tensors(fbuf), 1, split, torch.float32), signs)
    s.tensors(pbuf)[1] = sr.to_split(planted) if split else planted
    code, pb = s.backward(split, g6, pbuf)
    _lib.check(code, 'stof_train_sweep_bwd (planted)')
    pt = s.tensors(pb)
    got10 = sr.from_split(pt[10], torch.float64) if split else pt[10].double()
    pre10 = sr.conv_t(sr.from_split(pt[9], torch.float64) if split else pt[9].double(), s.p64['conv3.weight'])
    under = lambda pos: sr.rel(got10, pre10 * torch.where(pos, torch.ones_like(pre10), torch.full_like(pre10, 0.01)))          # noqa: E731
    pos_hi, pos_value = planted.half() > 0, planted > 0
    return dict(route=under(_positive(s.tensors(pbuf), 0, split)), hi_rule=under(pos_hi), value_rule=under(pos_value),
                differ=int((pos_hi != pos_value).sum()), planted=int((signs > 0).sum()))


def _measure_repeat(s, fbuf, y, bbuf, g6s):
    """the split sweeps a second time -> {'fwd': dumps and y bitwise equal, 'bwd': tensors 1..11 bitwise equal}"""
    from stofnet_amd import _lib
    code, fbuf2, y2 = s.forward(True)
    _lib.check(code, 'stof_train_sweep_split (again)')
    fwd = torch.equal(s.tensors(fbuf2).view(torch.int32), s.tensors(fbuf).view(torch.int32)) and torch.equal(y2, y)
    code, bbuf2 = s.backward(True, g6s, fbuf)
    _lib.check(code, 'stof_train_sweep_bwd_split (again)')
    return dict(fwd=fwd, bwd=torch.equal(s.tensors(bbuf2)[1:].view(torch.int32), s.tensors(bbuf)[1:].view(torch.int32)))


def _measure_cross_format(ft, y, f32, y_fp32):
    """the split forward sweep against the fp32-dump one (see test_split_dump_is_the_fp32_dump_split); rows of tensors 1..10 are
    counted as `codec` (split row = to_split(fp32 row)), `fixup` (only fp32 row = hi + lo of the split row) or `neither`"""
    c = dict(y_equal=torch.equal(y, y_fp32), t11_equal=sr.same_bits(ft[11], f32[11]), t0_is_codec=sr.same_bits(ft[0], sr.to_split(f32[0])),
             split_rows=all(not torch.equal(ft[i], f32[i]) for i in range(11)),               # tensors 0..10 are NOT fp32 tensors
             rows_codec=0, rows_fixup=0, rows_neither=0, rows_all=0)
    for i in range(1, 11):
        a = (sr.to_split(f32[i]).view(torch.int32) == ft[i].view(torch.int32)).all(-1)
        b = (sr.from_split(ft[i]).view(torch.int32) == f32[i].view(torch.int32)).all(-1)
        c['rows_codec'] += int(a.sum())
        c['rows_fixup'] += int((b & ~a).sum())
        c['rows_neither'] += int((~a & ~b).sum())
        c['rows_all'] += a.numel()
    return c


def _fixup_rows(t):
    """[rows, 64] of an fp32 dump -> per row: every element is exactly hi + lo of its own split.  The padding fix-up writes
    hi + lo from the LDS image, the fast path the full fp32 accumulator (a row of 64 such values passes with probability 4^-64):
    the dump itself tells which path wrote a row."""
    return (sr.from_split(sr.to_split(t)) == t).all(-1)


def _measure_cut_spans(s, policy, tensors_by_direction):
    """fp32 dumps of a one-waveform segment case: for every span that tests/split_route_inputs.spans_cut_by_waveform_end predicts to
    be kept off the fast path by the `tw < Ltrue` term alone, what the KERNEL did -- the span's rows up to the waveform end came from
    the fix-up, the 96 rows in front of it (the same layer's previous span, inside the segment) from the fast path"""
    nseg, seg_len, _, _ = sr.geometry(s.L, policy)
    out = []
    for j, tk in sr.spans_cut_by_waveform_end(s.L, policy):
        tw0 = (nseg - 1) * seg_len - sr.HALO + tk
        for direction, t in tensors_by_direction.items():
            out.append(dict(direction=direction, layer=j, tw0=tw0, fixup=bool(_fixup_rows(t[j][0, tw0:s.L]).all()),
                            fast_before=bool((~_fixup_rows(t[j][0, tw0 - 96:tw0])).all())))
    return out


@pytest.fixture(scope='module', params=SWEEP_RUNS, ids=lambda v: f'{v[0]}-r{v[1]}-s{v[2]}')
def sweep(request, lib, dev, cus):
    """Everything measured on one (case, r, scale), once, by the _measure_* helpers above: status codes, unwritten elements,
    canaries, the stage errors of both dump formats with the layer kernels' beside them, the bitwise relations.  The tests below
    assert on the figures."""
    from stofnet_amd import _lib
    case, r, scale = request.param
    s = _Sweeps(lib, dev, cus, case, r, scale)
    two_pass = case != 'control'
    m = dict(case=case, r=r, scale=scale, N=s.N, L=s.L, two_pass=two_pass, fwd={}, bwd={}, planted={}, codes={}, unwritten={}, canary={},
             repeat={}, layer={}, mask_on={}, cross={}, cut=[])
    tag = f'{case} r{r} s{scale}'
    g6s = _nan((s.N, s.L, 64), dev)
    _lib.check(lib.stof_train_to_split_rows(_lib.ptr(s.g6), _lib.ptr(g6s), s.N * s.L, s.st), 'stof_train_to_split_rows')
    m['g6_split_is_codec'] = sr.same_bits(g6s, sr.to_split(s.g6))
    signs = sr.planted_signs((s.N, s.L, 64), 17 + s.L)
    fp32_run, records = None, {}
    for split in (False, True):
        fmt = 'split' if split else 'fp32'
        g6 = g6s if split else s.g6
        code, fbuf, y = s.forward(split)
        m['codes']['fwd_' + fmt] = code
        if split and not two_pass:                                      # control: the documented fallback, nothing was launched
            m['codes']['bwd_split'] = s.backward(True, g6s, fbuf)[0]
            continue
        _lib.check(code, 'stof_train_sweep' + ('_split' if split else ''))
        m['fwd'][fmt], m['layer']['fwd_' + fmt], m['unwritten']['fwd_' + fmt], m['canary']['fwd_' + fmt] = _measure_forward(s, split, fbuf, y)
        bcode, bbuf = s.backward(split, g6, fbuf)
        m['codes']['bwd_' + fmt] = bcode
        _lib.check(bcode, 'stof_train_sweep_bwd' + ('_split' if split else ''))
        (m['bwd'][fmt], m['layer']['bwd_' + fmt], m['unwritten']['bwd_' + fmt], m['canary']['bwd_' + fmt],
         m['mask_on'][fmt]) = _measure_backward(s, split, s.tensors(fbuf), g6s, bbuf)
        m['planted'][fmt] = _measure_planted(s, split, fbuf, g6, signs)
        if split:
            m['repeat'] = _measure_repeat(s, fbuf, y, bbuf, g6s)
            m['cross'] = _measure_cross_format(s.tensors(fbuf), y, s.tensors(fp32_run[0]), fp32_run[1])
        else:
            fp32_run = (fbuf, y)
            if two_pass and s.N == 1 and s.desc.seg_policy > 1:
                m['cut'] = _measure_cut_spans(s, s.desc.seg_policy, {'fwd': s.tensors(fbuf), 'bwd': s.tensors(bbuf)})
        for grp in ('fwd', 'bwd'):
            for stage, err in m[grp][fmt].items():
                records[f'sweep {tag} {fmt} {grp} {stage}'] = {'rows': s.N * s.L, 'sweep': _rounded(err), 'bound': BOUND,
                                                               'layer_kernel': _rounded(m['layer'][grp + '_' + fmt][stage])}
    _record(records)
    print(tag, {k: v for k, v in m.items() if k not in ('fwd', 'bwd', 'layer')})
    return m


def _formats(m):
    return ('fp32', 'split') if m['two_pass'] else ('fp32',)


def test_sweep_entry_points_take_the_shape(sweep):
    """The split entry points return STOF_OK on every two-pass case (a fallback is a failure, not a skip) and
    STOF_ERR_UNSUPPORTED at the control shape, the documented fallback to the r3 kernel with fp32 dumps."""
    from stofnet_amd import _lib
    m = sweep
    print(m['case'], m['codes'])
    assert m['codes']['fwd_fp32'] == _lib.STOF_OK and m['codes']['bwd_fp32'] == _lib.STOF_OK
    want = _lib.STOF_OK if m['two_pass'] else _lib.STOF_ERR_UNSUPPORTED
    assert m['codes']['fwd_split'] == want and m['codes']['bwd_split'] == want
    assert m['g6_split_is_codec']


def test_sweep_writes_every_element_and_stays_inside(sweep):
    """NaN-prefilled outputs: no element of the twelve forward tensors, of y or of backward tensors 1..11 is left; the canary behind
    stof_train_sweep_dump_floats floats is untouched (the 1024 floats behind the twelve tensors are documented scrap)."""
    m = sweep
    for fmt in _formats(m):
        for d in ('fwd_', 'bwd_'):
            assert m['unwritten'][d + fmt] == 0, (d + fmt, m['unwritten'])
            assert m['canary'][d + fmt], d + fmt


def test_sweep_forward_stages(sweep):
    """Forward tensors 0..11 (0..10 decoded from split rows on the split route, 11 read as fp32) and y against their float64 stage
    references at 2e-6 x max|ref|, the bound of one split-fp16 convolution (test_conv_kernels_vs_torch); tensor 0 (conv1 on
    the vector pipe + the SemiGlobalBlock term) at the same bound."""
    m = sweep
    for fmt in _formats(m):
        worst = max(m['fwd'][fmt].items(), key=lambda kv: kv[1])
        print(m['case'], fmt, 'worst forward stage', worst, 'layer kernel', m['layer']['fwd_' + fmt][worst[0]])
        assert worst[1] <= BOUND, (fmt, m['fwd'][fmt], m['layer']['fwd_' + fmt])


def test_sweep_backward_stages(sweep):
    """Backward tensors 1..11 against their float64 stage references (masks read off the same dump bytes under the route's rule)
    at 2e-6 x max|ref|."""
    m = sweep
    for fmt in _formats(m):
        worst = max(m['bwd'][fmt].items(), key=lambda kv: kv[1])
        print(m['case'], fmt, 'worst backward stage', worst, 'layer kernel', m['layer']['bwd_' + fmt][worst[0]], 'masks on', m['mask_on'][fmt])
        assert all(0.05 < q < 0.95 for q in m['mask_on'][fmt])                              # both slopes are exercised
        assert worst[1] <= BOUND, (fmt, m['bwd'][fmt], m['layer']['bwd_' + fmt])


def test_split_dump_is_the_fp32_dump_split(sweep):
    """Both forward sweeps hold the same fp32 value v in front of their stores (the epilogue queue of body_p2.h computes v, then
    hi = fp16(v), lo = fp16(v - hi) in both; only instruction 41 differs), so y and tensor 11 are bitwise equal between them and
    tensor 0 of the split sweep is to_split(tensor 0 of the fp32 sweep) bit for bit.  For tensors 1..10 that holds on the rows of
    spans that lie inside one waveform (span_ok: fp32 dump = v, split dump = (hi, lo) of v).  A 96-row span that touches gap,
    halo or end rows stores into the scrap area and the fix-up writes its valid rows from the LDS image: the fp32 dump then
    holds hi + lo, NOT v, and to_split(hi + lo) differs from (hi, lo) where lo was rounded up to half an ulp of an odd hi.
    Hence per ROW: split = to_split(fp32) bit for bit, or fp32 = hi + lo of the split row bit for bit; both kinds occur."""
    m = sweep
    if not m['two_pass']:
        return
    c = m['cross']
    print(m['case'], 'rows: codec', c['rows_codec'], 'fix-up only', c['rows_fixup'], 'of', c['rows_all'])
    assert c['y_equal'] and c['t11_equal'] and c['t0_is_codec'] and c['split_rows']
    assert c['rows_neither'] == 0 and c['rows_codec'] > 0
    assert c['rows_codec'] + c['rows_fixup'] == c['rows_all']


def test_span_cut_by_the_waveform_end_takes_the_fix_up(sweep):
    """seg4_cut exists for ONE term of span_ok, `tww + 95 < Ltrue`: tests/split_route_inputs.spans_cut_by_waveform_end restates the
    kernel's span geometry (step, lag 3 j, 96-row wave spans) to find a span that only this term keeps off the fast path.  That
    restatement is checked here against what the kernel did: in the fp32 dumps of sweep layer 4, forward and backward, the rows
    from the predicted span start to the waveform end were written by the fix-up (they hold hi + lo exactly) and the 96 rows
    in front of them by the fast path.  If the kernel's lags or span widths change, the boundary moves and this fails; the
    case then needs a new length.  At seg2 and seg4 the restatement predicts no such span."""
    m = sweep
    if m['case'] == 'seg4_cut':
        print(m['cut'])
        assert {(c['direction'], c['layer']) for c in m['cut']} == {('fwd', 4), ('bwd', 4)}
        assert all(c['fixup'] and c['fast_before'] for c in m['cut']), m['cut']
    elif m['case'] in ('seg2', 'seg4'):
        assert m['cut'] == []


def test_split_sweeps_repeat_bitwise(sweep):
    m = sweep
    if m['two_pass']:
        assert m['repeat']['fwd'] and m['repeat']['bwd']


def test_mask_rule_on_planted_zeros(sweep):
    """Exact zeros and +-2^-26 planted in forward tensor 1: on fp32 dumps +2^-26 is positive (slope 1), on split dumps its hi half
    is +0 and it counts as not positive (slope 0.01), as documented for stof_train_sweep_bwd_split."""
    m = sweep
    for fmt in _formats(m):
        p = m['planted'][fmt]
        print(m['case'], fmt, p)
        assert p['planted'] > 0 and p['route'] <= BOUND, (fmt, p)
    assert m['planted']['fp32']['differ'] > 0
    assert m['planted']['fp32']['value_rule'] <= BOUND < m['planted']['fp32']['hi_rule']       # the fp32 route does NOT use the hi rule
    if m['two_pass']:
        assert m['planted']['split']['hi_rule'] <= BOUND


def test_sweeps_on_an_empty_batch(lib, dev, cus):
    """N = 0: STOF_OK without touching the buffers."""
    from stofnet_amd import _lib
    s = _Sweeps(lib, dev, cus, 'floor', 4, 80)
    for split in (False, True):
        code, buf, y = s.forward(split, n=0)
        bcode, bbuf = s.backward(split, s.g6, buf, n=0)
        assert code == _lib.STOF_OK and bcode == _lib.STOF_OK
        torch.cuda.synchronize()
        assert torch.isnan(buf[:s.floats]).all() and torch.isnan(y).all() and torch.isnan(bbuf[:s.floats]).all()


# ------------------------------------------------------------------------- the whole step on the route it is benchmarked on
def _make(dev, r, sgs, seed):
    from stofnet_amd import StofNet
    from stofnet_amd.training import StofNetTrainer
    sd = synth.synth_state_dict(r, seed=seed, semi_global_scale=sgs)
    model = StofNet(upsample_factor=r, semi_global_scale=sgs)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return sd, StofNetTrainer(model.to(dev), lr=5e-4, weight_decay=1e-8, precision='f16x3')


@pytest.mark.parametrize('shape', ['cu_x_380', '1_x_20000'])
def test_whole_step_on_the_split_route(dev, cus, monkeypatch, shape):
    """TrainEngine / StofNetTrainer at f16x3 with automatic geometry where the engine itself takes the split route -- (CU, 380),
    r = 4: one segment of 384 stream rows; (1, 20000), r = 10: 32 segments of 625 rows -- read off what the engine recorded
    (SavedForward.split and .sweep).  Against float64 autograd of the same network on the device (sr.network_forward and
    sr.loss_ref: matmuls, so that float64 runs on the device; pinned against oracle/'s forward and loss on the CPU, with one
    and with three pooling windows): loss 2e-6, predictions 1e-5,
    every parameter gradient 2e-3 x max|grad| (the f16x3 bar of DESIGN.md section 8).  Twice: bitwise.  Then one more step with
    `split_dumps = False`: the engine stays on the sweeps and leaves split rows (fp32 dumps, hence the register-staged
    weight-gradient kernel), and every gradient agrees with the split route's at 2e-4 x max|grad|."""
    from oracle.pickers_oracle import gaussian_kernel
    N, L, r = (cus, 380, 4) if shape == 'cu_x_380' else (1, 20000, 10)
    sd, tr = _make(dev, r, 80, seed=3008)
    frame = torch.from_numpy(synth.synth_echo(N, L, seed=41)).to(dev)
    rng = np.random.default_rng(5)
    gt = torch.from_numpy(np.stack([np.sort(rng.integers(1, L * r, size=2)) for _ in range(N)])[:, None, :].astype(np.int64)).to(dev)
    seen = []
    inner = tr._forward_saved

    def spy(p, fr, keep=True):
        out = inner(p, fr, keep)
        seen.append(out[1])
        return out
    monkeypatch.setattr(tr, '_forward_saved', spy)

    def step():
        loss, pred = tr.forward_backward(frame, gt)
        return float(loss), pred.detach().clone(), {n: tr.g[n].detach().clone() for n in tr.names}

    loss, pred, grads = step()
    print(shape, 'split', seen[-1].split, 'sweep', seen[-1].sweep)
    assert seen[-1].split is True and seen[-1].sweep is True
    # float64 autograd of the same network
    p64 = {k: torch.from_numpy(v).to(dev, torch.float64).requires_grad_() for k, v in sd.items()}
    pred64 = sr.network_forward(p64, frame[:, 0].double(), r, 80)
    loss64 = sr.loss_ref(pred64, gt[:, 0], gaussian_kernel(7, 1))
    g64 = dict(zip(p64, torch.autograd.grad(loss64, list(p64.values()))))
    loss64 = loss64.detach()
    ratios = {n: sr.rel(grads[n], g64[n]) for n in tr.names}
    _record({f'whole step {shape}': {'rows': N * L, 'loss': _rounded(abs(loss - float(loss64)) / float(loss64)),
                                     'pred': _rounded(sr.rel(pred[:, 0], pred64.detach())), 'grad_bound': 2e-3,
                                     'grads': {n: _rounded(v) for n, v in ratios.items()}}})
    assert abs(loss - float(loss64)) < 2e-6 * float(loss64)
    assert sr.rel(pred[:, 0], pred64.detach()) < 1e-5
    assert set(ratios) == set(g64) and max(ratios.values()) < 2e-3, ratios
    del p64, pred64, g64
    loss2, pred2, grads2 = step()
    # (the loss value is a float64 atomicAdd over work-groups, loss_grad_kernel: its last bit moves between runs; no gradient reads it)
    assert abs(loss2 - loss) <= 1e-12 * abs(loss) and torch.equal(pred2, pred)
    assert all(torch.equal(grads2[n], grads[n]) for n in grads)
    monkeypatch.setattr(tr, 'split_dumps', False)
    _, _, fp32_dumps = step()
    assert seen[-1].split is False and seen[-1].sweep is True
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * float(b.abs().max())          # noqa: E731
    for n in tr.names:
        assert close(fp32_dumps[n], grads[n], 2e-4), n

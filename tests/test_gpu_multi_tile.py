"""The training kernels where a work-group takes a second tile (tests/multi_tile_inputs.py has the grids and shapes).

Every kernel behind the training routes is persistent or grid-strided and writes one partial per work-group; the other
kernel tests stop at a few hundred rows, where no work-group loops and at most three partials exist.  Here:

  * each kernel alone through the C ABI at 1.3 .. 1.7 x the row count at which its grid saturates (the grid read off the
    workspace query where the ABI has one), many short rows and few long rows, on DYADIC operands: every output and every
    gradient BITWISE equal to the float64 reference cast to fp32 -- one dropped, doubled or stale tile fails it.  NaN-prefilled
    outputs, workspaces filled with 0xff, each weight gradient twice (bitwise).  The leaky ReLU (slope 0.01, not dyadic) at
    2e-6 x max|ref|, the bound of test_conv_kernels_vs_torch;
  * every reduce kernel, wgrad_reduce_kernel included, at 117 partials (117 mod 64 and mod 16 non-zero: slices that take the
    four-chain loop twice and slices that take it once and then three tail steps; no work-group loops);
  * each weight-gradient kernel once on Gaussian operands at its long-row shape: rel(dw), rel(db) <= max(2e-6, 4 x e32), e32
    the deviation from float64 of the same gradient evaluated by torch in fp32; kernel error, e32 and bound go to
    profiles/multi_tile.jsonl;
  * EDSR_1D(1, 64, 1, 4) and ESPCN_1D(4) with train_route = 'kernels', one step above their weight-gradient thresholds,
    against the same module in float64 (y 2e-5, gradients 2e-4 x max|ref|), twice (bitwise); EDSR with seeded parameters
    whose ReLU inputs all stay clear of zero, and once more with torch's default initialisation, where a few masks differ from
    float64's within rounding of zero: there against float64 autograd under the route's own saved masks.

The float64 references are matmuls / autograd on the device; they never touch the kernels under test."""
import copy
import json
import os

import pytest
import torch

import multi_tile_inputs as mt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'multi_tile.jsonl')
LRELU_BOUND, Y_BOUND, GRAD_BOUND = 2e-6, 2e-5, 2e-4
OUT_SCALE = 0.25


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib(dev):
    from stofnet_amd import _lib
    return _lib.lib()


def _nan(shape, dev):
    return torch.full(tuple(shape), float('nan'), device=dev)


def _record(name, entry):
    """print a case's figures and keep them in profiles/multi_tile.jsonl: one line per case; the lines of cases that this
    session did not run stay as they are"""
    print(name, json.dumps(entry))
    lines = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            for ln in fh.read().splitlines():
                if ln.strip():
                    lines[json.loads(ln)['case']] = ln
    lines[name] = json.dumps({'case': name, **entry})
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines[k] for k in sorted(lines)) + '\n')
    except OSError as exc:
        print(f'{PROFILE} not written: {exc}')


def _rounded(v):
    return float(f'{v:.3e}')


# --------------------------------------------------------------------------------------------------- stof_train_conv
_conv_cache = {}


def _conv_case(dev, cin, cout, K, which):
    """operands and float64 references of one (set, shape), shared by the two precisions"""
    key = (cin, cout, K, which)
    if key not in _conv_cache:
        _conv_cache.clear()
        G = mt.conv_groups(cout)
        N, L = mt.tile_shapes(G, mt.CONV_TILE, 1.3 if cin * G > 1 << 17 else 1.4)[which]
        seed = 100 * cin + 10 * cout + K
        x = mt.ints((N, L, cin), seed, dev)
        res = mt.ints((N, L, cout), seed + 1, dev)
        saved = mt.ints((N, L, cout), seed + 2, dev)
        w = mt.ints((cout, cin, K), seed + 3, dev)          # forward: a layer cin -> cout
        w2 = mt.ints((cin, cout, K), seed + 4, dev)         # data gradient: a layer cout -> cin, read flipped
        b = mt.ints((cout,), seed + 5, dev)
        mt.headroom(K * cin * 4 + 2 + 2, 0)
        x64, res64, s64, w64, w264, b64 = (v.double() for v in (x, res, saved, w, w2, b))
        pre = mt.conv_forward_ref(x64, w64, b64, None, mt.ACT_NONE)
        assert (pre > 0).any() and (pre < 0).any() and (saved > 0).any() and (saved <= 0).any()
        ref = {('y', act): mt.conv_forward_ref(x64, w64, b64, res64, act) for act in (mt.ACT_RELU, mt.ACT_LRELU)}
        ref.update({('gx', act): mt.conv_backward_ref(x64, w264, res64, s64, act) for act in (mt.ACT_NONE, mt.ACT_RELU, mt.ACT_LRELU)})
        _conv_cache[key] = dict(N=N, L=L, G=G, x=x, res=res, saved=saved, w=w, w2=w2, b=b, ref=ref)
    return _conv_cache[key]


@pytest.mark.parametrize('prec', [mt.FP32, mt.F16X3])
@pytest.mark.parametrize('which', ['short', 'long'])
@pytest.mark.parametrize('cin,cout,K', mt.CONV_SETS)
def test_conv_second_tile_exact(lib, dev, cin, cout, K, which, prec):
    """stof_train_conv forward (bias, ReLU, residual) and its data-gradient form (flipped image, residual, ReLU mask) where
    a work-group takes a second tile: bitwise; the leaky-ReLU forms at 2e-6 x max|ref|."""
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    c = _conv_case(dev, cin, cout, K, which)
    N, L, G = c['N'], c['L'], c['G']
    tiles = mt.tiles_of(N, L, mt.CONV_TILE)
    assert tiles > G and mt.in_loop_range(tiles, G), (tiles, G)              # some work-groups take two tiles, others one

    def image(w, co, ci, flip):
        out = _nan((lib.stof_train_repack_floats(co, ci, K, flip, prec),), dev)
        _lib.check(lib.stof_train_repack(_lib.ptr(w), _lib.ptr(out), co, ci, K, flip, prec, st), 'repack')
        return out

    def conv(img, bias, saved, act):
        y = _nan((N, L, cout), dev)
        _lib.check(lib.stof_train_conv(_lib.ptr(c['x']), _lib.ptr(img), _lib.ptr(bias), _lib.ptr(c['res']), _lib.ptr(saved), _lib.ptr(y),
                                       N, L, cin, cout, K, act, prec, st), 'conv')
        return y

    fwd, bwd = image(c['w'], cout, cin, 0), image(c['w2'], cin, cout, 1)
    saved, ref = c['saved'], c['ref']
    assert torch.equal(conv(fwd, c['b'], None, mt.ACT_RELU), mt.exact_fp32(ref['y', mt.ACT_RELU]))
    assert torch.equal(conv(bwd, None, saved, mt.ACT_RELU), mt.exact_fp32(ref['gx', mt.ACT_RELU]))
    assert torch.equal(conv(bwd, None, saved, mt.ACT_NONE), mt.exact_fp32(ref['gx', mt.ACT_NONE]))
    errs = {'y': mt.rel(conv(fwd, c['b'], None, mt.ACT_LRELU), ref['y', mt.ACT_LRELU]),
            'gx': mt.rel(conv(bwd, None, saved, mt.ACT_LRELU), ref['gx', mt.ACT_LRELU])}
    print('conv lrelu', (cin, cout, K, which, prec), errs)
    assert max(errs.values()) < LRELU_BOUND, errs


# -------------------------------------------------------------------------------------------------- the weight gradients
def _run_wgrad(dev, call, dw_shape, db_shape, ws_bytes, what):
    """the weight gradient twice into NaN-prefilled outputs through a 0xff-filled workspace -> (dw, db), bitwise repeatable"""
    from stofnet_amd import _lib
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        dw, db = _nan(dw_shape, dev), _nan(db_shape, dev)
        ws.fill_(0xff)                                          # NaN patterns: a partial that is read must have been written
        _lib.check(call(_lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), ws.numel()), what)
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what      # no float atomics
    return runs[0]


def _check_exact(dev, spec, what):
    x, dy = spec['ops'](torch.float64)
    dw_ref, db_ref = mt.wgrad_ref(x, dy, spec['K'])
    sums, bsum = mt.wgrad_ref(x.abs(), dy.abs(), spec['K'])
    mt.headroom(max(float(sums.max()), float(bsum.max())), spec['frac'])
    assert (dw_ref > 0).any() and (dw_ref < 0).any()
    dw, db = _run_wgrad(dev, spec['call'], spec['dw'], spec['db'], spec['ws'], what)
    assert torch.equal(dw.reshape(dw_ref.shape), mt.exact_fp32(OUT_SCALE * dw_ref)), what
    assert torch.equal(db.reshape(db_ref.shape), mt.exact_fp32(OUT_SCALE * db_ref)), what


def _check_gauss(dev, spec, what):
    x, dy = spec['ops'](torch.float64)
    dw_ref, db_ref = mt.wgrad_ref(x, dy, spec['K'])
    x32, dy32 = spec['ops'](torch.float32)
    dw32, db32 = mt.wgrad_ref(x32, dy32, spec['K'])
    dw, db = _run_wgrad(dev, spec['call'], spec['dw'], spec['db'], spec['ws'], what)
    entry, exact = {'rows': int(x.shape[0] * x.shape[1])}, {}
    for tag, got, t32, ref in (('dw', dw, dw32, dw_ref), ('db', db, db32, db_ref)):
        err, e32 = mt.rel(got.reshape(ref.shape), OUT_SCALE * ref), mt.rel(t32, ref)
        exact[tag] = (err, max(2e-6, 4 * e32))
        entry[tag] = {'kernel': _rounded(err), 'e32': _rounded(e32), 'bound': _rounded(exact[tag][1])}
    _record(what, entry)
    for tag, (err, bound) in exact.items():
        assert err <= bound, (what, tag, err, bound)


def _partials(ws_bytes, floats_per_partial):
    assert ws_bytes % (4 * floats_per_partial) == 0
    return ws_bytes // (4 * floats_per_partial)


def _operand(mode, dev, shape, seed, kind='ints'):
    """'dyadic': the integer / half / quarter operands of multi_tile_inputs; 'gauss': ordinary data of the same role"""
    if mode == 'dyadic':
        return getattr(mt, kind)(shape, seed, dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.randn(tuple(shape), generator=g, device=dev)
    return torch.tanh(v) if kind == 'halves' else torch.sigmoid(v) if kind == 'quarters' else v


def _stof_wgrad(lib, dev, cin, cout, K, prec, N, L, mode):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    seed = 7 * cin + 3 * cout + K
    x, dy = _operand(mode, dev, (N, L, cin), seed), _operand(mode, dev, (N, L, cout), seed + 1)
    ws = lib.stof_train_wgrad_workspace_bytes(cin, cout, K)
    call = lambda dw, db, w, n: lib.stof_train_wgrad(_lib.ptr(x), _lib.ptr(dy), dw, db, N, L, cin, cout, K, OUT_SCALE, prec, w, n, st)
    return dict(call=call, dw=(cout, cin, K), db=(cout,), ws=ws, K=K, frac=0, ops=lambda dt: (x.to(dt), dy.to(dt)))


def _wgrad_groups(lib, cin, cout, K):
    cin_pad, cout_pad = (cin + 63) // 64 * 64, (cout + 63) // 64 * 64
    return _partials(lib.stof_train_wgrad_workspace_bytes(cin, cout, K), K * cout_pad * cin_pad + cout_pad)


@pytest.mark.parametrize('prec', [mt.FP32, mt.F16X3])
@pytest.mark.parametrize('which', ['short', 'long'])
@pytest.mark.parametrize('K', mt.WGRAD_KS)
@pytest.mark.parametrize('cin,cout', mt.WGRAD_SETS)
def test_wgrad_second_tile_exact(lib, dev, cin, cout, K, which, prec):
    """stof_train_wgrad (conv_wgrad_cl_kernel / conv_wgrad_f16x3_kernel + wgrad_reduce_kernel) where a work-group takes a second
    tile: dw and db bitwise."""
    G = _wgrad_groups(lib, cin, cout, K)
    N, L = mt.tile_shapes(G, mt.WGRAD_TILE[prec])[which]
    tiles = mt.tiles_of(N, L, mt.WGRAD_TILE[prec])
    assert tiles > G and mt.in_loop_range(tiles, G), (tiles, G)
    _check_exact(dev, _stof_wgrad(lib, dev, cin, cout, K, prec, N, L, 'dyadic'), f'wgrad {cin}->{cout} k{K} {which} prec{prec}')


@pytest.mark.parametrize('prec', [mt.FP32, mt.F16X3])
@pytest.mark.parametrize('cin,cout,K', [(64, 64, 3), (64, 64, 5), (32, 32, 3), (96, 96, 5), (128, 128, 3)])
def test_wgrad_reduce_tail_exact(lib, dev, cin, cout, K, prec):
    """wgrad_reduce_kernel at 117 partials: stof_train_wgrad launches min(G, tiles) work-groups, so 117 one-tile waveforms give
    G = 117 -- slices 0 .. 4 take the four-chain loop twice, slices 5 .. 15 once and then three tail steps (a main loop that read
    past G would add 0xff patterns); no work-group loops.  dw and db bitwise."""
    N, L = mt.tail_tile_shape()
    tiles = mt.tiles_of(N, L, mt.WGRAD_TILE[prec])
    assert _wgrad_groups(lib, cin, cout, K) >= tiles == mt.REDUCE_TAIL_CHUNKS > 48 and tiles % 64 and tiles % 16
    _check_exact(dev, _stof_wgrad(lib, dev, cin, cout, K, prec, N, L, 'dyadic'), f'wgrad {cin}->{cout} k{K} tail prec{prec}')


@pytest.mark.parametrize('prec', [mt.FP32, mt.F16X3])
@pytest.mark.parametrize('cin,cout', [(64, 64), (96, 96), (64, 512)])
def test_wgrad_second_tile_gaussian(lib, dev, cin, cout, prec):
    G = _wgrad_groups(lib, cin, cout, 3)
    N, L = mt.tile_shapes(G, mt.WGRAD_TILE[prec])['long']
    assert mt.tiles_of(N, L, mt.WGRAD_TILE[prec]) > G
    _check_gauss(dev, _stof_wgrad(lib, dev, cin, cout, 3, prec, N, L, 'gauss'), f'stof_train_wgrad {cin}->{cout} k3 prec{prec}')


# the chunked weight gradients: name -> (partials(lib), spec(lib, dev, N, L, mode))
def _edsr_in(lib, dev, N, L, mode):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    x = _operand(mode, dev, (N, L), 11)
    g, g2, saved = (_operand(mode, dev, (N, L, 64), 12 + i) for i in range(3))
    call = lambda dw, db, w, n: lib.stof_train_edsr_in_wgrad(_lib.ptr(x), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(saved), dw, db, N, L,
                                                             OUT_SCALE, w, n, st)
    return dict(call=call, dw=(64, 1, 3), db=(64,), ws=lib.stof_train_edsr_in_wgrad_workspace_bytes(), K=3, frac=0,
                ops=lambda dt: (x.to(dt)[..., None], mt.masked_relu(g.to(dt), saved, g2.to(dt))))


def _edsr_out(lib, dev, N, L, mode, r=4):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    trunk, dy = _operand(mode, dev, (N, L, 64), 21), _operand(mode, dev, (N, L * r), 22)
    call = lambda dw, db, w, n: lib.stof_train_edsr_out_wgrad(_lib.ptr(trunk), _lib.ptr(dy), dw, db, N, L, r, OUT_SCALE, w, n, st)
    return dict(call=call, dw=(1, 64 // r, 3), db=(1,), ws=lib.stof_train_edsr_out_wgrad_workspace_bytes(r), K=3, frac=0,
                ops=lambda dt: mt.edsr_out_operands(trunk.to(dt), dy.to(dt), r))


def _espcn_in(lib, dev, N, L, mode):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    x, g1, h1 = _operand(mode, dev, (N, L), 31), _operand(mode, dev, (N, L, 64), 32), _operand(mode, dev, (N, L, 64), 33, 'halves')
    call = lambda dw, db, w, n: lib.stof_train_espcn_in_wgrad(_lib.ptr(x), _lib.ptr(g1), _lib.ptr(h1), dw, db, N, L, OUT_SCALE, w, n, st)
    return dict(call=call, dw=(64, 1, 5), db=(64,), ws=lib.stof_train_espcn_in_wgrad_workspace_bytes(), K=5, frac=2,
                ops=lambda dt: (x.to(dt)[..., None], mt.masked_tanh(g1.to(dt), h1.to(dt))))


def _espcn_out(lib, dev, N, L, mode, r=4):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    h2, y, dy = _operand(mode, dev, (N, L, 32), 41, 'halves'), _operand(mode, dev, (N, L * r), 42, 'quarters'), _operand(mode, dev, (N, L * r), 43)
    call = lambda dw, db, w, n: lib.stof_train_espcn_out_wgrad(_lib.ptr(h2), _lib.ptr(y), _lib.ptr(dy), dw, db, N, L, r, OUT_SCALE, w, n, st)
    return dict(call=call, dw=(r, 32, 3), db=(r,), ws=lib.stof_train_espcn_out_wgrad_workspace_bytes(r), K=3, frac=5,
                ops=lambda dt: (h2.to(dt), mt.masked_sigmoid(dy.to(dt), y.to(dt)).reshape(N, L, r)))


def _conv1_c(Cin, Fw):
    def spec(lib, dev, N, L, mode):
        from stofnet_amd import _lib
        st = _lib.stream_ptr(dev)
        x = _operand(mode, dev, (N, Cin, L), 51 + Cin)
        g, saved = _operand(mode, dev, (N, L, Fw), 52 + Fw), _operand(mode, dev, (N, L, Fw), 53 + Fw)
        call = lambda dw, db, w, n: lib.stof_train_conv1_c_wgrad(_lib.ptr(x), _lib.ptr(g), _lib.ptr(saved), dw, db, N, Cin, L, Fw, OUT_SCALE,
                                                                 w, n, st)
        return dict(call=call, dw=(Fw, Cin, 9), db=(Fw,), ws=lib.stof_train_conv1_c_wgrad_workspace_bytes(Cin, Fw), K=9, frac=0,
                    ops=lambda dt: (x.to(dt).permute(0, 2, 1), mt.masked_relu(g.to(dt), saved)))
    return spec


def _conv1(lib, dev, N, L, mode):
    from stofnet_amd import _lib
    st = _lib.stream_ptr(dev)
    x, g, saved = _operand(mode, dev, (N, L), 61), _operand(mode, dev, (N, L, 64), 62), _operand(mode, dev, (N, L, 64), 63)
    call = lambda dw, db, w, n: lib.stof_train_conv1_wgrad(_lib.ptr(x), _lib.ptr(g), _lib.ptr(saved), dw, db, N, L, OUT_SCALE, w, n, st)
    return dict(call=call, dw=(64, 1, 9), db=(64,), ws=lib.stof_train_conv1_wgrad_workspace_bytes(), K=9, frac=0,
                ops=lambda dt: (x.to(dt)[..., None], mt.masked_relu(g.to(dt), saved)))


# floats of one partial: edsr_train.hip `copies + blockIdx.x * 256` (EW_WORKSPACE), espcn_train.hip PW_IN_E = 64 * 5 + 64 and
# out_e(r) = r * 97, widths.hip `blockIdx.x * F * Cin * 10`, train.hip `C1_COPIES * 640`
CHUNKED = {
    'edsr_in': (lambda lib: _partials(lib.stof_train_edsr_in_wgrad_workspace_bytes(), 256), _edsr_in),
    'edsr_out': (lambda lib: _partials(lib.stof_train_edsr_out_wgrad_workspace_bytes(4), 256), _edsr_out),
    'espcn_in': (lambda lib: _partials(lib.stof_train_espcn_in_wgrad_workspace_bytes(), 384), _espcn_in),
    'espcn_out': (lambda lib: _partials(lib.stof_train_espcn_out_wgrad_workspace_bytes(4), 4 * 97), _espcn_out),
    'conv1': (lambda lib: _partials(lib.stof_train_conv1_wgrad_workspace_bytes(), 640), _conv1),
}
for _cin, _f in mt.CONV1_C_WIDTHS + [mt.CONV1_C_WIDE]:
    CHUNKED[f'conv1_c_{_cin}_{_f}'] = (lambda lib, c=_cin, f=_f: _partials(lib.stof_train_conv1_c_wgrad_workspace_bytes(c, f), f * c * 10),
                                      _conv1_c(_cin, _f))


def _chunk_shape(copies, which):
    return mt.chunk_shapes(copies, 1.3 if copies > 1024 else 1.4)[which]          # 2048 partials: 170 MB operands at 1.3


@pytest.mark.parametrize('which', ['short', 'long'])
@pytest.mark.parametrize('name', sorted(CHUNKED))
def test_chunked_wgrad_second_chunk_exact(lib, dev, name, which):
    """the grid-strided weight gradients where a work-group takes a second 256-row chunk (`c0 += gridDim.x * CHUNK`, the
    `t = r0 % L` re-seed) and the reduce kernel adds all its partials: dw and db bitwise."""
    copies = CHUNKED[name][0](lib)
    N, L = _chunk_shape(copies, which)
    chunks = mt.chunks_of(N, L)
    assert chunks > copies > 48 and mt.in_loop_range(chunks, copies) and (N * L) % mt.CHUNK, (chunks, copies)
    _check_exact(dev, CHUNKED[name][1](lib, dev, N, L, 'dyadic'), f'{name} {which}')


@pytest.mark.parametrize('name', sorted(CHUNKED))
def test_chunked_wgrad_reduce_tail_exact(lib, dev, name):
    """117 partials: slices 0 .. 4 of the reduce kernel take its four-chain loop twice, slices 5 .. 15 once and then three steps
    of the tail loop; no work-group loops."""
    copies = CHUNKED[name][0](lib)
    N, L = mt.tail_shape()
    chunks = mt.chunks_of(N, L)
    assert copies >= chunks == mt.REDUCE_TAIL_CHUNKS > 48 and chunks % 64 and chunks % 16
    _check_exact(dev, CHUNKED[name][1](lib, dev, N, L, 'dyadic'), f'{name} tail')


@pytest.mark.parametrize('name', sorted(CHUNKED))
def test_chunked_wgrad_second_chunk_gaussian(lib, dev, name):
    copies = CHUNKED[name][0](lib)
    N, L = _chunk_shape(copies, 'long')
    assert mt.chunks_of(N, L) > copies
    _check_gauss(dev, CHUNKED[name][1](lib, dev, N, L, 'gauss'), name)


# ------------------------------------------------------------------------------------------------------- module level
def _module_step(m, x, t, want_masks=False):
    """one forward + backward of loss = sum(y t) -> (y, dx, {name: gradient}, name of y's autograd node, saved ReLU masks)"""
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_()
    y = m(xd)
    masks = None
    if want_masks:                                     # what the kernel route's backward will read: channel-last [N, L, 64]
        saved = y.grad_fn.saved
        masks = [(a > 0).permute(0, 2, 1) for a in [saved.a0] + list(saved.hs)]
    (y * t).sum().backward()
    return y.detach(), xd.grad, {n: p.grad.clone() for n, p in m.named_parameters()}, type(y.grad_fn).__name__, masks


def _errors(y, dx, grads, y64, dx64, grads64):
    return {'y': mt.rel(y, y64), 'dx': mt.rel(dx, dx64), **{k: mt.rel(grads[k], grads64[k]) for k in grads}}


def _kernel_steps(dev, m, copies, r, seed, function, want_masks=False):
    """the module on the kernel route at its module-level shape, twice (bitwise) -> (float64 twin, x, t, first step)"""
    N, L = mt.module_shape(copies)
    assert mt.chunks_of(N, L) > copies                                       # its own weight-gradient kernels loop,
    assert mt.tiles_of(N, L, mt.WGRAD_TILE[mt.FP32]) > 512 and mt.tiles_of(N, L, mt.CONV_TILE) > mt.CONV_GROUPS      # and the 64 -> 64 ones
    m = m.to(dev).train()
    ref = copy.deepcopy(m).double()
    ref.train_route = 'aten'
    m.train_route = 'kernels'
    x, t = (v.to(dev) for v in mt.module_inputs(N, L, r, seed))
    first = _module_step(m, x, t, want_masks)
    assert first[3].startswith(function), first[3]                           # the kernel route, not ATen
    y2, dx2, grads2, _, _ = _module_step(m, x, t)
    assert torch.equal(first[0], y2) and torch.equal(first[1], dx2) and all(torch.equal(first[2][k], grads2[k]) for k in grads2)
    return ref, x, t, first


def _assert_bounds(name, shape, errs):
    print(name, shape, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    errs = dict(errs)
    assert errs.pop('y') < Y_BOUND
    assert max(errs.values()) < GRAD_BOUND, errs


def test_edsr_module_step_above_the_thresholds(lib, dev):
    """EDSR_1D(1, 64, 1, 4) above every threshold of its route against the same module in float64.  The seeded parameters
    keep every float64 ReLU input RELU_MARGIN away from zero (pinned on the CPU), so the route's saved masks ARE float64's.
    That takes biases 3.5 deviations from zero (multi_tile_inputs.edsr_module): each channel is about 99.98 % on or off, a weak
    exercise of the masks; the default-initialisation case below runs the ordinary ones."""
    ref, x, t, (y, dx, grads, _, masks) = _kernel_steps(dev, mt.edsr_module(mt.EDSR_SEED, True), CHUNKED['edsr_in'][0](lib), 4,
                                                        mt.EDSR_SEED, 'EdsrFunction', want_masks=True)
    pre64 = mt.edsr_relu_inputs(ref, x.double())
    assert min(float(p.abs().min()) for p in pre64) > mt.RELU_MARGIN
    for mk, p in zip(masks, pre64):
        assert torch.equal(mk, p > 0)
        on = (p > 0).float().mean(dim=(0, 2))
        assert float(on.min()) > 0 and float(on.max()) < 1                   # every channel: neither all-on nor all-off
    y64, dx64, grads64, _, _ = _module_step(ref, x.double(), t.double())
    _assert_bounds('EDSR_1D(1, 64, 1, 4) seeded', tuple(x.shape), _errors(y, dx, grads, y64, dx64, grads64))


def test_edsr_default_init_deviation_is_the_flipped_masks(lib, dev):
    """torch's default initialisation puts about twenty of the 44 M ReLU inputs of this shape within 1e-7 of zero, and an fp32
    forward takes the other side of zero for a few of them: three here (float64 inputs below 3e-8), one on torch's CPU route.
    One such element is one term of a gradient sum whose maximum grows like sqrt(rows), 1.7e-3 of it at 3.4e5 rows: with three
    the route lies 2.8e-3 (dx) and 1.1e-3 (the block's conv1.weight) from the float64 module, beyond GRAD_BOUND.  Shown here:
    every element whose saved mask differs from float64's has a float64 input below RELU_MARGIN, and against float64 autograd
    of the network WITH the route's own masks every gradient is within the bounds (6.2e-7); both sets of figures go to
    profiles/multi_tile.jsonl.  These are the ordinary, about half-on masks that the seeded case above gives up."""
    seed = 11
    ref, x, t, (y, dx, grads, _, masks) = _kernel_steps(dev, mt.edsr_module(seed, False), CHUNKED['edsr_in'][0](lib), 4, seed,
                                                        'EdsrFunction', want_masks=True)
    pre64 = mt.edsr_relu_inputs(ref, x.double())
    flipped = [mk != (p > 0) for mk, p in zip(masks, pre64)]
    worst = max([float(p[f].abs().max()) for p, f in zip(pre64, flipped) if f.any()], default=0.0)
    assert worst < mt.RELU_MARGIN, worst                                     # masks differ only within rounding of zero
    y64, dx64, grads64, _, _ = _module_step(ref, x.double(), t.double())
    plain = _errors(y, dx, grads, y64, dx64, grads64)
    for p in ref.parameters():
        p.grad = None
    xd = x.double().requires_grad_()
    ym = mt.edsr_masked_forward(ref, xd, [mk.double() for mk in masks])
    (ym * t.double()).sum().backward()
    forced = _errors(y, dx, grads, ym.detach(), xd.grad, {n: p.grad for n, p in ref.named_parameters()})
    _record('EDSR_1D(1, 64, 1, 4) default init, seed 11',
            {'rows': int(x.shape[0] * x.shape[2]), 'flipped_masks': [int(f.sum()) for f in flipped], 'largest_flipped_input': worst,
             'vs_float64_module': {k: _rounded(v) for k, v in plain.items()},
             'vs_float64_with_the_saved_masks': {k: _rounded(v) for k, v in forced.items()}})
    _assert_bounds('EDSR_1D(1, 64, 1, 4) default init, saved masks', tuple(x.shape), forced)


def test_espcn_module_step_above_the_thresholds(lib, dev):
    from stofnet_amd import ESPCN_1D
    torch.manual_seed(12)
    ref, x, t, (y, dx, grads, _, _) = _kernel_steps(dev, ESPCN_1D(4), CHUNKED['espcn_in'][0](lib), 4, 12, 'EspcnFunction')
    y64, dx64, grads64, _, _ = _module_step(ref, x.double(), t.double())
    _assert_bounds('ESPCN_1D(4)', tuple(x.shape), _errors(y, dx, grads, y64, dx64, grads64))

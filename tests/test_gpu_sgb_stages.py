"""The SemiGlobalBlock of the forward, stage by stage (GPU): the pooled map of sgb_contract_pool_kernel, the arg-max bytes
of its training form, and the expand map of sgb_expand_kernel (split fp16) / conv_cl_kernel in stream mode (exact fp32),
each against a float64 reference of that stage alone, at shapes chosen for the kernels' tiling (tests/sgb_stage_inputs.py
says what each shape reaches; tests/test_sgb_stage_refs_cpu.py pins the references and the caps on the CPU).

The end-to-end tests see these maps only after eleven 64->64 layers, three residual adds and the shuffle, and at batches
of at most 84 stream rows (one expand tile), or at the 1024- / 4096-row goldens.  Here a misplaced row is an O(1) error
at a named (waveform, window, channel).

What each assertion would catch (reasoned from the kernels, sgb_expand.hip and convstack.hip):
  1. the expand kernel's load without its `pp < p.P` predicate: a gap row would hold the next waveform's first pooled rows
     (for the last waveform: the first floats of the sgb region).  The first and last rows of every waveform of T3 / T7 / T27
     then differ from the expand reference by O(1) (test_expand_map), a waveform no longer equals itself run alone
     (test_rows_do_not_depend_on_the_batch), and the NaN left behind the pooled map reaches the last waveform
     (test_stages_read_only_what_the_call_wrote).
  2. `t0 - 1` for the halo base: every output row of every tile reads its five taps one row late, so each row holds the
     conv of its right neighbour; test_expand_map fails at every shape with an O(1) error.
  3. `oi < bi` -> `oi > bi` in the cross-lane step: equal values go to the larger row.  With period 4 the copies of row j sit
     in the neighbouring q4 lanes (rows j + 4, j + 8, j + 12), so arg >= 4 (test_argmax_on_exact_ties, q = 1, 4, 40).
  4. `v > mval` -> `v >= mval`: inside a lane the last copy wins.  With period 16 the copies of row j are the M-tiles of one
     lane (rows j + 16 m), so arg >= 64 (q = 1, 16, 40).
  5. an absent window that stores: N P is odd for T7 and R38, so the second window of the last tile would write one row past
     pooled and arg.  In the inference workspace that row is the head of the sgb region, which the expand kernel
     overwrites afterwards, so only the training form shows it: its outputs carry one guard row behind the last window
     (test_training_pooled_map, test_argmax_on_random_inputs)."""
import numpy as np
import pytest
import torch

import sgb_stage_inputs as si

pytestmark = pytest.mark.gpu

PRECISIONS = ['fp32', 'f16x3']
SHAPES = list(si.STAGE_SHAPES)
GUARD = 0xA5                 # byte of the guard rows behind the training form's outputs


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from stofnet_amd import _lib
    _lib.lib()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    return si.state_dict()


def make_model(dev, sd, precision):
    from stofnet_amd import StofNet
    m = StofNet(upsample_factor=si.R, semi_global_scale=si.SCALE, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def forward_stages(m, xd):
    """(y, pooled, sgb) of one forward, all cloned before anything else runs on the model"""
    n, _, L = xd.shape
    y = m(xd)
    torch.cuda.synchronize()
    pooled, sgb = si.read_stages(m, n, L)
    return y, pooled, sgb


@pytest.fixture(scope='module')
def refs(sd):
    """name -> (x, float64 pooled [N, P, 512], float64 expand of it [N, P, 64], float64 contract [N, 512, L] or None);
    computed once per shape, shared by every test and both precisions, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            x = si.stage_input(name)
            r = si.stage_reference(sd, x, keep_contract=name in si.ARG_SHAPES)
            pooled = r['pooled'].permute(0, 2, 1).contiguous()
            cache[name] = (x, pooled, si.expand_reference(sd, pooled), r['contract'])
        return cache[name]
    return get


@pytest.fixture(scope='module')
def runs(dev, sd):
    """(name, precision) -> (y, pooled, sgb) of the inference forward on the GPU, on the CPU; one run per pair"""
    cache = {}

    def get(name, precision):
        if (name, precision) not in cache:
            m = make_model(dev, sd, precision)
            xd = torch.from_numpy(si.stage_input(name)).to(dev)
            cache[(name, precision)] = tuple(t.cpu() for t in forward_stages(m, xd))
        return cache[(name, precision)]
    return get


def where(k, shape):
    n, w, c = np.unravel_index(k, shape)
    return f'waveform {n}, window {w}, channel {c}'


# Second, tighter bound for the stages whose measured error lies at least ten times under the bar: four times the larger of
# the kernel's measured error (the largest over the six shapes, profiles/sgb_stages.jsonl) and the float32 torch oracle's own
# error against float64 on the same inputs (pooled 2.4e-7, expand 3.6e-7: the kernels' figures are the larger ones
# throughout).  The factor leaves room for input dependence of the 320- and 2560-term sums.  The split-fp16 expand map
# measures 1.55e-6 (1.78e-6 for both stages), less than ten times under the bar, and keeps the bar alone.
MEASURED = {('pooled', 'fp32'): 5.549e-7, ('pooled', 'f16x3'): 6.969e-7, ('expand', 'fp32'): 4.942e-7, ('both', 'fp32'): 5.876e-7}
ORACLE_F32 = {'pooled': 2.38e-7, 'expand': 3.56e-7, 'both': 3.56e-7}
TIGHT = {k: 4 * max(v, ORACLE_F32[k[0]]) for k, v in MEASURED.items()}
assert all(10 * v <= si.MAP_TOL for v in MEASURED.values())


def check_map(tag, got, ref, tol=si.MAP_TOL):
    assert tuple(got.shape) == tuple(ref.shape), tag
    err, k = si.rel_err(got, ref)
    print(f'{tag}: rel err {err:.3e}')
    assert np.isfinite(err) and err < tol, f'{tag}: rel err {err:.3e} at {where(k, tuple(ref.shape))}'
    return err


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('name', SHAPES)
def test_pooled_map(refs, runs, name, precision):
    """pooled[N][P][512] of the contract + pool kernel against float64, element-wise, relative to max|ref|"""
    _, pooled64, _, _ = refs(name)
    _, pooled, _ = runs(name, precision)
    err = check_map(f'pooled {name} {precision}', pooled, pooled64)
    assert err < TIGHT[('pooled', precision)], f'pooled {name} {precision}: {err:.3e} against {TIGHT[("pooled", precision)]:.3e}'


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('name', SHAPES)
def test_expand_map(sd, refs, runs, name, precision):
    """sgb[N][P][64] against the float64 expand conv of the pooled map the GPU produced (the expand stage on its own), and
    against the float64 expand of the float64 pooled map (both stages together)"""
    _, _, expand64, _ = refs(name)
    _, pooled, sgb = runs(name, precision)
    err = check_map(f'expand {name} {precision} (of the GPU pooled map)', sgb, si.expand_reference(sd, pooled))
    both = check_map(f'expand {name} {precision} (both stages)', sgb, expand64)
    assert err < TIGHT.get(('expand', precision), si.MAP_TOL), f'expand {name} {precision}: {err:.3e}'
    assert both < TIGHT.get(('both', precision), si.MAP_TOL), f'both stages {name} {precision}: {both:.3e}'


# T7: the first and last waveform, and the ones that straddle the first three expand tile starts of the split-fp16 kernel
# (stream rows 252-258, 511-517, 763-769 around 256, 512, 768); 36 and 73 also straddle fp32 tile starts (256 and 512)
INDEPENDENT_ROWS = {'T7': (0, 36, 73, 109, 256), 'TL': (0, 1)}


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('name', list(INDEPENDENT_ROWS))
def test_rows_do_not_depend_on_the_batch(dev, sd, runs, name, precision):
    """The pooled and sgb rows of a waveform inside the batch are bit-identical to those of the waveform run alone (where
    its windows pair with no other waveform and its stream rows sit at the start of tile 0)."""
    _, pooled, sgb = runs(name, precision)
    x = si.stage_input(name)
    m = make_model(dev, sd, precision)
    for i in INDEPENDENT_ROWS[name]:
        _, p1, s1 = forward_stages(m, torch.from_numpy(x[i:i + 1]).to(dev))
        assert torch.equal(p1.cpu()[0], pooled[i]), f'pooled rows of waveform {i} of {name} depend on the batch'
        assert torch.equal(s1.cpu()[0], sgb[i]), f'sgb rows of waveform {i} of {name} depend on the batch'


@pytest.mark.parametrize('grown', [False, True])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_stages_read_only_what_the_call_wrote(dev, sd, runs, precision, grown):
    """T7 again on a workspace whose every float is NaN (the pooled and sgb regions and what follows them): the map and both
    stages stay finite and bit-identical.  `grown`: the workspace was first sized and filled by a larger batch, so stale
    finite rows of other waveforms lie behind and between the regions of this call.  Every access stays inside the
    buffer the module allocated."""
    n, L = si.STAGE_SHAPES['T7']
    y0, pooled0, sgb0 = runs('T7', precision)
    m = make_model(dev, sd, precision)
    xd = torch.from_numpy(si.stage_input('T7')).to(dev)
    if grown:
        m(torch.from_numpy(si.synth.synth_randn(300, L, seed=99)).to(dev))
        torch.cuda.synchronize()
        big = m._workspace.numel()
        got = forward_stages(m, xd)
        assert m._workspace.numel() == big, 'the smaller call replaced the workspace'
        for a, b, what in zip(got, (y0, pooled0, sgb0), ('y', 'pooled', 'sgb')):
            assert torch.equal(a.cpu(), b), f'{what} differs on a workspace that a larger batch used before'
    else:
        forward_stages(m, xd)
    ws = m._workspace
    assert ws.numel() % 4 == 0 and ws.numel() > 4 * n * (L // si.SCALE) * (si.NF_SGB + si.NF)
    ws.view(torch.float32).fill_(float('nan'))
    torch.cuda.synchronize()
    got = forward_stages(m, xd)
    for a, b, what in zip(got, (y0, pooled0, sgb0), ('y', 'pooled', 'sgb')):
        a = a.cpu()
        assert bool(torch.isfinite(a).all()), f'{what} picked up a NaN the call did not write'
        assert torch.equal(a, b), f'{what} depends on what the workspace held before the call'


# ---- the training form: stof_train_sgb_contract_pool, called as TrainEngine._sgb_contract_pool calls it ----------------
def train_contract_pool(dev, sd, x):
    """x [N, 1, L] float32 -> (pooled [N, P, 512] float32, arg [N, P, 512] uint8) on the CPU.  Both outputs carry one guard
    row behind the last window, asserted untouched: the absent second window of a last tile must store nothing."""
    from stofnet_amd import _lib
    lib = _lib.lib()
    p = {k: torch.from_numpy(np.ascontiguousarray(sd[k])).to(dev) for k in
         ('conv1.weight', 'conv1.bias', si.SG + 'contract_conv.weight', si.SG + 'contract_conv.bias')}
    xd = torch.from_numpy(np.ascontiguousarray(x[:, 0])).to(dev)
    n, L = xd.shape
    P = L // si.SCALE
    pooled = torch.full(((n * P + 1) * si.NF_SGB * 4,), GUARD, dtype=torch.uint8, device=dev)
    arg = torch.full(((n * P + 1) * si.NF_SGB,), GUARD, dtype=torch.uint8, device=dev)
    blob = torch.empty(lib.stof_train_sgb_blob_bytes(), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        code = lib.stof_train_sgb_contract_pool(_lib.ptr(p['conv1.weight']), _lib.ptr(p['conv1.bias']),
                                                _lib.ptr(p[si.SG + 'contract_conv.weight']),
                                                _lib.ptr(p[si.SG + 'contract_conv.bias']), _lib.ptr(blob), _lib.ptr(xd),
                                                _lib.ptr(pooled), _lib.ptr(arg), n, L, _lib.stream_ptr(dev))
    _lib.check(code, 'stof_train_sgb_contract_pool')
    torch.cuda.synchronize()
    pooled, arg = pooled.cpu(), arg.cpu()
    assert bool((pooled[n * P * si.NF_SGB * 4:] == GUARD).all()), 'a store behind the last window of pooled'
    assert bool((arg[n * P * si.NF_SGB:] == GUARD).all()), 'a store behind the last window of arg'
    return (pooled[:n * P * si.NF_SGB * 4].view(torch.float32).view(n, P, si.NF_SGB).clone(),
            arg[:n * P * si.NF_SGB].view(n, P, si.NF_SGB).clone())


@pytest.fixture(scope='module')
def train_runs(dev, sd):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = train_contract_pool(dev, sd, si.stage_input(name))
        return cache[name]
    return get


@pytest.mark.parametrize('name', si.TRAIN_POOLED_SHAPES)
def test_training_pooled_map(refs, runs, train_runs, name):
    """The training form's pooled map is within the stage bound of float64 and bit-identical to the inference split-fp16
    map: sgb_pack_kernel and pack_chunk16_sgb (pack_weights.cpp) build the same hi | lo fragments with the same
    roundings, the MFMAs run in the same order, and the arg form only replaces fmaxf by a compare that keeps the value."""
    _, pooled64, _, _ = refs(name)
    pooled, _ = train_runs(name)
    check_map(f'training pooled {name}', pooled, pooled64)
    _, inference, _ = runs(name, 'f16x3')
    diff = (pooled != inference)
    assert not bool(diff.any()), (f'{int(diff.sum())} elements differ from the inference map, first at '
                                  f'{where(int(diff.reshape(-1).to(torch.uint8).argmax()), tuple(pooled.shape))}')


def check_arg(tag, arg, win, s):
    """arg [..., 512] bytes against float64 windows win [..., 512, rows]: in range, never a row that is more than the gate
    below the window's maximum, and the float64 first maximum wherever that stands clear of the gate"""
    gate = si.ARG_GATE * s
    assert tuple(arg.shape) == tuple(win.shape[:-1]), tag
    assert int(arg.max()) < win.shape[-1], f'{tag}: arg byte {int(arg.max())} out of range'
    first, top, clear = si.gated_argmax(win, gate)
    at = torch.gather(win, -1, arg.long()[..., None])[..., 0]
    short = (top - at) / s
    print(f'{tag}: {1 - float(clear.double().mean()):.4%} under the gate; arg differs from the float64 first maximum in '
          f'{int((arg.long() != first).sum())} of {arg.numel()} pairs, {int(((arg.long() != first) & clear).sum())} of them gated; '
          f'largest shortfall {float(short.max()):.3e} of max|contract|')
    assert bool((at >= top - gate).all()), f'{tag}: arg names a row {float(short.max()):.3e} max|contract| below the maximum'
    bad = (arg.long() != first) & clear
    assert not bool(bad.any()), f'{tag}: {int(bad.sum())} gated pairs off the first maximum, first at flat index {int(bad.reshape(-1).to(torch.uint8).argmax())}'
    return clear


@pytest.mark.parametrize('name', si.ARG_SHAPES)
def test_argmax_on_random_inputs(refs, train_runs, name):
    """The arg-max bytes that route the pool's backward: with c the float64 contract map and s = max|c|, every byte is in
    0..79, c[arg] >= window maximum - 1e-4 s without exception, and arg is the float64 arg-max wherever the window's
    top-2 gap exceeds 1e-4 s (ten times the map bar, so a kernel that meets the bar cannot legitimately flip such a pair)."""
    _, _, _, contract = refs(name)
    _, arg = train_runs(name)
    s = float(contract.abs().max())
    clear = check_arg(f'arg {name}', arg, si.windows(contract), s)
    assert 1 - float(clear.double().mean()) < si.EXCLUDED_CAP


@pytest.mark.parametrize('q', si.TIE_PERIODS)
def test_argmax_on_exact_ties(dev, sd, q):
    """Inputs of period q: in windows 1 .. P - 2 row j + q is an exact copy of row j in the kernel too (same operands, same
    operations in the same order), so the FIRST maximum lies in rows 0 .. q - 1, and it is the float64 arg-max over those
    q rows wherever they stand clear of the gate.  Lane (j16, q4) of the kernel holds rows 16 m + 4 q4 + e, so
    q = 1 hits the strict compare inside a lane, q = 4 the neighbouring q4 lanes, q = 16 the M-tiles of one lane and
    q = 40 = 2 * 16 + 8 both.  With q = 1 the end windows (whose first / last rows differ through the zero padding and
    whose other rows tie) must also name the float64 first maximum wherever it stands clear of every row that is no
    copy of it."""
    x = si.periodic_input(q)
    contract = si.stage_reference(sd, x)['contract']
    _, arg = train_contract_pool(dev, sd, x)
    s = float(contract.abs().max())
    inner = arg[:, 1:-1]
    assert inner.shape[1] == 3
    assert int(inner.max()) < q, f'q = {q}: a tie went to row {int(inner.max())}, a later copy'
    clear = check_arg(f'arg ties q = {q}', inner, si.tie_windows(contract, q), s)
    assert 1 - float(clear.double().mean()) < si.EXCLUDED_CAP
    if q == 1:
        check_arg('arg ties q = 1, end windows', arg[:, [0, -1]], si.windows(contract)[:, [0, -1]], s)


def test_entry_point_edges(dev, sd):
    """L = 79 (no pooling window) is STOF_ERR_POOL_EMPTY, N = 0 is STOF_OK, a null arg is STOF_ERR_BAD_ARG; none of them
    touches pooled or arg."""
    from stofnet_amd import _lib
    lib = _lib.lib()
    p = [torch.from_numpy(np.ascontiguousarray(sd[k])).to(dev) for k in
         ('conv1.weight', 'conv1.bias', si.SG + 'contract_conv.weight', si.SG + 'contract_conv.bias')]
    blob = torch.empty(lib.stof_train_sgb_blob_bytes(), dtype=torch.uint8, device=dev)
    pooled = torch.full((4, 5, si.NF_SGB), 7.25, dtype=torch.float32, device=dev)
    arg = torch.full((4, 5, si.NF_SGB), GUARD, dtype=torch.uint8, device=dev)
    x = torch.from_numpy(si.synth.synth_randn(4, 400, seed=1)[:, 0]).to(dev)

    def call(xd, n, L, arg_t):
        with torch.cuda.device(dev):
            code = lib.stof_train_sgb_contract_pool(*[_lib.ptr(t) for t in p], _lib.ptr(blob), _lib.ptr(xd), _lib.ptr(pooled),
                                                    _lib.ptr(arg_t), n, L, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        assert bool((pooled == 7.25).all()) and bool((arg == GUARD).all()), 'an output was touched'
        return code

    assert call(x[:, :79].contiguous(), 4, 79, arg) == _lib.STOF_ERR_POOL_EMPTY
    assert call(x, 0, 400, arg) == _lib.STOF_OK
    assert call(x, 4, 400, None) == _lib.STOF_ERR_BAD_ARG

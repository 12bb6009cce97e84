"""The range contract of the split-fp16 modes on the MI355X, driven from every interior stage.

`precision='auto'` promises the bits of the fp32 mode whenever an activation leaves the fp16 range, `'f16x3'` (and the default
training precision) that `raise_if_overflow()` reports it.  The guard word is set from conv_last's accumulators alone, on the
claim that a non-finite activation stays non-finite through everything between its split and conv_last.  The inputs of
tests/range_contract_inputs.py put ONE overflow at a known interior stage (hidden activation behind the leaky ReLU, positive
or negative; pooled SemiGlobalBlock tensor; residual stream), on one row, at a known sample, by an exact power-of-two
rescaling -- so the expected result is known to the bit: the unscaled network's fp32 output.  tests/test_range_contract_cpu.py
checks those inputs (stage maxima, float64 equality, fp32 bit-equality on the oracle) on any machine.

A failing id names geometry, stage, k and burst position: the epilogue behind that stage dropped the NaN.
"""
import numpy as np
import pytest
import torch

import range_contract_inputs as rc

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-5          # relative to max|truth|: the project's bar for a map against the float64 oracle (test_gpu_parity.py)

FUSED_OVERFLOW = [c for c in rc.OVERFLOW_CASES if c.geom == 'fused']
LAYER_OVERFLOW = [c for c in rc.OVERFLOW_CASES if c.geom != 'fused']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import stofnet_amd  # noqa: F401
    from stofnet_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def make_model(dev, geom, sd, r, precision, seg_policy=0, train_precision='f16x3'):
    from stofnet_amd import StofNet
    g = rc.GEOMETRIES[geom]
    m = StofNet(upsample_factor=r, num_features=g['num_features'], num_blocks=g['num_blocks'],
                kernel_sizes=[9, g['body_kernel'], 3], semi_global_scale=g['semi_global_scale'], precision=precision,
                train_precision=train_precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    assert m._fused_sweep() == (geom == 'fused')
    if seg_policy:
        m._seg_policy = seg_policy          # the body sweep's segment policy (2: two segments per row)
    return m


def case_model(dev, c, precision, scaled=True):
    return make_model(dev, c.geom, c.scaled() if scaled else c.base(), c.r, precision, c.seg_policy)


def quiet(c):
    """The case's input with the loud row as quiet as the others: in range (every row is then one `check_case` bounds)."""
    return rc.burst_rows(c.n, c.L, c.pos, 1.0)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


_unscaled = {}


def unscaled_fp32(dev, geom, r, variant, x, seg_policy=0):
    """fp32-mode output of the UNSCALED network on x: computed once per (network, input), shared, never written to."""
    key = (geom, r, variant, seg_policy, x.shape, x.tobytes())
    if key not in _unscaled:
        m = make_model(dev, geom, rc.base_state_dict(geom, r, variant), r, 'fp32', seg_policy)
        _unscaled[key] = m(torch.from_numpy(x).to(dev))
    return _unscaled[key]


# ---- exact fp32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom,spec', [(g, s) for g in rc.GEOMETRIES for s in rc.EXACT_SPECS[g]])
def test_fp32_mode_returns_the_same_bits_for_every_rescaling(dev, geom, spec):
    """Fused sweep and every layer-by-layer geometry: the fp32 mode of a rescaled network is `torch.equal` to the unscaled
    one's, at every k (an exact-fp32 route has no rounding that does not commute with a power of two)."""
    x = rc.exact_input()
    xd = torch.from_numpy(x).to(dev)
    base = rc.base_state_dict(geom, 4)
    y0 = unscaled_fp32(dev, geom, 4, 'plain', x)
    c0, i0 = make_model(dev, geom, base, 4, 'fp32').forward_onsets(xd)
    for k in rc.EXACT_KS:
        m = make_model(dev, geom, rc.rescale(base, spec, k), 4, 'fp32')
        assert torch.equal(m(xd), y0), f'k={k}'
        ck, ik = m.forward_onsets(xd)
        assert torch.equal(ck, c0) and torch.equal(ik, i0), f'k={k}: onsets'


@pytest.mark.parametrize('r,n,seg_policy', [(10, 8, 0), (20, 8, 0), (4, 300, 0), (4, 8, 2)])
@pytest.mark.parametrize('spec,k', [('hid2', 12), ('stream', -12), ('sgb', 20)])
def test_fp32_mode_same_bits_other_epilogues_and_batches(dev, r, n, seg_policy, spec, k):
    """Both conv_last epilogues (r = 4, 10), conv_last_wide (r = 20), more than one work-group (300 rows), two segments."""
    x = rc.exact_input(n)
    m = make_model(dev, 'fused', rc.rescale(rc.base_state_dict('fused', r), spec, k), r, 'fp32', seg_policy)
    assert torch.equal(m(torch.from_numpy(x).to(dev)), unscaled_fp32(dev, 'fused', r, 'plain', x, seg_policy))


# ---- the guard fires from every interior stage ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', FUSED_OVERFLOW, ids=lambda c: c.id)
def test_guard_fires_from_every_interior_stage(dev, case):
    c = case
    x, xq = torch.from_numpy(c.x()).to(dev), torch.from_numpy(quiet(c)).to(dev)
    y_unscaled = unscaled_fp32(dev, c.geom, c.r, c.variant, c.x(), c.seg_policy)
    y32 = case_model(dev, c, 'fp32')(x)
    assert torch.isfinite(y32).all() and torch.equal(y32, y_unscaled)
    # 'f16x3': raise_if_overflow() reports it, once
    m16 = case_model(dev, c, 'f16x3')
    y16 = m16(x)
    print(f'{c.id}: f16x3 output finite: {bool(torch.isfinite(y16).all())}, '
          f'non-finite rows: {(~torch.isfinite(y16[:, 0])).any(-1).nonzero().flatten().tolist()}')
    with pytest.raises(FloatingPointError):
        m16.raise_if_overflow()
    m16.raise_if_overflow()
    # 'auto': the same call ends with the fp32 mode's bits -- which are the unscaled network's
    ma = case_model(dev, c, 'auto')
    ya = ma(x)
    assert ma.fell_back_to_fp32()
    assert torch.equal(ya, y32) and torch.equal(ya, y_unscaled)
    # the next in-range call is the f16x3 result to the bit and has not fallen back
    yq = ma(xq)
    assert not ma.fell_back_to_fp32()
    assert torch.equal(yq, m16(xq))
    m16.raise_if_overflow()


@pytest.mark.parametrize('case', [c for c in FUSED_OVERFLOW if c.r <= 16], ids=lambda c: c.id)
def test_forward_onsets_sync_takes_the_overflow_branch(dev, case):
    """forward_onsets(sync=True) on an interior overflow: 'auto' re-runs through the fp32 map and returns its counts and
    indices (the unscaled network's); 'f16x3' raises."""
    c = case
    x = torch.from_numpy(c.x()).to(dev)
    c32, i32 = case_model(dev, c, 'fp32').forward_onsets(x)
    c0, i0 = case_model(dev, c, 'fp32', scaled=False).forward_onsets(x)
    assert torch.equal(c32, c0) and torch.equal(i32, i0)
    ca, ia, ya = case_model(dev, c, 'auto').forward_onsets(x, return_map=True)
    assert torch.equal(ca, c32) and torch.equal(ia, i32)
    assert torch.equal(ya, unscaled_fp32(dev, c.geom, c.r, c.variant, c.x(), c.seg_policy))
    with pytest.raises(FloatingPointError):
        case_model(dev, c, 'f16x3').forward_onsets(x)


@pytest.mark.parametrize('precision', ['auto', 'f16x3'])
@pytest.mark.parametrize('case', [c for c in FUSED_OVERFLOW if c.where == 'boundary' and c.n == 8], ids=lambda c: c.id)
def test_forward_onsets_sticky_word(dev, case, precision):
    """forward_onsets(sync=False): the sticky word stays clear over safe calls, is set by ONE overflowing call among
    several safe ones, survives a read with clear=False and is cleared by the next read."""
    c = case
    x, xq = torch.from_numpy(c.x()).to(dev), torch.from_numpy(quiet(c)).to(dev)
    m = case_model(dev, c, precision)
    assert not m.onsets_overflowed()                    # before any call
    for _ in range(3):
        m.forward_onsets(xq, sync=False)
    assert not m.onsets_overflowed()
    for inp in (xq, xq, x, xq, xq):
        m.forward_onsets(inp, sync=False)
    assert m.onsets_overflowed(clear=False)
    assert m.onsets_overflowed()
    assert not m.onsets_overflowed()
    m.forward_onsets(xq, sync=False)
    assert not m.onsets_overflowed()


# ---- ... and does not fire when nothing overflowed; in-range accuracy ------------------------------------------------------
@pytest.mark.parametrize('case', rc.SAFE_CASES, ids=lambda c: c.id)
def test_guard_stays_silent_and_accuracy_holds_in_range(dev, case):
    """Ragged shapes ([1,1,96], [5,1,160], [3,1,200], [300,1,400]: rows that exist only as tile padding must not trip the
    word), activations moved by 2^+-3 within the fp16 range: 'auto' does not fall back, 'f16x3' does not raise, the sticky
    word stays clear, and the map stays within MAP_TOL of the float64 oracle with equal arg-max indices."""
    c = case
    x = torch.from_numpy(c.x()).to(dev)
    ma, m16 = case_model(dev, c, 'auto'), case_model(dev, c, 'f16x3')
    ya = ma(x)
    assert not ma.fell_back_to_fp32()
    y16 = m16(x)
    m16.raise_if_overflow()
    assert torch.equal(ya, y16)
    m16.forward_onsets(x, sync=False)
    ma.forward_onsets(x, sync=False)
    assert not m16.onsets_overflowed() and not ma.onsets_overflowed()
    ma.forward_onsets(x)
    assert not ma.fell_back_to_fp32()
    truth = rc.forward(c.scaled(), c.x(), c.r, c.geom).numpy()
    err = rel_err(y16.cpu().numpy(), truth)
    print(f'{c.id}: f16x3 rel err {err:.3e}')
    assert err < MAP_TOL
    assert np.array_equal(y16.cpu().numpy()[:, 0].argmax(-1), truth[:, 0].argmax(-1))


# ---- layer-by-layer 'f16x3' -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LAYER_OVERFLOW, ids=lambda c: c.id)
def test_layerwise_f16x3_reports_an_interior_overflow(dev, case):
    """The geometries off the fused sweep (width 32, 3-tap body, scale 40, 5 blocks) run layer by layer; with
    precision='f16x3' `raise_if_overflow()` must report an overflow there as on the fused route.  The printed line records
    whether the output itself stayed finite (the silent case: a stage swallowed the NaN)."""
    c = case
    x, xq = torch.from_numpy(c.x()).to(dev), torch.from_numpy(quiet(c)).to(dev)
    assert torch.equal(case_model(dev, c, 'fp32')(x), unscaled_fp32(dev, c.geom, c.r, c.variant, c.x()))
    m16 = case_model(dev, c, 'f16x3')
    m16(xq)
    m16.raise_if_overflow()                                 # in range: nothing to report
    y16 = m16(x)
    print(f'{c.id}: layer-by-layer f16x3 output finite (silent): {bool(torch.isfinite(y16).all())}')
    with pytest.raises(FloatingPointError):
        m16.raise_if_overflow()
    m16.raise_if_overflow()
    m16(x)
    m16(xq)                                                 # the word is sticky until it is read
    with pytest.raises(FloatingPointError):
        m16.raise_if_overflow()


# ---- training -------------------------------------------------------------------------------------------------------------
def _train_inputs(dev, n=4, L=400, r=4):
    gt = torch.randint(1, L * r, (n, 1, 2), generator=torch.Generator().manual_seed(1)).sort(-1).values.to(dev)
    return torch.from_numpy(rc.exact_input(n, L)).to(dev), gt


def _fp32_step(dev, sd, x, gt):
    from stofnet_amd.training import StofNetTrainer
    tr = StofNetTrainer(make_model(dev, 'fused', sd, 4, 'fp32', train_precision='fp32'), precision='fp32')
    loss, pred = tr.forward_backward(x, gt)
    return tr, loss.clone(), pred.clone(), {k: v.clone() for k, v in tr.g.items()}


@pytest.fixture(scope='module')
def unscaled_fp32_step(dev):
    x, gt = _train_inputs(dev)
    tr, loss, pred, g = _fp32_step(dev, rc.base_state_dict('fused', 4), x, gt)
    loss2, pred2 = tr.forward_backward(x, gt)             # a second plain fp32 step from the same state
    return loss, pred, g, (loss2.clone(), pred2.clone(), {k: v.clone() for k, v in tr.g.items()})


def test_fp32_training_step_is_bitwise_repeatable(dev, unscaled_fp32_step):
    loss, pred, g, (loss2, pred2, g2) = unscaled_fp32_step
    assert torch.equal(loss, loss2) and torch.equal(pred, pred2)
    for name in g:
        assert torch.equal(g[name], g2[name]), name


@pytest.mark.parametrize('k', [-3, 3, 12])
@pytest.mark.parametrize('spec', ['hid2', 'hid10', 'sgb', 'stream'])
def test_fp32_training_obeys_the_exact_gradient_law(dev, unscaled_fp32_step, spec, k):
    """Loss and prediction of the rescaled trainer equal the unscaled ones bitwise; a producer's weight and bias gradients are
    the unscaled ones times 2^-k, a consumer's weight gradient times 2^k, every other gradient equal -- to the bit."""
    loss0, pred0, g0, second = unscaled_fp32_step
    for name in g0:                                         # the law means nothing unless the step is repeatable
        assert torch.equal(g0[name], second[2][name]), name
    x, gt = _train_inputs(dev)
    base = rc.base_state_dict('fused', 4)
    _, loss, pred, g = _fp32_step(dev, rc.rescale(base, spec, k), x, gt)
    assert torch.equal(loss, loss0) and torch.equal(pred, pred0)
    law = rc.gradient_law(base, spec, k)
    assert set(law) == set(g)
    for name, e in law.items():
        assert torch.equal(g[name], g0[name] * 2.0 ** e), f'{name}: expected the unscaled gradient times 2^{e}'


@pytest.mark.parametrize('case', rc.TRAIN_OVERFLOW_CASES, ids=lambda c: c.id)
def test_f16x3_training_guard_sees_an_interior_overflow(dev, case):
    """An overflow behind the leaky ReLU / on the residual stream (not at the first split): the fused trainer skips the
    step (the flat buffer moves by weight decay only) and raise_if_overflow() raises once; the autograd-boundary route
    raises from backward()."""
    from stofnet_amd.training import StofNetTrainer
    c = case
    x = torch.from_numpy(c.x()).to(dev)
    _, gt = _train_inputs(dev, c.n, c.L, c.r)
    tr = StofNetTrainer(make_model(dev, 'fused', c.scaled(), c.r, 'auto'), precision='f16x3')
    before = tr.flat.clone()
    tr.train_step(x, gt)
    assert bool(torch.isfinite(tr.flat).all())
    # weight decay alone: lr * wd * |w| = 5e-4 * 1e-8 * |w|, |w| < 2^11 here
    assert float((tr.flat - before).abs().max()) < 1e-6
    with pytest.raises(FloatingPointError):
        tr.raise_if_overflow()
    tr.raise_if_overflow()
    m2 = make_model(dev, 'fused', c.scaled(), c.r, 'auto').train()
    with pytest.raises(FloatingPointError):
        (m2(x) ** 2).mean().backward()


@pytest.mark.parametrize('n,m', [(1, 64), (3, 4099), (64, 8000)])
def test_loss_sum_is_the_same_bits_run_after_run(dev, n, m):
    """The bitwise loss law above needs a loss that is repeatable to the bit: the block partials of the loss kernel meet in a
    fixed order.  One block, 49 blocks with a scalar tail, and the 512-block cap with grid-striding; five runs each, and the
    value against a float64 sum of the fp32 differences (all terms are non-negative, so two summation orders differ by at most
    count * 2^-53 of the sum)."""
    from stofnet_amd.training import StofNetTrainer
    tr = StofNetTrainer(make_model(dev, 'fused', rc.base_state_dict('fused', 4), 4, 'fp32'), precision='fp32')
    gen = torch.Generator().manual_seed(7)
    pred = torch.randn((n, m), generator=gen).to(dev)
    gt = torch.randint(1, m, (n, 2), generator=gen).sort(-1).values.to(dev)
    runs = []
    for _ in range(5):
        target, dpred = torch.empty_like(pred), torch.empty_like(pred)
        tmax = torch.empty(1, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float64, device=dev)
        tr._loss_kernels(pred, gt, n, m, 1.0, target, tmax, dpred, loss, sharded=False)
        runs.append(loss.clone())
    assert all(torch.equal(r, runs[0]) for r in runs[1:])
    lam = float(np.float32(tr.lam))                            # the kernel takes lambda as a float
    d = (pred - target).double()
    ref = ((d ** 2 + lam * pred.abs().double()).sum() / (n * m)).item()
    # the kernel forms pred - raw / max * amplitude with one rounding less than `pred - target` has (a contracted
    # multiply-subtract): each difference may be off by 2^-24 |target|, each square by 2 |d| times that
    slack = ((2.0 * d.abs() * target.abs().double()).sum() / (n * m)).item() * 2.0 ** -24
    assert abs(runs[0].item() - ref) <= slack + n * m * 2.0 ** -53 * ref

"""The references and the caps that tests/test_gpu_sgb_stages.py leans on, checked on the CPU so that the GPU file cannot
hide behind them: the float64 stage reference against the reference project's own taps, the tie policy of torch's
max-pool (the one the arg-max kernel claims to copy), the share of (window, channel) pairs that the arg-max gate sets
aside on the very inputs the GPU tests use, and the exact periodicity the tie tests rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sgb_stage_inputs as si
from conftest import golden, load_weights

MAP_TOL = 1e-5          # tests/test_oracle_golden.py


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope='module')
def sd():
    return si.state_dict()


def test_stage_reference_reproduces_the_reference_taps():
    """Fixture f1_armadillo_r4_L2000: the reference's forward hooks on contract_pool and expand_conv (the latter sees the
    conv output before its leaky ReLU, as tests/test_oracle_golden.py::test_layer_taps handles it)."""
    g = golden('f1_armadillo_r4_L2000')
    p = load_weights('different-armadillo')
    ref = si.stage_reference(p, g['x'][:1])
    assert tuple(ref['contract'].shape) == (1, 512, 2000) and tuple(ref['conv1'].shape) == (1, 64, 2000)
    assert rel_err(ref['conv1'][0].numpy(), np.maximum(g['tap_conv1'], 0)) < MAP_TOL
    assert rel_err(ref['pooled'][0].numpy(), g['tap_sgb_pooled']) < MAP_TOL
    # the pooled map is the maximum over the windows of the contract map
    assert torch.equal(si.windows(ref['contract']).amax(-1), ref['pooled'].permute(0, 2, 1))
    want = np.where(g['tap_sgb_expand'] > 0, g['tap_sgb_expand'], 0.01 * g['tap_sgb_expand'])
    e = si.expand_reference(p, ref['pooled'].permute(0, 2, 1))
    assert tuple(e.shape) == (1, 25, 64)
    assert rel_err(e[0].numpy().T, want) < MAP_TOL
    # and on the reference's own float32 pooled map: the expand reference alone
    e = si.expand_reference(p, torch.from_numpy(g['tap_sgb_pooled'].T[None]))
    assert rel_err(e[0].numpy().T, want) < MAP_TOL


def test_max_pool_returns_the_first_maximum():
    """torch's max_pool1d on float64 rows with exact ties: the index (where its backward puts the gradient) is the FIRST
    maximum of the window; gated_argmax picks the same row."""
    rng = np.random.default_rng(11)
    row = rng.standard_normal((3, 6, 2 * si.SCALE))
    top = np.abs(row).max() + 1.0
    cases = [(0, 0, (0, 79)), (0, 1, (3, 19, 35, 51, 67)), (1, 2, (16, 15)), (1, 3, (79, 40, 41)), (2, 4, (4, 8, 20, 36))]
    for n, c, rows in cases:
        for w in range(2):
            row[n, c, [si.SCALE * w + r for r in rows]] = top
    row[2, 5] = 0.25                                                     # a constant row: every sample ties
    row[0, 5, [10, si.SCALE + 10]] = top                                 # a runner-up 0.25 below the maximum, ahead of it or behind
    row[0, 5, [5, si.SCALE + 50]] = top - 0.25
    t = torch.from_numpy(row)
    val, idx = F.max_pool1d(t, si.SCALE, si.SCALE, return_indices=True)
    for n, c, rows in cases:
        assert idx[n, c].tolist() == [min(rows), si.SCALE + min(rows)]
        assert val[n, c].tolist() == [top, top]
    assert idx[2, 5].tolist() == [0, si.SCALE]
    first, best, clear = si.gated_argmax(t.reshape(3, 6, 2, si.SCALE), 0.5)
    assert torch.equal(first + si.SCALE * torch.arange(2), idx) and torch.equal(best, val)
    for n, c, _ in cases:
        assert clear[n, c].all()                                         # exact copies of the maximum do not close the gate
    assert clear[2, 5].all()
    assert idx[0, 5].tolist() == [10, si.SCALE + 10] and not clear[0, 5].any()   # a runner-up within the gate closes it
    assert si.top2_gap(t.reshape(3, 6, 2, si.SCALE))[0, 0].tolist() == [0.0, 0.0]


@pytest.mark.parametrize('name', si.ARG_SHAPES)
def test_gate_excludes_few_pairs_on_the_random_inputs(sd, name):
    """The arg-max test is only as sharp as the share of pairs it pins: under 5 % may fall under the gate, from the float64
    reference alone."""
    c = si.stage_reference(sd, si.stage_input(name))['contract']
    w = si.windows(c)
    n, L = si.STAGE_SHAPES[name]
    assert tuple(w.shape) == (n, L // si.SCALE, si.NF_SGB, si.SCALE)
    gate = si.ARG_GATE * float(c.abs().max())
    share = si.excluded_share(w, gate)
    print(f'{name}: {share:.4%} of (window, channel) pairs under the gate')
    assert share < si.EXCLUDED_CAP
    # without exact ties the tie-aware gate is the top-2 gate
    assert torch.equal(si.gated_argmax(w, gate)[2], si.top2_gap(w) > gate)


@pytest.mark.parametrize('q', si.TIE_PERIODS)
def test_periodic_inputs_tie_exactly_and_few_pairs_are_excluded(sd, q):
    """For windows 1 .. P - 2 of the periodic inputs the float64 contract map is exactly q-periodic (so the reference's
    first maximum lies in rows 0 .. q - 1), and among the q distinct rows the gate sets aside under 5 % of the pairs."""
    x = si.periodic_input(q)
    assert x.shape == (2, 1, 400) and x.dtype == np.float32
    assert np.array_equal(x[..., q:], x[..., :-q])
    c = si.stage_reference(sd, x)['contract']
    w = si.windows(c)[:, 1:-1]
    assert w.shape[1] == 3
    assert torch.equal(w[..., q:], w[..., :-q])
    assert torch.equal(w[:, 0], w[:, 1]) and torch.equal(w[:, 0], w[:, 2])
    first, _, _ = si.gated_argmax(w, 0.0)
    assert int(first.max()) < q
    tw = si.tie_windows(c, q)
    assert tuple(tw.shape) == (2, 3, si.NF_SGB, q)
    share = si.excluded_share(tw, si.ARG_GATE * float(c.abs().max()))
    print(f'q = {q}: {share:.4%} of (window, channel) pairs under the gate')
    assert share < si.EXCLUDED_CAP
    if q == 1:
        # the end windows differ from the rest through the zero padding: their first rows / last rows are no copies
        full = si.windows(c)
        assert not torch.equal(full[:, 0], full[:, 1]) and not torch.equal(full[:, -1], full[:, 1])
        assert torch.equal(full[:, 0, :, 6:], full[:, 1, :, 6:]) and torch.equal(full[:, -1, :, :74], full[:, 1, :, :74])

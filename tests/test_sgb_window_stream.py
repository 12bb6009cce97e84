"""SemiGlobalBlock contract + pool over the flat stream of N * P pooling windows (GPU).

A work-group of the contract kernel takes two consecutive entries of the flat window sequence, so its two windows may
belong to different waveforms and the last tile of a launch may hold one window only.  The shapes below put every such
arrangement in front of the float32 oracle at the project's bar (1e-5 of max|y|) and check that no row of a batch sees
its neighbours (a window that read the other waveform's samples, or zeroed the wrong edge, would show there).

Lengths at which the reference model itself raises (fewer than 80 samples: max_pool1d has no output; an odd remainder
L - 80 * (L // 80): the SemiGlobalBlock add fails) are kept as cases: the oracle raises there and the model has to raise
the same error, as tests/test_gpu_parity.py pins for other lengths of that kind.
"""
import numpy as np
import pytest
import torch

from oracle import stofnet_oracle as so
from oracle import train_oracle as to
from stofnet_amd import synth

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-5          # relative to max|y|: the project's bar (tests/test_gpu_parity.py)
GRAD_TOL = 2e-4         # tests/test_gpu_training.py::test_loss_and_all_gradients_vs_autograd, both precisions
R = 4
SEED = 3008

SHAPES = [
    (1, 2000),          # odd window count (P = 25): the last tile has an absent second window
    (3, 240),           # P = 3: tiles pair windows of different waveforms
    (5, 80),            # P = 1: every tile spans two waveforms; the last one holds one window
    (2, 159),           # P = 1, remainder 79
    (2, 1999),          # P = 24, remainder 79
    (4, 1536),          # the C4 length, P = 19
    (3, 79),            # P = 0
]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from stofnet_amd import _lib
    _lib.lib()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sd():
    return synth.synth_state_dict(R, seed=SEED)


@pytest.fixture(scope='module')
def oracle_maps(sd):
    """(N, L) -> the oracle's fp32 map, or the RuntimeError it raises; computed once for both precisions"""
    out = {}
    for n, L in SHAPES:
        x = synth.synth_randn(n, L, seed=SEED + L)
        try:
            out[(n, L)] = (x, so.stofnet_forward(sd, x, R, 80).numpy())
        except RuntimeError as e:
            out[(n, L)] = (x, e)
    return out


def make_model(dev, sd, precision):
    from stofnet_amd import StofNet
    m = StofNet(upsample_factor=R, semi_global_scale=80, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('n,L', SHAPES)
def test_forward_matches_oracle_and_rows_are_independent(dev, sd, oracle_maps, n, L, precision):
    x, want = oracle_maps[(n, L)]
    m = make_model(dev, sd, precision)
    xd = torch.from_numpy(x).to(dev)
    if isinstance(want, RuntimeError):
        # the reference has no result at this length: the same failure, for the batch and for every single row
        # (the oracle words the empty pool differently from torch's max_pool1d, so only the add's message is matched)
        key = 'must match the size of tensor b'
        key = key if key in str(want) else None
        for xi in [xd] + [xd[i:i + 1] for i in range(n)]:
            with pytest.raises(RuntimeError, match=key):
                m(xi)
        return
    y = m(xd)
    assert tuple(y.shape) == want.shape
    err = rel_err(y.cpu().numpy(), want)
    print(f'(N, L) = ({n}, {L}) {precision}: rel err {err:.3e}')
    assert err < MAP_TOL, f'({n}, {L}) {precision}: rel err {err:.3e}'
    for i in range(n):
        assert torch.equal(y[i], m(xd[i:i + 1])[0]), f'row {i} of ({n}, {L}) depends on its batch'


def test_training_forward_backward_on_paired_windows(dev):
    """(3, 240): P = 3, so the training contract kernel (arg-max bytes for the pool's backward) pairs windows of
    different waveforms and ends on a tile with one window.  Against autograd in float64."""
    from stofnet_amd import StofNet
    from stofnet_amd.training import StofNetTrainer
    n, L = 3, 240
    sd = synth.synth_state_dict(R, seed=SEED)
    m = StofNet(upsample_factor=R, semi_global_scale=80)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    tr = StofNetTrainer(m.to(dev), lr=5e-4, weight_decay=1e-8, precision='f16x3')
    x = synth.synth_echo(n, L, seed=11)
    rng = np.random.default_rng(5)
    gt = np.stack([np.sort(rng.integers(1, L * R, size=2)) for _ in range(n)])[:, None, :].astype(np.int64)
    loss_ref, grads_ref, pred_ref = to.loss_and_grads(sd, x, gt, R, 80)
    loss, pred = tr.forward_backward(torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev))
    assert rel_err(pred.cpu().numpy(), pred_ref) < 1e-5
    assert abs(float(loss) - loss_ref) < 1e-5 * abs(loss_ref)
    for name, gref in grads_ref.items():
        got = tr.g[name].cpu().numpy()
        assert got.shape == gref.shape
        err = rel_err(got, gref)
        assert err < GRAD_TOL, (name, err)

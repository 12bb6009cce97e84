"""GPU parity tests: the HIP path (through the C ABI) against the committed golden
vectors and the CPU oracle.  Run on the MI355X box: pytest -m gpu."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_weights
from oracle import pickers_oracle as po
from oracle import stofnet_oracle as so
from stofnet_amd import synth

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
MAP_TOL = 1e-5          # relative to max-abs(y), SURVEY.md 8c: exact-fp32 mode vs the reference's fp32 maps
# f16x3 mode vs the reference's fp32 maps: two independent fp32-level roundings apart (the reference
# itself sits 2e-6 from the fp64 truth on these cases, this mode 1e-6..7e-6); against the fp64
# ground truth both modes must stay within MAP_TOL (test_forward_vs_fp64_truth).
MAP_TOL_F16X3_VS_REF = 1e-5    # measured worst case over the golden set: 4.3e-6 (profiles/r02_precision.json)
ENV_TOL = 1e-5          # absolute, on max-abs-normalised inputs (north_star)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import stofnet_amd  # noqa: F401
    from stofnet_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def make_model(dev, sd, r, sgs=80, precision='fp32'):
    from stofnet_amd import StofNet
    m = StofNet(upsample_factor=r, semi_global_scale=sgs, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


FWD_CASES = [
    ('f1_armadillo_r4_L2000', 'different-armadillo', 4, 80),
    ('f1_snow_r4_L1536', 'graceful-snow', 4, 80),
    ('f1_armadillo_r4_L20000', 'different-armadillo', 4, 80),
    ('f1_armadillo_r10_L2000', 'different-armadillo', 10, 80),
    ('f1_snow_r20_L2000', 'graceful-snow', 20, 80),
    ('f1_serenity_nosgb_r4_L2000', 'clean-serenity', 4, 1),
]


PRECISIONS = ['fp32', 'f16x3']


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case,wkey,r,sgs', FWD_CASES)
def test_forward_matches_reference_golden(dev, case, wkey, r, sgs, precision):
    g = golden(case)
    sd = load_weights(wkey)
    if 'conv_last_weight' in g.files:
        sd['conv_last.weight'], sd['conv_last.bias'] = g['conv_last_weight'], g['conv_last_bias']
    m = make_model(dev, sd, r, sgs, precision)
    y = m(torch.from_numpy(g['x']).to(dev)).cpu().numpy()
    assert y.shape == g['y'].shape
    err = rel_err(y, g['y'])
    tol = MAP_TOL if precision == 'fp32' else MAP_TOL_F16X3_VS_REF
    assert err < tol, f'{case}: rel err {err:.3e}'
    # integer onset indices (arg-max mode) bit-exact against the reference's maps
    assert np.array_equal(y[:, 0].argmax(-1), g['y'][:, 0].argmax(-1))


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case,wkey,r,sgs', FWD_CASES[:2] + FWD_CASES[3:])
def test_forward_vs_fp64_truth(dev, case, wkey, r, sgs, precision):
    """Accuracy against the float64 oracle (independent shifted-matmul conv): both modes within 1e-5."""
    g = golden(case)
    sd = load_weights(wkey)
    if 'conv_last_weight' in g.files:
        sd['conv_last.weight'], sd['conv_last.bias'] = g['conv_last_weight'], g['conv_last_bias']
    m = make_model(dev, sd, r, sgs, precision)
    x = g['x'][:2]
    y = m(torch.from_numpy(x).to(dev)).cpu().numpy()
    truth = so.stofnet_forward(sd, x, r, sgs, torch.float64, conv=so.conv1d_shifted_matmul).numpy()
    assert rel_err(y, truth) < MAP_TOL


@pytest.mark.parametrize('precision', PRECISIONS + ['auto'])
@pytest.mark.parametrize('scale', [1e-2, 1e-4, 1e-6])
def test_forward_small_amplitude_inputs(dev, precision, scale):
    """Un-normalised, small-amplitude inputs: the fp16 split hi = fp16(v), lo = fp16(v - hi) loses the lo
    term's low bits to fp16 underflow for |v| < 2^-3, but the loss is ABSOLUTE (<= 2^-25 per operand, the half quantum
    of an fp16 subnormal), i.e. below the fp32 rounding of any accumulator of magnitude >= 0.5 -- so maps and onset
    indices of tiny inputs must still meet the fp32 bar against the float64 truth."""
    g = golden('f1_armadillo_r4_L2000')
    sd = load_weights('different-armadillo')
    m = make_model(dev, sd, 4, 80, precision)
    x = (g['x'][:4] * scale).astype(np.float32)
    y = m(torch.from_numpy(x).to(dev)).cpu().numpy()
    truth = so.stofnet_forward(sd, x, 4, 80, torch.float64, conv=so.conv1d_shifted_matmul).numpy()
    ref32 = so.stofnet_forward(sd, x, 4, 80).numpy()
    err, err_ref = rel_err(y, truth), rel_err(ref32, truth)
    assert err < MAP_TOL, f'scale {scale}: rel err {err:.3e} (torch fp32 itself: {err_ref:.3e})'
    # the input-dependent part of the map (what a tiny input changes against a silent one), relative to ITS size
    z = np.zeros_like(x)
    y0 = m(torch.from_numpy(z).to(dev)).cpu().numpy()
    t0 = so.stofnet_forward(sd, z, 4, 80, torch.float64, conv=so.conv1d_shifted_matmul).numpy()
    r0 = so.stofnet_forward(sd, z, 4, 80).numpy()
    resp_err = np.abs((y - y0) - (truth - t0)).max() / max(np.abs(truth - t0).max(), 1e-30)
    resp_ref = np.abs((ref32 - r0) - (truth - t0)).max() / max(np.abs(truth - t0).max(), 1e-30)
    print(f'small-amplitude scale {scale} {precision}: map err {err:.2e} (torch fp32 {err_ref:.2e}); '
          f'response err {resp_err:.2e} (torch fp32 {resp_ref:.2e})')
    if precision == 'fp32':
        assert resp_err < max(4 * resp_ref, 1e-4), f'response err {resp_err:.3e} vs torch fp32 {resp_ref:.3e}'
    assert np.array_equal(y[:, 0].argmax(-1), truth[:, 0].argmax(-1))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_forward_seeded_r10(dev, precision):
    g = golden('f1_seeded_r10_L2000')
    m = make_model(dev, synth.synth_state_dict(10, seed=3008), 10, precision=precision)
    y = m(torch.from_numpy(g['x']).to(dev)).cpu().numpy()
    assert rel_err(y, g['y']) < MAP_TOL


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('L', [1536, 2000, 2040, 2578, 160, 96])
def test_sgb_length_quirks(dev, L, precision):
    g = golden('f3_sgb_lengths')
    m = make_model(dev, load_weights('different-armadillo'), 4, precision=precision)
    y = m(torch.from_numpy(g[f'x_L{L}']).to(dev)).cpu().numpy()
    assert rel_err(y, g[f'y_L{L}']) < MAP_TOL


@pytest.mark.parametrize('precision', PRECISIONS + ['auto'])
def test_short_rows_like_reference(dev, precision):
    """Fewer than one pooling window: the reference's SemiGlobalBlock fails in max_pool1d (L = 40, 78, 79; recorded in
    tests/golden/manifest_r2.json f3_short_status); exactly one window (L = 80) and 80 + 2 work."""
    status = json.load(open(os.path.join(GOLDEN, 'manifest_r2.json')))['f3_short_status']
    g = golden('f3_short_lengths')
    m = make_model(dev, load_weights('different-armadillo'), 4, precision=precision)
    for L in (40, 78, 79):
        assert status[str(L)][0] == 'RuntimeError'
        with pytest.raises(RuntimeError, match=r'max_pool1d\(\) Invalid computed output size: 0'):
            m(torch.from_numpy(g[f'x_L{L}']).to(dev))
    for L in (80, 82):
        y = m(torch.from_numpy(g[f'x_L{L}']).to(dev)).cpu().numpy()
        assert rel_err(y, g[f'y_L{L}']) < MAP_TOL_F16X3_VS_REF
    nosgb = make_model(dev, load_weights('clean-serenity'), 4, 1, precision)        # no pooling: any length works
    x = torch.from_numpy(g['x_L40']).to(dev)
    ref = so.stofnet_forward(load_weights('clean-serenity'), g['x_L40'], 4, 1).numpy()
    assert rel_err(nosgb(x).cpu().numpy(), ref) < MAP_TOL_F16X3_VS_REF


@pytest.mark.parametrize('L', [1999, 2001, 2041])
def test_sgb_odd_remainder_raises_like_reference(dev, L):
    m = make_model(dev, load_weights('different-armadillo'), 4)
    with pytest.raises(RuntimeError, match=r'must match the size of tensor b'):
        m(torch.zeros(1, 1, L, device=dev))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_argmax_indices_1024_rows_bit_exact(dev, precision):
    from stofnet_amd.mask2samples import onset_indices, mask2coords
    g = golden('f1_armadillo_r4_argmax1024')
    m = make_model(dev, load_weights('different-armadillo'), 4, precision=precision)
    x = torch.from_numpy(synth.synth_echo(1024, 2000, seed=int(g['seed']))).to(dev)
    y = m(x)
    counts, idx = onset_indices(y, 20, None)
    ref = g['indices']
    margins = g['top2'][:, 0] - g['top2'][:, 1]
    assert np.array_equal(counts.cpu().numpy(), np.ones(1024, np.int32)), 'a row has a tie the reference does not have'
    got = idx[:, 0].cpu().numpy()
    bad = np.nonzero(got != ref[:, 1])[0]
    mae = np.abs(got.astype(np.int64) - ref[:, 1]).mean()
    assert bad.size == 0, f'{bad.size} flips, MAE {mae}; min margin {margins.min():.3g}; margins at flips {margins[bad]}'
    assert np.array_equal(mask2coords(y, 20, None, 4).cpu().numpy(), g['coords'])


@pytest.mark.parametrize('precision', PRECISIONS + ['auto'])
def test_argmax_indices_4096_rows_bit_exact(dev, precision):
    """arg-max onset indices of the reference forward for 4096 seeded echoes (make_golden_r2.py argmax4096)."""
    from stofnet_amd.mask2samples import onset_indices
    g = golden('f1_armadillo_r4_argmax4096')
    m = make_model(dev, load_weights('different-armadillo'), 4, precision=precision)
    x = torch.from_numpy(synth.synth_echo(4096, 2000, seed=int(g['seed']))).to(dev)
    counts, idx = onset_indices(m(x), 20, None)
    assert np.array_equal(counts.cpu().numpy(), np.ones(4096, np.int32)), 'a row has a tie the reference does not have'
    got = idx[:, 0].cpu().numpy()
    bad = np.nonzero(got != g['indices'])[0]
    margins = g['top2'][:, 0] - g['top2'][:, 1]
    assert bad.size == 0, f'{bad.size} flips; min margin {margins.min():.3g}; margins at flips {margins[bad]}'


@pytest.mark.parametrize('precision', PRECISIONS + ['auto'])
def test_argmax_indices_4096_rows_at_the_benched_shape_r10(dev, precision):
    """The benched configuration C2 ([4096,1,2000] -> [4096,1,20000], upsample_factor 10): arg-max onset indices of the
    reference forward (different-armadillo body + the seeded conv_last of f1_armadillo_r10_L2000) for 4096 seeded echoes
    (tests/golden/make_golden_r3.py argmax4096_r10), through the map + picker kernel AND through the picker fused into
    the sweep (stof_forward_onsets)."""
    from stofnet_amd.mask2samples import onset_indices
    g = golden('f1_armadillo_r10_argmax4096')
    sd = load_weights('different-armadillo')
    sd['conv_last.weight'], sd['conv_last.bias'] = synth.synth_conv_last(10, seed=int(g['conv_last_seed']))
    m = make_model(dev, sd, 10, precision=precision)
    x = torch.from_numpy(synth.synth_echo(4096, 2000, seed=int(g['seed']))).to(dev)
    counts, idx = onset_indices(m(x), 20, None)
    margins = g['top2'][:, 0] - g['top2'][:, 1]
    assert np.array_equal(counts.cpu().numpy(), np.ones(4096, np.int32)), 'a row has a tie the reference does not have'
    got = idx[:, 0].cpu().numpy()
    bad = np.nonzero(got != g['indices'])[0]
    assert bad.size == 0, f'{bad.size} flips; min margin {margins.min():.3g}; margins at flips {margins[bad]}'
    fc, fi = m.forward_onsets(x, 20)
    assert torch.equal(fc, counts) and torch.equal(fi, idx)
    print(f'r10 argmax 4096 rows {precision}: 0 flips, smallest top-2 margin {margins.min():.3g} (median {np.median(margins):.3g})')


@pytest.mark.parametrize('precision', PRECISIONS)
def test_forward_batch_and_workgroup_splits(dev, precision):
    """Rows are independent: any batch split gives identical bits (the sweep walks several
    waveforms per work-group; row 0 alone must equal row 0 inside a batch of 300)."""
    m = make_model(dev, synth.synth_state_dict(4, seed=12), 4, precision=precision)
    x = torch.from_numpy(synth.synth_randn(300, 400, seed=5)).to(dev)
    y = m(x)
    y1 = torch.cat([m(x[:1]), m(x[1:7]), m(x[7:])], 0)
    assert torch.equal(y, y1)
    ref = so.stofnet_forward(synth.synth_state_dict(4, seed=12), x[:4].cpu().numpy(), 4, 80).numpy()
    assert rel_err(y[:4].cpu().numpy(), ref) < MAP_TOL


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('L', [2000, 1536, 2578, 960])
def test_small_batch_segment_mode_is_bit_identical(dev, precision, L):
    """Small batches are swept as 2^k overlapping segments per waveform (+-38 rows of context) so the CUs are not idle:
    every output row sees the same arithmetic, so forcing 1, 2, 4 or 8 segments must give identical bits, and the
    automatic choice must match the oracle."""
    sd = load_weights('different-armadillo')
    x = torch.from_numpy(synth.synth_echo(3, L, seed=17)).to(dev)
    outs = []
    for policy in (1, 2, 3, 4, 0):                        # 1, 2, 4, 8 segments, automatic
        m = make_model(dev, sd, 4, precision=precision)
        m._seg_policy = policy
        outs.append(m(x))
    for y in outs[1:]:
        assert torch.equal(outs[0], y)
    ref = so.stofnet_forward(sd, x.cpu().numpy(), 4, 80).numpy()
    assert rel_err(outs[-1].cpu().numpy(), ref) < (MAP_TOL if precision == 'fp32' else MAP_TOL_F16X3_VS_REF)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_forward_full_size_row_independence(dev, precision):
    """Full-size property check at C2 shape [4096,1,2000]: every row equals the same row
    computed in a small batch (no cross-row leakage at full occupancy)."""
    m = make_model(dev, synth.synth_state_dict(10, seed=3008), 10, precision=precision)
    x = torch.from_numpy(synth.synth_randn(4096, 2000, seed=3008)).to(dev)
    y = m(x)
    assert y.shape == (4096, 1, 20000)
    sel = [0, 1, 255, 256, 2047, 4095]
    y_small = m(x[sel])
    assert torch.equal(y[sel], y_small)
    ref = so.stofnet_forward(synth.synth_state_dict(10, seed=3008), x[sel[:3]].cpu().numpy(), 10, 80).numpy()
    assert rel_err(y[sel[:3]].cpu().numpy(), ref) < MAP_TOL


@pytest.mark.parametrize('precision', PRECISIONS)
def test_config_c3_r20_full_size(dev, precision):
    """BASELINE config C3: [4096,1,2000] -> [4096,1,40000] at r=20 (shuffle-stress shape)."""
    sd = load_weights('graceful-snow')
    g = golden('f1_snow_r20_L2000')
    sd['conv_last.weight'], sd['conv_last.bias'] = g['conv_last_weight'], g['conv_last_bias']
    m = make_model(dev, sd, 20, precision=precision)
    x = torch.from_numpy(synth.synth_echo(4096, 2000, seed=21)).to(dev)
    x[:2] = torch.from_numpy(g['x']).to(dev)
    y = m(x)
    assert y.shape == (4096, 1, 40000)
    tol = MAP_TOL if precision == 'fp32' else MAP_TOL_F16X3_VS_REF
    assert rel_err(y[:2].cpu().numpy(), g['y']) < tol                 # golden rows inside the full batch
    sel = [5, 1000, 4095]
    assert torch.equal(y[sel], m(x[sel]))                             # row independence at full occupancy
    ref = so.stofnet_forward(sd, x[sel[:2]].cpu().numpy(), 20, 80).numpy()
    assert rel_err(y[sel[:2]].cpu().numpy(), ref) < tol


@pytest.mark.parametrize('precision', PRECISIONS)
def test_config_c4_pala_chunk_threshold_mode(dev, precision):
    """BASELINE config C4, one per-GPU chunk and a bit: [8192+50 rows,1,1536] (L mod 80 = 16 -> the SGB
    pad quirk), graceful-snow, mask2coords in threshold mode th=0.015 (bash_scripts/array_pala_params.txt:1).
    N > 4096 also exercises the internal sub-batching of stof_forward."""
    from stofnet_amd import mask2coords
    sd = load_weights('graceful-snow')
    m = make_model(dev, sd, 4, precision=precision)
    n = 8192 + 50
    x = torch.from_numpy(synth.synth_echo(n, 1536, seed=31)).to(dev)
    y = m(x)
    assert y.shape == (n, 1, 6144)
    sel = [0, 4095, 4096, 8191, 8192, n - 1]                          # both sides of the sub-batch seams
    ref = so.stofnet_forward(sd, x[sel].cpu().numpy(), 4, 80).numpy()
    tol = MAP_TOL if precision == 'fp32' else MAP_TOL_F16X3_VS_REF
    assert rel_err(y[sel].cpu().numpy(), ref) < tol
    coords = mask2coords(y, 20, 0.015, 4)
    exp = po.mask2coords(y[sel].cpu().numpy(), 20, 0.015, 4)          # picker parity on the GPU's own maps
    got = coords[sel].cpu().numpy()
    k = exp.shape[1]
    assert np.array_equal(got[:, :k], exp) and not got[:, k:].any()
    # onset indices of the network output vs the oracle's maps (index parity of the whole chain)
    assert np.array_equal(po.mask2coords(ref, 20, None, 4), mask2coords(y[sel], 20, None, 4).cpu().numpy())


def test_empty_batch(dev):
    m = make_model(dev, synth.synth_state_dict(4, seed=1), 4)
    assert m(torch.zeros(0, 1, 160, device=dev)).shape == (0, 1, 640)


# ---------------------------------------------------------------- shuffle
def test_shuffle_bit_exact(dev):
    from stofnet_amd import SampleShuffle1D
    g = golden('f2_shuffle')
    for r, c in [(4, 1), (10, 1), (20, 1), (4, 16), (3, 2)]:
        out = SampleShuffle1D(r)(torch.from_numpy(g[f'in_r{r}_c{c}']).to(dev)).cpu().numpy()
        assert np.array_equal(out, g[f'out_r{r}_c{c}'])
    with pytest.raises(RuntimeError):
        SampleShuffle1D(3)(torch.zeros(1, 7, 4, device=dev))


@pytest.mark.parametrize('r,C,W,N', [(20, 1, 2000, 64), (10, 1, 2000, 16), (4, 16, 777, 3), (4, 1, 1, 5)])
def test_shuffle_against_oracle_large(dev, r, C, W, N):
    from stofnet_amd import SampleShuffle1D
    x = torch.randn(N, r * C, W, generator=torch.Generator().manual_seed(r * W))
    out = SampleShuffle1D(r)(x.to(dev)).cpu()
    assert torch.equal(out, so.sample_shuffle(x, r))


@pytest.mark.parametrize('dtype', [torch.int64, torch.float64, torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool,
                                   torch.complex64, torch.complex128, torch.int32])
def test_shuffle_is_dtype_agnostic_bit_for_bit(dev, dtype):
    """utils/sample_shuffle.py:24-27 is view / permute / contiguous: any dtype, no arithmetic.  int64 ramps beyond 2^24 (which a
    detour through fp32 would round), float64, the 16-bit floats, bool and the complex types come back bit for bit, dtype kept."""
    from stofnet_amd import SampleShuffle1D
    n, r, c, w = 3, 5, 2, 301
    g = torch.Generator().manual_seed(11)
    if dtype == torch.bool:
        x = torch.randint(0, 2, (n, r * c, w), generator=g).bool()
    elif dtype.is_complex:
        x = torch.complex(torch.randn(n, r * c, w, generator=g, dtype=torch.float64), torch.randn(n, r * c, w, generator=g, dtype=torch.float64)).to(dtype)
    elif dtype.is_floating_point:
        x = (torch.randn(n, r * c, w, generator=g, dtype=torch.float64) * 1e3).to(dtype)
    elif dtype == torch.uint8:
        x = torch.randint(0, 256, (n, r * c, w), generator=g).to(dtype)
    else:
        hi = min(torch.iinfo(dtype).max, 2 ** 62)
        x = (torch.arange(n * r * c * w, dtype=torch.int64).reshape(n, r * c, w) * 7919 + (2 ** 40 if dtype == torch.int64 else 0)) % hi
        x = x.to(dtype)
    out = SampleShuffle1D(r)(x.to(dev))
    want = so.sample_shuffle(x, r)
    assert out.dtype == dtype and out.shape == want.shape
    assert torch.equal(out.cpu().view(torch.uint8) if dtype != torch.bool else out.cpu(), want.view(torch.uint8) if dtype != torch.bool else want)


def test_shuffle_roundtrip_property_full_size(dev):
    """C3 size [4096,20,2000] -> [4096,1,40000]: the shuffle is a permutation, so sums of
    every k-strided slice must equal the channel sums."""
    from stofnet_amd import SampleShuffle1D
    x = torch.randint(-8, 8, (4096, 20, 2000), device=dev, dtype=torch.int32).float()
    out = SampleShuffle1D(20)(x)
    assert out.shape == (4096, 1, 40000)
    assert torch.equal(out.view(4096, 2000, 20).permute(0, 2, 1), x)


# ---------------------------------------------------------------- picker
TH = {'none': None, 'zero': 0, '1p5': 1.5, 'neg': -0.75}


def test_picker_hand_cases_bit_exact(dev):
    from stofnet_amd import mask2coords, get_maxima_positions
    g = golden('f4_picker_hand')
    names = sorted({f[3:] for f in g.files if f.startswith('in_')})
    for name in names:
        s = torch.from_numpy(g['in_' + name]).to(dev)
        for thn, th in TH.items():
            idx = get_maxima_positions(s, 20, th).cpu().numpy()
            assert np.array_equal(idx, g[f'idx_{name}_th{thn}'].reshape(-1, 2)), (name, thn)
            for em in [None, 3]:
                exp = g[f'out_{name}_th{thn}_em{em}']
                out = mask2coords(s, 20, th, 4, em).cpu().numpy()
                assert out.shape == exp.shape, (name, thn, em)
                if name == 'tie_nms_neg' and em == 3:
                    out, exp = out[:2], exp[:2]          # amplitude ties: unspecified in the reference
                assert np.array_equal(out, exp), (name, thn, em)
        assert np.array_equal(mask2coords(s, 5, None, 1).cpu().numpy(), g[f'out_{name}_w5'])
        assert np.array_equal(mask2coords(s, 4, 0.5, 2).cpu().numpy(), g[f'out_{name}_w4_th'])


def test_picker_on_network_maps(dev):
    from stofnet_amd import mask2coords, get_maxima_positions
    g = golden('f4_picker_on_maps')
    y = torch.from_numpy(g['y']).to(dev)
    assert np.array_equal(get_maxima_positions(y, 20, None).cpu().numpy(), g['idx_none'])
    assert np.array_equal(get_maxima_positions(y, 20, 0.015).cpu().numpy(), g['idx_th'])
    assert np.array_equal(mask2coords(y, 20, 0.015, 4).cpu().numpy(), g['coords_th'])
    assert np.array_equal(mask2coords(y, 20, None, 4).cpu().numpy(), g['coords_none'])
    assert np.array_equal(mask2coords(y, 20, 0.015, 4, 3).cpu().numpy(), g['coords_th_echo3'])
    assert np.array_equal(mask2coords(y, 20, 0.015, 4, 40).cpu().numpy(), g['coords_th_echo40'])


def test_batch_mask2coords_and_nested_list_vs_reference(dev):
    """utils/mask2samples.py:37-79 (the two helpers main.py:19 imports besides mask2coords) and the echo_max reduction
    kernel, against the reference's outputs (make_golden_r2.py batch_coords)."""
    from utils.mask2samples import batch_mask2coords, mask2coords, mask2nested_list      # the drop-in module path
    g = golden('f4_batch_coords')
    s = torch.from_numpy(g['scores']).to(dev)
    assert np.array_equal(batch_mask2coords(s, 20, 1.0, 4).cpu().numpy(), g['coords'])
    nested = mask2nested_list(s, 20, 1.0, 4)
    assert np.array_equal(np.array([[len(c) for c in b] for b in nested], np.int64), g['nested_len'])
    assert np.array_equal(np.concatenate([np.asarray(c, np.float32) for b in nested for c in b]), g['nested_val'])
    s1 = torch.from_numpy(g['scores1']).to(dev)
    for em in (2, 3):
        assert np.array_equal(mask2coords(s1, 20, 0.8, 4, em).cpu().numpy(), g[f'm2c_em{em}'])


@pytest.mark.parametrize('M,win,th', [(1000, 20, None), (1025, 20, 0.3), (3000, 7, 0.0), (5000, 1, 1.0),
                                      (40000, 20, None), (17, 20, None), (4097, 128, 0.5)])
def test_picker_random_vs_oracle(dev, M, win, th):
    from stofnet_amd import mask2coords
    rng = np.random.default_rng(M + win)
    s = rng.standard_normal((5, 1, M)).astype(np.float32)
    s[1, 0, ::3] = np.round(s[1, 0, ::3])            # exact ties and exact zeros
    s[2, 0] = np.round(s[2, 0] * 2) / 2
    out = mask2coords(torch.from_numpy(s).to(dev), win, th, 4).cpu().numpy()
    assert np.array_equal(out, po.mask2coords(s, win, th, 4))


def test_picker_full_size_property(dev):
    """[4096,1,20000] arg-max mode: every row reports exactly the positions of its maximum."""
    from stofnet_amd.mask2samples import onset_indices
    y = torch.randn(4096, 1, 20000, device=dev)
    counts, idx = onset_indices(y, 20, None)
    assert torch.equal(counts, torch.ones_like(counts))
    assert torch.equal(idx[:, 0].long(), y[:, 0].argmax(-1))


# ---------------------------------------------------------------- Hilbert
@pytest.mark.parametrize('n', [7, 16, 1536, 2000, 2001, 8000, 20000])
def test_hilbert_golden(dev, n):
    from stofnet_amd import hilbert_transform
    from stofnet_amd.hilbert import hilbert_envelope
    g = golden('f5_hilbert')
    x = torch.from_numpy(g[f'x_n{n}']).to(dev)
    env = hilbert_envelope(x).cpu().numpy()
    assert np.abs(env - g[f'env_n{n}']).max() < ENV_TOL
    v = hilbert_transform(x)
    assert v.dtype == torch.complex64 and v.shape == x.shape
    if n <= 2001:
        assert np.abs(v.real.cpu().numpy() - g[f're_n{n}']).max() < ENV_TOL
        assert np.abs(v.imag.cpu().numpy() - g[f'im_n{n}']).max() < ENV_TOL
    # ground truth in float64
    assert np.abs(env - po.hilbert_envelope(g[f'x_n{n}'])).max() < ENV_TOL


@pytest.mark.parametrize('n', [1, 2, 3, 5, 31, 97, 1999, 4096, 6000, 10007, 20480])
def test_hilbert_more_lengths_vs_oracle(dev, n):
    from stofnet_amd.hilbert import hilbert_envelope
    x = synth.synth_randn(3, n, seed=n)
    env = hilbert_envelope(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert np.abs(env - po.hilbert_envelope(x)).max() < ENV_TOL


@pytest.mark.parametrize('n', [1536, 2000, 2048, 4000, 4096, 6144, 8000, 15360, 20000])
@pytest.mark.parametrize('rows', [1, 2, 7, 1030])
def test_hilbert_compile_time_plan_lengths(dev, n, rows):
    """Row lengths served by the compile-time plans (hilbert_ct_kernel): odd batches leave a lone row in the last pair,
    1030 rows = more pairs than one pass of the persistent grid's slots on a small grid; analytic signal and envelope
    against the float64 oracle; an unaligned view must fall back to the run-time-plan kernel with the same result."""
    from stofnet_amd import hilbert_transform
    from stofnet_amd.hilbert import hilbert_envelope
    x = synth.synth_randn(rows, n, seed=n + rows)[:, 0]
    xd = torch.from_numpy(x).to(dev)
    env = hilbert_envelope(xd).cpu().numpy()
    want = po.hilbert_transform(x)
    assert np.abs(env - np.abs(want)).max() < ENV_TOL
    v = hilbert_transform(xd).cpu().numpy()
    assert np.abs(v.real - want.real).max() < ENV_TOL and np.abs(v.imag - want.imag).max() < ENV_TOL
    if rows == 7:
        big = torch.zeros(rows * n + 1, device=dev)
        big[1:] = xd.reshape(-1)
        shifted = big[1:].view(rows, n)                      # 4-byte aligned rows only
        assert np.abs(hilbert_envelope(shifted).cpu().numpy() - env).max() < ENV_TOL


@pytest.mark.parametrize('n', [1, 2, 7, 16, 250, 2000, 2001])
def test_hilbert_float64_golden(dev, n):
    """utils/hilbert.py:11: a float64 input stays in complex128 (torch.fft.fft's dtype rule); reference golden f15."""
    from stofnet_amd import hilbert_transform, HilbertTransform
    g = golden('f15_hilbert_f64')
    x = torch.from_numpy(g[f'x_n{n}']).to(dev)
    v = hilbert_transform(x)
    assert v.dtype == torch.complex128 and v.shape == x.shape
    scale = max(1.0, float(np.abs(g[f'x_n{n}']).max()))
    assert np.abs(v.real.cpu().numpy() - g[f're_n{n}']).max() < 1e-12 * scale
    assert np.abs(v.imag.cpu().numpy() - g[f'im_n{n}']).max() < 1e-12 * scale
    env = HilbertTransform()(x[:, None, :])
    assert env.dtype == torch.float64
    assert np.abs(env[:, 0].cpu().numpy() - np.hypot(g[f're_n{n}'], g[f'im_n{n}'])).max() < 1e-12 * scale


@pytest.mark.parametrize('rows,n', [(1, 3), (5, 31), (2, 97), (3, 1999), (700, 1536), (4, 4096), (2, 10007), (3, 20000), (2, 30720)])
def test_hilbert_float64_more_lengths_vs_oracle(dev, rows, n):
    """Any n (prime lengths run as one O(n^2) stage), more rows than the persistent grid (700 > 512), long rows."""
    from stofnet_amd import hilbert_transform
    x = np.random.RandomState(n).standard_normal((rows, n))
    v = hilbert_transform(torch.from_numpy(x).to(dev)).cpu().numpy()
    want = po.hilbert_transform(x)
    assert np.abs(v - want).max() < 1e-11


def test_hilbert_module_concat(dev):
    from stofnet_amd import HilbertTransform
    g = golden('f5_hilbert')
    out = HilbertTransform(concat_oscil=True)(torch.from_numpy(g['concat_in']).to(dev)).cpu().numpy()
    assert out.shape == g['concat_out'].shape
    assert np.abs(out - g['concat_out']).max() < ENV_TOL


def test_hilbert_real_part_property_full_size(dev):
    """[4096, 2000]: the real part of the analytic signal is the input (to fp32 rounding)."""
    from stofnet_amd import hilbert_transform
    x = torch.from_numpy(synth.synth_randn(4096, 2000, seed=1)).to(dev)
    v = hilbert_transform(x)
    assert (v.real - x).abs().max().item() < 1e-5


# ---------------------------------------------------------------- GradPeak
@pytest.mark.parametrize('rf', [10, 20])
@pytest.mark.parametrize('thn,th', [('none', None), ('1em3', 1e-3), ('1em5', 1e-5)])
def test_gradpeak_golden(dev, rf, thn, th):
    from stofnet_amd import GradPeak, toa_detect
    g = golden('f6_gradpeak')
    x = torch.from_numpy(g[f'x_rf{rf}']).to(dev)
    exp_e = g[f'echoes_rf{rf}_th{thn}']
    got_e = toa_detect(x.squeeze(1), threshold=th, rescale_factor=rf).cpu().numpy()
    assert got_e.shape == exp_e.shape
    assert np.array_equal(got_e[..., :2], exp_e[..., :2])          # integer onset / peak indices: exact
    assert np.abs(got_e[..., 2] - exp_e[..., 2]).max() < ENV_TOL
    for oo in [True, False]:
        for emn, em in [('1', 1), ('inf', float('inf')), ('2', 2)]:
            key = f'out_rf{rf}_th{thn}_onset{int(oo)}_em{emn}'
            out = GradPeak(threshold=th, rescale_factor=rf, echo_max=em, onset_opt=oo)(x).cpu().numpy()
            assert np.array_equal(out, g[key]), key


def test_gradpeak_gradient_stage(dev):
    from stofnet_amd import _lib
    from stofnet_amd.gradpeak import gaussian_kernel_1d
    g = golden('f6_gradpeak')
    for rf in [10, 20]:
        gs = rf // 6 * 5
        assert np.allclose(gaussian_kernel_1d((gs * 2 - 1) / 6).numpy(), g[f'taps_rf{rf}'], rtol=0, atol=1e-15)


def test_gradpeak_degenerate_cases(dev):
    from stofnet_amd import GradPeak, grad_peak_detect
    g = golden('f6_gradpeak')
    out = grad_peak_detect(torch.from_numpy(g['env_q9']).to(dev), grad_step=5, threshold=1e-3, ival_smin=6, ival_smax=300)
    assert list(out.shape) == MANIFEST['f6_status']['q9_direct'][1] == [3, 0]        # Q9
    out = grad_peak_detect(torch.from_numpy(g['env_q9'][1:]).to(dev), grad_step=5, threshold=1e-3, ival_smin=6, ival_smax=300)
    assert np.array_equal(out.cpu().numpy()[..., :2], g['q9_direct_row1_only'][..., :2])
    assert MANIFEST['f6_status']['noedges'][0] == 'IndexError'
    with pytest.raises(IndexError):
        GradPeak(threshold=1e-3, rescale_factor=10, echo_max=1, onset_opt=True)(torch.zeros(2, 1, 300, device=dev))
    with pytest.raises(ValueError):      # rescale_factor < 6 -> sigma < 0, as in the reference
        GradPeak(threshold=1e-2, rescale_factor=1)(torch.zeros(2, 1, 300, device=dev))


@pytest.mark.parametrize('rf', [10, 20])
@pytest.mark.parametrize('thn,th', [('1em3', 1e-3), ('none', None)])
def test_gradpeak_1024_rows_exact_vs_reference(dev, rf, thn, th):
    """1024 seeded echoes through the reference's own toa_detect / GradPeak (tests/golden/make_golden_r2.py): every
    integer onset / peak index, the chirp-config output (echo_max = 1, onset) and the echo_max = 3 reduction must be
    identical; amplitudes within the envelope tolerance.  rf 10 -> L = 2000 takes the fused one-launch kernel when a
    threshold is given, rf 20 -> L = 4000 the envelope kernel + row-streaming kernel; th = None exercises the
    device-side default threshold (Q7)."""
    from stofnet_amd import GradPeak, toa_detect
    g = golden('f9_gradpeak_1024')
    L, seed = int(g[f'L_rf{rf}']), int(g[f'seed_rf{rf}'])
    x = torch.from_numpy(synth.synth_echo(1024, L, seed=seed, noise=0.01)).to(dev)
    got = toa_detect(x.squeeze(1), threshold=th, rescale_factor=rf).cpu().numpy()
    idx, amp = g[f'idx_rf{rf}_th{thn}'], g[f'amp_rf{rf}_th{thn}']
    assert got.shape == idx.shape[:2] + (3,)
    differs = (got[..., :2] != idx).any(axis=(1, 2))
    # Measured (tools/gradpeak_exactness.py -> profiles/r03_gradpeak_exactness.json): 0 of 1024 rows differ in each of the
    # four cases, and both the reference's fp32 and the kernels agree with the float64-exact pipeline on every row, so the
    # bar is the north star's: integer indices bit-exact (r2 allowed 2 borderline rows without recording how many there were).
    assert differs.sum() == 0, f'{differs.sum()} of 1024 rows differ from the reference: rows {np.nonzero(differs)[0][:8]}'
    same = ~differs
    assert np.abs(got[same, :, 2] - amp[same]).max() < ENV_TOL
    chirp = GradPeak(threshold=th, rescale_factor=rf, echo_max=1, onset_opt=True)(x).cpu().numpy()
    assert np.array_equal(chirp[same], g[f'chirp_rf{rf}_th{thn}'][same])
    em3 = GradPeak(threshold=th, rescale_factor=rf, echo_max=3, onset_opt=False)(x).cpu().numpy()
    assert np.array_equal(em3[same], g[f'em3_rf{rf}_th{thn}'][same])


@pytest.mark.parametrize('rf', [10, 20])
def test_gradpeak_default_threshold_paths_agree(dev, rf):
    """The default threshold (Q7) three ways through the C ABI: (a) toa_detect's own path (rf 10: stof_toa_moments from
    the waveforms + stof_grad_peak_detect; rf 20: envelope kernel + stof_gradpeak_moments + detect), (b) moments of the
    envelope rows (stof_gradpeak_moments), (c) the pre-pass that keeps the smoothed gradient and the detection that only
    thresholds and pairs it (stof_gradpeak_moments_store + stof_grad_peak_detect_blurred).  Same threshold bits, same
    echoes, and the reference's indices on the 1024-row golden."""
    import stofnet_amd.gradpeak as gp
    from stofnet_amd import _lib, toa_detect
    from stofnet_amd.hilbert import hilbert_envelope
    lib = _lib.lib()
    g = golden('f9_gradpeak_1024')
    L, seed = int(g[f'L_rf{rf}']), int(g[f'seed_rf{rf}'])
    x = torch.from_numpy(synth.synth_echo(1024, L, seed=seed, noise=0.01)).to(dev).squeeze(1)
    a = toa_detect(x, threshold=None, rescale_factor=rf).cpu().numpy()
    idx = g[f'idx_rf{rf}_thnone']
    differs = (a[..., :2] != idx).any(axis=(1, 2))
    assert differs.sum() == 0, f'rows {np.nonzero(differs)[0][:8]} differ from the reference'
    e3 = gp.GradPeak(threshold=None, rescale_factor=rf, echo_max=3, onset_opt=False)(x.unsqueeze(1)).cpu().numpy()
    assert np.array_equal(e3, g[f'em3_rf{rf}_thnone'])

    n, gs, st = x.shape[0], rf // 6 * 5, _lib.stream_ptr(dev)
    taps = gp.gaussian_kernel_1d((gs * 2 - 1) / 6).to(dev).float()
    rad = (taps.numel() - 1) // 2
    env = hilbert_envelope(x)

    def threshold_of(stats):
        th = torch.empty(1, device=dev)
        _lib.check(lib.stof_gradpeak_threshold(_lib.ptr(stats), _lib.ptr(th), st), 'threshold')
        return th

    stats_b = torch.tensor([0.0, 0.0, float(n * L)], dtype=torch.float64, device=dev)
    _lib.check(lib.stof_gradpeak_moments(_lib.ptr(env), n, L, gs, _lib.ptr(taps), rad, _lib.ptr(stats_b), st), 'moments')
    stats_c = torch.tensor([0.0, 0.0, float(n * L)], dtype=torch.float64, device=dev)
    blurred = torch.empty((n, lib.stof_gradpeak_blurred_stride(L, rad)), device=dev)
    _lib.check(lib.stof_gradpeak_moments_store(_lib.ptr(env), n, L, gs, _lib.ptr(taps), rad, _lib.ptr(stats_c), _lib.ptr(blurred), st), 'store')
    th_b, th_c = threshold_of(stats_b), threshold_of(stats_c)
    assert torch.allclose(stats_b, stats_c, rtol=1e-12, atol=0) and th_b.item() == th_c.item()
    if lib.stof_toa_detect_fused_ok(L, rad):
        stats_a = torch.tensor([0.0, 0.0, float(n * L)], dtype=torch.float64, device=dev)
        env_a = torch.empty_like(x)
        partials = torch.empty(64 * 16, dtype=torch.float64, device=dev)
        _lib.check(lib.stof_toa_moments(_lib.ptr(x), n, L, gs, _lib.ptr(taps), rad, _lib.ptr(env_a), _lib.ptr(partials),
                                        _lib.ptr(stats_a), st), 'toa_moments')
        # the fused kernel's envelope comes from a different FFT plan than stof_hilbert's: values within ENV_TOL, moments
        # to ~1e-6, and the threshold -- a 16th power -- to ~1e-4 relative
        assert (env_a - env).abs().max().item() < ENV_TOL
        assert torch.allclose(stats_a, stats_b, rtol=1e-5, atol=0)
        assert threshold_of(stats_a).item() == pytest.approx(th_b.item(), rel=1e-3)      # (0 on this data: std**16 underflows)
    cap = a.shape[1] + 4
    outs = []
    for use_blurred in (False, True):
        e = torch.zeros(n, cap, 3, device=dev)
        c = torch.zeros(n, dtype=torch.int32, device=dev)
        f = torch.zeros(2, dtype=torch.int32, device=dev)
        if use_blurred:
            code = lib.stof_grad_peak_detect_blurred(_lib.ptr(env), _lib.ptr(blurred), n, L, rad, 0.0, _lib.ptr(th_c), rf, 50 * rf, 0,
                                                     _lib.ptr(e), cap, None, _lib.ptr(c), _lib.ptr(f), st)
        else:
            code = lib.stof_grad_peak_detect(_lib.ptr(env), n, L, gs, _lib.ptr(taps), rad, 0.0, _lib.ptr(th_b), rf, 50 * rf, 0,
                                             _lib.ptr(e), cap, None, _lib.ptr(c), _lib.ptr(f), st)
        _lib.check(code, 'detect')
        outs.append((e.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy()))
    for u, v in zip(outs[0], outs[1]):
        assert np.array_equal(u, v)
    kmax = int(outs[0][2][1])
    assert kmax == a.shape[1] and np.array_equal(outs[0][0][:, :kmax, :2], idx)


@pytest.mark.parametrize('W', [1, 2, 4])
def test_gradpeak_split_kernel_matches_row_kernel(dev, W, monkeypatch):
    """gradpeak_split_kernel (rows split over W waves, envelope staged through LDS, stored flag words paired afterwards)
    against gradpeak_rows_kernel (one wave per row, pairing on the fly) through the C ABI: identical echoes, counts and
    moments for explicit, zero and device-side thresholds, short rows (fewer words than waves) included.  The library
    reads STOF_GP_SPLIT on every call: 0 = row kernel, 2 / 3 / 4 = split kernel with 1 / 2 / 4 waves per row."""
    from stofnet_amd import _lib
    from stofnet_amd.gradpeak import gaussian_kernel_1d
    from stofnet_amd.hilbert import hilbert_envelope
    lib = _lib.lib()

    def run(rows, L, rf, th):
        x = torch.from_numpy(synth.synth_echo(rows, L, seed=rows + L, noise=0.01)).to(dev)[:, 0].contiguous()
        env = hilbert_envelope(x)
        gs = rf // 6 * 5
        taps = gaussian_kernel_1d((gs * 2 - 1) / 6).to(dev).float()
        rad = (taps.numel() - 1) // 2
        stats = torch.tensor([0.0, 0.0, float(rows * L)], dtype=torch.float64, device=dev)
        _lib.check(lib.stof_gradpeak_moments(_lib.ptr(env), rows, L, gs, _lib.ptr(taps), rad, _lib.ptr(stats), _lib.stream_ptr(dev)), 'moments')
        cap = 128
        e = torch.zeros(rows, cap, 3, device=dev)
        c = torch.zeros(rows, dtype=torch.int32, device=dev)
        f = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(lib.stof_grad_peak_detect(_lib.ptr(env), rows, L, gs, _lib.ptr(taps), rad, th, None, rf, 50 * rf, 0, _lib.ptr(e), cap,
                                             None, _lib.ptr(c), _lib.ptr(f), _lib.stream_ptr(dev)), 'detect')
        torch.cuda.synchronize()
        return stats.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy(), e.cpu().numpy()

    for case in ((6, 2000, 10, 1e-3), (6, 2000, 10, 0.0), (5, 4000, 20, 1e-3), (3, 9000, 20, 1e-4), (2, 300, 10, 1e-3), (7, 64, 10, 1e-3)):
        monkeypatch.setenv('STOF_GP_SPLIT', '0')
        s0, c0, f0, e0 = run(*case)
        monkeypatch.setenv('STOF_GP_SPLIT', {1: '2', 2: '3', 4: '4'}[W])
        s1, c1, f1, e1 = run(*case)
        assert np.array_equal(c0, c1) and np.array_equal(f0, f1) and np.array_equal(e0, e1), case
        assert np.allclose(s0, s1, rtol=1e-12, atol=0), case          # double sums in a different order
        assert c0.sum() > 0 or case[1] < 400


@pytest.mark.parametrize('L', [30720, 40000])
def test_long_rows_hilbert_and_gradpeak_vs_reference(dev, L):
    """Rows beyond LDS (the reference's PALA GradPeak run uses rf_scale_factor 20 on ~30,720-sample frames,
    bash_scripts/pala_benchmark.sh:34): envelope within 1e-5 of the reference's, onset / peak indices identical."""
    from stofnet_amd import toa_detect
    from stofnet_amd.hilbert import hilbert_envelope
    g = golden('f9_long_rows')
    rows, seed = int(g[f'rows_L{L}']), int(g[f'seed_L{L}'])
    x = torch.from_numpy(synth.synth_echo(rows, L, seed=seed, noise=0.0005, attack=300, tau=3000.0, carrier=0.001)).to(dev)
    env = hilbert_envelope(x.squeeze(1)).cpu().numpy()
    assert np.abs(env[:, ::7] - g[f'env_L{L}']).max() < ENV_TOL
    assert np.abs(env - po.hilbert_envelope(x.squeeze(1).cpu().numpy())).max() < ENV_TOL      # every sample, fp64 truth
    for thn, th in (('1em4', 1e-4), ('5em5', 5e-5)):
        got = toa_detect(x.squeeze(1), threshold=th, rescale_factor=20).cpu().numpy()
        idx, amp = g[f'idx_L{L}_th{thn}'], g[f'amp_L{L}_th{thn}']
        assert got.shape == idx.shape[:2] + (3,) and np.array_equal(got[..., :2], idx)
        assert np.abs(got[..., 2] - amp).max() < ENV_TOL


@pytest.mark.parametrize('n', [20482, 24000, 32768, 30011, 45000])
def test_hilbert_beyond_lds_vs_oracle(dev, n):
    """Any length works beyond LDS too: even 5-smooth, powers of two, a prime (30011), odd."""
    from stofnet_amd.hilbert import hilbert_envelope
    x = synth.synth_randn(3, n, seed=n)
    env = hilbert_envelope(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert np.abs(env - po.hilbert_envelope(x)).max() < ENV_TOL


@pytest.mark.parametrize('n', [23040, 30000, 65536, 81920])
def test_hilbert_four_step_factorisations(dev, n):
    """Rows beyond LDS as n = R0 * M: every outer radix and inner compile-time length the planner can pick beyond the
    lengths of the other tests (23040 = 15 * 1536, 30000 = 15 * 2000, 65536 = 16 * 4096, 81920 = 20 * 4096), odd batch."""
    from stofnet_amd import hilbert_transform
    x = synth.synth_randn(3, n, seed=n)[:, 0]
    v = hilbert_transform(torch.from_numpy(x).to(dev)).cpu().numpy()
    want = po.hilbert_transform(x)
    assert np.abs(v.real - want.real).max() < ENV_TOL and np.abs(v.imag - want.imag).max() < ENV_TOL


def test_hilbert_four_step_several_chunks(dev):
    """The four-step scratch is sized for a chunk of pairs (64 MB); 601 rows of 30,720 samples = 301 pairs = two chunks,
    the second one short and ending in a lone row."""
    from stofnet_amd.hilbert import hilbert_envelope
    rows, n = 601, 30720
    x = synth.synth_randn(rows, n, seed=9)[:, 0]
    env = hilbert_envelope(torch.from_numpy(x).to(dev)).cpu().numpy()
    pick = np.r_[0:4, 270:280, 544:550, 596:601]                 # rows around the chunk boundary (pairs 272 | 273) and the tail
    assert np.abs(env[pick] - po.hilbert_envelope(x[pick])).max() < ENV_TOL
    assert np.isfinite(env).all() and np.abs(env).max() < 10


def test_gradpeak_many_rows_margin_gated_exactness(dev):
    """4096 rows against the float64 oracle.  A threshold crossing is decided by one comparison of a float that the
    two implementations round differently, so exactness is asserted for every row whose smoothed gradient stays
    clear of both thresholds by 2e-6 of its peak value at every sample; the rest (reported) may move by a sample."""
    from stofnet_amd import toa_detect
    n, L, rf, th = 4096, 2000, 10, 1e-3
    x = synth.synth_echo(n, L, seed=77, noise=0.01)
    got = toa_detect(torch.from_numpy(x[:, 0]).to(dev), threshold=th, rescale_factor=rf).cpu().numpy()
    env = po.hilbert_envelope(x[:, 0])
    sm = po.smoothed_gradient(env, rf // 6 * 5)
    exp = po.toa_detect(x[:, 0], th, rf, env=env)
    eps = 2e-6 * np.abs(sm).max()
    clear = (np.minimum(np.abs(sm - th), np.abs(sm + th / 4)) > eps).all(axis=1)
    assert clear.mean() > 0.85, f'only {clear.mean():.3f} of the rows are clear of the thresholds'
    k = max(got.shape[1], exp.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, k - a.shape[1]), (0, 0)))
    same = (pad(got)[..., :2] == pad(exp)[..., :2]).all(axis=(1, 2))
    assert same[clear].all(), f'{(~same[clear]).sum()} clear rows differ'
    print(f'borderline rows: {(~clear).sum()} of {n}, of which {(~same[~clear]).sum()} differ from the float64 oracle')
    # r4: what the borderline rows must equal is settled by the REFERENCE's own fp32 result on this very batch
    # (tests/golden/f9_gradpeak_4096, make_golden_r4.py), which agrees with the float64 oracle on all 4096 rows
    ref = golden('f9_gradpeak_4096')['rf10_th1e-3']
    assert got.shape == ref.shape
    moved = (got[..., :2] != ref[..., :2]).any(axis=(1, 2))
    # measured r4 (profiles/r04_gradpeak_4096_paths.jsonl): ONE row (2184, a smoothed-gradient sample 1.7e-7 of the peak gradient
    # from the threshold) -- with either launch sequence; the reference's fp32 happens to fall on the float64 side there.  A row
    # may move only if it is borderline, and at most one does.
    assert moved.sum() <= 1 and not (moved & clear).any(), f'{moved.sum()} rows differ from the reference, {(moved & clear).sum()} of them clear of the thresholds'


@pytest.mark.parametrize('rf', [10, 20])
@pytest.mark.parametrize('tag,th', [('th1e-3', 1e-3), ('thdef', None)])
def test_gradpeak_4096_rows_match_reference_golden(dev, rf, tag, th):
    """models/gradpeak.py:99-116 on the C2 batch size: the reference's toa_detect on 4096 rows (explicit threshold and the
    batch-wide default one, Q7; rescale_factor 10 and 20) -- onset and peak indices identical on every row, amplitudes as the
    envelope tolerance."""
    from stofnet_amd import toa_detect
    g = golden('f9_gradpeak_4096')
    x = synth.synth_echo(int(g['rows']), int(g['L']), seed=int(g['seed']), noise=float(g['noise']))
    got = toa_detect(torch.from_numpy(x[:, 0]).to(dev), threshold=th, rescale_factor=rf).cpu().numpy()
    ref = g[f'rf{rf}_{tag}']
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = (got[..., :2] != ref[..., :2]).any(axis=(1, 2))
    # Identical on every row in two of the four cases, on all but ONE row in the other two (rf 10 / th 1e-3: row 2184; rf 20 /
    # default threshold: row 1730), measured with both launch sequences (profiles/r04_gradpeak_4096_paths.jsonl).  Such a row must
    # be borderline: in the float64-exact pipeline one of its smoothed-gradient samples lies within 2e-6 of the peak gradient of
    # a threshold, where one rounding of an fp32 transform decides the comparison (the reference's fp32 and float64 agree on all
    # 4096 rows of all four cases: tests/test_oracle_golden.py).
    assert diff.sum() <= 1, f'{diff.sum()} of {len(diff)} rows differ from the reference: {np.nonzero(diff)[0][:8]}'
    if diff.any():
        xs = x[:, 0]
        env = po.hilbert_envelope(xs)
        sm = po.smoothed_gradient(env, rf // 6 * 5)
        thv = th if th is not None else float(po.default_threshold(sm))
        row = int(np.nonzero(diff)[0][0])
        margin = np.minimum(np.abs(sm[row] - thv), np.abs(sm[row] + thv / 4)).min()
        assert margin < 2e-6 * np.abs(sm).max(), f'row {row} is clear of the thresholds (margin {margin:.3e}) and still differs'
    same_rows = ~diff
    assert np.abs(got[same_rows][..., 2] - ref[same_rows][..., 2]).max() < ENV_TOL


def test_gradpeak_odd_batch_and_single_row(dev):
    """The fused kernel pairs rows: an odd batch leaves one row alone, and every row must equal its batch-of-one result."""
    from stofnet_amd import toa_detect
    x = torch.from_numpy(synth.synth_echo(7, 2000, seed=5, noise=0.01)).to(dev)[:, 0]
    full = toa_detect(x, threshold=1e-3, rescale_factor=10)
    for i in range(7):
        one = toa_detect(x[i:i + 1], threshold=1e-3, rescale_factor=10)
        k = one.shape[1]
        assert torch.equal(full[i, :k, :2], one[0, :, :2]) and not full[i, k:].any()      # indices exact
        assert (full[i, :k, 2] - one[0, :, 2]).abs().max() < ENV_TOL       # a lone row rides its own transform: other rounding


# ---------------------------------------------------------------- baselines riding on the shuffle
@pytest.mark.parametrize('tag', ['edsr_r4', 'edsr_r2', 'espcn_r4', 'espcn_r10'])
def test_shuffle_riders_match_reference(dev, tag):
    """EDSR_1D / ESPCN_1D with the reference's own parameters and input (tests/golden/make_golden_r2b.py): stock ATen
    convolutions + the gfx950 SampleShuffle1D kernel reproduce the reference's output."""
    from stofnet_amd import EDSR_1D, ESPCN_1D
    g = golden('f11_shuffle_riders')
    model = {'edsr_r4': lambda: EDSR_1D(1, 16, 2, 4), 'edsr_r2': lambda: EDSR_1D(1, 8, 1, 2),
             'espcn_r4': lambda: ESPCN_1D(4), 'espcn_r10': lambda: ESPCN_1D(10)}[tag]()
    model.load_state_dict({k.split('__p__')[1]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + '__p__')}, strict=True)
    model = model.to(dev).eval()
    with torch.no_grad():
        y = model(torch.from_numpy(g[f'{tag}__x']).to(dev)).cpu().numpy()
    want = g[f'{tag}__y']
    assert y.shape == want.shape
    assert np.abs(y - want).max() < 1e-5 * max(1.0, np.abs(want).max())


def test_sample_shuffle_backward_is_the_inverse_permutation(dev):
    """Training the riders needs d(shuffle): compare autograd through the kernel module with autograd through the
    reference's view / permute formulation (utils/sample_shuffle.py:24-27)."""
    from stofnet_amd import SampleShuffle1D
    torch.manual_seed(3)
    n, r, c, w = 3, 4, 5, 37
    x = torch.randn(n, r * c, w, device=dev, requires_grad=True)
    wgt = torch.randn(n, c, w * r, device=dev)
    y = SampleShuffle1D(r)(x)
    (y * wgt).sum().backward()
    x2 = x.detach().clone().requires_grad_(True)
    y2 = x2.view(n, r, c, w).permute(0, 2, 3, 1).contiguous().view(n, c, w * r)
    (y2 * wgt).sum().backward()
    assert torch.equal(y, y2) and torch.equal(x.grad, x2.grad)


# ---------------------------------------------------------------- neighbours of the path
def test_toa_rmse_device(dev):
    from stofnet_amd.metrics import toa_rmse
    g = golden('f7_metrics')
    for tol in [1, 4]:
        got = toa_rmse(torch.from_numpy(g['gt']).to(dev), torch.from_numpy(g['es']).to(dev), tol=tol).cpu().numpy()
        assert np.allclose(got, g[f'rmse_tol{tol}'], rtol=1e-6, atol=0, equal_nan=True)
    rng = np.random.default_rng(3)
    gt = np.where(rng.random((500, 6)) < 0.3, 0, rng.uniform(1, 2000, (500, 6))).astype(np.float32)
    es = np.where(rng.random((500, 9)) < 0.3, 0, gt[:, :1] + rng.normal(0, 1.5, (500, 9))).astype(np.float32)
    es[7, 2] = np.nan
    es[8, 1] = np.inf
    got = toa_rmse(torch.from_numpy(gt).to(dev), torch.from_numpy(es).to(dev), tol=1).cpu().numpy()
    exp = po.toa_rmse(gt, es, 1)
    assert np.allclose(got, exp, rtol=1e-5, atol=0, equal_nan=True)


@pytest.mark.parametrize('rf', [10, 20, 1, 2.5])
def test_iq2rf_matches_numpy_scipy_chain(dev, rf):
    """datasets/chirp_dataset.py:80-91 + NormalizeVol, float64 oracle (same numpy/scipy calls)."""
    from stofnet_amd.chirp import iq2rf
    rng = np.random.default_rng(int(rf * 10))
    n, ln = 7, 200
    fs, fc = 2.0e7, 5.2e6
    env = np.exp(-((np.arange(ln)[None, :] - rng.uniform(40, 160, (n, 1))) / 12.0) ** 2)
    iq = (env * np.exp(1j * rng.uniform(0, 6.28, (n, 1))) + 0.02 * (rng.standard_normal((n, ln)) + 1j * rng.standard_normal((n, ln))))
    got = iq2rf(torch.from_numpy(iq.astype(np.complex64)).to(dev), fc, fs, rf).cpu().numpy()
    exp = po.iq2rf(iq.astype(np.complex64), fc, fs, rf)
    assert got.shape == exp.shape == (n, int(ln * rf))
    assert np.abs(got - exp).max() < 1e-5           # max-abs normalised output, fp32 vs float64
    raw = iq2rf(torch.from_numpy(iq.astype(np.complex64)).to(dev), fc, fs, rf, normalize=False).cpu().numpy()
    assert np.abs(raw - po.iq2rf(iq.astype(np.complex64), fc, fs, rf, normalize=False)).max() < 1e-5 * np.abs(raw).max() + 1e-6


def test_iq2rf_matches_reference_golden(dev):
    """ChirpDataset.iq2rf of the reference itself (compiled from its AST node, make_golden_r2.py iq2rf)."""
    from stofnet_amd.chirp import iq2rf
    g = golden('f10_iq2rf')
    iq = torch.from_numpy(g['iq']).to(dev)
    for rf in (1, 2.5, 10, 20):
        exp = g[f'rf_{rf}']
        got = iq2rf(iq, float(g['fc']), float(g['fs']), rf, normalize=False).cpu().numpy()
        assert got.shape == exp.shape
        assert np.abs(got - exp).max() < 1e-5 * np.abs(exp).max() + 1e-6


def test_f16x3_range_guard(dev):
    m = make_model(dev, synth.synth_state_dict(4, seed=12), 4, precision='f16x3')
    x = torch.from_numpy(synth.synth_randn(8, 400, seed=5)).to(dev)
    m(x)
    m.raise_if_overflow()                                   # normalised input: fine
    m(x * 3.0e6)                                            # raw, un-normalised amplitudes: beyond fp16
    with pytest.raises(FloatingPointError):
        m.raise_if_overflow()
    m32 = make_model(dev, synth.synth_state_dict(4, seed=12), 4, precision='fp32')
    assert torch.isfinite(m32(x * 3.0e6)).all()             # the exact mode handles the same input


def test_auto_precision_is_f16x3_with_device_side_fp32_rerun(dev):
    """The module default: bits of the f16x3 mode on in-range inputs; on a range overflow the same call ends with the
    exact-fp32 result (kernels gated on the device by the guard word, no host sync in forward)."""
    from stofnet_amd import StofNet
    assert StofNet().precision == 'auto'
    sd = synth.synth_state_dict(4, seed=12)
    x = torch.from_numpy(synth.synth_randn(300, 400, seed=5)).to(dev)
    ma, m16, m32 = (make_model(dev, sd, 4, precision=p) for p in ('auto', 'f16x3', 'fp32'))
    assert torch.equal(ma(x), m16(x)) and not ma.fell_back_to_fp32()
    big = x * 3.0e6                                          # raw, un-normalised amplitudes: beyond fp16
    ya = ma(big)
    assert ma.fell_back_to_fp32()
    assert torch.isfinite(ya).all() and torch.equal(ya, m32(big))
    assert torch.equal(ma(x), m16(x)) and not ma.fell_back_to_fp32()      # the guard word is re-armed by every call
    # no-SGB variant and N > 4096 (two sub-batches, overflow only in the second one)
    sd1 = synth.synth_state_dict(4, seed=3, semi_global_scale=1)
    mb, mb32 = make_model(dev, sd1, 4, 1, 'auto'), make_model(dev, sd1, 4, 1, 'fp32')
    xl = torch.from_numpy(synth.synth_randn(4100, 160, seed=9)).to(dev)
    xl[4098] *= 3.0e6
    yb = mb(xl)
    assert mb.fell_back_to_fp32() and torch.equal(yb, mb32(xl))


def test_main_entry_point_end_to_end(dev, tmp_path):
    """`python main.py key=value ...` (reference README.md:25 style): config merge, checkpoint lookup by
    prefix with strict load, forward, mask2coords, device toa_rmse -- against the oracle chain."""
    import main as entry
    sd = load_weights('different-armadillo')
    ck = tmp_path / 'ckpts'
    ck.mkdir()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, ck / 'different-armadillo-1439_rf-scale10_epoch_46.pth')
    es, summary = entry.main(['model=stofnet', 'model_file=different-armadillo_x', 'th=Null', 'evaluate=True',
                              'batch_size=4', 'num_waveforms=10', 'num_samples=2000', f'ckpt_dir={ck}', 'seed=5'])
    assert summary['waveforms'] == 8                                      # drop_last=True
    x = synth.synth_echo(10, 2000, seed=5)[:8]
    ref = po.mask2coords(so.stofnet_forward(sd, x, 4, 80).numpy(), 20, None, 4)
    assert np.array_equal(es, ref)
    es2, s2 = entry.main(['model=gradpeak', 'th=1e-3', 'rf_scale_factor=10', 'batch_size=2', 'num_waveforms=4',
                          'num_samples=2000', 'seed=5'])
    assert es2.shape[0] == 4 and s2['model'] == 'gradpeak'


# ---------------------------------------------------------------- arg-max picker fused into the sweep
@pytest.mark.parametrize('precision', ['auto', 'f16x3'])
def test_forward_onsets_matches_forward_plus_picker_on_golden(dev, precision):
    """stof_forward_onsets == stof_forward + stof_pick_maxima, bit for bit, and equals the reference's indices."""
    from stofnet_amd.mask2samples import onset_indices
    g = golden('f1_armadillo_r4_argmax1024')
    m = make_model(dev, load_weights('different-armadillo'), 4, precision=precision)
    x = torch.from_numpy(synth.synth_echo(1024, 2000, seed=int(g['seed']))).to(dev)
    counts, idx, y = m.forward_onsets(x, 20, return_map=True)
    c2, i2 = onset_indices(m(x), 20, None)
    assert torch.equal(y, m(x))
    assert torch.equal(counts, c2) and torch.equal(idx, i2)
    assert np.array_equal(idx[:, 0].cpu().numpy(), g['indices'][:, 1])
    c3, i3 = m.forward_onsets(x, 20)                       # picker-only: the map is never written
    assert torch.equal(c3, counts) and torch.equal(i3, idx)


@pytest.mark.parametrize('r,L,n', [(4, 2000, 300), (10, 2000, 64), (16, 1536, 33), (1, 400, 5), (4, 96, 7), (10, 2000, 3), (4, 1536, 4100),
                                   (2, 400, 5), (3, 2000, 64), (5, 1536, 33), (13, 400, 7), (15, 2000, 3)])
def test_forward_onsets_shapes_batches_segments(dev, r, L, n):
    """Row lengths that are no multiple of the 16-row tiles, waveform boundaries inside tiles, small batches (segment
    mode), several sub-batches, r that is no multiple of 4: always the same indices as the map + picker kernel."""
    from stofnet_amd.mask2samples import onset_indices
    m = make_model(dev, synth.synth_state_dict(r, seed=r + L), r, precision='auto')
    x = torch.from_numpy(synth.synth_echo(n, L, seed=n)).to(dev)
    counts, idx = m.forward_onsets(x, 20)
    c2, i2 = onset_indices(m(x), 20, None)
    assert torch.equal(counts, c2) and torch.equal(idx, i2)
    ref = po.maxima_positions(so.stofnet_forward(synth.synth_state_dict(r, seed=r + L), x[:3].cpu().numpy(), r, 80).numpy(), 20, None)
    got = [(row, int(t)) for row in range(min(3, n)) for t in idx[row, :int(counts[row])].cpu().numpy()]
    assert got == [tuple(v) for v in ref.tolist()]


def test_forward_onsets_ties_and_degenerate_rows(dev):
    """Q5 through the fused path: weights that make the network output piecewise constant give plateaus (every tied
    position is a detection), an all-zero map (no detection), and a constant negative map (every position)."""
    from stofnet_amd.mask2samples import onset_indices
    r, L = 4, 320
    sd = synth.synth_state_dict(r, seed=2)
    for k in sd:
        if k.startswith('conv_last'):
            sd[k] = np.zeros_like(sd[k])
    x = torch.from_numpy(synth.synth_echo(6, L, seed=1)).to(dev)
    for bias, expect_count in ((np.zeros(r, np.float32), 0), (np.full(r, -0.5, np.float32), L * r),
                               (np.array([0.25, 0.25, -1, 0.25], np.float32), 3 * L)):
        sd['conv_last.bias'] = bias
        m = make_model(dev, sd, r, precision='auto')
        counts, idx = m.forward_onsets(x, 20)
        c2, i2 = onset_indices(m(x), 20, None)
        assert torch.equal(counts, c2) and torch.equal(idx, i2)
        assert int(counts[0]) == expect_count
    # a plateau inside one tile: pin conv_last to copy one channel so neighbouring outputs tie exactly
    sd = synth.synth_state_dict(r, seed=3)
    sd['conv_last.weight'][1:] = sd['conv_last.weight'][:1]
    sd['conv_last.bias'][1:] = sd['conv_last.bias'][:1]
    m = make_model(dev, sd, r, precision='auto')
    counts, idx = m.forward_onsets(x, 20)
    c2, i2 = onset_indices(m(x), 20, None)
    assert torch.equal(counts, c2) and torch.equal(idx, i2) and int(counts.min()) >= r


def test_forward_onsets_falls_back_outside_the_fused_tile(dev):
    from stofnet_amd.mask2samples import onset_indices
    x = torch.from_numpy(synth.synth_echo(5, 400, seed=4)).to(dev)
    for r, precision in ((20, 'auto'), (4, 'fp32'), (17, 'auto'), (64, 'auto')):
        m = make_model(dev, synth.synth_state_dict(r, seed=9), r, precision=precision)
        counts, idx = m.forward_onsets(x, 20)
        c2, i2 = onset_indices(m(x), 20, None)
        assert torch.equal(counts, c2) and torch.equal(idx, i2)
        if r in (17, 64):
            ref = po.maxima_positions(so.stofnet_forward(synth.synth_state_dict(r, seed=9), x[:2].cpu().numpy(), r, 80).numpy(), 20, None)
            got = [(row, int(t)) for row in range(2) for t in idx[row, :int(counts[row])].cpu().numpy()]
            assert got == [tuple(v) for v in ref.tolist()]
    m = make_model(dev, synth.synth_state_dict(4, seed=12), 4, precision='auto')
    big = x * 3.0e6                                          # fp16 range overflow: exact-fp32 map path
    counts, idx = m.forward_onsets(big, 20)
    m32 = make_model(dev, synth.synth_state_dict(4, seed=12), 4, precision='fp32')
    c2, i2 = onset_indices(m32(big), 20, None)
    assert torch.equal(counts, c2) and torch.equal(idx, i2)


def test_main_logging_switch_without_wandb(dev):
    """`logging=<group>` (main.py:113-130): with wandb absent the same metric and summary keys go to a JSON-lines file."""
    import main as entry
    path = os.path.join(os.path.dirname(entry.__file__), 'lgtest_unit.jsonl')
    try:
        entry.main(['model=stofnet', 'th=Null', 'evaluate=True', 'batch_size=4', 'num_waveforms=8', 'num_samples=400',
                    'seed=5', 'logging=unit', 'run_name=lgtest'])
        recs = [json.loads(ln) for ln in open(path)]
        summ = [r['summary'] for r in recs if 'summary' in r][0]
        assert set(entry.RunLog.SUMMARY_KEYS) <= set(summ) and summ['total_parameters'] == 645764 and summ['model_name'] == 'stofnet'
        assert any('val_toa_jaccard' in r for r in recs) and any('inference_time' in r for r in recs)
    finally:
        if os.path.exists(path):
            os.remove(path)
    entry.main(['model=stofnet', 'th=Null', 'evaluate=True', 'batch_size=4', 'num_waveforms=4', 'num_samples=400'])   # logging: False
    assert not os.path.exists(path)


# ---------------------------------------------------------------- round 3: API widening (VERDICT r2 missing 2-4)
def _sgb_input(n, L, seed):
    return np.random.default_rng(seed).standard_normal((n, 64, L)).astype(np.float32)


@pytest.mark.parametrize('L', [2000, 1536, 160])
def test_semi_global_block_forward_standalone(dev, L):
    """SemiGlobalBlock.forward called directly (models/stofnet.py:98-117), [N,64,L] -> [N,64,L], with the checkpoint's
    block: the reference's output (tests/golden/make_golden_r3.py sgb_standalone), and its errors."""
    g = golden('f13_sgb_standalone')
    m = make_model(dev, load_weights('different-armadillo'), 4)
    blk = m.semi_global_block
    y = blk(torch.from_numpy(_sgb_input(2, L, 1300 + L)).to(dev))
    assert tuple(y.shape) == (2, 64, L)
    want = g[f'y80_L{L}']
    assert np.abs(y.cpu().numpy()[..., ::5] - want).max() < MAP_TOL * np.abs(want).max()
    with pytest.raises(RuntimeError, match='must match the size of tensor b'):          # Q1, odd remainder
        blk(torch.from_numpy(_sgb_input(1, 2001, 1)).to(dev))
    with pytest.raises(RuntimeError):                                                      # fewer samples than one pooling window
        blk(torch.from_numpy(_sgb_input(1, 40, 1)).to(dev))


@pytest.mark.parametrize('precision', ['fp32', 'f16x3', 'auto'])
@pytest.mark.parametrize('scale', [40, 20])
def test_other_semi_global_scales(dev, scale, precision):
    """StofNet(semi_global_scale=40 / 20) (models/stofnet.py:11 accepts any scale; feat_scale = scale // 10): forward on
    the layer-by-layer MFMA kernels equals the reference's; the standalone block with that scale too."""
    g = golden('f13_sgb_standalone')
    sd = synth.synth_state_dict(4, seed=3000 + scale, semi_global_scale=scale)
    m = make_model(dev, sd, 4, sgs=scale, precision=precision)
    for L in (2000, 1536):
        y = m(torch.from_numpy(synth.synth_echo(2, L, seed=scale + L)).to(dev)).cpu().numpy()
        want = g[f'net{scale}_y_L{L}']
        assert y.shape == want.shape and rel_err(y, want) < MAP_TOL
        assert np.array_equal(y[:, 0].argmax(-1), want[:, 0].argmax(-1))
    yb = m.semi_global_block(torch.from_numpy(_sgb_input(2, 1000, 1300 + scale)).to(dev)).cpu().numpy()
    assert np.abs(yb[..., ::5] - g[f'y{scale}_L1000']).max() < MAP_TOL * np.abs(g[f'y{scale}_L1000']).max()
    from stofnet_amd.mask2samples import onset_indices
    x = torch.from_numpy(synth.synth_echo(3, 800, seed=3)).to(dev)
    c, i = m.forward_onsets(x, 20)
    c2, i2 = onset_indices(m(x), 20, None)
    assert torch.equal(c, c2) and torch.equal(i, i2)


@pytest.mark.parametrize('thn,th', [('1em5', 1e-5), ('1em4', 1e-4)])
def test_pala_gradpeak_configuration_end_to_end(dev, tmp_path, thn, th):
    """`python main.py model=gradpeak data_dir=<pala> rf_scale_factor=20 th=1e-5` (bash_scripts/array_pala_params.txt:7) on a
    PALA-shaped input file [B, C, S]: main.py:301 flattens the frames to [B*C, 1, S], GradPeak(echo_max=inf, onset_opt=False)
    returns the PEAK column -- identical to the reference (tests/golden/make_golden_r3.py pala_gradpeak)."""
    import main as entry
    from stofnet_amd import GradPeak
    g = golden('f12_pala_gradpeak')
    B, C, S, seed = (int(g[k]) for k in ('B', 'C', 'S', 'seed'))
    frames = synth.pala_frames(B, C, S, seed)
    path = tmp_path / 'pala_frames.npy'
    np.save(path, frames)
    es, summary = entry.main(['model=gradpeak', f'input_file={path}', 'data_dir=/data/PALA_data_InSilicoFlow', 'rf_scale_factor=20',
                              f'th={th}', 'batch_size=1'])
    want = g[f'peaks_th{thn}']
    assert summary['waveforms'] == B * C
    k = max(es.shape[1], want.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, k - a.shape[1])))
    assert np.array_equal(pad(es), pad(want))
    x = torch.from_numpy(frames.reshape(-1, 1, S)).to(dev)
    onsets = GradPeak(threshold=th, rescale_factor=20, echo_max=float('inf'), onset_opt=True)(x).cpu().numpy()
    assert np.array_equal(onsets, g[f'onsets_th{thn}'])
    # a [B, waves, C, S] file: main.py:301 takes wave index 1
    np.save(path, np.stack([np.zeros_like(frames), frames, 2 * frames], 1))
    es4, _ = entry.main(['model=gradpeak', f'input_file={path}', 'data_dir=/data/PALA_data_InSilicoFlow', 'rf_scale_factor=20',
                         f'th={th}', 'batch_size=2'])
    assert np.array_equal(pad(es4), pad(want))

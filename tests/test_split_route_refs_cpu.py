"""CPU pins of tests/split_route_inputs.py: the split-row codec (bit layout, exact round trip, error bound), the forward and
backward stage references chained against oracle/'s float64 forward and torch autograd at N = 2, L = 100, r = 4 with and
without the SemiGlobalBlock (and at L = 260: three pooling windows), the batched weight-gradient reference against autograd, the loss restatement against
oracle/train_oracle.py, and the geometry every case of tests/test_gpu_split_route.py is named after."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multi_tile_inputs as mt
import split_route_inputs as sr
from oracle import stofnet_oracle as so
from oracle import train_oracle as to
from oracle.pickers_oracle import gaussian_kernel
from stofnet_amd import synth

N, R = 2, 4


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# --------------------------------------------------------------------------------------------------------------- codec
def test_split_row_bit_layout():
    v = torch.arange(64, dtype=torch.float32)[None] * 0.37 + 0.001
    raw = sr.to_split(v).view(torch.uint8).reshape(256).numpy()
    hi = np.frombuffer(raw[:128].tobytes(), dtype=np.float16)
    lo = np.frombuffer(raw[128:].tobytes(), dtype=np.float16)
    for c in (0, 1, 17, 63):
        h = np.float16(v[0, c].item())
        assert raw[2 * c: 2 * c + 2].tobytes() == h.tobytes()                                 # hi of channel c at byte 2c
        assert raw[128 + 2 * c: 130 + 2 * c].tobytes() == np.float16(np.float32(v[0, c].item()) - np.float32(h)).tobytes()
    assert np.array_equal(hi, v[0].numpy().astype(np.float16)) and (lo != 0).any()
    assert sr.to_split(v).dtype == torch.float32 and sr.to_split(v).shape == v.shape
    h2, l2 = sr.split_halves(sr.to_split(v))
    assert np.array_equal(h2[0].numpy(), hi) and np.array_equal(l2[0].numpy(), lo)


def test_split_round_trip_is_exact_for_fp16_values():
    every = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.float16)
    every = every[torch.isfinite(every)].float().reshape(-1, 64)                               # 63,488 finite fp16 values
    rows = sr.to_split(every)
    assert torch.equal(sr.from_split(rows), every)                                           # (-0 comes back as hi + lo = +0)
    assert sr.same_bits(sr.from_split(rows)[every != 0], every[every != 0])
    assert not sr.split_halves(rows)[1].view(torch.int16).bitwise_and(0x7fff).any()          # lo = +-0
    d = mt.ints((50, 64), 3)
    assert torch.equal(sr.from_split(sr.to_split(d)), d)


def test_split_round_trip_error_bound():
    g = torch.Generator().manual_seed(1)
    mags = torch.exp(torch.empty(4000, 64).uniform_(float(np.log(2.0 ** -30)), float(np.log(65000.0)), generator=g))
    v = torch.cat([mags * torch.where(torch.rand(mags.shape, generator=g) < 0.5, -1.0, 1.0), sr.codec_edge_values(),
                   torch.randn(500, 64, generator=g)])
    assert float(v.abs().max()) < 65520 and float(v.abs()[v != 0].min()) < 2.0 ** -26
    back = sr.from_split(sr.to_split(v), torch.float64)
    assert torch.isfinite(back).all()
    err = (back - v.double()).abs()
    assert (err <= 2.0 ** -22 * v.double().abs() + 2.0 ** -25).all()
    assert float((err / v.double().abs().clamp(min=1.0)).max()) > 2.0 ** -24                 # the bound is not vacuous
    assert torch.equal(sr.from_split(sr.to_split(v)).double(), back)                         # hi + lo is an fp32 number
    # the documented mask rule: |y| < 2^-25 has hi = +-0
    tiny = torch.tensor([2.0 ** -26, -2.0 ** -26, 0.0, -0.0] * 16).reshape(1, 64)
    assert not sr.split_halves(sr.to_split(tiny))[0].view(torch.int16).bitwise_and(0x7fff).any()
    assert (sr.split_halves(sr.to_split(torch.full((1, 64), 2.0 ** -24)))[0] > 0).all()


# ------------------------------------------------------------------------------------------------------------ geometry
def test_cases_reach_what_they_are_named_after():
    two_s = 2 * sr.S_ROWS
    assert sr.geometry(380, 1) == (1, 380, two_s, True) and sr.geometry(379, 1)[3] is False    # floor: Lp = 384 exactly
    nseg, seg_len, rows, p2 = sr.geometry(778, 1)
    assert p2 and rows % 16 and rows % 96 and (778 - 9 * 80) == 58
    assert sr.geometry(612, 2) == (2, 306, 306 + 76 + 4, True) and 2 * 306 == 612
    assert sr.geometry(1218, 3) == (4, 305, 305 + 76 + 4, True) and 1218 - 3 * 305 == 303
    assert sr.geometry(336, 1)[3] is False                                                     # control: the r3 kernel
    # the `tw < Ltrue` term of span_ok: never the deciding one at 1218 (no span ends on rows 1218, 1219 inside its segment's own
    # rows), the deciding one at 1334 for a span of sweep layer 4 (forward and backward)
    assert sr.geometry(1334, 3) == (4, 334, 334 + 76 + 4, True) and 4 * 334 - 1334 == 2
    assert sr.spans_cut_by_waveform_end(1218, 3) == [] and sr.spans_cut_by_waveform_end(612, 2) == []
    assert sr.spans_cut_by_waveform_end(1334, 3) == [(4, 276)]
    for name in sr.CASES:
        n, length, policy = sr.case_shape(name, 256)
        assert (length - sr.SGB_SCALE * (length // sr.SGB_SCALE)) % 2 == 0                     # the SemiGlobalBlock takes it
        assert 12 * n * length * 64 * 4 < 0.35e9                                               # one dump
    assert sr.case_shape('pairs', 256) == (261, 380, 1) and -(-261 // 256) == 2 and -(-261 // 2) == 131 and 261 % 2 == 1
    assert sr.geometry(380, 1)[3] and sr.geometry(625, 1)[3]                                   # the end-to-end shapes' rows
    assert sr.TWO_PASS_CASES == ['floor', 'odd', 'pairs', 'seg2', 'seg4', 'seg4_cut']


# ---------------------------------------------------------------------------------------------------- stage references
def _autograd_network(p, x, e):
    """the forward of the stage references restated on autograd leaves: every dump tensor and every pre-activation retained"""
    conv = lambda i, v: F.conv1d(v.permute(0, 2, 1), p[f'conv{i}.weight'], p[f'conv{i}.bias'], padding=3).permute(0, 2, 1)   # noqa: E731
    t = [sr.x0_ref(p, x, e).requires_grad_()]
    pre = []
    for k in range(5):
        pre.append(conv(2 * k + 2, t[2 * k]))
        t.append(F.leaky_relu(pre[k], 0.01))
        t.append(conv(2 * k + 3, t[2 * k + 1]) + t[2 * k])
    t.append(conv(12, t[10]) + t[0])
    for v in t + pre:
        v.retain_grad()
    return t, pre


@pytest.mark.parametrize('scale,L', [(80, 100), (1, 100), (80, 260)])          # 260: three pooling windows, 10 rows of zero on each side
def test_stage_references_chain_to_the_oracle_and_autograd(scale, L):
    sd = synth.synth_state_dict(R, seed=7, semi_global_scale=scale)
    p = sr.params64(sd)
    x = torch.from_numpy(synth.synth_echo(N, L, seed=2)).double()
    taps = {}
    pred = so.stofnet_forward(sd, x, R, scale, torch.float64, taps=taps)
    cl = lambda v: v.permute(0, 2, 1)                                                       # noqa: E731
    e = cl(taps['sgb_expand']) if scale != 1 else None
    if e is not None:
        assert e.shape == (N, L // 80, 64)
        assert _close(sr.sgb_expand_ref(p, sr.x0_ref(p, x[:, 0], None)), e)
    ref, y = sr.forward_refs(p, x[:, 0], e, R)
    assert len(ref) == 12 and y.shape == (N, L * R)
    assert _close(ref[0], cl(taps['x0'])) and _close(ref[11], cl(taps['conv12'])) and _close(y, pred[:, 0])
    for k in range(1, 6):
        assert _close(ref[2 * k], cl(taps[f'res{2 * k + 1}']))
    assert _close(sr.network_forward(p, x[:, 0], R, scale), pred[:, 0])
    # stage by stage from GIVEN tensors: perturbing one input moves only the stages that read it
    given = [v.clone() for v in ref]
    given[4] = given[4] + 1.0
    ref2, _ = sr.forward_refs(p, x[:, 0], e, R, given)
    moved = [i for i in range(12) if not torch.equal(ref2[i], ref[i])]
    assert moved == [5, 6]

    # backward: masks and g6 from the float64 forward, against autograd's gradients of the same tensors
    t, pre = _autograd_network(p, x[:, 0], e)
    g6 = sr.gauss((N, L, 64), 5).double()
    (t[11] * g6).sum().backward()
    positive = [t[2 * k + 1].detach() > 0 for k in range(5)]
    assert all(m.any() and (~m).any() for m in positive)
    T = sr.backward_refs(p, g6, positive)
    assert sorted(T) == list(range(1, 12))
    assert _close(T[1], t[10].grad)
    for k in range(5):
        assert _close(T[10 - 2 * k], pre[k].grad), k
        if k > 0:
            assert _close(T[11 - 2 * k], t[2 * k].grad), k
    assert _close(T[11] + g6, t[0].grad)                                                     # the long skip joins outside the sweep
    # the weight-gradient reference on the engine's eleven (x, dy) pairs
    w = [p[f'conv{i}.weight'].clone().requires_grad_() for i in range(2, 13)]
    b = [p[f'conv{i}.bias'].clone().requires_grad_() for i in range(2, 13)]
    q = dict(p)
    q.update({f'conv{i}.weight': w[i - 2] for i in range(2, 13)})
    q.update({f'conv{i}.bias': b[i - 2] for i in range(2, 13)})
    t2, _ = _autograd_network(q, x[:, 0], e)
    gw = torch.autograd.grad((t2[11] * g6).sum(), w + b)
    fwd = [v.detach() for v in t]
    pairs = sr.wgrad_pairs(fwd, T, g6)
    assert [nm for _, _, nm in pairs] == ['conv12', 'conv11', 'conv10', 'conv9', 'conv8', 'conv7', 'conv6', 'conv5', 'conv4', 'conv3', 'conv2']
    for xin, dy, nm in pairs:
        i = int(nm[4:])
        dw, db = sr.wgrad_ref(xin, dy, 0.25)
        assert dw.shape == (64, 64, 7) and _close(dw, 0.25 * gw[i - 2]) and _close(db, 0.25 * gw[11 + i - 2]), nm


def test_loss_restatement_matches_the_oracle():
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(3, 400, generator=g, dtype=torch.float64)
    gt = torch.tensor([[5, 390], [0, 17], [398, 399]])
    taps = gaussian_kernel(7, 1)
    want = to.loss_fn(pred[:, None], gt[:, None])
    assert abs(float(sr.loss_ref(pred, gt, taps)) - float(want)) <= 1e-12 * abs(float(want))


def test_operand_helpers():
    s = sr.planted_signs((200, 64), 1)
    assert set(s.unique().tolist()) == {0, 1, 2, 3, 4}
    t = sr.plant(torch.ones(200, 64), s)
    assert (t[s == 0] == 1).all() and (t[s == 3] == 2.0 ** -26).all() and (t[s == 4] == -2.0 ** -26).all()
    assert torch.signbit(t[s == 2]).all() and not torch.signbit(t[s == 1]).any() and (t[(s == 1) | (s == 2)] == 0).all()
    assert sr.wgrad_batch_groups(11 * 46 * (7 * 64 * 64 + 64) * 4, 11) == 46
    ev = sr.codec_edge_values()
    assert ev.shape[1] == 64 and float(ev.abs().max()) == 65519.0 and torch.isfinite(sr.from_split(sr.to_split(ev))).all()

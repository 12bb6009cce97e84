"""The range-contract inputs (tests/range_contract_inputs.py), checked on the CPU against the oracle: every rescaling is the
same function in float64 and the same BITS in fp32, every declared case puts its overflow where it says, and the burst
positions and k of every case are pinned.  tests/test_gpu_range_contract.py runs the kernels on exactly these inputs."""
import numpy as np
import pytest
import torch

import range_contract_inputs as rc
from oracle import stofnet_oracle as so
from stofnet_amd import synth

ALL_CASES = rc.OVERFLOW_CASES + rc.SAFE_CASES + rc.TRAIN_OVERFLOW_CASES


def test_fused_base_network_is_the_synth_state_dict():
    for r in (4, 10):
        a, b = rc.base_state_dict('fused', r), synth.synth_state_dict(r, seed=12)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_stream_roles_of_the_shipped_network():
    up_wb, up_b, down_w = rc.stream_roles(13)
    assert up_wb == ['conv1', rc.SG + 'expand_conv'] + [f'conv{i}' for i in (3, 5, 7, 9, 11)]
    assert up_b == ['conv12']
    assert down_w == [rc.SG + 'contract_conv', 'conv_last'] + [f'conv{i}' for i in (2, 4, 6, 8, 10)]
    assert rc.stream_roles(5) == (['conv1', rc.SG + 'expand_conv', 'conv3'], ['conv4'], [rc.SG + 'contract_conv', 'conv_last', 'conv2'])


@pytest.mark.parametrize('geom', list(rc.GEOMETRIES))
def test_rescaled_networks_are_the_same_function_and_the_same_fp32_bits(geom):
    """float64: identical output.  fp32: bitwise identical, with ATen's convolution and with the shifted-matmul one -- so an
    exact-fp32 kernel route owes the same bits for the rescaled network as for the unscaled one.  Every k the GPU tests use,
    and the low-side sweep's and the overflow cases' as well."""
    sd, x = rc.base_state_dict(geom, 4), rc.exact_input()
    ref64 = rc.forward(sd, x, 4, geom)
    ref32 = [rc.forward(sd, x, 4, geom, torch.float32, conv) for conv in (so.conv1d_same, so.conv1d_shifted_matmul)]
    for spec in rc.EXACT_SPECS[geom]:
        for k in sorted(set(rc.EXACT_KS) | {-16, -4, 4, 11, 14, 17}):
            sk = rc.rescale(sd, spec, k)
            assert torch.equal(rc.forward(sk, x, 4, geom), ref64), f'{geom} {spec} k={k}: float64'
            for conv, ref in zip((so.conv1d_same, so.conv1d_shifted_matmul), ref32):
                assert torch.equal(rc.forward(sk, x, 4, geom, torch.float32, conv), ref), f'{geom} {spec} k={k}: fp32 {conv.__name__}'


@pytest.mark.parametrize('case', ALL_CASES, ids=lambda c: c.id)
def test_declared_case(case):
    """The stage conditions (overflow >= 2^17 on the one row and stage, <= 2^14 elsewhere; safe cases <= 2^14 everywhere and
    >= 2^-3 on the target), and on the case's own input: float64 output equal, fp32 output bitwise equal to the unscaled."""
    rc.check_case(case)
    base, scaled, x = case.base(), case.scaled(), case.x()
    assert torch.equal(rc.forward(scaled, x, case.r, case.geom), rc.forward(base, x, case.r, case.geom))
    if case.n <= 8:
        for conv in (so.conv1d_same, so.conv1d_shifted_matmul):
            assert torch.equal(rc.forward(scaled, x, case.r, case.geom, torch.float32, conv),
                               rc.forward(base, x, case.r, case.geom, torch.float32, conv))


def test_case_ids_are_unique_and_name_stage_k_and_position():
    ids = [c.id for c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    for c in ALL_CASES:
        assert c.stage in c.id and f'-k{c.k}-' in c.id and f'@{int(c.pos[max(c.row, 0)])}of{c.L}' in c.id


def test_burst_positions_and_k_are_pinned():
    """What the GPU tests' ids promise: the burst's first sample per place, and one k (and burst amplitude) per stage."""
    c = rc.Case('fused', 'hid2', 12, 'first')
    assert [int(rc.Case('fused', 'hid2', 12, w, L=L).pos[0]) for w, L in
            (('first', 400), ('last', 400), ('boundary', 400), ('remainder', 200))] == [0, 392, 196, 184]
    # 'boundary' straddles sample 200, where two segments of a 400-sample row meet; 'remainder' lies in 160..199, behind the
    # two pooling windows of a 200-sample row, and past 179, where the up-sampled map ends
    assert 196 < 200 < 196 + len(rc.BURST) and 180 <= 184 and 184 + len(rc.BURST) <= 200
    assert rc.OVERFLOW_SPECS == [('hid2', 1, 12), ('hid2', -1, 17), ('hid10', 1, 12), ('sgb', 1, 12), ('stream', 1, 11)]
    assert rc.LOUD == 128.0 and c.row == 5
    assert {(c.spec, c.sign): c.k for c in rc.OVERFLOW_CASES} == {(s, g): k for s, g, k in rc.OVERFLOW_SPECS}
    assert all(c.amp == rc.LOUD and 0 <= c.row < c.n for c in rc.OVERFLOW_CASES + rc.TRAIN_OVERFLOW_CASES)
    assert all(c.k in (-3, 3) and not c.overflows for c in rc.SAFE_CASES)
    assert sorted({(c.n, c.L) for c in rc.SAFE_CASES}) == [(1, 96), (3, 200), (5, 160), (300, 400)]
    assert len(rc.OVERFLOW_CASES) == 19 + 3 + 4 * 12 + 1
    # every fused overflow place and stage is there
    fused = {(c.stage, c.sign, c.where) for c in rc.OVERFLOW_CASES if c.geom == 'fused' and c.n == 8 and c.r == 4}
    assert len(fused) == 19
    assert {c.r for c in rc.OVERFLOW_CASES} == {4, 10, 20} and max(c.n for c in rc.OVERFLOW_CASES) == 300


def test_gradient_law_matches_autograd_in_float64():
    """The exact gradient law of a rescaling (the GPU training test asserts it bitwise in fp32), against autograd on the
    float64 oracle: producer gradients times 2^-k, consumer weight gradients times 2^k, every other one equal."""
    x = rc.exact_input(2, 160)
    base = rc.base_state_dict('fused', 4)

    def grads(sd):
        p = {k: torch.from_numpy(v).double().requires_grad_() for k, v in sd.items()}
        y = so.stofnet_forward(p, x, 4, 80, torch.float64)
        (y * torch.linspace(-1, 1, y.numel(), dtype=torch.float64).view_as(y)).sum().backward()
        return {k: v.grad for k, v in p.items()}

    g0 = grads(base)
    for spec in ('hid2', 'sgb', 'stream'):
        g = grads(rc.rescale(base, spec, 3))
        law = rc.gradient_law(base, spec, 3)
        assert any(law.values())
        for name in base:
            assert torch.equal(g[name], g0[name] * 2.0 ** law[name]), f'{spec}: {name}'

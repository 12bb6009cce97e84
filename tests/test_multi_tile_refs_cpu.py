"""CPU pins of tests/multi_tile_inputs.py: every reference restatement against torch autograd at tiny shapes, the shape
choosers against the grids as the code stands, and the dyadic operands' headroom at every shape tests/test_gpu_multi_tile.py
uses (worst case: every term at its largest magnitude, which bounds the sum of |terms| of any draw)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import multi_tile_inputs as mt
from riders_inputs import edsr64, shuffle64


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize('N,L,cin,cout,K', [(2, 7, 3, 5, 3), (1, 2, 4, 2, 5), (3, 1, 2, 3, 7), (2, 9, 5, 4, 1), (1, 11, 1, 6, 9)])
def test_conv_references_match_conv1d_and_autograd(N, L, cin, cout, K):
    x, w, b = _rand(N, L, cin, seed=1), _rand(cout, cin, K, seed=2).requires_grad_(), _rand(cout, seed=3).requires_grad_()
    res, gy = _rand(N, L, cout, seed=4), _rand(N, L, cout, seed=5)
    pre = F.conv1d(x.permute(0, 2, 1), w, b, padding=K // 2).permute(0, 2, 1)
    assert _close(mt.conv_same(x, w.detach()) + b.detach(), pre.detach())
    for act, fn in ((mt.ACT_NONE, lambda v: v), (mt.ACT_RELU, torch.relu), (mt.ACT_LRELU, lambda v: F.leaky_relu(v, 0.01))):
        assert _close(mt.conv_forward_ref(x, w.detach(), b.detach(), res, act), fn(pre).detach() + res)
        assert _close(mt.conv_forward_ref(x, w.detach(), b.detach(), None, act), fn(pre).detach())
        # the data-gradient form: u -> z = act(u) -> conv(z, w) (+ a second consumer of z with gradient `res2`); d/du
        u = _rand(N, L, cin, seed=6).requires_grad_()
        res2 = _rand(N, L, cin, seed=7)
        z = fn(u)
        out = F.conv1d(z.permute(0, 2, 1), w.detach(), None, padding=K // 2).permute(0, 2, 1)
        gu, = torch.autograd.grad((out * gy).sum() + (z * res2).sum(), u)
        assert _close(mt.conv_backward_ref(gy, w.detach(), res2, z.detach(), act), gu)       # saved = the OUTPUT of the activation
    # weight / bias gradient
    gw, gb = torch.autograd.grad((pre * gy).sum(), [w, b])
    dw, db = mt.wgrad_ref(x, gy, K)
    assert dw.shape == (cout, cin, K) and _close(dw, gw) and _close(db, gb)


def test_masked_gradients_match_autograd():
    u, g, g2 = (_rand(2, 9, 4, seed=s).requires_grad_(s == 1) for s in (1, 2, 3))
    for fn, masked in ((torch.relu, lambda s: mt.masked_relu(g, s, g2)), (torch.tanh, lambda s: mt.masked_tanh(g + g2, s)),
                       (torch.sigmoid, lambda s: mt.masked_sigmoid(g + g2, s))):
        s = fn(u)
        gu, = torch.autograd.grad((s * (g + g2)).sum(), u)
        assert _close(masked(s.detach()), gu)
    assert _close(mt.masked_relu(g, torch.relu(u).detach()), g * (u > 0))


@pytest.mark.parametrize('r', [1, 4, 16, 64])
def test_edsr_out_operands_are_the_shuffled_convolution(r):
    N, L, cq = 2, 5, 64 // r
    trunk, w, b = _rand(N, L, 64, seed=1), _rand(1, cq, 3, seed=2).requires_grad_(), _rand(1, seed=3).requires_grad_()
    dy = _rand(N, L * r, seed=4)
    y = F.conv1d(shuffle64(trunk.permute(0, 2, 1).contiguous(), r), w, b, padding=1)            # [N, 1, L r]
    gw, gb = torch.autograd.grad((y[:, 0] * dy).sum(), [w, b])
    dw, db = mt.wgrad_ref(*mt.edsr_out_operands(trunk, dy, r), 3)
    assert _close(dw, gw) and _close(db, gb)


def test_chunked_kernel_restatements_match_autograd():
    N, L, r = 2, 7, 3
    # ESPCN conv3 + shuffle + sigmoid: y[n][l r + j] = sigmoid(z[n][j][l]); the saved OUTPUT y drives the derivative
    h2, w, b = _rand(N, L, 32, seed=1), _rand(r, 32, 3, seed=2).requires_grad_(), _rand(r, seed=3).requires_grad_()
    dy = _rand(N, L * r, seed=4)
    y = torch.sigmoid(F.conv1d(h2.permute(0, 2, 1), w, b, padding=1).permute(0, 2, 1).reshape(N, L * r))
    gw, gb = torch.autograd.grad((y * dy).sum(), [w, b])
    dw, db = mt.wgrad_ref(h2, mt.masked_sigmoid(dy, y.detach()).reshape(N, L, r), 3)
    assert _close(dw, gw) and _close(db, gb)
    # ESPCN conv1 + tanh, EDSR conv_input + ReLU with the long skip's g2, conv1_c (x NCL, Cin channels) + ReLU
    for K, Cin, fn, masked in ((5, 1, torch.tanh, mt.masked_tanh), (3, 1, torch.relu, None), (9, 3, torch.relu, None)):
        x, w, b = _rand(N, Cin, L, seed=5), _rand(64, Cin, K, seed=6).requires_grad_(), _rand(64, seed=7).requires_grad_()
        g, g2 = _rand(N, L, 64, seed=8), _rand(N, L, 64, seed=9)
        s = fn(F.conv1d(x, w, b, padding=K // 2)).permute(0, 2, 1)
        gw, gb = torch.autograd.grad((s * (g + g2)).sum(), [w, b])
        gm = masked(g + g2, s.detach()) if masked else mt.masked_relu(g, s.detach(), g2)
        dw, db = mt.wgrad_ref(x.permute(0, 2, 1), gm, K)
        assert _close(dw, gw) and _close(db, gb)


# -------------------------------------------------------------------------------------------------------------- shapes
# partials of the chunked weight gradients as the code stands (the GPU module reads them off the workspace queries):
# EW_MAX_COPIES, PW_MAX_COPIES, C1_COPIES, wgrad_copies(Cin, F) of widths.hip
COPIES = {'edsr_in': 1024, 'edsr_out': 1024, 'espcn_in': 512, 'espcn_out': 512, 'conv1': 2048, 'conv1_c_1_64': 2048,
          'conv1_c_2_24': 2048, 'conv1_c_5_96': 512, 'conv1_c_16_256': 128}
# name -> (largest |dy| after the mask, largest |x|, fraction bits of a product, positions per row)
WORST = {'edsr_in': (4.0, 2.0, 0, 1), 'edsr_out': (2.0, 2.0, 0, 4), 'espcn_in': (2.0, 2.0, 2, 1), 'espcn_out': (0.5, 1.0, 5, 1),
         'conv1': (2.0, 2.0, 0, 1)}


def _wgrad_groups(cin, cout):
    return max(1, 512 // (((cin + 63) // 64) * ((cout + 63) // 64)))          # wgrad_groups, train.hip


def test_tile_shapes_loop_and_keep_headroom():
    seen = set()
    for groups, tile in ([(mt.conv_groups(co), mt.CONV_TILE) for _, co, _ in mt.CONV_SETS]
                         + [(_wgrad_groups(ci, co), mt.WGRAD_TILE[p]) for ci, co in mt.WGRAD_SETS for p in (mt.FP32, mt.F16X3)]):
        for factor in (1.3, 1.4):
            shapes = mt.tile_shapes(groups, tile, factor)
            for which, (N, L) in shapes.items():
                tiles = mt.tiles_of(N, L, tile)
                assert tiles > groups and mt.in_loop_range(tiles, groups), (groups, tile, which)
                assert tiles % groups                                       # some work-groups take two tiles, others one
                mt.headroom(N * L * 2.0 * 2.0, 0)                           # a weight gradient over every row
                seen.add(which)
            assert shapes['short'][1] in (3, 5) and shapes['short'][0] % 2 == 1
            N, L = shapes['long']
            assert N in (2, 3) and L % 16 and L % 64 and L % 128 and L > tile
    assert seen == {'short', 'long'}
    for cin, _, K in mt.CONV_SETS:
        mt.headroom(K * cin * 4 + 4, 0)                                     # a forward / data-gradient sum, bias and residual
    assert {mt.conv_groups(co) for _, co, _ in mt.CONV_SETS} == {512, 256, 128, 64}
    assert min(_wgrad_groups(ci, co) for ci, co in mt.WGRAD_SETS) == 32        # 256 x 256: the only set below 48 partials


def test_chunk_shapes_loop_and_keep_headroom():
    for name, copies in COPIES.items():
        dy_max, x_max, frac, per_row = WORST[name if name in WORST else 'conv1']
        shapes = mt.chunk_shapes(copies, 1.3 if copies > 1024 else 1.4)
        for which, (N, L) in shapes.items():
            chunks = mt.chunks_of(N, L)
            assert chunks > copies > 48 and mt.in_loop_range(chunks, copies), (name, which)
            assert (N * L) % mt.CHUNK and chunks % copies                   # a partial last chunk; one or two chunks per work-group
            mt.headroom(N * L * per_row * dy_max * x_max, frac)
            assert N * L * 64 < 2 ** 31                                     # E_MAX_ROWS / P_MAX_ROWS
            assert N * L * 64 * 4 <= 175e6                                  # the largest operand on the device
        assert shapes['short'][1] == 3 and shapes['long'][0] == 3
        L = shapes['long'][1]
        assert L % 16 and L % 64 and L % 128
    N, L = mt.tail_shape()
    c = mt.chunks_of(N, L)
    assert c == mt.REDUCE_TAIL_CHUNKS > 48 and c % 64 and c % 16 and c <= min(COPIES.values()) and (N * L) % mt.CHUNK
    N, L = mt.tail_tile_shape()                                             # stof_train_wgrad: one tile per waveform, G = min(G, tiles)
    for p in (mt.FP32, mt.F16X3):
        assert mt.tiles_of(N, L, mt.WGRAD_TILE[p]) == mt.REDUCE_TAIL_CHUNKS
    assert sorted(_wgrad_groups(ci, co) for ci, co in mt.WGRAD_SETS if _wgrad_groups(ci, co) >= mt.REDUCE_TAIL_CHUNKS) == [128, 128, 512, 512]
    mt.headroom(N * L * 2.0 * 2.0, 0)
    # the reduce kernels' loops at 117 partials: `for (; k + 48 < n; k += 64)`, then `for (; k < n; k += 16)`, k starting at the slice
    steps = []
    for k in range(16):
        main = 0
        while k + 48 < mt.REDUCE_TAIL_CHUNKS:
            k, main = k + 64, main + 1
        steps.append((main, len(range(k, mt.REDUCE_TAIL_CHUNKS, 16))))
    assert steps == [(2, 0)] * 5 + [(1, 3)] * 11


# ------------------------------------------------------------------------------------------------------------ operands
def test_dyadic_operands():
    shape = (4000,)
    x, h, y = mt.ints(shape, 1), mt.halves(shape, 2), mt.quarters(shape, 3)
    assert x.dtype == torch.float32 and set(x.tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(h.tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0} and set(y.tolist()) == {0.25, 0.5, 0.75}
    assert torch.equal(mt.ints(shape, 1), x) and not torch.equal(mt.ints(shape, 4), x)         # reproducible, seeded
    on = (x > 0).float().mean()
    assert 0.3 < on < 0.5                                                   # ReLU masks: neither all-on nor all-off
    assert set((1 - h * h).tolist()) == {0.0, 0.75, 1.0} and set((y * (1 - y)).tolist()) == {0.1875, 0.25}
    # the masked gradients stay dyadic with the fraction bits the GPU module states
    for v, frac in ((mt.masked_tanh(x, h), 2), (mt.masked_sigmoid(x, y), 4), (mt.masked_sigmoid(x, y)[:, None] * h[None, :100], 5)):
        scaled = v.double() * 2 ** frac
        assert torch.equal(scaled, scaled.round()) and (v > 0).any() and (v < 0).any()
    assert float(mt.masked_sigmoid(x, y).abs().max()) == 0.5 and float(mt.masked_relu(x, x, x).abs().max()) == 4.0
    with pytest.raises(AssertionError):
        mt.headroom(2 ** 24, 0)
    with pytest.raises(AssertionError):
        mt.headroom(2 ** 20, 4)
    mt.headroom(2 ** 20 - 1, 4)
    with pytest.raises(AssertionError):
        mt.exact_fp32(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    assert mt.exact_fp32(torch.tensor([0.1875 * 3], dtype=torch.float64)).dtype == torch.float32


# -------------------------------------------------------------------------------------------------------- module level
def test_edsr_masked_forward_is_the_module_under_its_own_masks():
    m = mt.edsr_module(3, False).double()
    x, t = (v.double() for v in mt.module_inputs(2, 37, 4, 3))
    sh = lambda v: shuffle64(v, 4)                                           # noqa: E731
    pre = mt.edsr_relu_inputs(m, x)
    assert len(pre) == 2 and all(p.shape == (2, 64, 37) for p in pre) and all((p > 0).any() and (p < 0).any() for p in pre)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    assert _close(mt.edsr_masked_forward(m, x, None, sh).detach(), torch.from_numpy(edsr64(sd, 1, 4, x.numpy())[0]))      # masks = None: the module
    grads = []
    for masks in (None, [(p > 0).double() for p in pre], [(p > 0.05).double() for p in pre]):
        for p in m.parameters():
            p.grad = None
        xd = x.clone().requires_grad_()
        y = mt.edsr_masked_forward(m, xd, masks, sh)
        (y * t).sum().backward()
        grads.append([y.detach(), xd.grad] + [p.grad.clone() for p in m.parameters()])
    assert all(_close(a, b) for a, b in zip(grads[0], grads[1]))
    assert not _close(grads[2][1], grads[0][1])                              # other masks, another gradient: they are used


def test_edsr_seed_keeps_every_relu_input_clear_of_zero():
    """At the module-level shape of the GPU test: the seeded, bias-shifted EDSR's float64 ReLU inputs all lie RELU_MARGIN away from
    zero, torch's fp32 forward is ten times closer to float64 than that and agrees on every mask, and every channel keeps
    both mask values.  With the default initialisation the same shape has ReLU inputs within 1e-7 of zero."""
    N, L = mt.module_shape(COPIES['edsr_in'])
    assert mt.chunks_of(N, L) > COPIES['edsr_in'] and mt.tiles_of(N, L, mt.CONV_TILE) > mt.CONV_GROUPS
    m = mt.edsr_module(mt.EDSR_SEED, True)
    x, _ = mt.module_inputs(N, L, 4, mt.EDSR_SEED)
    p32, p64 = mt.edsr_relu_inputs(m, x), mt.edsr_relu_inputs(copy.deepcopy(m).double(), x.double())
    for a, b in zip(p32, p64):
        assert float(b.abs().min()) > mt.RELU_MARGIN
        assert float((a.double() - b).abs().max()) < 0.1 * mt.RELU_MARGIN
        assert torch.equal(a > 0, b > 0)
        on = (b > 0).float().mean(dim=(0, 2))
        assert 1e-4 < float(on.min()) and float(on.max()) < 1 - 1e-4
    d = mt.edsr_module(11, False).double()
    x, _ = mt.module_inputs(N, L, 4, 11)
    near = [int((p.abs() < 1e-7).sum()) for p in mt.edsr_relu_inputs(d, x.double())]
    print('default init: ReLU inputs within 1e-7 of zero', near)
    assert near[1] >= 5

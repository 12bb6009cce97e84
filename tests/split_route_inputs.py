"""Shapes, the split-row codec and the float64 stage references of the split-route tests (tests/test_split_route_refs_cpu.py
pins them on the CPU, tests/test_gpu_split_route.py drives the two-pass training sweeps, the small split-row kernels and
stof_train_wgrad_batch_split through the C ABI).  Holds no tests.

SPLIT ROWS (include/stofnet_amd.h, stof_train_wgrad_batch_split): a [rows][64] fp32 tensor's 256-byte rows rewritten as
[64 x fp16 hi | 64 x fp16 lo] with hi = fp16(v), lo = fp16(v - float(hi)), value = hi + lo.  Here such a tensor keeps the
dtype and shape of the fp32 tensor it replaces (as on the device); `to_split` / `from_split` convert.

WHICH SWEEP KERNEL RUNS (convstack.hip, train_sweep_geometry + body_p2_rows_ok): a waveform of L rows is cut into nseg = 2^k
segments of seg_len = ceil(L / nseg) rows with halo = 38 rows of context on each side (0 for nseg = 1); a (virtual) waveform
takes seg_len + 2 halo + 4 stream rows, and the two-pass kernel (body_p2.h) runs when that is at least 2 S = 384, otherwise the
r3 kernel with fp32 dumps.  stof_net_desc.seg_policy = k + 1 forces nseg = 2^k, 0 leaves the choice to the launch.

STAGE REFERENCES: every dump tensor of the sweeps from the kernel's OWN previous tensor, in float64, channel-last [N, L, 64]:
  forward   t0 = relu(conv1(x)) + pad(upsample80(e)), t[2k+1] = lrelu(conv{2k+2}(t[2k])), t[2k+2] = conv{2k+3}(t[2k+1]) + t[2k]
            (k = 0..4), t11 = conv12(t10) + t0, y[n][l r + j] = conv_last(t11)[n][l][j]
  backward  T1 = conv12^T(g6), T[10-2k] = conv{2k+3}^T(T[9-2k]) * m_k, T[11-2k] = conv{2k+2}^T(T[10-2k]) + T[9-2k] (k = 4..0),
            m_k = 1 where forward tensor 2k+1 is positive, else 0.01
With `given` = None the functions chain their own outputs: the network itself (pinned against oracle/ and autograd)."""
import torch
import torch.nn.functional as F

import multi_tile_inputs as mt

S_ROWS, GAP_ROWS, HALO = 192, 4, 38          # convstack.hip BODY_S, stof_common.h GAP, train_sweep_geometry `bp.halo`
SGB_SCALE = 80
STAGE_BOUND = 2e-6                           # one split-fp16 convolution against float64 (test_conv_kernels_vs_torch)
ROW_COUNTS = (1, 15, 16, 4099)               # the small split-row kernels: below / at / above one work-group, a ragged end
CONV_LAST_SHAPES = [(3, 2000), (2, 517), (1, 7)]          # (N, L) of test_conv_last_data_gradient_kernel

# name -> (N, L, seg_policy); N = None: multi_processor_count + 5.  What each one reaches:
CASES = {
    'floor': (2, 380, 1),        # L + 4 = 384 = 2 S exactly: the smallest shape the two-pass kernel takes
    'odd': (2, 778, 1),          # last step partial, rows no multiple of 16 or 96; 778 - 9 * 80 = 58
    'pairs': (None, 380, 1),     # two waveforms per work-group, the last work-group takes one; ring wrap across the gap rows
    'seg2': (2, 612, 2),         # halo 38, seg_len 306, both segments full width
    'seg4': (1, 1218, 3),        # seg_len 305, the last segment 303 rows: its two rows behind the waveform are cut row by row
                                 # (`valid` in the padding fix-up and in conv_last), never by span_ok
    'seg4_cut': (1, 1334, 3),    # seg_len 334, the last segment 332 rows, and a 96-row span of layer 4 ends on the two rows behind
                                 # the waveform while inside the segment's own rows: the `tw < Ltrue` term of span_ok alone keeps
                                 # it off the fast path (at 1218 no span of any layer ends there: spans_cut_by_waveform_end)
    'control': (2, 336, 0),      # the r3 kernel, fp32 dumps only
}
TWO_PASS_CASES = [c for c in CASES if c != 'control']


def case_shape(name, cus):
    N, L, policy = CASES[name]
    return (cus + 5 if N is None else N), L, policy


def geometry(L, seg_policy):
    """(segments, seg_len, stream rows per virtual waveform, two-pass kernel?) of a FORCED seg_policy >= 1"""
    assert seg_policy >= 1
    nseg = 1 << (seg_policy - 1)
    seg_len = (L + nseg - 1) // nseg
    rows = seg_len + (2 * HALO if nseg > 1 else 0) + GAP_ROWS
    return nseg, seg_len, rows, rows >= 2 * S_ROWS


def spans_cut_by_waveform_end(L, seg_policy):
    """[(sweep layer j, first row tk)] of the 96-row wave spans of the LAST segment that lie inside the segment's own rows but end
    behind the waveform (tw >= L): where only `tww + 95 < Ltrue` makes span_ok false (body_p2.h).  One virtual waveform per
    work-group (N nseg <= CUs): span starts are S (step - 1) - 3 j + 96 ni, j = 1..11, ni = 0, 1.

    This RESTATES the kernel's schedule (F = S step, R0 = F - S - 3 j, waves of 96 rows) and is no part of its interface: the CPU
    test only pins the literals it yields today.  What ties it to body_p2.h is
    tests/test_gpu_split_route.py::test_span_cut_by_the_waveform_end_takes_the_fix_up, which reads off the kernel's fp32 dumps
    which path wrote the predicted rows; if the lags or span widths change, that test fails and 'seg4_cut' needs a new length."""
    nseg, seg_len, rows, _ = geometry(L, seg_policy)
    halo = HALO if nseg > 1 else 0
    Lv = seg_len + 2 * halo
    steps = (Lv + 34 + S_ROWS - 1) // S_ROWS                    # convstack.hip: (gend - GAP + LAG_LAST + S - 1) / S, LAG_LAST = 34
    out = []
    for step in range(1, steps + 1):
        for j in range(1, 12):
            for ni in (0, 1):
                tk = S_ROWS * (step - 1) - 3 * j + 96 * ni
                if tk < halo or tk + 95 >= halo + seg_len:
                    continue
                if (nseg - 1) * seg_len - halo + tk + 95 >= L:
                    out.append((j, tk))
    return out


# --------------------------------------------------------------------------------------------------------------- codec
def to_split(v):
    """fp32 [..., 64] -> split rows, same dtype and shape: bytes 2c .. 2c+1 = hi of channel c, 128 + 2c .. = lo"""
    v = v.float().contiguous()
    assert v.shape[-1] == 64
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi, lo], dim=-1).view(torch.float32)


def split_halves(rows):
    """split rows [..., 64] -> (hi, lo) fp16 [..., 64] each"""
    assert rows.dtype == torch.float32 and rows.shape[-1] == 64
    h = rows.contiguous().view(torch.float16)
    return h[..., :64], h[..., 64:]


def from_split(rows, dtype=torch.float32):
    """split rows -> hi + lo, added in `dtype` (fp32: what add_split_kernel computes; float64: the exact value)"""
    hi, lo = split_halves(rows)
    return hi.to(dtype) + lo.to(dtype)


def same_bits(a, b):
    """bitwise equality of two fp32 tensors (NaN patterns and the sign of zero included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------------- references
def lrelu(v):
    return torch.where(v > 0, v, 0.01 * v)


def conv_t(gy, w):
    """conv^T: gy [N, L, cout], w (cout, cin, K) -> [N, L, cin]"""
    return mt.conv_same(gy, w.permute(1, 0, 2).flip(2))


def upsample_pad(e, L, scale=SGB_SCALE):
    """e [N, P, 64] -> [N, L, 64]: nearest up-sampling by `scale`, (L - P scale) / 2 rows of zero on each side"""
    N, P, C = e.shape
    rem_half = (L - P * scale) // 2
    assert (L - P * scale) % 2 == 0 and P == L // scale
    up = e.repeat_interleave(scale, dim=1)
    return F.pad(up, (0, 0, rem_half, L - P * scale - rem_half))


def x0_ref(p, x, e):
    """t0 = relu(conv1(x)) + pad(upsample80(e)); x [N, L], e [N, P, 64] or None (semi_global_scale 1)"""
    a1 = torch.relu(mt.conv_same(x[..., None], p['conv1.weight']) + p['conv1.bias'])
    return a1 if e is None else a1 + upsample_pad(e, x.shape[1])


def sgb_expand_ref(p, a1, scale=SGB_SCALE):
    """lrelu(expand_conv(maxpool(lrelu(contract_conv(a1))))) [N, P, 64]: the sweeps' sgb_expand operand (models/stofnet.py:100-107)"""
    N, L, _ = a1.shape
    P = L // scale
    z = lrelu(mt.conv_same(a1, p['semi_global_block.contract_conv.weight']) + p['semi_global_block.contract_conv.bias'])
    z = z[:, :P * scale].reshape(N, P, scale, z.shape[2]).amax(2)
    return lrelu(mt.conv_same(z, p['semi_global_block.expand_conv.weight']) + p['semi_global_block.expand_conv.bias'])


def forward_refs(p, x, e, r, given=None):
    """([ref of t0 .. t11], ref of y [N, L r]); stage i is computed from given[i - 1] (the kernel's own tensors, float64), or
    from the references themselves when given is None."""
    conv = lambda i, v: mt.conv_same(v, p[f'conv{i}.weight']) + p[f'conv{i}.bias']          # noqa: E731
    ref = [x0_ref(p, x, e)]
    t = ref if given is None else given
    for k in range(5):
        ref.append(lrelu(conv(2 * k + 2, t[2 * k])))
        ref.append(conv(2 * k + 3, t[2 * k + 1]) + t[2 * k])
    ref.append(conv(12, t[10]) + t[0])
    y = mt.conv_same(t[11], p['conv_last.weight']) + p['conv_last.bias']
    assert y.shape[2] == r
    return ref, y.reshape(y.shape[0], -1)


def backward_refs(p, g6, positive, given=None):
    """{j: ref of T[j]}, j = 1..11; positive[k] = the boolean mask `forward tensor 2k+1 is positive` under the route's rule;
    stage j from given[j - 1] (and given[9 - 2k] for the residual joins), or chained when given is None."""
    wt = lambda i, g: conv_t(g, p[f'conv{i}.weight'])                                           # noqa: E731
    ref = {1: wt(12, g6)}
    T = ref if given is None else given
    for k in range(4, -1, -1):
        m = torch.where(positive[k], torch.ones_like(g6), torch.full_like(g6, 0.01))      # (0.01 in g6's own dtype)
        ref[10 - 2 * k] = wt(2 * k + 3, T[9 - 2 * k]) * m
        ref[11 - 2 * k] = wt(2 * k + 2, T[10 - 2 * k]) + T[9 - 2 * k]
    return ref


def wgrad_pairs(fwd, T, g6):
    """[(x, dy, layer)] of the eleven k7 weight gradients in the engine's order (TrainEngine._backward_body_sweep)"""
    pairs = [(fwd[10], g6, 'conv12')]
    for k in range(4, -1, -1):
        pairs.append((fwd[2 * k + 1], T[9 - 2 * k], f'conv{2 * k + 3}'))
        pairs.append((fwd[2 * k], T[10 - 2 * k], f'conv{2 * k + 2}'))
    return pairs


def wgrad_ref(x, dy, out_scale=1.0, K=7):
    """dw[o][c][d] = out_scale sum dy[n][t][o] x[n][t + d - K // 2][c], db[o] = out_scale sum dy"""
    dw, db = mt.wgrad_ref(x, dy, K)
    return out_scale * dw, out_scale * db


def network_forward(p, x, r, scale):
    """pred [N, L r] of StofNet (13 blocks, k7) from the stage references chained; scale = 80 or 1"""
    e = None
    if scale != 1:
        e = sgb_expand_ref(p, x0_ref(p, x, None), scale)
    return forward_refs(p, x, e, r)[1]


def loss_ref(pred, gt, taps, amplitude=20.0, lam=1e-2):
    """main.py:228-232 on pred [N, M], gt [N, G] int64, taps = the 7 blur taps: MSE(pred, 20 blur7(onehot) / max) + lam mean|pred|"""
    mask = torch.zeros_like(pred)
    mask.scatter_(1, gt.clamp(min=0), 1.0)
    mask[:, :1] = 0
    mp = F.pad(mask, (3, 3))
    blur = sum(float(taps[d]) * mp[:, d:d + pred.shape[1]] for d in range(7))
    target = blur / blur.max() * amplitude
    return ((pred - target) ** 2).mean() + lam * pred.abs().mean()


def params64(sd, device='cpu'):
    return {k: torch.as_tensor(v).to(device, torch.float64) for k, v in sd.items()}


def rel(a, ref):
    return mt.rel(a, ref)


# ------------------------------------------------------------------------------------------------------------- operands
def gauss(shape, seed, device='cpu', scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(tuple(shape), generator=g)).to(device)


def codec_edge_values():
    """fp32 values at the codec's edges: zeros of both signs, fp16 subnormals and values below them, the largest finite fp16
    and the fp32 values just inside the rounding boundary to infinity, ties of the hi rounding"""
    v = [0.0, -0.0, 2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 1.5 * 2.0 ** -24, 6.1e-5, 5.9e-8,
         65504.0, 65519.0, 65503.99, 60000.5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -23, 0.1, 1e-3]
    t = torch.tensor(v + [-a for a in v], dtype=torch.float32)
    return torch.cat([t, torch.zeros(64 - t.numel() % 64)]).reshape(-1, 64)


def wgrad_batch_groups(ws_bytes, count, K=7):
    per = count * (K * 64 * 64 + 64) * 4
    assert ws_bytes % per == 0
    return ws_bytes // per


def in_loop_range(tiles, groups):
    return mt.in_loop_range(tiles, groups)


def planted_signs(shape, seed):
    """int8 tensor: 0 = keep, 1 = +0, 2 = -0, 3 = +2^-26, 4 = -2^-26, about 2 % of the elements each"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 50, tuple(shape), generator=g, dtype=torch.int8)
    return torch.where(u < 5, u, torch.zeros_like(u))


def plant(t, signs):
    vals = torch.tensor([0.0, 0.0, -0.0, 2.0 ** -26, -2.0 ** -26], dtype=t.dtype, device=t.device)
    return torch.where(signs.to(t.device) > 0, vals[signs.to(t.device).long()], t)

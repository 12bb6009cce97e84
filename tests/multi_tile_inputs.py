"""Shapes, dyadic operands and float64 references of the multi-tile tests (tests/test_multi_tile_refs_cpu.py pins the
references against torch autograd and the operands' headroom on the CPU, tests/test_gpu_multi_tile.py runs the training
kernels through the C ABI at the smallest shapes at which a work-group takes a second tile).  Holds no tests.

Every kernel behind the training routes is persistent or grid-strided: work-group g walks tiles g, g + G, .. (or 256-row
chunks) and writes ONE partial; a reduce kernel adds the G partials, four chains of sixteen slices while more than 48 are
left.  The grids, as the code stands (the tests read G off the workspace queries where the ABI has one):

  stof_train_conv         G = 512 / ceil(cout / 64) work-groups per output block, tiles of 128 rows that never span two
                          waveforms (launch_conv_cl, train.hip: CT = CT16 = 128, `512 / oblocks`, `512 / ob`)
  stof_train_wgrad        G = 512 / (cin blocks x cout blocks) = workspace bytes / bytes of one partial; tiles of 128 rows
                          (fp32, WG_ROWS) or 64 rows (f16x3, WG_ROWS_H), never spanning two waveforms
  chunked weight gradients  G = workspace bytes / bytes of one partial; chunks of 256 rows of the flat [N L] row sequence
                          (EW_CHUNK, PW_CHUNK, WC_CHUNK, C1_CHUNK)

Once a work-group loops, the number of partials IS G (a power of two >= 32), so `partials mod 64` and `mod 16` non-zero
cannot be had together with a second tile; REDUCE_TAIL_CHUNKS gives the reduce kernels that case on its own.

Operands are DYADIC: small integers times a power of two, so that every product and every partial sum is an fp32 number
and the result does not depend on the order of the sums.  `headroom` states the condition: (largest sum of |terms|) x 2^f
< 2^24 with f the fraction bits in use.

The module-level cases (EDSR_1D(1, 64, 1, 4), ESPCN_1D(4)) run on Gaussian frames; at their 3.4e5 rows a ReLU input within
fp32 rounding of zero is a certainty under torch's default initialisation, so the seeded EDSR case moves its biases
(`edsr_module`) and `edsr_masked_forward` restates the network under given masks."""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
FP32, F16X3 = 0, 1

CONV_GROUPS = 512                 # launch_conv_cl: `int64_t gx = 512 / oblocks`, `int64_t g16 = 512 / ob`
CONV_TILE = 128                   # train.hip: `constexpr int CT = 128`, `constexpr int CT16 = 128`
WGRAD_TILE = {FP32: 128, F16X3: 64}      # train.hip: WG_ROWS, WG_ROWS_H
CHUNK = 256                       # EW_CHUNK (edsr_train.hip), PW_CHUNK (espcn_train.hip), WC_CHUNK (widths.hip), C1_CHUNK (train.hip)
LOOP_RANGE = (1.3, 1.7)           # tiles / G: some work-groups take two tiles, the others one
# partials > 48 with 117 mod 64 = 53 and 117 mod 16 = 5: of a reduce kernel's sixteen slices, 0 .. 4 take the four-chain loop
# twice and no tail step, 5 .. 15 take it once and then three tail steps
REDUCE_TAIL_CHUNKS = 117

# (cin, cout, K) of stof_train_conv: EDSR's body, the other kernel sizes, the padded widths, more than one output block
# (a smaller grid), the SemiGlobalBlock pair
CONV_SETS = [(64, 64, 3), (64, 64, 5), (64, 64, 1), (32, 32, 3), (96, 96, 5), (128, 128, 7), (256, 256, 1), (64, 512, 5),
             (512, 64, 5)]
WGRAD_SETS = [(64, 64), (32, 32), (96, 96), (128, 128), (256, 256), (64, 512), (512, 64)]
WGRAD_KS = (3, 5)
CONV1_C_WIDTHS = [(1, 64), (2, 24), (5, 96)]          # (Cin, F): wgrad_cgroup 1, 2, 4 (widths.hip)
CONV1_C_WIDE = (16, 256)                               # four channel tiles x four channel groups: 128 partials


def conv_groups(cout):
    return max(1, CONV_GROUPS // ((cout + 63) // 64))


def tile_shapes(groups, tile, factor=1.4):
    """{'short': (N, L), 'long': (N, L)} for a kernel whose tiles hold `tile` rows of ONE waveform: about factor x groups
    tiles.  short: L = 5, one tile per waveform, an odd N; long: N = 3, the last tile of each waveform 37 rows short."""
    n_short = int(math.ceil(factor * groups)) | 1
    per = int(math.ceil(factor * groups / 3))
    return {'short': (n_short, 5), 'long': (3, per * tile - 37)}


def tiles_of(N, L, tile):
    return N * ((L + tile - 1) // tile)


def chunk_shapes(copies, factor=1.4):
    """The same for a kernel that walks CHUNK-row chunks of the flat row sequence: short rows of L = 3 (`t` wraps five times
    per pass of 16 rows), and N = 3 long rows of an odd length; the last chunk is partial in both."""
    rows = int(math.ceil(factor * copies * CHUNK))
    n_short = rows // 3 + 1
    L_long = (rows // 3) | 1
    if (3 * L_long) % CHUNK == 0:
        L_long += 2
    if (3 * n_short) % CHUNK == 0:
        n_short += 1
    return {'short': (n_short, 3), 'long': (3, L_long)}


def chunks_of(N, L):
    return (N * L + CHUNK - 1) // CHUNK


def tail_shape():
    """(N, L) with REDUCE_TAIL_CHUNKS chunks, the last one partial: no work-group loops, the reduce kernel runs both loops."""
    return 3, (REDUCE_TAIL_CHUNKS * CHUNK - 100) // 3


def tail_tile_shape():
    """(N, L) with REDUCE_TAIL_CHUNKS tiles for a kernel whose tiles never span two waveforms (stof_train_wgrad launches
    min(G, tiles) work-groups, train.hip `if (G > tiles) G = (int)tiles`): one short waveform per tile."""
    return REDUCE_TAIL_CHUNKS, 5


def in_loop_range(tiles, groups):
    return LOOP_RANGE[0] * groups <= tiles <= LOOP_RANGE[1] * groups


# ------------------------------------------------------------------------------------------------------------ operands
def dyadic(shape, lo, hi, scale=1.0, seed=0, device='cpu'):
    """float32 tensor of scale x integers drawn uniformly from lo .. hi (scale a power of two), reproducible from `seed`."""
    assert math.log2(scale) == int(math.log2(scale)) and -128 <= lo <= hi <= 127
    gen = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int8)
    return v.to(device).float() * scale


def ints(shape, seed, device='cpu'):
    """x, g, w, b, dy: integers -2 .. 2"""
    return dyadic(shape, -2, 2, 1.0, seed, device)


def halves(shape, seed, device='cpu'):
    """saved tanh activations in {0, +-1/2, +-1}: 1 - h^2 in {1, 3/4, 0}"""
    return dyadic(shape, -2, 2, 0.5, seed, device)


def quarters(shape, seed, device='cpu'):
    """saved sigmoid outputs in {1/4, 1/2, 3/4}: y (1 - y) in {3/16, 1/4}"""
    return dyadic(shape, 1, 3, 0.25, seed, device)


def headroom(sum_abs_max, frac_bits):
    """A sum whose terms are multiples of 2^-frac_bits and whose |terms| add up to at most sum_abs_max is exact in fp32, in
    any order, when every partial sum is below 2^24 units."""
    assert float(sum_abs_max) * 2.0 ** frac_bits < 2.0 ** 24, (float(sum_abs_max), frac_bits)


def exact_fp32(t):
    """float64 -> float32, asserting that nothing is lost (the reference itself must be an fp32 number)."""
    f = t.float()
    assert torch.equal(f.double(), t)
    return f


# ---------------------------------------------------------------------------------------------------------- references
def conv_same(x, w):
    """x [N, L, cin], w (cout, cin, K) -> [N, L, cout] = F.conv1d(x^T, w, padding = K // 2)^T, as K matmuls (any device)."""
    K = w.shape[2]
    L = x.shape[1]
    xp = F.pad(x, (0, 0, K // 2, K // 2))
    y = xp[:, 0:L] @ w[:, :, 0].T
    for d in range(1, K):
        y += xp[:, d:d + L] @ w[:, :, d].T
    return y


def act_fwd(v, act):
    return torch.relu(v) if act == ACT_RELU else torch.where(v > 0, v, 0.01 * v) if act == ACT_LRELU else v


def act_mask(saved, act):
    if act == ACT_NONE:
        return torch.ones_like(saved)
    off = torch.full_like(saved, 0.0 if act == ACT_RELU else 0.01)            # (0.01 in the operands' own dtype)
    return torch.where(saved > 0, torch.ones_like(saved), off)


def conv_forward_ref(x, w, b, residual, act):
    """stof_train_conv with saved == NULL: act(bias + conv_same(x, w)) + residual, channel-last, in the operands' dtype."""
    y = act_fwd(conv_same(x, w) + b, act)
    return y + residual if residual is not None else y


def conv_backward_ref(gy, w, residual, saved, act):
    """stof_train_conv with the flipped weight image and `saved`: (conv_transpose(gy, w) + residual) * act'(saved);
    gy [N, L, cout], w (cout, cin, K) -> [N, L, cin]."""
    wt = w.permute(1, 0, 2).flip(2)
    g = conv_same(gy, wt)
    if residual is not None:
        g = g + residual
    return g * act_mask(saved, act)


def wgrad_ref(x, dy, K):
    """dw (cout, cin, K)[o][c][d] = sum dy[n][t][o] x[n][t + d - K // 2][c], db (cout) = sum dy; x [N, L, cin], dy [N, L, cout]."""
    L = x.shape[1]
    xp = F.pad(x, (0, 0, K // 2, K // 2))
    dyf = dy.reshape(-1, dy.shape[2])
    dw = torch.stack([dyf.T @ xp[:, d:d + L].reshape(-1, x.shape[2]) for d in range(K)], dim=2)
    return dw, dyf.sum(0)


def masked_relu(g, saved, g2=None):
    """(g + g2) * [saved > 0]: the gradient in front of a ReLU (conv1, conv1_c, EDSR's conv_input)"""
    return (g if g2 is None else g + g2) * (saved > 0)


def masked_tanh(g, h):
    """g * (1 - h^2): the gradient in front of a tanh whose OUTPUT h was saved (ESPCN conv1 / conv2)"""
    return g * (1.0 - h * h)


def masked_sigmoid(dy, y):
    """dy * y * (1 - y): the gradient in front of a sigmoid whose OUTPUT y was saved (ESPCN conv3)"""
    return dy * y * (1.0 - y)


def edsr_out_operands(trunk, dy, r):
    """EDSR's conv_output reads the trunk [N, L, 64] as its SampleShuffle1D(r) image [N, L r, 64 / r] (the same memory);
    dy [N, L r] -> ([N, L r, 64 / r], [N, L r, 1]) = the (x, dy) of wgrad_ref with K = 3."""
    N, L, C = trunk.shape
    return trunk.reshape(N, L * r, C // r), dy.reshape(N, L * r, 1)


def rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


# -------------------------------------------------------------------------------------------------------- module level
EDSR_SEED = 5                     # of seeds 1 .. 8 the one whose ReLU inputs stay farthest from zero (1.3e-5 and 6.4e-6)
RELU_MARGIN = 4e-6                # the float64 ReLU inputs of the seeded EDSR case stay this far from zero: ten times the largest
                                  # deviation of torch's fp32 pre-activations from float64 at that shape (4e-7, on the CPU)


def module_shape(copies):
    """(N, L) of the module-level cases: 1.3 x the rows at which `copies` partials of 256-row chunks saturate"""
    return chunk_shapes(copies, 1.3)['long']


def module_inputs(N, L, r, seed):
    """x [N, 1, L] and the cotangent t [N, 1, L r] of loss = sum(y t), float32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn((N, 1, L), generator=g), torch.randn((N, 1, L * r), generator=g)


def edsr_module(seed, shifted):
    """EDSR_1D(1, 64, 1, 4) with torch's seeded default initialisation.  shifted: the biases in front of the two ReLUs are
    moved 3.5 standard deviations of their pre-activation (inputs 0.5 x N(0, 1)) away from zero, alternating in sign over
    the channels, so that about a hundred times fewer of the 44 M ReLU inputs of the module-level shape fall within fp32
    rounding of zero, where the mask may legitimately differ from float64's.  With the default initialisation no seed has
    fp32 and float64 agree on every mask robustly (about twenty inputs within 1e-7 of zero, whatever the seed), hence the
    shift.  The price: every channel is then about 99.98 % on or 99.98 % off (some 70 rows of 3.4e5 on the other side), so
    this case exercises the masks weakly.  The ordinary, half-on masks are exercised by the default-initialisation case
    of the GPU module, which compares with float64 autograd under the route's own saved masks and admits a differing mask
    only where the float64 input is below RELU_MARGIN."""
    from stofnet_amd import EDSR_1D
    torch.manual_seed(seed)
    m = EDSR_1D(1, 64, 1, 4)
    if shifted:
        sign = 1.0 - 2.0 * (torch.arange(64) % 2)
        with torch.no_grad():
            m.conv_input.bias.copy_(3.5 * 0.5 * m.conv_input.weight.norm(dim=(1, 2)) * sign)
            blk = m.residual_blocks[0].conv1                 # mean and deviation per channel off a pilot row
            pilot = 0.5 * torch.randn((1, 1, 8192), generator=torch.Generator().manual_seed(seed + 1000))
            pre = F.conv1d(torch.relu(m.conv_input(pilot)), blk.weight, None, padding=1)
            blk.bias.copy_(3.5 * pre.std(dim=(0, 2)) * sign - pre.mean(dim=(0, 2)))
    return m


def edsr_relu_inputs(m, x):
    """the pre-activations of EDSR_1D's ReLUs in the module's dtype: [conv_input(x), conv1 of every block], [N, 64, L] each"""
    with torch.no_grad():
        pre = [m.conv_input(x)]
        out = torch.relu(pre[0])
        for blk in m.residual_blocks:
            pre.append(blk.conv1(out))
            out = blk(out)
    return pre


def edsr_masked_forward(m, x, masks, shuffle=None):
    """EDSR_1D.forward_aten with every ReLU replaced by a multiplication with a given 0 / 1 mask [N, 64, L] (masks[0]:
    conv_input's, masks[1 + i]: block i's): the network as the kernel route's backward sees it through its saved masks.
    masks = None: the ReLUs themselves.  shuffle: SampleShuffle1D for tensors the module's own (device-only) one refuses."""
    shuffle = shuffle or m.upscale
    gate = (lambda v, i: torch.relu(v)) if masks is None else (lambda v, i: v * masks[i])      # noqa: E731
    first = gate(m.conv_input(x), 0)
    out = first
    for i, blk in enumerate(m.residual_blocks):
        out = out + blk.conv2(gate(blk.conv1(out), 1 + i))
    out = m.conv_mid(out) + first
    return m.conv_output(shuffle(out))

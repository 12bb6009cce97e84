"""Shapes, inputs, float64 references and the workspace reader of the SemiGlobalBlock stage tests
(tests/test_sgb_stage_refs_cpu.py pins the references and the caps on the CPU, tests/test_gpu_sgb_stages.py compares the
kernels' pooled map, arg-max bytes and expand map with them).  Holds no tests.

The stages of the inference forward are  relu(conv1) -> contract conv 64->512 k5 -> lrelu -> max-pool 80 => pooled[N][P][512]
-> expand conv 512->64 k5 -> lrelu => sgb[N][P][64];  both maps sit at the front of the forward workspace (launch_forward,
convstack.hip).  The expand kernels walk a row stream of period P + 2 (the P pooled rows of a waveform, then 2 gap rows) in
tiles of 256 rows (sgb_expand.hip, split fp16) or 128 rows (conv_cl_kernel in stream mode, exact fp32); the contract kernel
takes two consecutive entries of the flat sequence of N * P pooling windows per work-group."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import stofnet_oracle as so
from stofnet_amd import synth

R = 4
SCALE = 80
SEED = 3008                 # the weights of tests/test_sgb_window_stream.py
SG = 'semi_global_block.'
NF_SGB = 512
NF = 64
SUB_BATCH = 4096            # rows whose maps share one workspace (convstack.hip): read_stages holds for one sub-batch

MAP_TOL = 1e-5              # stage bound relative to max|ref|: the project's bar (tests/test_gpu_parity.py)
ARG_GATE = 1e-4             # arg-max is pinned where the float64 gap exceeds this share of max|contract|: ten times the bar
EXCLUDED_CAP = 0.05         # at most this share of (window, channel) pairs may fall under the gate

# name -> (N, L); P = L // 80, stream period P + 2, N (P + 2) stream rows.  Each is the smallest that reaches its arrangement.
STAGE_SHAPES = {
    # 1799 stream rows: eight expand tiles whose starts 256 k mod 7 = 0, 4, 1, 5, 2, 6, 3, 0 are every phase (both gap rows,
    # the first and the last pooled row), fp32 tiles with starts 128 k mod 7 likewise; N P = 1285 is odd (the last contract
    # tile holds one window) and P is odd (contract tiles pair windows of different waveforms)
    'T7': (257, 400),
    # P = 1, 300 stream rows: every pooled row has gap rows on both sides, tile 1 starts on a gap row (256 mod 3 = 1), every
    # contract tile spans two waveforms
    'T3': (100, 80),
    # the benched length, 540 stream rows: tile starts at phases 256 mod 27 = 13 and 512 mod 27 = 26 (the last gap row)
    'T27': (20, 2000),
    # a waveform (300 pooled rows) longer than a tile: tile boundaries with real pooled rows on both sides, all four halo
    # rows live
    'TL': (2, 24000),
    # remainder 38: the last window's right halo (t = 400, 401) holds real samples and conv1 reaches t = 405
    'R38': (3, 438),
    # remainder 2, P = 1: the left halo is zero, the right halo is real
    'R2': (4, 82),
}
ARG_SHAPES = ('T7', 'R38', 'R2')            # arg-max bytes on random inputs
TRAIN_POOLED_SHAPES = ('T7', 'T3', 'R38', 'R2')
TIE_SHAPE = (2, 400)
TIE_PERIODS = (1, 4, 16, 40)                # every one divides 80, so window w repeats window 1 for w = 1 .. P - 2


def state_dict():
    return synth.synth_state_dict(R, seed=SEED)


def stage_input(name):
    """[N, 1, L] float32 of a STAGE_SHAPES entry."""
    n, L = STAGE_SHAPES[name]
    return synth.synth_randn(n, L, seed=SEED + L)


def periodic_input(q):
    """[2, 1, 400] float32 with x[n, 0, t] = base[n, t mod q]: away from the ends of the waveform every contract row j sees
    the operands of row j + q, so every window 1 .. P - 2 holds 80 / q exact copies of q rows."""
    n, L = TIE_SHAPE
    base = np.random.default_rng(7).standard_normal((n, q)).astype(np.float32)
    return np.ascontiguousarray(base[:, np.arange(L) % q][:, None, :])


def _p64(sd, name):
    return torch.from_numpy(np.ascontiguousarray(sd[name])).double()


def stage_reference(sd, x, keep_contract=True, rows_per_chunk=32):
    """float64 stages of x [N, 1, L]: {'conv1': [N, 64, L] relu(conv1), 'contract': [N, 512, L] lrelu(contract conv) before
    the pool (None unless keep_contract), 'pooled': [N, 512, P]}.  The SemiGlobalBlock of the oracle on relu(conv1) only:
    the body is not under test.  Waveforms do not see each other, so they go through in chunks to bound the memory."""
    x64 = torch.from_numpy(np.ascontiguousarray(x)).double()
    w1, b1 = _p64(sd, 'conv1.weight'), _p64(sd, 'conv1.bias')
    out = {'conv1': [], 'contract': [], 'pooled': []}
    for i in range(0, x64.shape[0], rows_per_chunk):
        a1 = F.relu(so.conv1d_same(x64[i:i + rows_per_chunk], w1, b1, 4))
        taps = {}
        so.semi_global_block(a1, sd, SG, SCALE, dtype=torch.float64, taps=taps)
        out['conv1'].append(a1)
        out['pooled'].append(taps['sgb_pooled'])
        if keep_contract:
            out['contract'].append(taps['sgb_contract'])
    return {k: (torch.cat(v) if v else None) for k, v in out.items()}


def expand_reference(sd, pooled):
    """float64 lrelu(expand conv) [N, P, 64] of a pooled map [N, P, 512] (any float dtype, e.g. the one the GPU produced, so
    that the expand stage is judged on its own)."""
    z = torch.as_tensor(pooled).detach().cpu().double().permute(0, 2, 1)
    z = F.leaky_relu(F.conv1d(z, _p64(sd, SG + 'expand_conv.weight'), _p64(sd, SG + 'expand_conv.bias'), padding=2), 0.01)
    return z.permute(0, 2, 1).contiguous()


def windows(contract):
    """[N, 512, L] -> [N, P, 512, 80]: the pooling windows in the layout of the kernels' pooled / arg maps."""
    n, c, L = contract.shape
    P = L // SCALE
    return contract[..., :P * SCALE].reshape(n, c, P, SCALE).permute(0, 2, 1, 3)


def gated_argmax(win, gate_abs):
    """win [..., rows] float64 -> (first arg-max, top value, clear): `clear` where the largest value stands more than
    gate_abs above every row that is not an exact copy of it (for rows without exact ties: above the second-largest), i.e.
    where a map within the stage bound cannot legitimately move the arg-max off the first maximum."""
    top, arg = win.max(-1)
    first = (win == top[..., None]).to(torch.uint8).argmax(-1)          # torch.max promises no tie order; argmax of 0 / 1 bytes gives the first
    assert torch.equal(torch.gather(win, -1, first[..., None])[..., 0], top)
    below = torch.where(win == top[..., None], torch.full_like(win, -float('inf')), win).amax(-1)
    return first, top, (top - below) > gate_abs


def top2_gap(win):
    """largest minus second-largest value of every window (0 at an exact tie)"""
    if win.shape[-1] < 2:
        return torch.full(win.shape[:-1], float('inf'), dtype=win.dtype)
    t = win.topk(2, dim=-1).values
    return t[..., 0] - t[..., 1]


def excluded_share(win, gate_abs):
    """share of windows whose top-2 gap is not above the gate"""
    return float((top2_gap(win) <= gate_abs).double().mean())


def tie_windows(contract, q):
    """the q distinct rows of windows 1 .. P - 2 of a periodic input: [N, P - 2, 512, q]"""
    return windows(contract)[:, 1:-1, :, :q]


def read_stages(model, n, L):
    """Clones of pooled [n, P, 512] and sgb [n, P, 64] out of the workspace of the forward that `model` has just run on
    [n, 1, L]: the layout of launch_forward (convstack.hip), valid for one sub-batch."""
    assert 0 < n <= SUB_BATCH, 'the second sub-batch of a larger call overwrites the maps of the first'
    P = L // SCALE
    assert P > 0
    ws = model._workspace
    nfl = n * P * (NF_SGB + NF)
    assert ws is not None and ws.numel() >= 4 * nfl, 'workspace smaller than the two maps'
    f = ws[:ws.numel() // 4 * 4].view(torch.float32)
    pooled = f[:n * P * NF_SGB].view(n, P, NF_SGB).clone()
    sgb = f[n * P * NF_SGB:nfl].view(n, P, NF).clone()
    return pooled, sgb


def rel_err(got, ref):
    """(max |got - ref| / max |ref|, flat index of the worst element) in float64"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).double()
    d = (got - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)
    k = int(d.argmax())
    return float(d.reshape(-1)[k] / ref.abs().max().clamp_min(1e-300)), k

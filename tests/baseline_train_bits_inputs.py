"""Cases of the bit fixture of the baselines' training kernels (tests/golden/f31_baseline_train_bits.npz), shared by its
recorder (tests/golden/make_golden_baseline_train_bits.py) and the tests.  The fixture holds what the C ABI entry points of
csrc/sincnet_train.hip, csrc/waveunet_train.hip, csrc/zonzini_train.hip and the ESPCN weight repack wrote, bit for bit, on
seeded Gaussian operands; the operands are regenerated from the seed on the CPU (`operands`), the manifest keeps their SHA-256.

A case is (name, family, parameters, seed).  A family has a function that draws its operands (CPU tensors, in a fixed order
from one generator, correctly rounded operations only) and one that runs its entries through the C ABI.  Outputs start as NaN
(float) or 0xff bytes (workspaces, blobs), so whatever is read back must have been written; buffers in SincNet's GAP layout are
returned whole, zeroed gap rows included.

The shapes are the smallest at which each kernel can go wrong (constants of the .hip files):
  BatchNorm of SincNet (statistics, apply, backward; chunks of ST_CHUNK = 256 rows, 1024 partials at the most) and of
  Wave-U-Net (ST_ROWS = 256, ST_MAX = 256): 2 rows, 255 / 256 / 257 (one chunk, the exact boundary, the first split), 3 x 171
  (ragged last chunk) and one grown case each (rows per partial above the minimum).  z has a per-channel offset of a few
  standard deviations, so the variance's cancellation is part of the bits.
  weight gradients: one row below, at and above the chunk (SincNet conv 64, out 256; Zonzini conv 64, in 256; Wave-U-Net in /
  head 256) and a grown case each; the bank gradient one sample below and above a 128-sample tile, and 70 tiles (above 64).
  packers: every fragment image on one seeded parameter set."""
import ctypes
import hashlib

import numpy as np
import torch

C, GAP = 128, 8
SN_TAPS = (1023, 11, 9, 7)
SN_FS, SN_EPS, SN_MOMENTUM = 16000.0, 1e-5, 0.05
WU_EPS, WU_MOMENTUM = 1e-5, 0.1
ZZ_CH = {0: (16, 32, 64, 64), 1: (50, 100, 150, 200, 250)}
RAW_BYTES = 8192          # an output larger than this is stored as the SHA-256 of its bytes (manifest), smaller ones raw (.npz)


# ------------------------------------------------------------------------------------------------------------ operands
def _n(gen, *shape):
    return torch.randn(shape, generator=gen, dtype=torch.float32)


def _pos(gen, *shape):
    return _n(gen, *shape).abs().add(0.5)


def _tanh_like(gen, *shape):
    return _n(gen, *shape).mul(0.6).clamp(-0.999, 0.999)


def gap_buffer(t):
    """[N, L, 128] -> SincNet's GAP layout, flat, zero gap rows"""
    N, L = int(t.shape[0]), int(t.shape[1])
    buf = torch.zeros((GAP + N * (L + GAP)) * C, dtype=torch.float32)
    buf[GAP * C:].view(N, L + GAP, C)[:, :L] = t
    return buf


def _zz_pad(t, c):
    t[..., c:] = 0
    return t


def zz_lens(variant, L):
    lens = [L]
    for _ in ZZ_CH[variant]:
        lens.append(((lens[-1] - 10) // 2 + 1) // 2 if lens[-1] >= 10 else 0)
    return lens


def zz_length_for(pooled, depth):
    """the shortest input whose length after `depth` conv + pool layers is `pooled`"""
    for _ in range(depth):
        pooled = 4 * pooled + 8
    return pooled


def _zz_cpad(variant):
    return [(c + 3) & ~3 for c in ZZ_CH[variant]]


def _ops_sn_bn(p, gen):
    ch, N, L = p['ch'], p['N'], p['L']
    z = _n(gen, N, L, ch) + _n(gen, ch).mul(3.0)
    da = _n(gen, N, L, ch)
    ops = {'z': gap_buffer(z) if ch == C else z.reshape(-1), 'da': gap_buffer(da) if ch == C else da.reshape(-1)}
    ops.update(gamma=_n(gen, ch), beta=_n(gen, ch), run_mean=_n(gen, ch), run_var=_pos(gen, ch))
    return ops


def _ops_wu_bn(p, gen):
    ch, rows = p['ch'], p['rows']
    return {'z': _n(gen, rows, ch) + _n(gen, ch).mul(3.0), 'da': _n(gen, rows, ch), 'gamma': _n(gen, ch), 'beta': _n(gen, ch),
            'run_mean': _n(gen, ch), 'run_var': _pos(gen, ch)}


def _ops_sn_conv_wgrad(p, gen):
    return {'a_prev': gap_buffer(_n(gen, p['N'], p['L'], C)), 'dz': gap_buffer(_n(gen, p['N'], p['L'], C))}


def _ops_sn_out_wgrad(p, gen):
    return {'a2': gap_buffer(_n(gen, p['N'], p['L'], C)), 'dz3': _n(gen, p['N'] * p['L'])}


def _ops_sn_bank_grad(p, gen):
    return {'x': _n(gen, p['N'], p['L']), 'dz0': gap_buffer(_n(gen, p['N'], p['L'], C))}


def _ops_sn_pack(p, gen):
    ops = {'low_hz': torch.rand(C, generator=gen).mul(2000.0).add(30.0), 'band_hz': torch.rand(C, generator=gen).mul(1000.0).add(50.0)}
    for l in (1, 2, 3):
        cout = C if l < 3 else 1
        ops[f'w{l}'] = _n(gen, cout, C, SN_TAPS[l]).mul(0.05)
        ops[f'b{l}'] = _n(gen, cout)
    for l in range(4):
        ch = C if l < 3 else 1
        ops.update({f'bn{l}_w': _n(gen, ch), f'bn{l}_b': _n(gen, ch), f'bn{l}_mean': _n(gen, ch), f'bn{l}_var': _pos(gen, ch)})
    return ops


def _ops_wu_wgrad(p, gen):
    N, Lout, cin, cu, cout = p['N'], p['Lout'], p['cin'], p['cu'], p['cout']
    if p['mode'] == 0:
        ops = {'src': _n(gen, N, 2 * Lout, cin)}
    elif p['mode'] == 1:
        ops = {'src': _n(gen, N, Lout, cin - cu), 'low': _n(gen, N, Lout // 2, cu)}
    else:
        ops = {'src': _n(gen, N, Lout, cin)}
    ops['dz'] = _n(gen, N, Lout, cout)
    return ops


def _ops_wu_in_wgrad(p, gen):
    return {'x': _n(gen, p['N'], p['L']), 'dz': _n(gen, p['N'], p['L'], 16)}


def _ops_wu_head_bwd(p, gen):
    N, L = p['N'], p['L']
    return {'dy': _n(gen, N, L), 'y': _tanh_like(gen, N, L), 'o': _n(gen, N, L, 16), 'x': _n(gen, N, L), 'w': _n(gen, 17)}


def _ops_wu_pack_frag(p, gen):
    return {'w': _n(gen, p['cout'], p['cin'], p['taps'])}


def _zz_params(variant, gen):
    ch = ZZ_CH[variant]
    ops = {}
    for i, c in enumerate(ch):
        ops[f'conv_layers.{i}.weight'] = _n(gen, c, 1 if i == 0 else ch[i - 1], 10).mul(0.1)
        ops[f'conv_layers.{i}.bias'] = _n(gen, c)
    ops.update({'fc1.weight': _n(gen, 1024, ch[-1]).mul(0.05), 'fc1.bias': _n(gen, 1024), 'fc2.weight': _n(gen, 1, 1024).mul(0.05),
                'fc2.bias': _n(gen, 1)})
    return ops


def _ops_zz_pack(p, gen):
    return _zz_params(p['variant'], gen)


def _sel(gen, shape, c):
    return _zz_pad(torch.randint(0, 3, shape, generator=gen, dtype=torch.uint8), c)


def _ops_zz_conv_wgrad(p, gen):
    v, l, N = p['variant'], p['layer'], p['N']
    ch, cp, lens = ZZ_CH[v], _zz_cpad(v), zz_lens(v, p['L'])
    last = l == len(ch) - 1
    return {'in': _zz_pad(_n(gen, N, lens[l], cp[l - 1]), ch[l - 1]),
            'dout': _n(gen, N, cp[l]) if last else _n(gen, N, lens[l + 1], cp[l]),
            'sel': _sel(gen, (N, lens[l + 1], cp[l]), ch[l])}


def _ops_zz_in_wgrad(p, gen):
    v, N, L = p['variant'], p['N'], p['L']
    lp, cp = zz_lens(v, L)[1], _zz_cpad(v)[0]
    return {'x': _n(gen, N, L), 'dout': _n(gen, N, lp, cp), 'sel': _sel(gen, (N, lp, cp), ZZ_CH[v][0])}


def _ops_ep_repack(p, gen):
    return {'w2': _n(gen, 32, 64, 3).mul(0.1), 'b2': _n(gen, 32), 'h1': _tanh_like(gen, p['N'], p['L'], 64)}


# ----------------------------------------------------------------------------------------------------------- the C ABI
class _Abi:
    """the library's entries by name: tensors as pointers, ctypes structures by reference, a status checked under the name"""

    def __init__(self, lib, dev):
        from stofnet_amd import _lib
        self._lib, self.lib, self.dev = _lib, lib, dev
        self.stream = _lib.stream_ptr(dev)

    def __call__(self, name, *args):
        conv = [self._lib.ptr(a) if isinstance(a, torch.Tensor) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a
                for a in args]
        fn = getattr(self.lib, name)
        out = fn(*conv)
        if fn.restype is ctypes.c_int:
            self._lib.check(out, name)
            return None
        return int(out)

    def nan(self, *shape, dtype=torch.float32):
        return torch.full(shape, float('nan'), dtype=dtype, device=self.dev)

    def ws(self, nbytes):
        assert nbytes > 0
        return torch.full((int(nbytes),), 0xff, dtype=torch.uint8, device=self.dev)

    def ptrs(self, tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _run_sn_bn(abi, p, d):
    from stofnet_amd import _lib
    ch, N, L = p['ch'], p['N'], p['L']
    desc = _lib.SincNetDesc(SN_FS, SN_EPS, 0, 0)
    ws = abi.ws(abi('stof_sincnet_train_stats_workspace_bytes'))
    stat, new_mean, new_var = abi.nan(4, ch, dtype=torch.float64), abi.nan(ch), abi.nan(ch)
    abi('stof_sincnet_train_stats', desc, d['z'], N, L, ch, d['gamma'], d['beta'], d['run_mean'], d['run_var'], SN_MOMENTUM, stat,
        new_mean, new_var, ws, ws.numel(), abi.stream)
    a = abi.nan(d['z'].numel())
    abi('stof_sincnet_train_apply', d['z'], N, L, ch, stat, a, abi.stream)
    dgamma, dbeta, dz = abi.nan(ch), abi.nan(ch), abi.nan(d['z'].numel())
    ws.fill_(0xff)
    abi('stof_sincnet_train_bn_bwd', d['da'], a if ch == C else None, d['z'], stat, d['gamma'], N, L, ch, dgamma, dbeta, dz, ws,
        ws.numel(), abi.stream)
    return {'stat': stat, 'new_mean': new_mean, 'new_var': new_var, 'apply': a, 'dgamma': dgamma, 'dbeta': dbeta, 'dz': dz}


def _run_wu_bn(abi, p, d):
    ch, rows = p['ch'], p['rows']
    ws = abi.ws(abi('stof_waveunet_train_stats_workspace_bytes'))
    stat, new_mean, new_var = abi.nan(4, ch, dtype=torch.float64), abi.nan(ch), abi.nan(ch)
    abi('stof_waveunet_train_stats', d['z'], rows, ch, d['gamma'], d['beta'], d['run_mean'], d['run_var'], WU_EPS, WU_MOMENTUM, stat,
        new_mean, new_var, ws, ws.numel(), abi.stream)
    a = abi.nan(rows, ch)
    abi('stof_waveunet_train_apply', d['z'], rows, ch, stat, a, abi.stream)
    dgamma, dbeta, dz = abi.nan(ch), abi.nan(ch), abi.nan(rows, ch)
    ws.fill_(0xff)
    abi('stof_waveunet_train_bn_bwd', d['da'], a, d['z'], stat, rows, ch, dgamma, dbeta, dz, ws, ws.numel(), abi.stream)
    return {'stat': stat, 'new_mean': new_mean, 'new_var': new_var, 'apply': a, 'dgamma': dgamma, 'dbeta': dbeta, 'dz': dz}


def _run_sn_conv_wgrad(abi, p, d):
    l = p['layer']
    ws = abi.ws(abi('stof_sincnet_train_conv_wgrad_workspace_bytes', l))
    dw, db = abi.nan(C, C, SN_TAPS[l]), abi.nan(C)
    abi('stof_sincnet_train_conv_wgrad', l, d['a_prev'], d['dz'], p['N'], p['L'], dw, db, ws, ws.numel(), abi.stream)
    return {'dw': dw, 'db': db}


def _run_sn_out_wgrad(abi, p, d):
    ws = abi.ws(abi('stof_sincnet_train_out_wgrad_workspace_bytes'))
    dw, db = abi.nan(1, C, 7), abi.nan(1)
    abi('stof_sincnet_train_out_wgrad', d['a2'], d['dz3'], p['N'], p['L'], dw, db, ws, ws.numel(), abi.stream)
    return {'dw': dw, 'db': db}


def _run_sn_bank_grad(abi, p, d):
    ws = abi.ws(abi('stof_sincnet_train_bank_grad_workspace_bytes'))
    G = abi.nan(C, SN_TAPS[0])
    abi('stof_sincnet_train_bank_grad', d['x'], d['dz0'], p['N'], p['L'], G, ws, ws.numel(), abi.stream)
    return {'G': G}


def _run_sn_pack(abi, p, d):
    from stofnet_amd import _lib
    desc = _lib.SincNetDesc(SN_FS, SN_EPS, 0, 0)
    lay = (ctypes.c_int64 * 6)()
    abi('stof_sincnet_train_blob_layout', lay)
    train = abi.ws(4 * int(lay[5]))
    abi('stof_sincnet_train_pack', desc, abi.ptrs([d['low_hz'], d['band_hz'], d['w1'], d['w2'], d['w3']]), train, train.numel(), abi.stream)
    order = ['low_hz', 'band_hz', 'w1', 'b1', 'w2', 'b2', 'w3', 'b3'] + [f'bn{l}_{k}' for l in range(4) for k in ('w', 'b', 'mean', 'var')]
    infer = abi.ws(abi('stof_sincnet_packed_bytes', desc))
    abi('stof_sincnet_device_pack', desc, abi.ptrs([d[k] for k in order]), infer, infer.numel(), abi.stream)
    out = {'train_blob': train, 'infer_blob': infer}
    for l in (1, 2):
        img = abi.nan(C * SN_TAPS[l] * C)
        abi('stof_sincnet_train_dgrad_image', l, d[f'w{l}'], img, abi.stream)
        out[f'dgrad_image{l}'] = img
    return out


def _run_wu_wgrad(abi, p, d):
    N, Lout, cin, cu, cout, taps, mode = (p[k] for k in ('N', 'Lout', 'cin', 'cu', 'cout', 'taps', 'mode'))
    ws = abi.ws(abi('stof_waveunet_train_wgrad_workspace_bytes', N, Lout, cin, cout, taps))
    dw, db = abi.nan(cout, cin, taps), abi.nan(cout)
    abi('stof_waveunet_train_wgrad', d['src'], d.get('low'), d['dz'], N, Lout, cin, cu, cout, taps, mode, dw, db, ws, ws.numel(), abi.stream)
    return {'dw': dw, 'db': db}


def _run_wu_in_wgrad(abi, p, d):
    ws = abi.ws(abi('stof_waveunet_train_in_wgrad_workspace_bytes'))
    dw, db = abi.nan(16, 1, 15), abi.nan(16)
    abi('stof_waveunet_train_in_wgrad', d['x'], d['dz'], p['N'], p['L'], dw, db, ws, ws.numel(), abi.stream)
    return {'dw': dw, 'db': db}


def _run_wu_head_bwd(abi, p, d):
    N, L = p['N'], p['L']
    ws = abi.ws(abi('stof_waveunet_train_head_bwd_workspace_bytes'))
    dout, dxh, dw, db = abi.nan(N, L, 16), abi.nan(N, L), abi.nan(17), abi.nan(1)
    abi('stof_waveunet_train_head_bwd', d['dy'], d['y'], d['o'], d['x'], N, L, d['w'], dout, dxh, dw, db, ws, ws.numel(), abi.stream)
    return {'da': dout, 'dxh': dxh, 'dw': dw, 'db': db}


def _run_wu_pack_frag(abi, p, d):
    out = {}
    for flip in (0, 1):
        img = abi.nan(abi('stof_waveunet_train_frag_floats', p['cin'], p['cout'], p['taps'], flip))
        abi('stof_waveunet_train_pack_frag', d['w'], p['cin'], p['cout'], p['taps'], flip, img, abi.stream)
        out[f'image_flip{flip}'] = img
    return out


def _run_zz_pack(abi, p, d):
    from stofnet_amd import _lib
    desc = _lib.ZonziniDesc(p['variant'], 0)
    blob = abi.ws(abi('stof_zonzini_packed_bytes', desc))
    abi('stof_zonzini_train_pack', desc, abi.ptrs(list(d.values())), blob, blob.numel(), abi.stream)
    out = {'blob': blob}
    for l in range(1, len(ZZ_CH[p['variant']])):
        img = abi.nan(abi('stof_zonzini_train_dgrad_image_floats', desc, l))
        abi('stof_zonzini_train_dgrad_image', desc, l, d[f'conv_layers.{l}.weight'], img, abi.stream)
        out[f'dgrad_image{l}'] = img
    return out


def _run_zz_conv_wgrad(abi, p, d):
    from stofnet_amd import _lib
    v, l = p['variant'], p['layer']
    desc = _lib.ZonziniDesc(v, 0)
    ws = abi.ws(abi('stof_zonzini_train_conv_wgrad_workspace_bytes', desc, l))
    dw, db = abi.nan(ZZ_CH[v][l], ZZ_CH[v][l - 1], 10), abi.nan(ZZ_CH[v][l])
    abi('stof_zonzini_train_conv_wgrad', desc, l, d['in'], d['dout'], d['sel'], dw, db, p['N'], p['L'], ws, ws.numel(), abi.stream)
    return {'dw': dw, 'db': db}


def _run_zz_in_wgrad(abi, p, d):
    from stofnet_amd import _lib
    v = p['variant']
    desc = _lib.ZonziniDesc(v, 0)
    ws = abi.ws(abi('stof_zonzini_train_in_wgrad_workspace_bytes', desc))
    dw, db = abi.nan(ZZ_CH[v][0], 1, 10), abi.nan(ZZ_CH[v][0])
    abi('stof_zonzini_train_in_wgrad', desc, d['x'], d['dout'], d['sel'], dw, db, p['N'], p['L'], ws, ws.numel(), abi.stream)
    return {'dw': dw, 'db': db}


def _run_ep_repack(abi, p, d):
    """ep_repack_kernel's image, and stof_train_espcn_mid, the entry that consumes it"""
    frag = abi.nan(abi('stof_train_espcn_repack_floats'))
    abi('stof_train_espcn_repack', d['w2'], frag, abi.stream)
    h2 = abi.nan(p['N'], p['L'], 32)
    abi('stof_train_espcn_mid', d['h1'], frag, d['b2'], h2, p['N'], p['L'], abi.stream)
    return {'frag2': frag, 'h2': h2}


FAMILIES = {
    'sn_bn': (_ops_sn_bn, _run_sn_bn), 'wu_bn': (_ops_wu_bn, _run_wu_bn),
    'sn_conv_wgrad': (_ops_sn_conv_wgrad, _run_sn_conv_wgrad), 'sn_out_wgrad': (_ops_sn_out_wgrad, _run_sn_out_wgrad),
    'sn_bank_grad': (_ops_sn_bank_grad, _run_sn_bank_grad), 'sn_pack': (_ops_sn_pack, _run_sn_pack),
    'wu_wgrad': (_ops_wu_wgrad, _run_wu_wgrad), 'wu_in_wgrad': (_ops_wu_in_wgrad, _run_wu_in_wgrad),
    'wu_head_bwd': (_ops_wu_head_bwd, _run_wu_head_bwd), 'wu_pack_frag': (_ops_wu_pack_frag, _run_wu_pack_frag),
    'zz_pack': (_ops_zz_pack, _run_zz_pack), 'zz_conv_wgrad': (_ops_zz_conv_wgrad, _run_zz_conv_wgrad),
    'zz_in_wgrad': (_ops_zz_in_wgrad, _run_zz_in_wgrad), 'ep_repack': (_ops_ep_repack, _run_ep_repack),
}


# --------------------------------------------------------------------------------------------------------------- cases
def _cases():
    out = []

    def add(family, **p):
        out.append((family + ''.join(f'_{k}{v}' for k, v in p.items()), family, p, 3100 + len(out)))

    rows = ((1, 2), (1, 255), (1, 256), (1, 257), (3, 171))
    for ch in (C, 1):
        for N, L in rows:
            add('sn_bn', ch=ch, N=N, L=L)
    add('sn_bn', ch=1, N=5, L=52829)                              # 264 145 rows: above 256 x 1024, 258 rows per partial
    for layer in (1, 2):
        for N, L in ((1, 63), (1, 64), (1, 65), (5, 1700)):       # 8 500 rows: above 64 x 64
            add('sn_conv_wgrad', layer=layer, N=N, L=L)
    for N, L in ((1, 255), (1, 257), (33, 2000)):                 # 66 000 rows: above 256 x 256
        add('sn_out_wgrad', N=N, L=L)
    for N, L in ((2, 127), (2, 129), (5, 1700)):                  # 5 x 14 = 70 tiles: above 64
        add('sn_bank_grad', N=N, L=L)
    add('sn_pack')
    for ch in (16, 80):                                           # 80: two 64-channel groups, the second partly empty
        for N, L in rows:
            add('wu_bn', ch=ch, rows=N * L)
    add('wu_bn', ch=16, rows=65837)                               # above 256 x 256: 258 rows per partial
    add('wu_wgrad', mode=0, N=2, Lout=3, cin=16, cu=0, cout=32, taps=15)
    add('wu_wgrad', mode=1, N=2, Lout=4, cin=32, cu=16, cout=16, taps=5)
    add('wu_wgrad', mode=2, N=2, Lout=3, cin=16, cu=0, cout=16, taps=15)
    add('wu_wgrad', mode=2, N=2, Lout=3, cin=16, cu=0, cout=16, taps=5)
    add('wu_wgrad', mode=2, N=3, Lout=2757, cin=16, cu=0, cout=16, taps=5)      # 3 x 44 = 132 tiles: above 128, 2 tiles per partial
    for N, L in ((1, 255), (1, 257), (3, 21947)):                 # 65 841 rows: above 256 x 256
        add('wu_in_wgrad', N=N, L=L)
        add('wu_head_bwd', N=N, L=L)
    for cin, cout, taps in ((16, 32, 15), (48, 16, 5), (208, 16, 5)):            # 208 crosses the 192-channel split of the image
        add('wu_pack_frag', cin=cin, cout=cout, taps=taps)
    for variant in (0, 1):
        add('zz_pack', variant=variant)
    for N, lp in ((1, 63), (1, 64), (1, 65), (3, 57), (74, 56)):  # 171 rows: three chunks; 4 144 rows: above 64 x 64
        add('zz_conv_wgrad', variant=0, layer=1, N=N, L=zz_length_for(lp, 2))
    add('zz_conv_wgrad', variant=1, layer=4, N=2, L=3752)         # pad channels, cout = 250 is no multiple of 32, the mean's gradient
    for N, lp in ((1, 255), (1, 257), (566, 232)):                # 131 312 rows: above 512 x 256
        add('zz_in_wgrad', variant=0, N=N, L=zz_length_for(lp, 1))
    add('ep_repack', N=2, L=37)
    return out


CASES = _cases()          # name, family, parameters, seed
IDS = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


def operands(c, seed=None):
    """the inputs of case `c` as CPU tensors, drawn in the family's order from one generator"""
    _, family, p, own = c
    return FAMILIES[family][0](p, torch.Generator().manual_seed(own if seed is None else seed))


def digest(ops):
    """SHA-256 over the operands' bytes, in order"""
    h = hashlib.sha256()
    for name, v in ops.items():
        h.update(name.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


def run(lib, dev, c, seed=None):
    """case `c` through the C ABI on `dev` -> {output name: numpy array}"""
    _, family, p, _ = c
    abi = _Abi(lib, dev)
    out = FAMILIES[family][1](abi, p, {k: v.to(dev) for k, v in operands(c, seed).items()})
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def stored_raw(v):
    return v.nbytes <= RAW_BYTES


def sha(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()

"""Inputs of the split-fp16 range-contract tests (CPU only: numpy / torch and the float64 oracle, no GPU import).

Rescaling by a power of two is exact in fp32.  Scale a producer layer's weight and bias by 2^k and its consumer's weight by
2^-k: leaky ReLU, ReLU and max-pool are positively homogeneous, so the network is the same function, and away from fp32's
own limits every fp32 rounding commutes with the scaling -- an fp32 route returns the SAME BITS.  Only the chosen interior
activation moves, by 2^k, into or out of the fp16 range.  Together with rows that are silent except for one short burst,
this puts an fp16 overflow at a known stage, on a known row, at a known sample, with an exactly known expected result: the
unscaled network's.

What the GPU tests rely on is asserted here in float64 (`check_case`), as conditions on the inputs, not as tolerances:
  overflowing case: on the targeted row and stage max|a| >= 2^17 (fp16 rounds to infinity from 65520 on); on every other
                    stage, and on every other row of the targeted stage, max|a| <= 2^14;
  safe case:        every stage <= 2^14 and the targeted stage's maximum >= 2^-3.
The factor of 8 on either side keeps any fp32 or split-fp16 rounding from moving a case across the line.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle import stofnet_oracle as so

SG = 'semi_global_block.'
OVERFLOW_MIN = 2.0 ** 17        # the targeted stage of an overflowing case reaches at least this
SAFE_MAX = 2.0 ** 14            # every other stage (every stage of a safe case) stays below this
SAFE_TARGET_MIN = 2.0 ** -3     # a safe case's targeted stage is at least this large: the rescaling did not empty it
ARGMAX_LEAD = 2.0 ** -10       # a safe case's row maximum leads the runner-up by this much of max|y| (100x the map tolerance)
BURST = np.array([1.0, -0.75, 0.5, 1.0, -0.25, 0.75, -1.0, 0.5])      # the burst's samples, times the row's amplitude

# name -> constructor geometry.  'fused' is the shipped network (the persistent sweep); each other one leaves the sweep by
# exactly one argument and runs layer by layer.
GEOMETRIES = {
    'fused': dict(num_features=64, body_kernel=7, semi_global_scale=80, num_blocks=13),
    'f32': dict(num_features=32, body_kernel=7, semi_global_scale=80, num_blocks=13),
    'k3': dict(num_features=64, body_kernel=3, semi_global_scale=80, num_blocks=13),
    's40': dict(num_features=64, body_kernel=7, semi_global_scale=40, num_blocks=13),
    'nb5': dict(num_features=64, body_kernel=7, semi_global_scale=80, num_blocks=5),
}
LAYERWISE = ('f32', 'k3', 's40', 'nb5')


def base_state_dict(geom: str, r: int, variant: str = 'plain') -> dict:
    """The unscaled network of geometry `geom`: seeded uniform parameters with PyTorch's default bounds (the fused geometry
    is `synth.synth_state_dict(r, seed=12)`, parameter for parameter).  variant 'neg<i>': conv<i>'s weight and bias replaced
    by minus their absolute values, so that a positive stream gives a NEGATIVE pre-activation in every channel and the hidden
    activation behind the leaky slope overflows on the negative side only.  That is another network, with its own
    unscaled result, not a rescaling."""
    g = GEOMETRIES[geom]
    nf, kb, sgs, nb = g['num_features'], g['body_kernel'], g['semi_global_scale'], g['num_blocks']
    rng = np.random.default_rng(12)
    sd = {}

    def conv(name, co, ci, k):
        bound = 1.0 / np.sqrt(ci * k)
        sd[name + '.weight'] = rng.uniform(-bound, bound, size=(co, ci, k)).astype(np.float32)
        sd[name + '.bias'] = rng.uniform(-bound, bound, size=(co,)).astype(np.float32)

    conv('conv1', nf, 1, 9)
    conv('conv_last', r, nf, 3)
    fs = max(1, sgs // 10)
    conv(SG + 'contract_conv', fs * nf, nf, 5)
    conv(SG + 'expand_conv', nf, fs * nf, 5)
    for i in range(2, nb):
        conv(f'conv{i}', nf, nf, kb)
    if variant != 'plain':
        assert variant.startswith('neg')
        name = 'conv' + variant[3:]
        sd[name + '.weight'] = -np.abs(sd[name + '.weight'])
        sd[name + '.bias'] = -np.abs(sd[name + '.bias'])
    return sd


def num_blocks_of(sd: dict) -> int:
    return 1 + max(int(k[4:-7]) for k in sd if k.startswith('conv') and k.endswith('.weight') and k[4:-7].isdigit())


def _scaled(sd, names, k):
    f = np.float32(2.0 ** k)
    out = dict(sd)
    for nm in names:
        out[nm] = (sd[nm] * f).astype(np.float32)
        assert np.array_equal(out[nm].astype(np.float64), sd[nm].astype(np.float64) * 2.0 ** k), f'{nm}: 2^{k} is not exact'
    return out


def pair(sd: dict, producer: str, consumer: str, k: int) -> dict:
    """Producer's weight and bias times 2^k, consumer's weight times 2^-k: the activation between them moves by 2^k."""
    return _scaled(_scaled(sd, [producer + '.weight', producer + '.bias'], k), [consumer + '.weight'], -k)


def stream_roles(nb: int):
    """Which layers write the residual stream (weight and bias times 2^k), which only add to it from the stream itself (bias
    times 2^k) and which read it (weight times 2^-k), for a network of `nb` blocks with the oracle's `residual_layers`."""
    residual_layers = list(range(3, nb - 1, 2)) + [nb - 1, nb]
    up_wb, up_b, down_w = ['conv1', SG + 'expand_conv'], [], [SG + 'contract_conv', 'conv_last']
    on_stream = True                                # is the running activation x the stream (or a hidden activation)?
    for i in range(2, nb - 1):
        if i in residual_layers:
            (up_b if on_stream else up_wb).append(f'conv{i}')
            on_stream = True
        else:
            if on_stream:
                down_w.append(f'conv{i}')
            on_stream = False
    (up_b if on_stream else up_wb).append(f'conv{nb - 1}')
    return up_wb, up_b, down_w


def stream(sd: dict, k: int) -> dict:
    """The whole residual stream times 2^k: conv1's output, x0, every res*, the input of conv_last."""
    up_wb, up_b, down_w = stream_roles(num_blocks_of(sd))
    out = _scaled(sd, [n + s for n in up_wb for s in ('.weight', '.bias')] + [n + '.bias' for n in up_b], k)
    return _scaled(out, [n + '.weight' for n in down_w], -k)


def rescale(sd: dict, spec: str, k: int) -> dict:
    """spec: 'hid<i>' = pair(conv<i>, conv<i+1>), 'sgb' = pair(contract_conv, expand_conv), 'stream'."""
    if spec == 'stream':
        return stream(sd, k)
    if spec == 'sgb':
        return pair(sd, SG + 'contract_conv', SG + 'expand_conv', k)
    i = int(spec[3:])
    return pair(sd, f'conv{i}', f'conv{i + 1}', k)


def gradient_law(sd: dict, spec: str, k: int) -> dict:
    """parameter name -> exponent e: the rescaled network's gradient is the unscaled one times 2^e (a parameter that was
    multiplied by 2^j has its gradient divided by 2^j; every other gradient is unchanged)."""
    law = {n: 0 for n in sd}
    if spec == 'stream':
        up_wb, up_b, down_w = stream_roles(num_blocks_of(sd))
        for n in up_wb:
            law[n + '.weight'] = law[n + '.bias'] = -k
        for n in up_b:
            law[n + '.bias'] = -k
        for n in down_w:
            law[n + '.weight'] = k
        return law
    prod, cons = ((SG + 'contract_conv', SG + 'expand_conv') if spec == 'sgb'
                  else (f'conv{int(spec[3:])}', f'conv{int(spec[3:]) + 1}'))
    law[prod + '.weight'] = law[prod + '.bias'] = -k
    law[cons + '.weight'] = k
    return law


def target_stage(spec: str) -> str:
    return {'stream': 'x0', 'sgb': 'sgb_pooled'}.get(spec, 'hidden' + spec[3:])


def moved_stages(spec: str, nb: int):
    """Every stage the rescaling `spec` moves by 2^k (the targeted one among them)."""
    if spec == 'stream':
        return ['conv1', 'sgb_expand', 'x0'] + [f'res{i}' for i in range(3, nb - 1, 2)] + [f'conv{nb - 1}']
    if spec == 'sgb':
        return ['sgb_contract', 'sgb_pooled']
    return ['hidden' + spec[3:]]


def burst_rows(n: int, L: int, pos, amp) -> np.ndarray:
    """[n, 1, L] float32: row i is silent except for `BURST` times amp[i] at samples pos[i] .. pos[i] + 7."""
    pos = np.broadcast_to(np.asarray(pos), (n,))
    amp = np.broadcast_to(np.asarray(amp, np.float64), (n,))
    x = np.zeros((n, 1, L), np.float32)
    for i in range(n):
        assert 0 <= pos[i] <= L - len(BURST)
        x[i, 0, pos[i]:pos[i] + len(BURST)] = (amp[i] * BURST).astype(np.float32)
    return x


def forward(sd, x, r, geom, dtype=torch.float64, conv=so.conv1d_shifted_matmul, taps=None):
    return so.stofnet_forward(sd, x, r, GEOMETRIES[geom]['semi_global_scale'], dtype, conv=conv, taps=taps)


def stages(sd: dict, x, r: int, geom: str) -> dict:
    """name -> float64 array [N, C, L'] of every activation a kernel may hand to a split-fp16 convolution: the oracle's taps
    plus the hidden activations behind the leaky ReLU, recomputed here from the taps on either side."""
    taps = {}
    forward(sd, x, r, geom, taps=taps)
    nb = num_blocks_of(sd)
    out = {'input': torch.from_numpy(np.asarray(x)).double()}
    out.update(taps)
    residual_layers = list(range(3, nb - 1, 2)) + [nb - 1, nb]
    cur = taps['x0']
    for i in range(2, nb - 1):
        if i in residual_layers:
            cur = taps[f'res{i}']
        else:
            w = torch.from_numpy(sd[f'conv{i}.weight']).double()
            b = torch.from_numpy(sd[f'conv{i}.bias']).double()
            cur = out[f'hidden{i}'] = F.leaky_relu(so.conv1d_shifted_matmul(cur, w, b, w.shape[-1] // 2), 0.01)
    return {k: v.numpy() for k, v in out.items()}


@dataclass(frozen=True)
class Case:
    geom: str
    spec: str               # the rescaling: 'hid2', 'hid10', 'sgb', 'stream'
    k: int
    where: str              # the burst's place: 'first', 'last', 'boundary', 'remainder', 'spread' (safe cases)
    L: int = 400
    n: int = 8
    r: int = 4
    row: int = 5            # the one row that carries the overflow (-1: a safe case)
    amp: float = 1.0        # its burst amplitude; every other row's is 1
    sign: int = 1           # which side of the targeted stage overflows (-1: the 'neg' network, behind the leaky slope)
    seg_policy: int = 0     # body-sweep segment policy of the fused route (2: two segments per row, boundary at L // 2)

    @property
    def overflows(self):
        return self.row >= 0

    @property
    def variant(self):
        return 'plain' if self.sign > 0 else 'neg' + self.spec[3:]

    @property
    def stage(self):
        return target_stage(self.spec)

    @property
    def pos(self):
        """First sample of the burst, per row."""
        w = len(BURST)
        if self.where == 'spread':                                  # safe cases: every row somewhere else
            return np.array([(37 * i) % (self.L - w + 1) for i in range(self.n)])
        p = {'first': 0, 'last': self.L - w,
             'boundary': self.L // 2 - w // 2,                      # across the boundary of two segments of L // 2 rows
             # L = 200, scale 80: two pooling windows [0, 160), the remainder 160..199 is dropped by the pool, and the
             # up-sampled map covers 20..179 -- the burst sits where the SemiGlobalBlock neither reads nor writes
             'remainder': self.L - 16}[self.where]
        return np.full(self.n, p)

    @property
    def id(self):
        sgn = '' if self.sign > 0 else 'neg'
        tail = f'-n{self.n}' if self.n != 8 else ''
        tail += f'-r{self.r}' if self.r != 4 else ''
        return f'{self.geom}-{self.stage}{sgn}-k{self.k}-{self.where}@{int(self.pos[max(self.row, 0)])}of{self.L}{tail}'

    def x(self):
        amp = np.ones(self.n) if self.overflows else np.full(self.n, self.amp)      # safe cases: every row alike
        if self.overflows:
            amp[self.row] = self.amp
        return burst_rows(self.n, self.L, self.pos, amp)

    def base(self):
        return base_state_dict(self.geom, self.r, self.variant)

    def scaled(self):
        return rescale(self.base(), self.spec, self.k)


def check_case(c: Case) -> dict:
    """Assert the case's stage conditions in float64 on the RESCALED network; returns stage -> per-row max|a|."""
    st = stages(c.scaled(), c.x(), c.r, c.geom)
    nb = GEOMETRIES[c.geom]['num_blocks']
    rowmax = {s: np.abs(a).reshape(a.shape[0], -1).max(1) for s, a in st.items()}
    moved = moved_stages(c.spec, nb)
    assert c.stage in st, f'{c.id}: no stage {c.stage}'
    if not c.overflows:
        for s, m in rowmax.items():
            assert m.max() <= SAFE_MAX, f'{c.id}: safe case, stage {s} reaches {m.max():.4g}'
        assert rowmax[c.stage].max() >= SAFE_TARGET_MIN, f'{c.id}: targeted stage only {rowmax[c.stage].max():.4g}'
        # the GPU test compares arg-max indices: every row's maximum leads the runner-up by far more than the map tolerance
        y = so.sample_shuffle(torch.from_numpy(st['conv_last']), c.r).numpy()[:, 0]
        top = np.sort(y, axis=-1)[:, -2:]
        assert (top[:, 1] - top[:, 0]).min() >= ARGMAX_LEAD * np.abs(y).max(), \
            f'{c.id}: a row maximum leads by only {(top[:, 1] - top[:, 0]).min() / np.abs(y).max():.3g} of max|y|'
        return rowmax
    a = st[c.stage][c.row]
    hit = (a.max() if c.sign > 0 else -a.min())
    assert hit >= OVERFLOW_MIN, f'{c.id}: targeted stage reaches only {hit:.4g} on row {c.row}'
    if c.sign < 0:      # the negative case overflows behind the leaky slope only
        assert a.max() <= SAFE_MAX, f'{c.id}: positive side of {c.stage} reaches {a.max():.4g}'
    if c.spec != 'sgb' and c.where in ('first', 'last', 'boundary', 'remainder'):
        # the overflow sits where the burst is (a pooled sample stands for a whole window, so not asked of 'sgb')
        at = int(np.abs(a).max(0).argmax())
        assert c.pos[c.row] - 40 <= at <= c.pos[c.row] + len(BURST) + 40, f'{c.id}: peak of {c.stage} at {at}'
    others = np.arange(c.n) != c.row
    for s, m in rowmax.items():
        if s in moved:          # moved with the target by the same 2^k: bounded on the rows that must not overflow
            if others.any():
                assert m[others].max() <= SAFE_MAX, f'{c.id}: stage {s} reaches {m[others].max():.4g} on another row'
        else:
            assert m.max() <= SAFE_MAX, f'{c.id}: stage {s} reaches {m.max():.4g}'
    return rowmax


# ---- the declared cases ---------------------------------------------------------------------------------------------
# One burst amplitude and one k per targeted stage, from the unscaled stage maxima of these networks (float64 oracle; a
# burst of amplitude 1 gives hidden ~ 0.4 .. 0.8, pooled ~ 0.5 .. 0.7, stream ~ 1.1 .. 1.8; the leaky side of the 'neg'
# network ~ 0.02; everything is linear in the amplitude up to the biases): the loud row lands >= 2^17, the others <= 2^14.
LOUD = 128.0
OVERFLOW_SPECS = [('hid2', 1, 12), ('hid2', -1, 17), ('hid10', 1, 12), ('sgb', 1, 12), ('stream', 1, 11)]


def _overflow_cases():
    out = []
    for spec, sign, k in OVERFLOW_SPECS:
        for where in ('first', 'last', 'boundary', 'remainder'):
            if where == 'remainder' and spec == 'sgb':
                continue        # a burst the pool drops never reaches the expand conv's split: nothing overflows
            out.append(Case('fused', spec, k, where, L=200 if where == 'remainder' else 400, amp=LOUD, sign=sign,
                            seg_policy=2 if where == 'boundary' else 0))
    out.append(Case('fused', 'stream', 11, 'first', r=10, amp=LOUD))                        # conv_last's other epilogue
    out.append(Case('fused', 'hid2', 12, 'last', r=20, amp=LOUD))                           # conv_last_wide
    out.append(Case('fused', 'hid10', 12, 'boundary', n=300, row=217, amp=LOUD))            # more than one work-group
    for geom in LAYERWISE:
        for spec, sign, k in OVERFLOW_SPECS:
            if spec == 'hid10':
                continue
            for where in ('first', 'last', 'boundary'):
                out.append(Case(geom, spec, k, where, amp=LOUD, sign=sign))
    out.append(Case('k3', 'stream', 11, 'remainder', L=200, amp=LOUD))
    return out


def _safe_cases():
    out = []
    for n, L in ((1, 96), (5, 160), (3, 200)):
        for spec in ('hid2', 'hid10', 'sgb', 'stream'):
            for k in (-3, 3):
                out.append(Case('fused', spec, k, 'spread', L=L, n=n, row=-1, amp=8.0))
    out.append(Case('fused', 'stream', 3, 'spread', n=300, row=-1, amp=8.0))
    out.append(Case('fused', 'hid2', -3, 'spread', n=300, row=-1, amp=8.0))
    return out


OVERFLOW_CASES = _overflow_cases()
SAFE_CASES = _safe_cases()
# training: [4, 1, 400], r = 4, one interior overflow behind the leaky ReLU and one on the stream
TRAIN_OVERFLOW_CASES = [Case('fused', 'hid2', 12, 'boundary', n=4, row=2, amp=LOUD),
                        Case('fused', 'stream', 11, 'first', n=4, row=2, amp=LOUD)]
EXACT_KS = (-12, -3, 3, 12, 20)
EXACT_SPECS = {'fused': ('hid2', 'hid10', 'sgb', 'stream'), 'f32': ('hid2', 'hid10', 'sgb', 'stream'),
               'k3': ('hid2', 'hid10', 'sgb', 'stream'), 's40': ('hid2', 'hid10', 'sgb', 'stream'),
               'nb5': ('hid2', 'sgb', 'stream')}


def exact_input(n=8, L=400):
    """In-range rows for the fp32 invariance checks: a burst per row, every row somewhere else, amplitudes 1 .. 8."""
    return burst_rows(n, L, [(53 * i) % (L - len(BURST) + 1) for i in range(n)], 1.0 + np.arange(n) % 8)

"""Cases of the bit fixture of the training ends (tests/golden/f28_train_ends_bits.npz), shared by its recorder
(tests/golden/make_golden_train_ends.py) and the tests.  The fixture holds what the C ABI entry points of csrc/train_ends.h and
csrc/wgrad_reduce.h's users wrote, bit for bit, on seeded Gaussian operands; the operands themselves are regenerated from
the seed on the CPU (`operands`), the manifest keeps their SHA-256.

Shapes (N, L), rows = N L flat over the batch:
  1x1      every tap but the centre leaves the waveform
  2x2      halos longer than the row
  3x37     111 rows: row ends inside a 16-row pass, inside a 64-row tile and across waveforms
  5x103    515 rows: three 256-row chunks with a 3-row tail (three partials: the reduce's tail loop alone, like one partial)
  4x4100   16 400 rows, 65 partials: the reduce's four-chain loop and its tail.  Weight gradients only.
The forward activations ([rows][64] floats, 129 KiB at 5x103) are stored up to 3x37 only: the forward kernels work in 64-row
tiles without a chunk loop, and 111 rows already make a whole tile and a partial one.  The conv3 gradients of r = 33 and 64
(12 and 24 KiB each) are stored at two shapes each, which together see 1, 3 and 65 partials.
"""
import hashlib

import torch

SHAPES = {'1x1': (1, 1), '2x2': (2, 2), '3x37': (3, 37), '5x103': (5, 103), '4x4100': (4, 4100)}
SMALL, BIG = ('1x1', '2x2', '3x37', '5x103'), '4x4100'
OUT_SCALE = 0.37


def _act(c):
    return lambda N, L, p: (N, L, c)


def _vec(N, L, p):
    return (N, L)


# entry -> inputs [(name, shape(N, L, p), kind)], outputs [(name, shape)], arguments in the order of the C ABI.  Kinds: 'n' normal,
# 'g2' a normal or a NULL pointer (parameter g2), and the saved activations, made from a normal v with correctly rounded
# operations only, so that every machine draws the same bits (torch.tanh and torch.sigmoid on the CPU do not promise that):
# 'relu' max(v, 0), 'tanh' 0.6 v clamped to +-0.999 (the range of a tanh), 'sigmoid' 0.5 + 0.2 v clamped to 0.001 .. 0.999.
SAVED = {'relu': torch.relu, 'tanh': lambda v: v.mul(0.6).clamp(-0.999, 0.999), 'sigmoid': lambda v: v.mul(0.2).add(0.5).clamp(0.001, 0.999)}
ENTRIES = {
    'edsr_in': dict(ins=[('x', _vec, 'n'), ('w', (64, 1, 3), 'n'), ('b', (64,), 'n')], outs=[('y', _act(64))],
                    args='x w b y N L'),
    'edsr_in_wgrad': dict(ins=[('x', _vec, 'n'), ('g', _act(64), 'n'), ('g2', _act(64), 'g2'), ('saved', _act(64), 'relu')],
                          outs=[('dw', (64, 1, 3)), ('db', (64,))], args='x g g2 saved dw db N L scale ws'),
    'edsr_in_dgrad': dict(ins=[('g', _act(64), 'n'), ('g2', _act(64), 'g2'), ('saved', _act(64), 'relu'), ('w', (64, 1, 3), 'n')],
                          outs=[('dx', _vec)], args='g g2 saved w dx N L scale'),
    'edsr_out_wgrad': dict(ins=[('trunk', _act(64), 'n'), ('dy', lambda N, L, p: (N, L * p['r']), 'n')],
                           outs=[('dw', lambda N, L, p: (1, 64 // p['r'], 3)), ('db', (1,))], args='trunk dy dw db N L r scale ws'),
    'espcn_in': dict(ins=[('x', _vec, 'n'), ('w', (64, 1, 5), 'n'), ('b', (64,), 'n')], outs=[('h1', _act(64))],
                     args='x w b h1 N L'),
    'espcn_in_wgrad': dict(ins=[('x', _vec, 'n'), ('g1', _act(64), 'n'), ('h1', _act(64), 'tanh')],
                           outs=[('dw', (64, 1, 5)), ('db', (64,))], args='x g1 h1 dw db N L scale ws'),
    'espcn_in_dgrad': dict(ins=[('g1', _act(64), 'n'), ('h1', _act(64), 'tanh'), ('w', (64, 1, 5), 'n')], outs=[('dx', _vec)],
                           args='g1 h1 w dx N L scale'),
    'espcn_out_wgrad': dict(ins=[('h2', _act(32), 'tanh'), ('y', lambda N, L, p: (N, L * p['r']), 'sigmoid'),
                                 ('dy', lambda N, L, p: (N, L * p['r']), 'n')],
                            outs=[('dw', lambda N, L, p: (p['r'], 32, 3)), ('db', lambda N, L, p: (p['r'],))],
                            args='h2 y dy dw db N L r scale ws'),
    'conv1_wgrad': dict(ins=[('x', _vec, 'n'), ('g', _act(64), 'n'), ('saved', _act(64), 'relu')],
                        outs=[('dw', (64, 1, 9)), ('db', (64,))], args='x g saved dw db N L scale ws'),
    'conv1_c_wgrad': dict(ins=[('x', lambda N, L, p: (N, p['Cin'], L), 'n'), ('g', lambda N, L, p: (N, L, p['F']), 'n'),
                               ('saved', lambda N, L, p: (N, L, p['F']), 'relu')],
                          outs=[('dw', lambda N, L, p: (p['F'], p['Cin'], 9)), ('db', lambda N, L, p: (p['F'],))],
                          args='x g saved dw db N Cin L F scale ws'),
}


def _cases():
    out = []

    def add(entry, shapes, **p):
        for sh in shapes:
            tag = ''.join(f'_{k}{v}' for k, v in p.items())
            out.append((f'{entry}{tag}_{sh}', entry, sh, p, 2800 + len(out)))

    every = SMALL + (BIG,)
    add('edsr_in', SMALL[:3])
    add('espcn_in', SMALL[:3])
    for g2 in (1, 0):
        add('edsr_in_wgrad', every, g2=g2)
        add('edsr_in_dgrad', SMALL, g2=g2)
    add('espcn_in_wgrad', every)
    add('espcn_in_dgrad', SMALL)
    for r in (1, 4, 64):
        add('edsr_out_wgrad', every, r=r)
    for r in (1, 3):                                   # r = 3: the j slots round up to 4
        add('espcn_out_wgrad', every, r=r)
    add('espcn_out_wgrad', ('3x37', '5x103'), r=33)    # the second j slot
    add('espcn_out_wgrad', ('2x2', BIG), r=64)
    add('conv1_wgrad', every)
    add('conv1_c_wgrad', every, Cin=1, F=64)
    add('conv1_c_wgrad', ('2x2', '5x103', BIG), Cin=3, F=96)      # unused bias slots, a partial channel tile
    add('conv1_c_wgrad', ('5x103',), Cin=3, F=64)
    add('conv1_c_wgrad', ('5x103',), Cin=1, F=96)
    return out


CASES = _cases()          # name, entry, shape key, parameters, seed
IDS = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


def _shape(s, N, L, p):
    return tuple(s(N, L, p)) if callable(s) else tuple(s)


def operands(c, seed=None):
    """the inputs of case `c` as CPU float32 tensors (None for a NULL pointer), drawn in the entry's order from one generator"""
    _, entry, sh, p, own = c
    N, L = SHAPES[sh]
    gen = torch.Generator().manual_seed(own if seed is None else seed)
    ops = {}
    for name, s, kind in ENTRIES[entry]['ins']:
        if kind == 'g2' and not p['g2']:
            ops[name] = None
            continue
        v = torch.randn(_shape(s, N, L, p), generator=gen, dtype=torch.float32)
        ops[name] = SAVED[kind](v) if kind in SAVED else v
    return ops


def digest(ops):
    """SHA-256 over the operands' bytes, in order"""
    h = hashlib.sha256()
    for name, v in ops.items():
        h.update(name.encode())
        h.update(b'\0' if v is None else v.numpy().tobytes())
    return h.hexdigest()


def run(lib, dev, c, seed=None):
    """case `c` through the C ABI on `dev` -> {output name: numpy array}.  Outputs start as NaN and the workspace as 0xff
    bytes, so a float that is read or returned must have been written."""
    from stofnet_amd import _lib
    _, entry, sh, p, _ = c
    N, L = SHAPES[sh]
    spec = ENTRIES[entry]
    ops = {k: None if v is None else v.to(dev) for k, v in operands(c, seed).items()}
    outs = {name: torch.full(_shape(s, N, L, p), float('nan'), device=dev) for name, s in spec['outs']}
    fn = getattr(lib, 'stof_train_' + entry)
    args = []
    for a in spec['args'].split():
        if a == 'ws':
            nbytes = getattr(lib, f'stof_train_{entry}_workspace_bytes')(*[p[k] for k in ('Cin', 'F', 'r') if k in p])
            assert nbytes > 0, (entry, p)
            ws = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
            args += [_lib.ptr(ws), nbytes]
        elif a in ('N', 'L'):
            args.append(N if a == 'N' else L)
        elif a == 'scale':
            args.append(OUT_SCALE)
        elif a in p and a != 'g2':
            args.append(p[a])
        else:
            args.append(_lib.ptr(ops[a] if a in ops else outs[a]))
    _lib.check(fn(*args, _lib.stream_ptr(dev)), entry)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in outs.items()}

"""Seeded geometries and signals of the beamformer tests (tests/golden/make_golden_beamform.py, test_beamform_cpu.py,
test_gpu_beamform.py).  Nothing here is stored: a case is regenerated from its seed.

Geometry of every case: lambda pitch (c = 1540 m/s, f0 = 5 MHz), fs = 20 MHz, t0 = 2 us, depths from 0.05 mm to 1.3 x the
recorded depth (so sample indices fall below 1, above S - 1 and in between), lateral positions a little wider than the
aperture (so some pixels lie outside every receive cone), angles within +-5 degrees including 0.
Signals are normal deviates rounded to float32 first: 32-bit and 64-bit code see the same values."""
import numpy as np

C, F0, FS, T0 = 1540.0, 5e6, 20e6, 2e-6
LAM = C / F0
FNUMBER = 1.9
KINDS = ('real', 'cplx')
DTYPES = {('real', 32): np.float32, ('real', 64): np.float64, ('cplx', 32): np.complex64, ('cplx', 64): np.complex128}

#        name        Ne  Nx  Nz   A   S   seed  frames  kinds            planes (compound_opt=False stored too)
CASES = {
    'c8':      dict(Ne=8, Nx=7, Nz=13, A=3, S=96, seed=11, frames=1, kinds=KINDS, planes=True),
    'c12':     dict(Ne=12, Nx=5, Nz=9, A=1, S=64, seed=12, frames=1, kinds=KINDS, planes=True),
    'c65':     dict(Ne=65, Nx=6, Nz=67, A=2, S=160, seed=13, frames=1, kinds=KINDS, planes=True),
    'c128':    dict(Ne=128, Nx=9, Nz=130, A=3, S=256, seed=14, frames=1, kinds=KINDS, planes=True),
    'ne1':     dict(Ne=1, Nx=5, Nz=11, A=3, S=96, seed=15, frames=1, kinds=KINDS, planes=True),          # W = 0
    'a5':      dict(Ne=8, Nx=7, Nz=13, A=5, S=96, seed=16, frames=1, kinds=KINDS, planes=False),
    'realch':  dict(Ne=8, Nx=7, Nz=13, A=3, S=96, seed=17, frames=1, kinds=('cplx',), planes=False),     # channels 0..2 purely real
    'batch5':  dict(Ne=65, Nx=6, Nz=67, A=2, S=160, seed=18, frames=5, kinds=KINDS, planes=False),
}
BIG = dict(Ne=16, Nx=300, Nz=300, A=2, S=128, seed=19, frames=1, kinds=KINDS, planes=False)    # stored as every 53rd pixel + the sum
BIG_STEP = 53
SCATTER_OF = 'c8'           # its pixel list, permuted, through bf_das_rx as 2-D arrays, angle SCATTER_ANGLE
SCATTER_ANGLE = 2
SCATTER_SEED = 21


def angles(A):
    if A == 1:
        return np.array([0.0])
    if A == 2:
        return np.deg2rad(np.array([0.0, 5.0]))
    return np.deg2rad(np.linspace(-5.0, 5.0, A))


def param(case):
    """The plain dict a caller hands to bf_das."""
    Ne, S = case['Ne'], case['S']
    xe = (np.arange(Ne) - (Ne - 1) / 2) * LAM
    half = 0.6 * max(xe[-1] - xe[0], 4 * LAM)
    depth = (T0 + S / FS) * C / 2
    return {'param_x': np.linspace(-half, half, case['Nx']), 'param_z': np.linspace(0.05e-3, 1.3 * depth, case['Nz']),
            'angles_list': angles(case['A']), 'xe': xe, 'Nelements': Ne, 'c': C, 't0': T0, 'fs': FS, 'f0': F0}


def signal(name, case, kind, bits):
    """[A, S, Ne] ([frames, A, S, Ne] for a batch) of DTYPES[kind, bits]; the values are float32 numbers at either width."""
    rng = np.random.default_rng(case['seed'])
    shape = ((case['frames'],) if case['frames'] > 1 else ()) + (case['A'], case['S'], case['Ne'])
    re = (100 * rng.standard_normal(shape)).astype(np.float32)
    im = (100 * rng.standard_normal(shape)).astype(np.float32)
    if kind == 'real':
        return re.astype(DTYPES[kind, bits])
    if name == 'realch':
        im[..., :3] = 0
    return (re.astype(np.float64) + 1j * im.astype(np.float64)).astype(DTYPES[kind, bits])


def pixel_list(p):
    """(x, z) flat in the reference's order, p = ix Nz + iz."""
    x, z = np.meshgrid(p['param_x'], p['param_z'])
    return x.T.flatten(), z.T.flatten()


def scatter_grids():
    """The SCATTER_OF pixel list in a seeded permutation, as 2-D arrays [Nz, Nx], and the permutation."""
    case = CASES[SCATTER_OF]
    x, z = pixel_list(param(case))
    perm = np.random.default_rng(SCATTER_SEED).permutation(x.size)
    shape = (case['Nx'], case['Nz'])
    return x[perm].reshape(shape).T.copy(), z[perm].reshape(shape).T.copy(), perm       # .T.flatten() gives x[perm]


def tx_distance_numpy(xe, theta, x, z):
    """The transmit distance as a numpy expression (virtual source behind the aperture), in double."""
    beta = 1e-8
    width = xe[-1] - xe[0]
    v0 = -width * np.cos(theta) * np.sin(theta) / beta
    v1 = -width * np.cos(theta) ** 2 / beta
    return np.hypot(x - v0, z - v1) - np.hypot((abs(v0) - width / 2) * (abs(v0) > width / 2), v1)


def sample_indices(p, x, z):
    """i [A, P, Ne] and the cone margin z / fnumber / 2 - |x - xe| [P, Ne], in double."""
    xe = p['xe']
    dtx = np.stack([tx_distance_numpy(xe, t, x, z) for t in p['angles_list']])
    drx = np.hypot(x[:, None] - xe[None, :], z[:, None])
    i = ((dtx[:, :, None] + drx[None]) / p['c'] - p['t0']) * p['fs']
    return i, z[:, None] / FNUMBER / 2 - abs(x[:, None] - xe[None, :])

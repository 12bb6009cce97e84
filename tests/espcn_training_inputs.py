"""Cases of the ESPCN_1D training fixture (tests/golden/f27_espcn_training.npz), shared by its generator
(tests/golden/make_golden_espcn_training.py) and the tests, so that the fixture stores seeds and results only: the frames come
from riders_inputs.frames, the weights from riders_inputs.weights (shipped checkpoints or riders_inputs.seeded_espcn), the
cotangent t of loss = sum(y * t) from `cotangent`.

Per case the fixture holds y, dx and all six parameter gradients in full (`<name>.grad.<p>`; at most 6144 floats each).

`CASES` lists the input seeds the fixture was made with (the generator asserts, and stores them as `<name>.seed`).  The
`seeded_r4_1x*` cases put the end of the only waveform one row before, on and one row after the 64-, 128- and 256-row tiles
of the kernels of csrc/espcn_train.hip (rows are flat over the batch there, so with N = 1 the row count is L)."""
import numpy as np

TILES = (64, 128, 256)      # rows per work-group: ep_in / ep_out_dgrad (and the LDS stage of ep_out_wgrad); ep_mid; the
#                             weight-gradient chunk and ep_in_dgrad

# name, weights (a checkpoint key, or an int = the seed of seeded weights), r, N, L, input seed
CASES = ([('puddle_r4_2x130', 'vital-puddle', 4, 2, 130, 5400),
          ('sponge_r4_2x130', 'wobbly-sponge', 4, 2, 130, 5401),
          ('seeded_r1_3x65', 720, 1, 3, 65, 5402),
          ('seeded_r2_2x96', 721, 2, 2, 96, 5403),
          ('seeded_r3_2x31', 722, 3, 2, 31, 5404),
          ('seeded_r10_2x40', 723, 10, 2, 40, 5405),
          ('seeded_r17_2x1', 724, 17, 2, 1, 5406),
          ('seeded_r33_1x2', 725, 33, 1, 2, 5407),
          ('seeded_r64_3x127', 726, 64, 3, 127, 5408),
          ('seeded_r4_3x257', 727, 4, 3, 257, 5409)]      # 771 rows: across the 256-row chunks of the weight-gradient kernels
         + [(f'seeded_r4_1x{L}', 728 + i, 4, 1, L, 5410 + i)
            for i, L in enumerate(v for tile in TILES for v in (tile - 1, tile, tile + 1))])
IDS = [c[0] for c in CASES]
PARAMS = ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias']      # state_dict order


def case(name):
    return next(c for c in CASES if c[0] == name)


def cotangent(n, m, seed):
    """t [n, 1, m] float32 of loss = sum(y * t)"""
    return np.random.default_rng(seed + 90000).standard_normal((n, 1, m)).astype(np.float32)

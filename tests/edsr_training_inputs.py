"""Cases of the EDSR_1D training fixture (tests/golden/f26_edsr_training.npz), shared by its generator
(tests/golden/make_golden_edsr_training.py) and the tests, so that the fixture stores seeds and results only: the frames come
from riders_inputs.frames, the seeded weights from riders_inputs.seeded_edsr, the cotangent t of loss = sum(y * t) from
`cotangent`.

Per case the fixture holds y, dx and a record of EVERY parameter gradient.  Those named by `kept_grads` are stored in full
(`<name>.grad.<p>`): every bias, conv_input, conv_output and conv_mid, the first block's conv1 (the far end of the backward
chain) and, where `last_conv2` is set, the last block's conv2.  Each other 64 x 64 x 3 body weight gradient is stored as
f8_training_c5 stores its large tensors: `<name>.gmax.<p>` = max |grad|, `<name>.gsum.<p>` = the float64 sum of the whole
tensor and `<name>.grad_stride53.<p>` = every 53rd element of the flattened tensor (`sampled_grads`).  All of them in full
would be 2.2 MB; like the fixtures f17 .. f25 this one stays below 1 MiB.

`CASES` lists the input seeds the fixture was made with (the generator asserts, and stores them as `<name>.seed`)."""
import numpy as np

# name, weights (a checkpoint key, or an int = the seed of seeded weights), num_blocks, r, N, L, input seed, last_conv2
CASES = [('cherry_b8_r4_2x130', 'proud-cherry', 8, 4, 2, 130, 5300, True),
         ('seeded_b0_r1_3x65', 620, 0, 1, 3, 65, 7301, False),
         ('seeded_b1_r2_2x96', 621, 1, 2, 2, 96, 5302, True),
         ('seeded_b2_r16_2x31', 622, 2, 16, 2, 31, 5303, True),
         ('seeded_b1_r64_2x40', 623, 1, 64, 2, 40, 9304, True),
         ('seeded_b3_r8_2x1', 624, 3, 8, 2, 1, 5305, True),
         ('seeded_b2_r4_1x2', 625, 2, 4, 1, 2, 6306, True),
         ('seeded_b1_r4_3x171', 626, 1, 4, 3, 171, 7307, True)]      # 513 rows: across the 64- and 128-row tiles of the body kernels
IDS = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


def cotangent(n, m, seed):
    """t [n, 1, m] float32 of loss = sum(y * t)"""
    return np.random.default_rng(seed + 90000).standard_normal((n, 1, m)).astype(np.float32)


def param_names(num_blocks):
    """state_dict order of EDSR_1D"""
    layers = (['conv_input'] + [f'residual_blocks.{b}.conv{j}' for b in range(num_blocks) for j in (1, 2)]
              + ['conv_mid', 'conv_output'])
    return [f'{nm}.{k}' for nm in layers for k in ('weight', 'bias')]


STRIDE = 53


def sampled_grads(num_blocks, last_conv2):
    """the parameters whose gradient the fixture holds as (gmax, gsum, every STRIDE-th element)"""
    keep = set(kept_grads(num_blocks, last_conv2))
    return [n for n in param_names(num_blocks) if n not in keep]


def kept_grads(num_blocks, last_conv2):
    """the parameters whose gradient the fixture holds in full"""
    keep = [n for n in param_names(num_blocks) if n.endswith('.bias')]
    keep += ['conv_input.weight', 'conv_output.weight', 'conv_mid.weight']
    if num_blocks:
        keep.append('residual_blocks.0.conv1.weight')
        if last_conv2:
            keep.append(f'residual_blocks.{num_blocks - 1}.conv2.weight')
    return keep

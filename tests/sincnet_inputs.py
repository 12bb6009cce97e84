"""Seeded inputs and weights of the SincNet fixture (tests/golden/f19_sincnet.npz), shared by its generator
(tests/golden/make_golden_sincnet.py) and the tests, so that the fixture stores seeds and outputs only.

The two shipped checkpoints are 1.3 MB of incompressible fp32 each, almost all of it the two 128 x 128 conv matrices.
tests/golden/sincnet_ckpt_parts.npz keeps every other state_dict entry of each checkpoint exactly (the learned sinc
bands, biases, BatchNorm statistics, conv.3) plus the per-output-channel RMS of conv.1 / conv.2 weight;
`checkpoint_weights` regenerates those two matrices from a seed at that scale.  The result has the checkpoint's names,
shapes, dtypes and learned filter bank, and is what the fixture's reference outputs were computed with."""
import os

import numpy as np

from stofnet_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PARTS = 'sincnet_ckpt_parts'
SEEDED = ('conv.1.weight', 'conv.2.weight')
CKPT_SEEDS = {'pretty-brook': 4421, 'noble-monkey': 4422}

CHECKPOINTS = {'pretty-brook': 'pretty-brook-1442_rf-scale10_epoch_42.pth',
               'noble-monkey': 'noble-monkey-1550_rf-scale20_epoch_28.pth'}

# name, weights ('pretty-brook' | 'noble-monkey' | 'init'), fs, input shape, input seed, stored-row step: the whole
# batch runs, the fixture keeps rows 0, step, 2 step, ... of the output (rows are independent)
CASES = [('chirp', 'pretty-brook', 1e6, (64, 1, 2000), 3101, 4),
         ('pala', 'noble-monkey', 1.25e9, (32, 1, 1536), 3102, 4),
         ('clamp', 'pretty-brook', 2e5, (8, 1, 2000), 3103, 2),
         ('init', 'init', 1e6, (8, 1, 2000), 3104, 2),
         ('odd', 'pretty-brook', 1e6, (8, 1, 2001), 3105, 2),
         ('long', 'noble-monkey', 1.25e9, (4, 1, 20000), 3106, 2),
         ('tiny1', 'pretty-brook', 1e6, (4, 1, 1), 3107, 1),
         ('tiny7', 'pretty-brook', 1e6, (4, 1, 7), 3108, 1),
         ('flat', 'pretty-brook', 1e6, (3, 2000), 3109, 1)]
BANK_CASES = ('chirp', 'clamp', 'init')        # cases whose filter bank (conv[0].filters) is stored
BANK_STEP = 8                                  # ... for filters 0, 8, 16, ..., taps 0..511 (the left half and the centre)
LAYER_CASE = 'chirp'                           # row 0 of this case: act[0..2] outputs, samples 0..63 and L-64..L-1
LAYER_EDGE = 64
INIT_WSEED = 77


def options(fs, input_dim):
    """The option dict of main.py:145-157."""
    return {'input_dim': input_dim, 'fs': fs, 'cnn_N_filt': [128, 128, 128, 1], 'cnn_len_filt': [1023, 11, 9, 7],
            'cnn_max_pool_len': [1, 1, 1, 1], 'cnn_use_laynorm_inp': False, 'cnn_use_batchnorm_inp': False,
            'cnn_use_laynorm': [False, False, False, False], 'cnn_use_batchnorm': [True, True, True, True],
            'cnn_act': ['leaky_relu', 'leaky_relu', 'leaky_relu', 'linear'], 'cnn_drop': [0.0, 0.0, 0.0, 0.0],
            'use_sinc': True}


def frames(shape, seed):
    """float32 synthetic echoes (max-abs 1) of shape [n, 1, L] or [n, L]."""
    x = synth.synth_echo(shape[0], shape[-1], seed=seed)
    return x[:, 0, :] if len(shape) == 2 else x


def seeded_convs(seed):
    """conv.1..3 weights and biases with He-scaled Gaussian weights and small biases (the `init` case)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for i, (cin, cout, k) in enumerate(((128, 128, 11), (128, 128, 9), (128, 1, 7)), start=1):
        sd[f'conv.{i}.weight'] = (rng.standard_normal((cout, cin, k)) * np.sqrt(2.0 / (cin * k))).astype(np.float32)
        sd[f'conv.{i}.bias'] = (0.01 * rng.standard_normal(cout)).astype(np.float32)
    return sd


def checkpoint_weights(key):
    """float32 state_dict of checkpoint `key` with conv.1 / conv.2 weight regenerated at the checkpoint's scale."""
    d = np.load(os.path.join(GOLDEN, PARTS + '.npz'))
    rng = np.random.default_rng(CKPT_SEEDS[key])
    sd = {}
    for k in (str(v) for v in d[f'{key}/keys']):
        if k in SEEDED:
            shape = tuple(int(v) for v in d[f'{key}/{k}.shape'])
            sd[k] = (rng.standard_normal(shape) * d[f'{key}/{k}.rms'][:, None, None]).astype(np.float32)
        else:
            sd[k] = d[f'{key}/{k}']
    return sd

"""Seeded inputs and weights of the Zonzini fixture (tests/golden/f18_zonzini.npz), shared by its generator
(tests/golden/make_golden_zonzini.py) and the tests, so that the fixture stores seeds and outputs only."""
import numpy as np

from stofnet_amd import synth

SMALL_CHANNELS = (16, 32, 64, 64)
LARGE_CHANNELS = (50, 100, 150, 200, 250)


def echo_frames(n, L, seed):
    """[n, 1, L] float32 synthetic echoes (max-abs 1)."""
    return synth.synth_echo(n, L, seed=seed)


def seeded_weights(channels, seed):
    """state_dict (float32 arrays) of a Zonzini net with He-scaled Gaussian weights and small biases: unlike torch's
    default init, the outputs of such a net depend on the input rather than on fc2's bias."""
    rng = np.random.default_rng(seed)
    sd, cin = {}, 1
    for i, c in enumerate(channels):
        sd[f'conv_layers.{i}.weight'] = rng.standard_normal((c, cin, 10)) * np.sqrt(2.0 / (10 * cin))
        sd[f'conv_layers.{i}.bias'] = 0.01 * rng.standard_normal(c)
        cin = c
    sd['fc1.weight'] = rng.standard_normal((1024, cin)) * np.sqrt(2.0 / cin)
    sd['fc1.bias'] = 0.01 * rng.standard_normal(1024)
    sd['fc2.weight'] = rng.standard_normal((1, 1024)) * np.sqrt(1.0 / 1024)
    sd['fc2.bias'] = 0.01 * rng.standard_normal(1)
    return {k: v.astype(np.float32) for k, v in sd.items()}

"""Width variants of StofNet (models/stofnet.py:11 takes any num_features and in_channels) used by
tests/golden/make_golden_widths.py (reference side) and by the parity tests (oracle and gfx950 side): the geometry table and the
seeded input.  Parameters and the cotangent come from tests/ctor_variants.py, so the fixture holds seeds and expected outputs
only, not the weights."""
import numpy as np

from ctor_variants import variant_params, variant_cotangent  # noqa: F401  (re-exported for the tests)


def _ctor(r, F, nb, ks, cin, sgs):
    return dict(upsample_factor=r, num_features=F, num_blocks=nb, kernel_sizes=ks, in_channels=cin, semi_global_scale=sgs)


# name -> constructor arguments, input shape, which gradients the fixture keeps ('all' or a tuple of parameter names)
SG = 'semi_global_block.'
WIDTH_VARIANTS = {
    # half a 64-channel block; remainder 4 shifts the up-sampled map; even depth
    'f32_c1_nb6_k3_sgs20_r4': dict(ctor=_ctor(4, 32, 6, [9, 3, 3], 1, 20), N=2, L=244, grads='all'),
    # second block half full; two input channels
    'f96_c2_nb5_k5_nosgb_r3': dict(ctor=_ctor(3, 96, 5, [9, 5, 3], 2, 1), N=2, L=200,
                                   grads=('conv1.weight', 'conv1.bias', 'conv2.weight', 'conv4.bias', 'conv_last.weight',
                                          'conv_last.bias')),
    # two full blocks (the 64-multiple f16x3 kernel with cin = cout = 128); feat_scale 1
    'f128_c1_nb4_k7_sgs10_r2': dict(ctor=_ctor(2, 128, 4, [9, 7, 3], 1, 10), N=2, L=204,
                                    grads=('conv1.weight', 'conv1.bias', 'conv2.bias', 'conv3.bias', 'conv_last.weight',
                                           SG + 'contract_conv.weight', SG + 'expand_conv.bias')),
    # width not a multiple of 16; odd Cin; contracted width 96; remainder 6
    'f24_c3_nb7_k3_sgs40_r5': dict(ctor=_ctor(5, 24, 7, [9, 3, 3], 3, 40), N=3, L=166, grads='all'),
    # the sweep's geometry with two channels: must not take the sweep
    'f64_c2_nb13_k7_sgs80_r4': dict(ctor=_ctor(4, 64, 13, [9, 7, 3], 2, 80), N=1, L=164,
                                    grads=('conv1.weight', 'conv1.bias', 'conv7.bias', 'conv12.weight', SG + 'contract_conv.bias',
                                           SG + 'expand_conv.bias')),
    # Cin at its cap, narrowest multiple of 16, shipped depth
    'f16_c16_nb13_k7_nosgb_r4': dict(ctor=_ctor(4, 16, 13, [9, 7, 3], 16, 1), N=2, L=96, grads='all'),
    # four blocks, 1-tap body, smallest scale, r = 1
    'f256_c1_nb4_k1_sgs2_r1': dict(ctor=_ctor(1, 256, 4, [9, 1, 3], 1, 2), N=1, L=64,
                                   grads=('conv1.weight', 'conv1.bias', 'conv2.bias', 'conv_last.weight', SG + 'contract_conv.bias')),
}


def width_input(N: int, Cin: int, L: int, seed: int):
    return (0.3 * np.random.RandomState(seed).standard_normal((N, Cin, L))).astype(np.float32)


def rel(a, b):
    """max |a - b| / max |b| in float64."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def width_case(name):
    """(variant, StofNet module, parameters, x, cotangent t, reference y, reference dx, kept reference gradients) of one case."""
    from conftest import golden
    from stofnet_amd import StofNet
    var, g = WIDTH_VARIANTS[name], golden('f25_width_variants')
    seed = int(g[f'{name}.seed'])
    c = var['ctor']
    m = StofNet(**c)
    shapes = {n: tuple(t.shape) for n, t in m.state_dict().items()}
    params = variant_params(shapes, seed)
    x = width_input(var['N'], c['in_channels'], var['L'], seed)
    t = variant_cotangent(var['N'], var['L'] * c['upsample_factor'], seed)
    grads = {k[len(name) + 6:]: g[k] for k in g.files if k.startswith(name + '.grad.')}
    return var, m, params, x, t, g[f'{name}.y'], g[f'{name}.dx'], grads

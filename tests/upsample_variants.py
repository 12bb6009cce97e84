"""StofNet at upsample factors other than the benched 4 / 10 / 20 (models/stofnet.py:11 takes any; the gfx950 kernels take
1..64), used by tests/golden/make_golden_upsample.py (reference side) and the parity tests (oracle and gfx950 side).  The
factors sit where the kernels branch on r: 1 / 2 / 3 / 5 / 15 (no multiple of 4: scalar stores of the shuffle), 16 / 17 (the
16-channel conv_last tile of the split-fp16 sweep and the 64-wide block beyond it), 31 / 32 / 33 (the zero-padded upper
half of that block) and 63 / 64 (the full block).  Parameters and inputs come from the numpy seeds of tests/ctor_variants.py."""
from ctor_variants import variant_cotangent, variant_input, variant_params  # noqa: F401  (re-exported for the tests)

GRADS = ('conv1.weight', 'conv2.weight', 'conv_last.weight', 'conv_last.bias')


def kept_grads(name, r, body_kernel):
    """The fixture stays small: the body weight gradient (conv2) is kept on the 3- and 1-tap bodies only (the 7-tap one does
    not branch on r and is pinned by f8 / f14), the conv_last weight gradient (r x 64 x 3) up to r = 33 and at the shipped
    geometry's r = 64.  The GPU tests compare every parameter gradient with the fp64 oracle at every r besides."""
    keep = ['conv1.weight', 'conv_last.bias']
    if body_kernel < 7:
        keep.append('conv2.weight')
    if r <= 33 or name == 'g1_r64':
        keep.append('conv_last.weight')
    return tuple(k for k in GRADS if k in keep)


GEOMETRIES = {
    # the shipped geometry: fused sweep with the SemiGlobalBlock at scale 80
    'g1': (dict(num_blocks=13, kernel_sizes=[9, 7, 3], semi_global_scale=80), (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 63, 64)),
    # the shipped depth without the SemiGlobalBlock: fused sweep
    'g2': (dict(num_blocks=13, kernel_sizes=[9, 7, 3], semi_global_scale=1), (3, 17, 64)),
    # layer by layer: another depth, 3-tap body, SemiGlobalBlock at scale 20
    'g3': (dict(num_blocks=5, kernel_sizes=[9, 3, 3], semi_global_scale=20), (3, 33, 64)),
    # layer by layer with a 1-tap body (padding 0)
    'g4': (dict(num_blocks=6, kernel_sizes=[9, 1, 3], semi_global_scale=80), (2, 64)),
}

# name -> constructor arguments, input shape, kept gradients (the layout of ctor_variants.VARIANTS).  L = 160 holds two
# SemiGlobalBlock windows at scale 80; the maps grow with r, so the cases above r = 17 keep one row.
UPSAMPLE_CASES = {
    f'{g}_r{r}': dict(ctor=dict(upsample_factor=r, **ctor), N=2 if r <= 17 else 1, L=160,
                      grads=kept_grads(f'{g}_r{r}', r, ctor['kernel_sizes'][1]))
    for g, (ctor, rs) in GEOMETRIES.items() for r in rs
}

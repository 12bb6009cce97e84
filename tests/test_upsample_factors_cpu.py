"""StofNet across upsample factors 1..64 and four geometries (tests/upsample_variants.py): the fp32 and fp64 oracles against
the reference's own forward result and autograd gradients (golden f20_upsample_factors, tests/golden/make_golden_upsample.py),
so the GPU tests can compare the kernels with the oracle at any r."""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import stofnet_oracle as so
from upsample_variants import UPSAMPLE_CASES, variant_cotangent, variant_input, variant_params


def upsample_case(name):
    """(var, params, x, t, y_ref, dx_ref, grads_ref) of fixture case `name`; shapes from the reference-named state_dict."""
    from stofnet_amd import StofNet
    var, g = UPSAMPLE_CASES[name], golden('f20_upsample_factors')
    seed = int(g[f'{name}.seed'])
    m = StofNet(**var['ctor'])
    params = variant_params({n: tuple(t.shape) for n, t in m.state_dict().items()}, seed)
    x = variant_input(var['N'], var['L'], seed)
    t = variant_cotangent(var['N'], var['L'] * var['ctor']['upsample_factor'], seed)
    grads = {k[len(name) + 6:]: g[k] for k in g.files if k.startswith(name + '.grad.')}
    return var, params, x, t, g[f'{name}.y'], g[f'{name}.dx'], grads


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize('name', list(UPSAMPLE_CASES))
def test_oracle_forward_and_gradients_match_reference(name):
    var, params, x, t, y_ref, dx_ref, grads_ref = upsample_case(name)
    c = var['ctor']
    r = c['upsample_factor']
    y = so.stofnet_forward(params, x, r, c['semi_global_scale'], torch.float32)
    assert y.shape == y_ref.shape == (var['N'], 1, var['L'] * r)
    assert rel(y.numpy(), y_ref) < 2e-6
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (so.stofnet_forward(p64, x64, r, c['semi_global_scale'], torch.float64) * torch.from_numpy(t).double()).sum().backward()
    assert rel(x64.grad.numpy(), dx_ref) < 2e-5
    assert set(grads_ref) == set(var['grads'])
    for n, gr in grads_ref.items():
        assert rel(p64[n].grad.numpy(), gr) < 2e-5, n


def test_every_case_is_served_and_r_above_64_is_not():
    from stofnet_amd import StofNet
    for name, var in UPSAMPLE_CASES.items():
        m = StofNet(**var['ctor'])
        assert m._supported(), name
        assert m._fused_sweep() == name.startswith(('g1_', 'g2_')), name
    m = StofNet(upsample_factor=65)
    assert not m._supported()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 400))
    assert not StofNet(upsample_factor=0)._supported()

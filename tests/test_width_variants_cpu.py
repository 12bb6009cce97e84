"""StofNet at other widths (models/stofnet.py:11: any num_features / in_channels), CPU side: golden `f25_width_variants`
holds the reference's own forward result and autograd gradients (tests/golden/make_golden_widths.py); parameters and inputs
come from numpy seeds (tests/width_variants.py).  Pins the oracle on the fixture, the fixture on its manifest, and the
predicates that route a model to the kernels."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from width_variants import WIDTH_VARIANTS, rel, width_case
from oracle import stofnet_oracle as so

FIXTURE = 'f25_width_variants'


@pytest.mark.parametrize('name', list(WIDTH_VARIANTS))
def test_oracle_forward_and_gradients_match_reference(name):
    """The oracle reads the widths from the state_dict: it reproduces the reference's output and autograd gradients."""
    var, m, params, x, t, y_ref, dx_ref, grads_ref = width_case(name)
    c = var['ctor']
    assert set(params) == set(m.state_dict())          # same state_dict names as the reference's constructor gave
    y = so.stofnet_forward(params, x, c['upsample_factor'], c['semi_global_scale'], torch.float32)
    assert y.shape == y_ref.shape == (var['N'], 1, var['L'] * c['upsample_factor'])
    assert rel(y.numpy(), y_ref) < 2e-6
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (so.stofnet_forward(p64, x64, c['upsample_factor'], c['semi_global_scale'], torch.float64) * torch.from_numpy(t).double()).sum().backward()
    assert dx_ref.shape == x.shape
    assert rel(x64.grad.numpy(), dx_ref) < 2e-5
    keep = set(params) if var['grads'] == 'all' else set(var['grads'])
    assert set(grads_ref) == keep
    for n, gr in grads_ref.items():
        assert gr.shape == params[n].shape
        assert rel(p64[n].grad.numpy(), gr) < 2e-5, n


def test_fixture_size_and_manifest():
    path = os.path.join(GOLDEN, FIXTURE + '.npz')
    assert os.path.getsize(path) < 1_500_000
    g = golden(FIXTURE)
    manifest = json.load(open(os.path.join(GOLDEN, 'manifest_widths.json')))['cases'][FIXTURE]
    assert set(manifest) == set(g.files)
    for k in g.files:
        assert list(g[k].shape) == manifest[k], k
    for k, name in enumerate(WIDTH_VARIANTS):
        assert int(g[f'{name}.seed']) == 4500 + k


def test_predicates_route_the_width_variants():
    from stofnet_amd import StofNet
    m = StofNet()
    assert m._supported() and m._fused_sweep()
    for var in WIDTH_VARIANTS.values():
        m = StofNet(**var['ctor'])
        assert m._supported_wide() and not m._supported() and not m._fused_sweep()
    x = torch.zeros(1, 1, 64)
    for kw in (dict(num_features=257), dict(in_channels=17), dict(kernel_sizes=[7, 7, 3]), dict(kernel_sizes=[9, 7, 5])):
        m = StofNet(**kw)
        assert not m._supported() and not m._supported_wide()
        with pytest.raises(NotImplementedError) as err:
            m(torch.zeros(1, m.in_channels, 64))
        msg = str(err.value)
        assert 'num_features 1..256' in msg and 'in_channels 1..16' in msg and '[9, 1|3|5|7, 3]' in msg
    with pytest.raises(NotImplementedError):            # as before: the upsample factor's range
        StofNet(upsample_factor=65)(x)
    # the widths at the ends of the served ranges
    assert StofNet(num_features=1, in_channels=16)._supported_wide() and StofNet(num_features=256)._supported_wide()
    assert not StofNet(num_features=0)._supported_wide() and not StofNet(in_channels=0)._supported_wide()
    assert not StofNet(num_features=32, num_blocks=3)._supported_wide()
    assert not StofNet(num_features=32, semi_global_scale=257)._supported_wide()


def test_engine_constructor_defaults_unchanged():
    """Every present caller of TrainEngine / StofNetTrainer keeps its geometry: the widths are keyword arguments that
    default to the shipped 64 / 1."""
    from stofnet_amd.training import StofNetTrainer, TrainEngine
    sig = inspect.signature(TrainEngine.__init__).parameters
    assert list(sig)[:8] == ['self', 'dev', 'r', 'sgb', 'precision', 'scale', 'num_blocks', 'body_kernel']
    assert sig['num_features'].default == 64 and sig['in_channels'].default == 1
    assert (sig['precision'].default, sig['scale'].default, sig['num_blocks'].default, sig['body_kernel'].default) == ('fp32', 80, 13, 7)
    tsig = inspect.signature(StofNetTrainer.__init__).parameters
    assert list(tsig)[:2] == ['self', 'model'] and 'num_features' not in tsig and 'in_channels' not in tsig
    assert tsig['precision'].default == 'f16x3' and tsig['lr'].default == 5e-4

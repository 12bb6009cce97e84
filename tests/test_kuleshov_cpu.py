"""Kuleshov without a GPU: the float64 restatement of kuleshov_inputs.forward64 (plain conv1d, indexing and matmul; no
module forward) and `forward_aten` on the CPU against the reference's fp32 taps (tests/golden/f24_kuleshov.npz,
make_golden_kuleshov.py); state-dict names, shapes, strict loading and the seeded initial values; the constructor
contract; the drop-in import paths; the host packer's layout and its BatchNorm affines against a double computation.

Bound per tap: |got - ref| <= max(1e-5, 8 e_ref) max|ref|, e_ref = the reference's own fp32 deviation from its float64
run (manifest_kuleshov.json).  1e-5 is the standing bound of the baseline networks; the factor 8 covers an fp32 chain of
up to 16,896 terms in one accumulator against ATen's short blocked partial sums (about 4x from the ordering) and the
compounding through eleven layers (2x).  A wrong tap, stride, shuffle address or seam offset gives errors of 0.1 .. 1.

The state dict has 54 float arrays (8 blocks x 6, the bottleneck's 2, final_conv's 2, output_fc's 2) plus the eight
num_batches_tracked counters."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
import kuleshov_inputs as ki

_f64_cache = {}


def manifest():
    with open(os.path.join(GOLDEN, 'manifest_kuleshov.json')) as fh:
        return json.load(fh)['cases']


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def bound(name, tap):
    return max(1e-5, 8.0 * manifest()[name]['taps'][tap]['e_ref'])


def case64(g, name):
    """(state dict, x of the whole batch, the float64 taps of the kept rows) of a fixture case, computed once per session"""
    if name not in _f64_cache:
        _, N, L, O, X, _ = ki.case(name)
        sd = ki.seeded_kuleshov(L, O)
        x = ki.frames(N, X, int(g[f'{name}_seed']))
        taps = ki.forward64(sd, x[ki.kept_rows(N, L)], L)
        taps['fin_in'] = ki.final_in_window(taps['fin_in'], L)
        _f64_cache[name] = (sd, x, taps)
    return _f64_cache[name]


def make(sd, L, O, dev='cpu'):
    from stofnet_amd import Kuleshov
    m = Kuleshov(L, O)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


@pytest.mark.parametrize('name', ki.IDS)
def test_float64_restatement_reproduces_fixture(name):
    g = golden('f24_kuleshov')
    _, _, taps = case64(g, name)
    for tap in ki.TAPS:
        ref = g[f'{name}_{tap}']
        assert taps[tap].shape == ref.shape, tap
        err = rel(ref, taps[tap])
        print(name, tap, f'{err:.2e}')
        assert err <= bound(name, tap), tap


@pytest.mark.parametrize('name', ki.IDS)
def test_forward_aten_matches_fixture(name):
    g = golden('f24_kuleshov')
    _, N, L, O, X, _ = ki.case(name)
    sd, x, taps = case64(g, name)
    m = make(sd, L, O)
    with torch.no_grad():
        y = m(torch.from_numpy(x[ki.kept_rows(N, L)])).numpy()           # rows are independent in eval mode
    assert y.shape == (len(ki.kept_rows(N, L)), 1, O)
    assert rel(y, g[f'{name}_y']) <= bound(name, 'y') and rel(y, taps['y']) <= bound(name, 'y')


def test_state_dict_names_shapes_and_seeded_init():
    from stofnet_amd import Kuleshov
    g = golden('f24_kuleshov')
    torch.manual_seed(0)
    m = Kuleshov(641, 64)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['names']]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g['shapes']]
    assert len([k for k in sd if not k.endswith('num_batches_tracked')]) == 54 == len(m._kernel_params())
    for k in ('down_conv0.weight', 'up_conv3.bias', 'output_fc.weight'):
        assert np.array_equal(sd[k].flatten()[:8].numpy(), g['init_' + k.replace('.', '_')]), k
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ki.seeded_kuleshov(641, 64).items()}, strict=True)
    assert m.fc_dim == 1198 and Kuleshov(2000, 20000).fc_dim == 7952
    assert m.input_length == 641 and m.output_length == 64 and m.layers == 4


def test_constructor_is_silent(capsys):
    from stofnet_amd import Kuleshov
    Kuleshov(641, 2)
    assert capsys.readouterr().out == ''


def test_constructor_contract():
    from stofnet_amd import Kuleshov
    with pytest.raises(NotImplementedError, match='lengths'):
        Kuleshov()
    with pytest.raises(NotImplementedError, match='lengths'):
        Kuleshov(641)
    for n in (1, 2, 3, 5):
        with pytest.raises(NotImplementedError, match='num_layers'):
            Kuleshov(2000, 2000, num_layers=n)
    with pytest.raises(ValueError, match='641'):
        Kuleshov(640, 64)
    with pytest.raises(ValueError):
        Kuleshov(641, 0)
    assert Kuleshov(input_length=641, output_length=1, num_layers=4).output_fc.weight.shape == (1, 1198)


def test_dropin_import_paths():
    import models
    import models.kuleshov
    import stofnet_amd
    assert models.Kuleshov is stofnet_amd.Kuleshov is models.kuleshov.Kuleshov
    assert not hasattr(models, '_out_of_scope')


def test_chain_lengths():
    from stofnet_amd.kuleshov import chain_lengths
    d = chain_lengths(2000)
    assert d['down'] == [968, 468, 226, 109] and d['bottleneck'] == 51 and d['up'] == [43, 179, 552, 1508]
    assert d['cat'] == [195, 584, 1572, 3984] and d['final'] == 3976 and d['fc_dim'] == 7952
    d = chain_lengths(641)
    assert d['bottleneck'] == 9 and d['up'][0] == 1 and d['fc_dim'] == 1198
    assert chain_lengths(640)['up'][0] < 1


def test_train_mode_uses_batch_statistics_and_dropout():
    m = make(ki.seeded_kuleshov(641, 8), 641, 8)
    x = torch.from_numpy(ki.frames(2, 641, 3))
    with torch.no_grad():
        ye = m(x)
    m.train()
    mean0 = m.up_bn2.running_mean.clone()
    y = m(x)
    assert y.grad_fn is not None and y.shape == (2, 1, 8) and not torch.allclose(y.detach(), ye, atol=1e-3)
    assert not torch.equal(m.up_bn2.running_mean, mean0)
    y.sum().backward()
    assert m.down_conv0.weight.grad is not None and m.output_fc.weight.grad is not None


# ------------------------------------------------------------------------------------------------------- the packer
def align(v):
    return (v + 63) // 64 * 64


def layout(L, O):
    """float offsets of the packed sections (csrc/kuleshov.hip)"""
    from stofnet_amd.kuleshov import chain_lengths
    at, o = 0, {}

    def take(name, n):
        nonlocal at
        o[name] = at
        at = align(at + n)

    take('w0', 65 * 128)
    take('ep_down_conv0', 3 * 128)
    for conv, bn, co, ci, k in ki.block_names()[1:9]:
        take('frag_' + conv, co * ci * k)
        take('ep_' + conv, 3 * co)
    take('wf', 2 * 9 * 128)
    take('bf', 2)
    kp = (chain_lengths(L)['fc_dim'] + 7) // 8 * 8
    take('fcfrag', (O + 31) // 32 * 32 * kp)
    take('fcb', O)
    o['total'] = at
    return o, kp


def unfrag(f, cout, K):
    """fragment order [cout / 32][K / 8][64 lanes][4] -> dense [cout][K]"""
    return f.reshape(cout // 32, K // 8, 2, 32, 4).transpose(0, 3, 1, 2, 4).reshape(cout, K)


def test_packer_layout_and_affines():
    from stofnet_amd.kuleshov import pack_kuleshov_weights
    L, O, eps = 645, 37, 1e-5
    sd = ki.seeded_kuleshov(L, O)
    arrs = ki.kernel_arrays(sd)
    assert len(arrs) == 54
    blob = pack_kuleshov_weights(L, O, arrs, eps)
    o, kp = layout(L, O)
    assert blob.dtype == torch.uint8 and blob.numel() == 4 * o['total']
    f = blob.numpy().view(np.float32)
    for bad in (arrs[:-1], arrs + arrs[:1], arrs[:52]):
        with pytest.raises(ValueError, match='54'):
            pack_kuleshov_weights(L, O, bad, eps)
    with pytest.raises(ValueError):
        pack_kuleshov_weights(640, O, arrs, eps)
    d = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    assert np.array_equal(f[o['w0']:o['w0'] + 65 * 128].reshape(65, 128), sd['down_conv0.weight'][:, 0, :].T)
    for conv, bn, co, ci, k in ki.block_names()[:9]:
        ep = f[o['ep_' + conv]:o['ep_' + conv] + 3 * co].reshape(3, co)
        if conv != 'down_conv0':
            dense = unfrag(f[o['frag_' + conv]:o['frag_' + conv] + co * ci * k], co, ci * k)
            assert np.array_equal(dense, sd[conv + '.weight'].transpose(0, 2, 1).reshape(co, k * ci)), conv
        if bn is None:                                                   # the bottleneck: bias alone
            assert np.array_equal(ep[0], sd[conv + '.bias']) and np.all(ep[1] == 1) and np.all(ep[2] == 0)
            continue
        s = d[bn + '.weight'] / np.sqrt(d[bn + '.running_var'] + eps)
        assert np.array_equal(ep[1], s.astype(np.float32)), conv
        if conv.startswith('down'):                                      # lrelu0.2(s lrelu0.01(acc + b) + t)
            assert np.array_equal(ep[0], sd[conv + '.bias'])
            t = d[bn + '.bias'] - d[bn + '.running_mean'] * s
        else:                                                            # s acc + t', the bias folded into t'
            assert np.all(ep[0] == 0)
            t = (d[conv + '.bias'] - d[bn + '.running_mean']) * s + d[bn + '.bias']
        assert np.array_equal(ep[2], t.astype(np.float32)), conv
    assert np.array_equal(f[o['wf']:o['wf'] + 2 * 9 * 128].reshape(2, 9, 128), sd['final_conv.weight'].transpose(0, 2, 1))
    assert np.array_equal(f[o['bf']:o['bf'] + 2], sd['final_conv.bias'])
    fc = unfrag(f[o['fcfrag']:o['fcfrag'] + (O + 31) // 32 * 32 * kp], (O + 31) // 32 * 32, kp)
    K = sd['output_fc.weight'].shape[1]
    assert K % 8 != 0 and kp == K + 8 - K % 8                            # this shape has a K tail
    assert np.array_equal(fc[:O, :K], sd['output_fc.weight']) and not fc[O:].any() and not fc[:, K:].any()
    assert np.array_equal(f[o['fcb']:o['fcb'] + O], sd['output_fc.bias'])


def test_packer_follows_eps():
    from stofnet_amd.kuleshov import pack_kuleshov_weights
    sd = ki.seeded_kuleshov(641, 2)
    arrs = ki.kernel_arrays(sd)
    f = pack_kuleshov_weights(641, 2, arrs, 0.5).numpy().view(np.float32)
    o, _ = layout(641, 2)
    s = np.asarray(sd['up_bn0.weight'], np.float64) / np.sqrt(np.asarray(sd['up_bn0.running_var'], np.float64) + 0.5)
    assert np.array_equal(f[o['ep_up_conv0'] + 1024:o['ep_up_conv0'] + 2048], s.astype(np.float32))

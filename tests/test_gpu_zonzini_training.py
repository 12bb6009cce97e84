"""Training the Zonzini baselines on the gfx950 kernels (csrc/zonzini_train.hip, stofnet_amd/zonzini_training.py):

  * every new backward kernel alone against float64 torch on the same fp32 operands and a given seeded selector (so that no
    decision can flip) within 2e-6 x max|ref|, outputs pre-filled with NaN, each twice (bitwise), the exact-zero rows of the
    data gradients included; shapes at, one below and one above the chunk of each weight gradient, past the row count at
    which the chunks start to grow, channel counts that fill neither a 4-channel pad nor a 32-column tile;
  * the autograd boundary (`train_route = 'kernels'`) on every case of tests/golden/f28_zonzini_training.npz: y within 2e-5 of
    the fixture and bitwise the inference y; the saved decisions (sel, h > 0) equal to float64's outside the 8 x dev margin,
    at most 64 decisions inside it (a float64-only count); dx and all gradients within 2e-4 x max|ref| of float64 autograd
    taken with the route's own decisions; on the safe cases also within 2e-4 of the reference's own gradients (the fixture);
  * determinism, repacking after an AdamW step, the graph and error behaviour, the 'aten' route;
  * `main.py model=zonzini evaluate=False` end to end in a child process, chirp (Small) and PALA (Large) data paths.

rel(a, b) = max|a - b| / max|b|.  The measured maxima go to profiles/zonzini_training.jsonl (the `parity` line)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
import zonzini_inputs as zi
import zonzini_training_inputs as ti
from test_zonzini_training_cpu import grad_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'zonzini_training.jsonl')
KERNEL_BOUND, Y_BOUND, GRAD_BOUND, MAX_INSIDE = 2e-6, 2e-5, 2e-4, 64
VARIANT = {'small': 0, 'large': 1}
_errors, _runs = {}, {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a ROCm GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def lib(dev):
    from stofnet_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def g():
    return golden('f28_zonzini_training')


def rel(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def record(name, errs):
    """print the achieved errors and keep them in profiles/zonzini_training.jsonl (one `parity` line, rewritten as cases come in)"""
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    _errors[name] = {k: float(f'{v:.3e}') for k, v in errs.items()}
    lines = []
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip() and json.loads(ln).get('kind') != 'parity']
    try:
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join(lines + [json.dumps({'kind': 'parity', 'bounds': {'kernel': KERNEL_BOUND, 'y': Y_BOUND, 'grad': GRAD_BOUND},
                                                    'rel_err': _errors})]) + '\n')
    except OSError:
        pass


def make_net(net, sd, dev, route='kernels'):
    from stofnet_amd import ZonziniNetLarge, ZonziniNetSmall
    m = (ZonziniNetSmall if net == 'small' else ZonziniNetLarge)()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).train()
    m.train_route = route
    return m


def step(m, x, t, route='kernels', want_dx=True, keep=None):
    """One forward + backward of loss = sum(y * t) -> (y, dx or None, {name: gradient}); keep: receives the route's saved state."""
    m.train_route = route
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(want_dx)
    y = m(xd)
    if keep is not None:
        keep['saved'] = y.grad_fn.saved
    (y * t).sum().backward()
    return y.detach(), xd.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------- the kernels alone
def _nan(*shape, dev):
    return torch.full(shape, float('nan'), device=dev)


def layer_dims(net, N, L):
    """per conv layer (cout, cpad, input length, pooled length)"""
    dims, lin = [], L
    for c in ti.CHANNELS[net]:
        lp = ti.pooled_len(lin)
        dims.append((c, (c + 3) & ~3, lin, lp))
        lin = lp
    return dims


def seeded_operands(gen, N, lin, cin, cpin, lp, cout, cpout, head):
    """in [N, lin, cpin] (pad 0), sel [N, lp, cpout] in {0, 1, 2} (pad 0), dout: [N, cpout] (pad 0) for the head reader else
    [N, lp, cpout] with NaN in the pad channels (their selector is 0: never used), w [cout, cin, 10]"""
    inp = torch.zeros(N, lin, cpin)
    inp[..., :cin] = torch.randn(N, lin, cin, generator=gen)
    sel = torch.zeros(N, lp, cpout, dtype=torch.uint8)
    sel[..., :cout] = torch.randint(0, 3, (N, lp, cout), generator=gen, dtype=torch.uint8)
    if head:
        dout = torch.zeros(N, cpout)
        dout[:, :cout] = torch.randn(N, cout, generator=gen)
    else:
        dout = torch.full((N, lp, cpout), float('nan'))
        dout[..., :cout] = torch.randn(N, lp, cout, generator=gen)
    w = torch.randn(cout, cin, 10, generator=gen) * (2.0 / (10 * cin)) ** 0.5
    return inp, sel, dout, w


def conv_reference(inp, sel, dout, w, cin, cout, lp, head):
    """float64: dz from dout and sel, then the gradients of sum(conv1d(in, w, stride 2) * dz) -> dw, db, din [N, lin, cin]"""
    N = inp.shape[0]
    d = (dout[:, None, :cout].double() / lp).expand(N, lp, cout) if head else dout[..., :cout].double()
    s = sel[..., :cout].long()
    dz = torch.zeros(N, 2 * lp, cout, dtype=torch.float64)
    dz[:, 0::2][s == 1] = d[s == 1]
    dz[:, 1::2][s == 2] = d[s == 2]
    x64 = inp[..., :cin].double().permute(0, 2, 1).contiguous().requires_grad_()
    w64 = w.double().requires_grad_()
    b64 = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    z = F.conv1d(x64, w64, b64, stride=2)[..., :2 * lp]
    (z * dz.permute(0, 2, 1)).sum().backward()
    return w64.grad, b64.grad, x64.grad.permute(0, 2, 1), dz


# net, layer, N, L: the rows N Lp_layer one below / on / one above the 64-row chunk; row tiles across waveforms; the last layer
# (the mean's gradient is formed by the reader); more than 64 x 64 rows (the chunks grow); Large's odd channel counts
CONV_SHAPES = [('small', 1, 1, 1048), ('small', 1, 1, 1064), ('small', 1, 1, 1080), ('small', 2, 3, 937), ('small', 3, 2, 936),
               ('small', 3, 3, 2000), ('small', 1, 34, 2000), ('large', 1, 1, 3752), ('large', 2, 2, 4001), ('large', 3, 1, 3752),
               ('large', 4, 2, 4001), ('large', 4, 1, 3752)]


@pytest.mark.parametrize('net,layer,N,L', CONV_SHAPES)
def test_conv_gradient_kernels_vs_torch(lib, dev, net, layer, N, L):
    from stofnet_amd import _lib
    st, desc = _lib.stream_ptr(dev), _lib.ZonziniDesc(VARIANT[net], 0)
    D = ctypes.byref(desc)
    dims = layer_dims(net, N, L)
    (cin, cpin, _, lin), (cout, cpout, _, lp) = dims[layer - 1], dims[layer]
    head = layer == len(dims) - 1
    gen = torch.Generator().manual_seed(7000 + 100 * layer + N + L)
    inp, sel, dout, w = seeded_operands(gen, N, lin, cin, cpin, lp, cout, cpout, head)
    dw64, db64, din64, dz = conv_reference(inp, sel, dout, w, cin, cout, lp, head)
    inp_d, sel_d, dout_d, w_d = (t.to(dev).contiguous() for t in (inp, sel, dout, w))
    ws = torch.empty(lib.stof_zonzini_train_conv_wgrad_workspace_bytes(D, layer), dtype=torch.uint8, device=dev)
    assert ws.numel() <= 64 << 20
    outs = []
    for _ in range(2):
        ws.fill_(0xff)                                                       # NaN patterns: every partial the reduce reads is written
        dw, db = _nan(cout, cin, 10, dev=dev), _nan(cout, dev=dev)
        _lib.check(lib.stof_zonzini_train_conv_wgrad(D, layer, _lib.ptr(inp_d), _lib.ptr(dout_d), _lib.ptr(sel_d), _lib.ptr(dw), _lib.ptr(db),
                                                     N, L, _lib.ptr(ws), ws.numel(), st), 'conv_wgrad')
        img = _nan(lib.stof_zonzini_train_dgrad_image_floats(D, layer), dev=dev)
        _lib.check(lib.stof_zonzini_train_dgrad_image(D, layer, _lib.ptr(w_d), _lib.ptr(img), st), 'dgrad_image')
        din = _nan(N, lin, cpin, dev=dev)
        _lib.check(lib.stof_zonzini_train_conv_dgrad(D, layer, _lib.ptr(dout_d), _lib.ptr(sel_d), _lib.ptr(img), _lib.ptr(din), N, L, st),
                   'conv_dgrad')
        outs.append((dw, db, din))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    dw, db, din = (t.cpu() for t in outs[0])
    errs = {'dw': rel(dw, dw64), 'db': rel(db, db64), 'din': rel(din[..., :cin], din64)}
    record(f'conv_{net}_l{layer}_{N}x{L}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs
    assert not din[..., cin:].any()                                          # the pad channels of the data gradient are 0
    # rows that no kept conv output reads are exactly 0: past the last window, and wherever every dz in reach is 0
    reach = F.conv_transpose1d((dz != 0).double().permute(0, 2, 1), torch.ones(cout, 1, 10, dtype=torch.float64), stride=2).squeeze(1)
    dead = torch.zeros(N, lin, dtype=torch.bool)
    dead[:, :reach.shape[-1]] = reach == 0
    dead[:, reach.shape[-1]:] = True
    assert dead[:, 4 * lp + 8:].all() and not din[dead].any() and torch.isfinite(din).all()


# net, N, L: the rows N Lp_1 one below / on / one above the 256-row chunk; tiles across waveforms and dropped samples; more
# than 512 x 256 rows (the chunks grow); Large's 50 channels in a pad of 52
IN_SHAPES = [('small', 1, 1028), ('small', 1, 1032), ('small', 1, 1036), ('small', 3, 937), ('small', 2, 939), ('small', 264, 2000),
             ('large', 2, 4001)]


@pytest.mark.parametrize('net,N,L', IN_SHAPES)
def test_layer1_gradient_kernels_vs_torch(lib, dev, net, N, L):
    from stofnet_amd import _lib
    st, desc = _lib.stream_ptr(dev), _lib.ZonziniDesc(VARIANT[net], 0)
    D = ctypes.byref(desc)
    cout, cpout, _, lp = layer_dims(net, N, L)[0]
    gen = torch.Generator().manual_seed(8000 + N + L)
    x, sel, dout, w = seeded_operands(gen, N, L, 1, 1, lp, cout, cpout, False)
    dw64, db64, dx64, dz = conv_reference(x, sel, dout, w, 1, cout, lp, False)
    x_d, sel_d, dout_d, w_d = (t.to(dev).contiguous() for t in (x.reshape(N, L), sel, dout, w))
    ws = torch.empty(lib.stof_zonzini_train_in_wgrad_workspace_bytes(D), dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        ws.fill_(0xff)
        dw, db, dx = _nan(cout, 1, 10, dev=dev), _nan(cout, dev=dev), _nan(N, L, dev=dev)
        _lib.check(lib.stof_zonzini_train_in_wgrad(D, _lib.ptr(x_d), _lib.ptr(dout_d), _lib.ptr(sel_d), _lib.ptr(dw), _lib.ptr(db), N, L,
                                                   _lib.ptr(ws), ws.numel(), st), 'in_wgrad')
        _lib.check(lib.stof_zonzini_train_in_dgrad(D, _lib.ptr(dout_d), _lib.ptr(sel_d), _lib.ptr(w_d), _lib.ptr(dx), N, L, st), 'in_dgrad')
        outs.append((dw, db, dx))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    dw, db, dx = (t.cpu() for t in outs[0])
    errs = {'dw': rel(dw, dw64), 'db': rel(db, db64), 'dx': rel(dx, dx64[..., 0])}
    record(f'in_{net}_{N}x{L}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs
    assert not dx[:, 4 * lp + 8:].any() and torch.isfinite(dx).all()         # samples beyond the last kept window: exactly 0.0
    assert torch.equal(dx[:, 4 * lp + 8:], torch.zeros(N, L - 4 * lp - 8)) and not torch.signbit(dx[:, 4 * lp + 8:]).any()


@pytest.mark.parametrize('net', ['small', 'large'])
def test_device_packer_gives_the_host_packer_bytes(lib, dev, net):
    from stofnet_amd import _lib
    from stofnet_amd.zonzini import pack_weights
    sd = ti.weights(740 if net == 'small' else 741, net)
    arrs = [sd[k] for k in ti.param_names(net)]
    host = pack_weights(VARIANT[net], arrs)
    desc = _lib.ZonziniDesc(VARIANT[net], 0)
    on_dev = [torch.from_numpy(a).to(dev).contiguous() for a in arrs]
    ptrs = (ctypes.c_void_p * len(on_dev))(*[t.data_ptr() for t in on_dev])
    blob = torch.full((host.numel(),), 0xff, dtype=torch.uint8, device=dev)
    _lib.check(lib.stof_zonzini_train_pack(ctypes.byref(desc), ptrs, _lib.ptr(blob), blob.numel(), _lib.stream_ptr(dev)), 'train_pack')
    assert torch.equal(blob.cpu(), host)


@pytest.mark.parametrize('net,N', [('small', 1), ('small', 17), ('large', 3), ('large', 16)])
def test_head_backward_kernels_vs_torch(lib, dev, net, N):
    from stofnet_amd import _lib
    st, desc = _lib.stream_ptr(dev), _lib.ZonziniDesc(VARIANT[net], 0)
    C = ti.CHANNELS[net][-1]
    cpad = (C + 3) & ~3
    gen = torch.Generator().manual_seed(9000 + N + C)
    dy, f = torch.randn(N, generator=gen), torch.randn(N, C, generator=gen).abs()
    h = torch.randn(N, 1024, generator=gen).clamp_min(0.0)                    # post-ReLU: about half the units are off
    w1, w2 = torch.randn(1024, C, generator=gen) * (2.0 / C) ** 0.5, torch.randn(1, 1024, generator=gen) / 32
    dh = dy.double()[:, None] * w2.double() * (h > 0)
    ref = {'dw1': dh.T @ f.double(), 'db1': dh.sum(0), 'dw2': (dy.double()[:, None] * h.double()).sum(0, keepdim=True),
           'db2': dy.double().sum().reshape(1), 'df': dh @ w1.double()}
    dy_d, f_d, h_d, w1_d, w2_d = (t.to(dev).contiguous() for t in (dy, f, h, w1, w2))
    outs = []
    for _ in range(2):
        o = {'dw1': _nan(1024, C, dev=dev), 'db1': _nan(1024, dev=dev), 'dw2': _nan(1, 1024, dev=dev), 'db2': _nan(1, dev=dev),
             'df': _nan(N, cpad, dev=dev)}
        _lib.check(lib.stof_zonzini_train_head_bwd(ctypes.byref(desc), _lib.ptr(dy_d), _lib.ptr(f_d), _lib.ptr(h_d), _lib.ptr(w1_d), _lib.ptr(w2_d),
                                                   _lib.ptr(o['dw1']), _lib.ptr(o['db1']), _lib.ptr(o['dw2']), _lib.ptr(o['db2']), _lib.ptr(o['df']),
                                                   N, st), 'head_bwd')
        outs.append(o)
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    got = {k: v.cpu() for k, v in outs[0].items()}
    assert not got['df'][:, C:].any()
    got['df'] = got['df'][:, :C]
    errs = {k: rel(got[k], ref[k]) for k in ref}
    record(f'head_{net}_{N}', errs)
    assert max(errs.values()) <= KERNEL_BOUND, errs


# ------------------------------------------------------------------------------------------------ the cases of the fixture
def route_run(name, dev, g):
    """Everything the case tests share, computed once per case."""
    if name in _runs:
        return _runs[name]
    _, net, wkey, n, L, seed, safe = ti.case(name)
    sd = ti.weights(wkey, net)
    x, t = zi.echo_frames(n, L, seed), ti.cotangent(n, seed)
    m = make_net(net, sd, dev)
    keep = {}
    y, dx, grads = step(m, torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), keep=keep)
    saved = keep['saved']
    channels = ti.CHANNELS[net]
    sel = [s.cpu().numpy()[..., :c].transpose(0, 2, 1) for s, c in zip(saved.sel, channels)]            # -> [N, C, Lp]
    hmask = (saved.h > 0).cpu().numpy()
    m.eval()
    with torch.no_grad():
        y_inf = m(torch.from_numpy(x).to(dev))
    own = ti.restate64(sd, x, t)                                  # float64 with its own decisions: the margins
    routed = ti.restate64(sd, x, t, decisions=(sel, hmask))       # float64 autograd of the network with the route's decisions
    _runs[name] = dict(net=net, safe=safe, y=y.cpu().numpy(), dx=dx.cpu().numpy(), grads={k: v.cpu().numpy() for k, v in grads.items()},
                       sel=sel, hmask=hmask, y_inf=y_inf.cpu().numpy(), own=own, routed=routed, saved=saved)
    return _runs[name]


@pytest.mark.parametrize('name', ti.IDS)
def test_kernel_route_on_fixture_case(dev, g, name):
    r = route_run(name, dev, g)
    net = r['net']
    errs = {'y': rel(r['y'], g[f'{name}.y'])}
    # the saved decisions against float64's, outside the margin; the count inside it comes from float64 alone
    masks, hm = ti.margin_masks(r['own'], g[f'{name}.dev'])
    inside = int(sum(int(k.sum()) for k in masks) + int(hm.sum()))
    flipped = 0
    for l, (mine, ref, near) in enumerate(zip(r['sel'], r['own']['sel'], masks)):
        assert np.array_equal(mine[~near], ref[~near]), (name, l)
        flipped += int((mine != ref).sum())
    assert np.array_equal(r['hmask'][~hm], r['own']['hmask'][~hm])
    flipped += int((r['hmask'] != r['own']['hmask']).sum())
    # float64 autograd with the route's own decisions
    errs['dx'] = rel(r['dx'], r['routed']['dx'])
    for k in ti.param_names(net):
        errs[k] = rel(r['grads'][k], r['routed']['grads'][k])
    errs['y (float64, own decisions)'] = rel(r['y'], r['routed']['y'])
    record(name, {**errs, 'inside_margin': float(inside), 'flipped': float(flipped)})
    assert inside <= MAX_INSIDE and (inside == 0 or not r['safe'])
    assert errs.pop('y') <= Y_BOUND and errs.pop('y (float64, own decisions)') <= Y_BOUND
    assert np.array_equal(r['y'], r['y_inf'])                                # bitwise the inference y of the same module
    assert max(errs.values()) <= GRAD_BOUND, errs
    # pad channels of the saved buffers, and the saved features
    for s, a, c in zip(r['saved'].sel, r['saved'].acts, ti.CHANNELS[net]):
        assert not s[..., c:].any() and not a[..., c:].any()
        assert torch.equal(s != 0, a > 0)


@pytest.mark.parametrize('name', ti.SAFE_IDS)
def test_safe_case_matches_the_reference_gradients(dev, g, name):
    r = route_run(name, dev, g)
    errs = {'dx': rel(r['dx'], g[f'{name}.dx']), **grad_errors(name, r['net'], r['grads'], g)}
    record(name + ' (reference)', errs)
    assert max(errs.values()) <= GRAD_BOUND, errs


# ----------------------------------------------------------------------------------------------- behaviour of the boundary
@pytest.fixture(scope='module')
def small_sd():
    return ti.weights(740, 'small')


@pytest.fixture(scope='module')
def x2(dev):
    return torch.from_numpy(zi.echo_frames(2, 939, 6005)).to(dev)


def test_determinism_and_repacking_after_an_optimizer_step(dev, small_sd, x2):
    m = make_net('small', small_sd, dev)
    t = torch.from_numpy(ti.cotangent(2, 6005)).to(dev)
    y1, dx1, g1 = step(m, x2, t)
    y2, dx2, g2 = step(m, x2, t)                                          # two full runs: bitwise equal
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    opt.step()                                                            # in-place parameter updates from the gradients of run 2
    y3, dx3, g3 = step(m, x2, t)
    fresh = make_net('small', {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, dev)
    y4, dx4, g4 = step(fresh, x2, t)
    assert not torch.equal(y3, y1)                                        # the next forward sees the new weights ...
    assert torch.equal(y3, y4) and torch.equal(dx3, dx4) and all(torch.equal(g3[k], g4[k]) for k in g3)      # ... and so do all images
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x2), y3)


def test_graph_and_error_behaviour(dev, small_sd, x2):
    from stofnet_amd import ZonziniNetSmall
    m = make_net('small', small_sd, dev)
    t = torch.from_numpy(ti.cotangent(2, 6005)).to(dev)
    y, dx, grads = step(m, x2, t, want_dx=False)
    assert dx is None and y.shape == (2, 1) and all(v is not None for v in grads.values())      # dx only when the frame asks
    yy = m(x2)
    assert type(yy.grad_fn).__name__.startswith('ZonziniFunction')
    loss = yy.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()
    for pname in ('conv_layers.0.weight', 'conv_layers.2.bias', 'fc1.weight'):
        loss = m(x2).sum()
        with torch.no_grad():
            dict(m.named_parameters())[pname].mul_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            loss.backward()
    m(x2).sum().backward()                                                # the next step is fine
    # an empty batch: empty y and dx, zero parameter gradients of the right shapes
    for p in m.parameters():
        p.grad = None
    xe = torch.zeros((0, 1, 939), device=dev, requires_grad=True)
    ye = m(xe)
    assert ye.shape == (0, 1)
    ye.sum().backward()
    assert xe.grad.shape == (0, 1, 939)
    assert all(p.grad is not None and p.grad.shape == p.shape and not p.grad.any() for p in m.parameters())
    # eval mode without a gradient request, and no_grad in train mode: the inference kernels, no graph
    with torch.no_grad():
        assert m(x2).grad_fn is None
    m.eval()
    assert m(x2).grad_fn is None and m(x2.clone().requires_grad_(True)).grad_fn is not None
    # too short, wrong dtype, wrong device
    m.train()
    with pytest.raises(RuntimeError, match='too short'):
        m(torch.zeros(2, 1, 935, device=dev))
    with pytest.raises(TypeError):
        m(x2.double())
    with pytest.raises(RuntimeError, match='ROCm device'):
        m(x2.cpu())
    # the default route still raises as before
    d = ZonziniNetSmall().to(dev).train()
    assert d.train_route is None
    with pytest.raises(NotImplementedError, match='training is not implemented'):
        d(x2)
    d.eval()
    with pytest.raises(NotImplementedError, match='training is not implemented'):
        d(x2.clone().requires_grad_(True))
    d.train_route = 'kernel'
    with pytest.raises(ValueError, match='train_route'):
        d(x2)


def test_aten_route_agrees_on_a_safe_case(dev, g):
    name = 'small_2x939'
    _, net, wkey, n, L, seed, safe = ti.case(name)
    assert safe
    m = make_net(net, ti.weights(wkey, net), dev)
    x, t = torch.from_numpy(zi.echo_frames(n, L, seed)).to(dev), torch.from_numpy(ti.cotangent(n, seed)).to(dev)
    yk, dxk, gk = step(m, x, t, 'kernels')
    ya, dxa, ga = step(m, x, t, 'aten')
    errs = {'y': rel(yk, ya), 'dx': rel(dxk, dxa), **{k: rel(gk[k], ga[k]) for k in gk}}
    record(name + ' (aten)', errs)
    assert errs.pop('y') <= Y_BOUND and max(errs.values()) <= GRAD_BOUND, errs


# ------------------------------------------------------------------------------------------------------------ main.py
def run_main_training(tmp_path, args, run):
    """`main.main` in a child process with model=zonzini evaluate=False, as `run_main` of test_gpu_zonzini.py runs it
    -> (summary, the JSON lines of the run log, checkpoint paths)"""
    ck = tmp_path / 'ckpts'
    code = ('import sys, json; sys.path.insert(0, sys.argv[1]); import main; '
            'es, s = main.main(sys.argv[2:]); print(json.dumps(s))')
    log = os.path.join(ROOT, f'{run}_unit.jsonl')                        # RunLog without wandb: JSON lines next to main.py
    try:
        res = subprocess.run([sys.executable, '-c', code, ROOT, 'model=zonzini', 'evaluate=False', 'train_route=kernels', f'ckpt_dir={ck}',
                              f'run_name={run}', 'logging=unit', 'epochs=2', 'batch_size=4'] + args,
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stdout + res.stderr
        recs = [json.loads(ln) for ln in open(log)] if os.path.exists(log) else []
    finally:
        if os.path.exists(log):
            os.remove(log)
    return json.loads(res.stdout.strip().splitlines()[-1]), recs, sorted(ck.iterdir())


def check_trained(summary, recs, paths, run, cls):
    hist = summary['train_history']
    assert summary['model'] == 'zonzini' and summary['train_route'] == 'kernels' and summary['train_precision'] == 'fp32'
    assert len(hist) == 2 and all(np.isfinite(h['train_loss']) and np.isfinite(h['val_loss']) for h in hist)
    losses = [r['train_loss'] for r in recs if 'train_loss' in r]
    assert len(losses) >= 2 and all(np.isfinite(v) for v in losses) and len(set(losses)) > 1       # finite, changing losses
    assert [p.name for p in paths] == [f'{run}_rf-scale10_epoch_2.pth']
    sd = torch.load(str(paths[0]), map_location='cpu', weights_only=True)
    cls().load_state_dict(sd, strict=True)
    return sd


def test_main_entry_point_trains_zonzini_on_chirp_data(dev, tmp_path):
    from stofnet_amd import ZonziniNetSmall
    run = f'zonzinitest{os.getpid()}small'
    summary, recs, paths = run_main_training(tmp_path, ['data_dir=./datasets/stof_chirp101_dataset', 'num_waveforms=16', 'num_samples=2000',
                                                        'seed=5'], run)
    sd = check_trained(summary, recs, paths, run, ZonziniNetSmall)
    torch.manual_seed(5)
    init = ZonziniNetSmall().state_dict()                                 # main.py seeds torch, then builds the model
    assert max(float((sd[k] - init[k]).abs().max()) for k in sd) > 0.0     # AdamW moved the parameters


def test_main_entry_point_trains_zonzini_on_the_pala_path(dev, tmp_path):
    from stofnet_amd import ZonziniNetLarge
    run = f'zonzinitest{os.getpid()}large'
    summary, recs, paths = run_main_training(tmp_path, ['data_dir=./PALA_data_InSilicoFlow', 'num_waveforms=12', 'num_samples=4000', 'seed=6'],
                                             run)
    check_trained(summary, recs, paths, run, ZonziniNetLarge)

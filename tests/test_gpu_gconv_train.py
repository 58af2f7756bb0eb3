"""GPU: the opt-in grouped 3x3 training route of the ResNeXt bottlenecks -- the device-side weight
pack bit for bit against the host pack, the autograd node train_fuse.grouped_conv3x3_train
(csrc/gconv.hip forward, csrc/gconv_bwd.hip backward) against F.conv2d autograd in fp64
(tests/gconv_ref.py; gates of tests/wino_ref.py), every dx element written, the same bits over a
poisoned workspace and in two runs, the weight gradient's reduction at the training size of
X-101-32x4d's stage 2, a ResNeXt bottleneck and a whole ResNeXt-50 with `train_gconv` on against the
module route."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import gconv_ref as G
import wino_ref as R

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# channels per group -> channels: supergroup counts 3, 3, 5, 3 (no multiple of 4: the last
# workgroup's spare wavefronts return early)
CHANNELS = {4: 48, 8: 48, 16: 80, 32: 96}


# ------------------------------------------------------------------ 1. the pack
@pytest.mark.parametrize('scale', [False, True])
@pytest.mark.parametrize('cg', [4, 8, 16, 32])
def test_device_pack_has_the_bits_of_the_host_pack(cg, scale):
    from iouaware import ops
    C = CHANNELS[cg]
    g = _gen(10 * cg + scale)
    w = torch.randn(C, cg, 3, 3, device='cuda', generator=g)
    s = torch.rand(C, device='cuda', generator=g) + 0.5 if scale else None
    want = ops.pack_grouped_weight(w, s)
    got = ops.pack_grouped_weight_dev(w, s)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert int((got != 0).sum()) == C * cg * 9


@pytest.mark.parametrize('cg', [4, 8, 16, 32])
def test_adjoint_pack_is_the_host_pack_of_the_flipped_transposed_weight(cg):
    from iouaware import ops
    C = CHANNELS[cg]
    w = torch.randn(C, cg, 3, 3, device='cuda', generator=_gen(20 * cg))
    want = ops.pack_grouped_weight(G.adjoint_weight(w, C // cg))
    got = ops.pack_grouped_weight_dev(w, adjoint=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, ops.pack_grouped_weight_dev(w))
    with pytest.raises(ValueError):
        ops.pack_grouped_weight_dev(w, torch.ones(C, device='cuda'), adjoint=True)
    # both packs from one launch: the bits of the two single launches, the scale on the plain one only
    sc = torch.rand(C, device='cuda', generator=_gen(21 * cg)) + 0.5
    for s_ in (None, sc):
        plain, adj = ops.pack_grouped_weight_dev(w, s_, adjoint='both')
        assert torch.equal(plain.view(torch.int32), ops.pack_grouped_weight_dev(w, s_).view(torch.int32))
        assert torch.equal(adj.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------ 2. the node against fp64
MAPS = [(1, 1), (7, 11), (16, 16), (5, 37), (6, 32)]     # the INPUT map; batch 3: slices do not divide evenly
B = 3


@functools.lru_cache(maxsize=2)
def _data(stride, cg, H, W, batch=B, C=None):
    C = CHANNELS[cg] if C is None else C
    g = _gen(1000 * stride + 100 * cg + 10 * H + W)
    w = torch.randn(C, cg, 3, 3, device='cuda', generator=g) * (1.0 / (9 * cg)) ** 0.5
    b = torch.randn(C, device='cuda', generator=g) * 0.1
    x = torch.randn(batch, C, H, W, device='cuda', generator=g)
    dy = torch.randn(batch, C, G.out_size(H, stride), G.out_size(W, stride), device='cuda', generator=g)
    return w, b, x, dy, C // cg


def _node(stride, cg, H, W, freeze=(), **kw):
    from iouaware.train_fuse import grouped_conv3x3_train
    w, b, x, dy, groups = _data(stride, cg, H, W, **kw)
    wp = w.clone().requires_grad_('w' not in freeze)
    bp = b.clone().requires_grad_('b' not in freeze)
    xp = _cl(x.clone()).requires_grad_('x' not in freeze)
    y = grouped_conv3x3_train(xp, wp, bp, groups, stride, True)
    assert y.is_contiguous(memory_format=torch.channels_last)
    (y * dy).sum().backward()
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xp.grad, dW=wp.grad, db=bp.grad)


def _assert_gates(tag, got, ref, helper):
    for name, t in got.items():
        if t is None:
            continue
        assert tuple(t.shape) == tuple(ref[name].shape), (tag, name)
        assert not bool(torch.isnan(t).any()), (tag, name)
        e, h, ratio = R.gates(t, helper[name], ref[name])
        print('  %-28s %-3s node %.3e  fp32 helper %.3e  ratio %.2f' % (tag, name, e, h, ratio))
        assert e <= R.GATE_A, 'gate A: %s %s %.3e' % (tag, name, e)
        assert ratio <= R.GATE_B, 'gate B: %s %s node %.3e vs helper %.3e = %.2f x' % (tag, name, e, h, ratio)


def _check_against_yardstick(tag, got, stride, cg, H, W, **kw):
    w, b, x, dy, groups = _data(stride, cg, H, W, **kw)
    assert bool((got['y'] >= 0).all())
    mask = got['y'] > 0                                   # the node's own mask (tests/gconv_ref.py)
    ref = G.conv_train(x, w, b, dy, stride, groups, True, torch.float64, mask=mask)
    helper = G.conv_train(x, w, b, dy, stride, groups, True, torch.float32, mask=mask)
    _assert_gates(tag, got, ref, helper)


@pytest.mark.parametrize('H,W', MAPS)
@pytest.mark.parametrize('cg', [4, 8, 16, 32])
@pytest.mark.parametrize('stride', [1, 2])
def test_node_vs_fp64(stride, cg, H, W):
    got = _node(stride, cg, H, W)
    assert all(got[k] is not None for k in ('y', 'dx', 'dW', 'db'))
    _check_against_yardstick('s%d cg%d %dx%d' % (stride, cg, H, W), got, stride, cg, H, W)
    again = _node(stride, cg, H, W)                       # the same bits in a second run
    for k in ('y', 'dx', 'dW', 'db'):
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize('H,W', MAPS)
@pytest.mark.parametrize('cg', [4, 8, 16, 32])
@pytest.mark.parametrize('stride', [1, 2])
def test_entries_write_every_element_and_ignore_the_workspace_contents(stride, cg, H, W):
    """dx allocated NaN-filled holds no NaN afterwards (and the bits of a second call); a workspace
    pre-filled with 0xA5 gives the weight gradient of a zeroed one"""
    from iouaware import _lib, ops
    w, b, x, dz, groups = _data(stride, cg, H, W)
    C = x.shape[1]
    x, dz = _cl(x), _cl(dz)
    wadj = ops.pack_grouped_weight_dev(w, adjoint=True)
    dx = _cl(torch.full((B, C, H, W), float('nan'), device='cuda'))
    assert _lib.lib().ia_grouped_conv3x3_bwd_data_nhwc(ops._ptr(dz), ops._ptr(wadj), ops._ptr(dx), B, H, W, C,
                                                      groups, stride, ops._stream()) == 0
    assert not bool(torch.isnan(dx).any())
    assert torch.equal(dx, ops.grouped_conv3x3_bwd_data(dz, wadj, groups, stride, (H, W)))
    nbytes = int(_lib.lib().ia_grouped_conv3x3_bwd_weight_workspace_bytes(B, H, W, C, groups, stride))
    rows = B * G.out_size(H, stride)
    per_slice = C * 16 * (2 if cg == 32 else 1) * 9 * 4   # the accumulators of every wavefront
    assert nbytes % per_slice == 0 and 1 <= nbytes // per_slice <= rows
    dws = []
    for fill in (0, 0xA5, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device='cuda')
        dws.append(ops.grouped_conv3x3_bwd_weight(x, dz, groups, stride, workspace=ws))
    assert not bool(torch.isnan(dws[0]).any())
    assert torch.equal(dws[0], dws[1]) and torch.equal(dws[0], dws[2])
    assert torch.equal(dws[0], ops.grouped_conv3x3_bwd_weight(x, dz, groups, stride))
    short = torch.zeros(nbytes - 1, dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.grouped_conv3x3_bwd_weight(x, dz, groups, stride, workspace=short)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('freeze', [('x',), ('w',), ('w', 'b'), ('x', 'b')])
def test_node_gradients_not_wanted_are_none(freeze, stride, monkeypatch):
    from iouaware import ops
    calls = []
    for name in ('grouped_conv3x3_bwd_data', 'grouped_conv3x3_bwd_weight'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    got = _node(stride, 8, 7, 11, freeze)
    for key, name in (('x', 'dx'), ('w', 'dW'), ('b', 'db')):
        assert (got[name] is None) == (key in freeze), name
    assert ('grouped_conv3x3_bwd_data' in calls) == ('x' not in freeze)      # skipped, not discarded
    assert ('grouped_conv3x3_bwd_weight' in calls) == ('w' not in freeze)
    _check_against_yardstick('s%d frozen %s' % (stride, '+'.join(freeze)), got, stride, 8, 7, 11)


# ------------------------------------------------------------------ 3. the reduction length
@pytest.mark.parametrize('stride,H,W', [(1, 100, 168), (2, 200, 336)])
def test_node_at_the_training_size_of_stage_2(stride, H, W):
    """X-101-32x4d stage 2: 256 channels in 32 groups, batch 2, 100 x 168 output pixels per image --
    33 600 terms per weight-gradient element, where a too-long fp32 chain shows"""
    kw = dict(batch=2, C=256)
    got = _node(stride, 8, H, W, **kw)
    _check_against_yardstick('stage 2, stride %d' % stride, got, stride, 8, H, W, **kw)


# ------------------------------------------------------------------ 4. the block
def _block(inplanes, planes, stride):
    from iouaware.backbones import Bottleneck
    from iouaware.layers import build_norm_layer
    ds = None
    if stride != 1 or inplanes != planes * 4:
        ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                           build_norm_layer(dict(type='BN'), planes * 4)[1])
    torch.manual_seed(4321 + inplanes + planes)
    m = Bottleneck(inplanes, planes, stride, downsample=ds, groups=32, base_width=4)
    assert m.conv2.groups == 32
    with torch.no_grad():                    # non-trivial statistics and affine parameters everywhere
        for b in m.modules():
            if isinstance(b, nn.modules.batchnorm._BatchNorm):
                b.running_mean.normal_(0, 0.1)
                b.running_var.uniform_(0.5, 1.5)
                b.weight.normal_(1, 0.1)
                b.bias.normal_(0, 0.1)
    m.train()
    for b in m.modules():
        if isinstance(b, nn.modules.batchnorm._BatchNorm):
            b.eval()                          # norm_eval=True
    return m


def _module_route(m, x0, up, dtype):
    mm = copy.deepcopy(m).cpu().to(dtype)
    x = x0.detach().cpu().to(dtype).requires_grad_(True)
    y = mm(x)
    (y * up.cpu().to(dtype)).sum().backward()
    out = {'y': y.detach(), 'dx': x.grad}
    out.update({k: p.grad for k, p in mm.named_parameters()})
    return out


@pytest.mark.parametrize('inplanes,planes,stride', [(256, 64, 1), (256, 128, 2)])
def test_resnext_bottleneck_switch_on_vs_fp64_module_route(inplanes, planes, stride, monkeypatch):
    """output, input gradient and every parameter gradient (three convolution weights, every
    BatchNorm's gamma / beta, the shortcut's) against the module in fp64, the module in fp32 on the
    CPU as the helper; with the switch off no call of the node and the bits of the unfused module"""
    from iouaware import train_fuse
    from iouaware.backbones import Bottleneck
    from iouaware.fuse import fuse_inference, unfuse_inference
    m = _block(inplanes, planes, stride).cuda()
    g = _gen(5 + stride)
    H, W = 14, 18
    x0 = torch.randn(2, inplanes, H, W, device='cuda', generator=g).relu()
    up = torch.randn(2, planes * 4, G.out_size(H, stride), G.out_size(W, stride), device='cuda', generator=g)
    ref, helper = _module_route(m, x0, up, torch.float64), _module_route(m, x0, up, torch.float32)
    calls = []
    real = train_fuse.grouped_conv3x3_train
    monkeypatch.setattr(train_fuse, 'grouped_conv3x3_train', lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(route):
        m.zero_grad(set_to_none=True)
        x = _cl(x0.clone()).requires_grad_(True)
        y = m(x)
        (y * up).sum().backward()
        torch.cuda.synchronize()
        out = {'y': y.detach().clone(), 'dx': x.grad.clone()}
        out.update({k: p.grad.clone() for k, p in m.named_parameters()})
        return out
    # The module route is the framework's.  Its library picks and warms its kernels in the first calls
    # of a shape, so two unfused iterations run before the reference is taken, and the framework's
    # switch for reproducible kernels is set for this test (the library's default backward kernels
    # for some shapes add with atomics): the module then has the same bits in every call, and the
    # fused block with the switch off -- which must run that very code -- has to have them too, in the
    # output, the input gradient and every parameter gradient.
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    run('unfused')
    run('unfused')
    plain, again = run('unfused'), run('unfused')
    forwards = []
    real_fwd = Bottleneck.forward
    monkeypatch.setattr(Bottleneck, 'forward', lambda self, x: (forwards.append(self), real_fwd(self, x))[1])
    assert fuse_inference(m, winograd=True, train=True) > 0
    assert m._ia_train_gconv is False                     # a block fused on its own: the class default
    off = run('off')
    monkeypatch.setattr(Bottleneck, 'forward', real_fwd)
    assert not calls and forwards == [m]                  # the module's own forward, nothing of the node
    assert set(off) == set(plain)
    for k in sorted(plain):
        print('  %-22s unfused twice differs by %.1e, switch off vs unfused by %.1e'
              % (k, float((again[k] - plain[k]).abs().max()), float((off[k] - plain[k]).abs().max())))
    for k in sorted(plain):
        assert torch.equal(again[k], plain[k]), 'the unfused module does not reproduce its own %s' % k
        assert torch.equal(off[k], plain[k]), 'switch off: %s has not the bits of the unfused module' % k
    # switch on.  A Bottleneck on its own has no ResNet whose public `train_gconv` fuse_inference
    # could read (the class default above is all that plumbing can give it), so the per-block
    # attribute it would have set is written directly; the public switch is exercised by the network
    # test below and by tests/test_host_gconv_train.py
    m._ia_train_gconv = True
    on = run('on')
    assert len(calls) == 1
    unfuse_inference(m)
    assert set(on) == set(ref) and len(on) >= 11
    _assert_gates('block stride %d' % stride, on, ref, helper)


# ------------------------------------------------------------------ 5. the network
def test_resnext50_gradient_norms_vs_the_module_route(monkeypatch):
    """ResNeXt-50 32x4d, stage 1 frozen, batch 2 at 64 x 96, a scalar loss on its four outputs:
    every parameter's gradient norm within the training contract (2e-4 relative, README "Parity")
    of the module route's; stage 1 and the stem get no gradient; the node ran in every block of
    stages 2-4"""
    from iouaware import train_fuse
    from iouaware.backbones import ResNeXt
    from iouaware.fuse import fuse_inference
    torch.manual_seed(7)
    net = ResNeXt(depth=50, groups=32, base_width=4, frozen_stages=1)
    with torch.no_grad():
        for b in net.modules():
            if isinstance(b, nn.modules.batchnorm._BatchNorm):
                b.running_mean.normal_(0, 0.1)
                b.running_var.uniform_(0.5, 1.5)
                b.weight.normal_(1, 0.1)
                b.bias.normal_(0, 0.1)
    net = net.cuda().train()
    g = _gen(11)
    img = torch.randn(2, 3, 64, 96, device='cuda', generator=g)
    ups = None

    def run(model):
        nonlocal ups
        model.zero_grad(set_to_none=True)
        outs = model(_cl(img))
        if ups is None:
            ups = [torch.randn(o.shape, device='cuda', generator=g) for o in outs]
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        torch.cuda.synchronize()
        return {k: (None if p.grad is None else p.grad.double().norm().item()) for k, p in model.named_parameters()}
    want = run(net)
    calls = []
    real = train_fuse.grouped_conv3x3_train
    monkeypatch.setattr(train_fuse, 'grouped_conv3x3_train', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    net.train_gconv = True
    assert fuse_inference(net, winograd=True, train=True) > 0
    got = run(net)
    assert len(calls) == 4 + 6 + 3
    assert set(got) == set(want)
    frozen = [k for k in got if k.startswith(('conv1.', 'bn1.', 'layer1.'))]
    assert frozen and all(got[k] is None and want[k] is None for k in frozen)
    dev = [(abs(got[k] - want[k]) / max(want[k], 1e-12), k) for k in got if k not in frozen]
    assert len(dev) > 100 and all(got[k] is not None for _, k in dev)
    print('  worst gradient-norm deviation %.3e at %s (bound 2e-4)' % max(dev))
    assert max(dev)[0] <= 2e-4, max(dev)

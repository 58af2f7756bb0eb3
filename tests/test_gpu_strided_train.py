"""GPU: the opt-in strided 3x3 training route -- k_col2im3x3 (csrc/im2col.hip) bit for bit against
the term-by-term restatement of its contract, the autograd node train_fuse.conv3x3_strided against
F.conv2d autograd in fp64 (tests/conv3s_ref.py; gates of tests/wino_ref.py), the same bits in two
runs over NaN-filled scratch, the stride-2 bottleneck and one whole detector iteration with
`ResNet.train_strided` / `FPN.train_strided` on against off, and the reference's training fixture."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

import conv3s_ref as S
import synth
import wino_ref as R

pytestmark = pytest.mark.gpu

IA_E_ARG = -1


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------ 1. the kernel, bit for bit
_KERNEL_CASES = [(2, h, w, c) for (h, w) in ((7, 9), (8, 6), (1, 1), (2, 3), (5, 4)) for c in (4, 12, 260)] \
    + [(1, 8, 8, 12), (3, 8, 8, 12), (4, 9, 9, 12)]


def _col2im_raw(dcol, dx, B, H, W, Cc, stride, dtype=0):
    from iouaware import _lib, ops
    return _lib.lib().ia_col2im3x3_nhwc(ops._ptr(dcol), ops._ptr(dx), B, H, W, Cc, stride, dtype, ops._stream())


@pytest.mark.parametrize('stride,H,W,Cc', _KERNEL_CASES)
def test_col2im_bit_for_bit(stride, H, W, Cc):
    """only adds, in a stated order: equality is exact.  dx is pre-filled with NaN: every element
    is written, also the pixels that no tap reads (stride 4 on 9 x 9: rows and columns 2 and 6)"""
    from iouaware import ops
    B = 3
    rows = B * S.out_size(H, stride) * S.out_size(W, stride)
    dcol = torch.randn(rows, 9 * Cc, device='cuda', generator=_gen(1000 * stride + 100 * H + W + Cc))
    want = S.col2im(dcol, B, H, W, Cc, stride)
    if stride == 4:
        assert bool((want[:, 2::4] == 0).all()) and bool((want[:, :, 2::4] == 0).all())
    got = ops.col2im3x3(dcol, B, H, W, Cc, stride)
    assert got.shape == (B, Cc, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.permute(0, 2, 3, 1).cpu(), want)
    dx = torch.full((B, H, W, Cc), float('nan'), device='cuda')
    assert _col2im_raw(dcol, dx, B, H, W, Cc, stride) == 0
    assert not bool(torch.isnan(dx).any())
    assert torch.equal(dx.cpu(), want)


def test_col2im_refuses_what_it_does_not_cover():
    """a misaligned pointer, C not a multiple of 4, bf16, strides outside 1..4: IA_E_ARG, nothing launched"""
    B, H, W = 2, 4, 4
    buf = torch.zeros(B * 2 * 2 * 9 * 8 + 4, device='cuda')
    dx = torch.full((B * H * W * 8 + 4,), 7.0, device='cuda')
    assert _col2im_raw(buf, dx, B, H, W, 8, 2) == 0
    assert _col2im_raw(buf[1:], dx, B, H, W, 8, 2) == IA_E_ARG
    assert _col2im_raw(buf, dx[1:], B, H, W, 8, 2) == IA_E_ARG
    assert _col2im_raw(buf, dx, B, H, W, 6, 2) == IA_E_ARG
    assert _col2im_raw(buf, dx, B, H, W, 8, 2, dtype=1) == IA_E_ARG           # IA_BF16
    assert _col2im_raw(buf, dx, B, H, W, 8, 0) == IA_E_ARG
    assert _col2im_raw(buf, dx, B, H, W, 8, 5) == IA_E_ARG
    assert _col2im_raw(None, dx, B, H, W, 8, 2) == IA_E_ARG
    torch.cuda.synchronize()
    assert bool((dx[B * H * W * 8:] == 7.0).all())                            # nothing past the map


# ------------------------------------------------------------------ 2. the node against fp64
@functools.lru_cache(maxsize=4)
def _yardsticks(cin, cout, B, H, W, relu, bias, seed=0):
    """data, the fp64 reference and the fp32 helper of one case (both F.conv2d autograd on the CPU).
    dy is zero in half of its elements.  With the ReLU, dy is also zeroed where the fp64
    pre-activation is within gate A's own tolerance of zero: a forward that passes gate A cannot put
    any other element on the wrong side of the mask (as tests/test_gpu_wino_fp64.py does)."""
    g = _gen(seed + 7 * cin + cout + H)
    w = torch.randn(cout, cin, 3, 3, device='cuda', generator=g) * (1.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, device='cuda', generator=g) * 0.1 if bias else None
    x = torch.randn(B, cin, H, W, device='cuda', generator=g)
    Ho, Wo = S.out_size(H, 2), S.out_size(W, 2)
    dy = torch.randn(B, cout, Ho, Wo, device='cuda', generator=g)
    dy = dy * (torch.rand(dy.shape, device='cuda', generator=g) < 0.5)
    if relu:
        z = S.preactivation(x, w, b, 2)
        keep = z.abs() >= R.GATE_A * z.abs().max()
        assert float((~keep).sum()) <= 0.002 * keep.numel() + 1
        dy = dy * keep.to(dy)
    ref = S.conv_train(x, w, b, dy, 2, relu, torch.float64)
    helper = S.conv_train(x, w, b, dy, 2, relu, torch.float32)
    return w, b, x, dy, ref, helper


def _node(cin, cout, B, H, W, relu, bias, freeze=()):
    """one forward + backward of the node -> {quantity: tensor} (None where it was not wanted)"""
    from iouaware.train_fuse import conv3x3_strided
    w, b, x, dy, ref, helper = _yardsticks(cin, cout, B, H, W, relu, bias)
    wp = w.clone().requires_grad_('w' not in freeze)
    bp = b.clone().requires_grad_('b' not in freeze) if bias else None
    xp = _cl(x.clone()).requires_grad_('x' not in freeze)
    y = conv3x3_strided(xp, wp, bp, 2, relu)
    assert y.is_contiguous(memory_format=torch.channels_last)
    (y * dy).sum().backward()
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xp.grad, dW=wp.grad, db=None if bp is None else bp.grad), ref, helper


def _assert_gates(tag, got, ref, helper):
    for name, t in got.items():
        if t is None:
            continue
        assert tuple(t.shape) == tuple(ref[name].shape), (tag, name)
        e, h, ratio = R.gates(t, helper[name], ref[name])
        print('  %-32s %-3s node %.3e  fp32 helper %.3e  ratio %.2f' % (tag, name, e, h, ratio))
        assert e <= R.GATE_A, 'gate A: %s %s %.3e' % (tag, name, e)
        assert ratio <= R.GATE_B, 'gate B: %s %s node %.3e vs helper %.3e = %.2f x' % (tag, name, e, h, ratio)


@pytest.mark.parametrize('relu_bias', [True, False])
@pytest.mark.parametrize('H,W', [(7, 9), (8, 6)])
@pytest.mark.parametrize('cin,cout', [(4, 8), (32, 36), (64, 32)])
def test_node_vs_fp64(cin, cout, H, W, relu_bias):
    got, ref, helper = _node(cin, cout, 3, H, W, relu_bias, relu_bias)
    assert all(got[k] is not None for k in ('y', 'dx', 'dW')) and (got['db'] is not None) == relu_bias
    _assert_gates('%d->%d %dx%d' % (cin, cout, H, W), got, ref, helper)


def test_node_longer_reduction_vs_fp64():
    """P = 2 * 32 * 48 = 3 072 output pixels: the weight gradient's reduction is cut into slices"""
    from iouaware.train_fuse import _split_for
    assert _split_for(3072, 32, 288) > 1
    got, ref, helper = _node(32, 32, 2, 64, 96, True, True)
    _assert_gates('32->32 64x96', got, ref, helper)


@pytest.mark.parametrize('freeze', [('x',), ('w',), ('w', 'b'), ('x', 'b')])
def test_node_gradients_not_wanted_are_none(freeze):
    got, ref, helper = _node(32, 36, 3, 7, 9, True, True, freeze)
    for key, name in (('x', 'dx'), ('w', 'dW'), ('b', 'db')):
        assert (got[name] is None) == (key in freeze), name
    _assert_gates('32->36 7x9 frozen %s' % '+'.join(freeze), got, ref, helper)


# ------------------------------------------------------------------ 3. the same bits
def _poison_scratch():
    """every scratch buffer of the front-end (column buffers, library / reduction workspaces): NaN bytes"""
    from iouaware import ops
    bufs = list(ops._col_cache.values()) + list(ops._ws_cache.values())
    for t in bufs:
        t.fill_(0xFF)
    return len(bufs)


def test_node_same_bits_over_poisoned_scratch():
    from iouaware import ops
    from iouaware.train_fuse import conv3x3_strided
    w, b, x, dy, ref, helper = _yardsticks(32, 32, 2, 64, 96, True, True)
    runs = []
    for i in range(3):                       # run 0 creates the buffers, runs 1 and 2 are compared
        if i:
            assert _poison_scratch() >= 2
            assert bool(torch.isnan(next(iter(ops._col_cache.values())).view(torch.float32)).all())
        wp, bp, xp = w.clone().requires_grad_(True), b.clone().requires_grad_(True), _cl(x.clone()).requires_grad_(True)
        y = conv3x3_strided(xp, wp, bp, 2, True)
        (y * dy).sum().backward()
        torch.cuda.synchronize()
        runs.append([y.detach().clone(), xp.grad.clone(), wp.grad.clone(), bp.grad.clone()])
    for a, c in zip(runs[1], runs[2]):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, c)


# ------------------------------------------------------------------ 4. the stride-2 bottleneck
def _block(inplanes, planes, stride):
    from iouaware.backbones import Bottleneck
    from iouaware.layers import build_norm_layer
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                       build_norm_layer(dict(type='BN'), planes * 4)[1])
    torch.manual_seed(1234 + inplanes + planes)
    m = Bottleneck(inplanes, planes, stride, downsample=ds).cuda()
    pre = 'backbone.layer2.0.'               # the fill rules are keyed on the detector's names
    state = {pre + k: v for k, v in m.state_dict().items()}
    synth.e2e_fill_state(state, 11)
    m.load_state_dict({k[len(pre):]: v for k, v in state.items()})
    with torch.no_grad():                    # non-trivial affine parameters everywhere
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    m.train()
    for b in m.modules():
        if isinstance(b, nn.modules.batchnorm._BatchNorm):
            b.eval()                          # norm_eval=True
    return m


def _spy(monkeypatch, mod, name):
    calls = []
    real = getattr(mod, name)

    def spy(*a, **k):
        calls.append(name)
        return real(*a, **k)
    monkeypatch.setattr(mod, name, spy)
    return calls


def test_stride2_bottleneck_switch_on_vs_off(monkeypatch):
    """The bounds of test_bottleneck_training_route_vs_module (tests/test_gpu_train_fuse.py), restated:
    float64 on the CPU is the yardstick; the output within 1e-4 of its maximum; every gradient
    norm-wise within max(4 x the other route's distance, 5e-3) of the yardstick (single ReLU-mask
    flips where a pre-activation is within fp32 rounding of zero move a gradient by ~1e-3 of its
    norm); the input gradient elementwise within 1e-4 of its rms on 98 % of the elements."""
    from iouaware import ops
    from iouaware.backbones import ResNet
    from iouaware.fuse import fuse_inference, unfuse_inference
    m = _block(64, 32, 2)
    g = _gen(2)
    x0 = torch.randn(2, 64, 14, 18, device='cuda', generator=g).relu()
    up = torch.randn(2, 128, 7, 9, device='cuda', generator=g)
    m64 = copy.deepcopy(m).cpu().double()
    x64 = x0.cpu().double().requires_grad_(True)
    (m64(x64) * up.cpu().double()).sum().backward()
    ref = (x64.grad, {k: p.grad for k, p in m64.named_parameters()})
    calls = _spy(monkeypatch, ops, 'col2im3x3')
    res = {}
    for mode in ('off', 'on'):
        monkeypatch.setattr(ResNet, 'train_strided', mode == 'on')   # a block fused on its own: the class default
        assert fuse_inference(m, winograd=True, train=True) > 0
        assert m._ia_train_strided is (mode == 'on')
        m.zero_grad(set_to_none=True)
        x = _cl(x0.clone()).requires_grad_(True)
        y = m(x)
        (y * up).sum().backward()
        res[mode] = (y.detach(), x.grad, {k: p.grad.clone() for k, p in m.named_parameters()})
        unfuse_inference(m)
        assert len(calls) == (1 if mode == 'on' else 0)
    (ya, xa, pa), (yb, xb, pb) = res['on'], res['off']
    assert ya.shape == yb.shape and float((ya - yb).abs().max() / yb.abs().max()) < 1e-4
    assert set(pa) == set(pb) == set(ref[1])

    def dist(t, r):
        return float((t.detach().cpu().double() - r).norm() / r.norm().clamp(min=1e-300))
    assert dist(xa, ref[0]) <= max(4 * dist(xb, ref[0]), 5e-3)
    err = (xa.detach().cpu().double() - ref[0]).abs().flatten()
    rms = float(ref[0].pow(2).mean().sqrt())
    assert float(torch.quantile(err[::7], 0.98)) <= 1e-4 * rms
    for k in pb:
        assert dist(pa[k], ref[1][k]) <= max(4 * dist(pb[k], ref[1][k]), 5e-3), \
            (k, dist(pa[k], ref[1][k]), dist(pb[k], ref[1][k]))


# ------------------------------------------------------------------ 5. the whole detector, one iteration
class _ConvCounter(TorchDispatchMode):
    """counts the aten convolution / convolution-backward operators that reach the dispatcher"""

    def __init__(self):
        super().__init__()
        self.fwd, self.bwd, self.names = 0, 0, set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if 'convolution' in name or 'conv2d' in name:
            self.names.add(name)
            if 'backward' in name:
                self.bwd += 1
            else:
                self.fwd += 1
        return func(*args, **(kwargs or {}))


_SMALL = (2, 256, 320, 250, 317)             # B, pad h, pad w, image h, image w (test_gpu_train_fuse.py's first size)


@functools.lru_cache(maxsize=None)
def _iteration(strided, run):
    """one training iteration of the R-50 IoU-aware RetinaNet on the fused training route, both
    switches `strided` -> (loss dict, total loss, {parameter: gradient}, conv ops forward, backward,
    their names).  `run` only separates repeated evaluations in the cache."""
    B, ph, pw, ih, iw = _SMALL
    gts, gls = synth.train_targets(11, B, ih, iw, max_gt=6)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    metas = [synth.img_meta(ih, iw, ph, pw) for _ in range(B)]
    img = _cl(torch.from_numpy(synth.e2e_image(3, B, ph, pw, ih, iw)).cuda())
    import bench
    import iouaware
    from iouaware.config import ConfigDict
    from iouaware.fuse import fuse_inference
    from iouaware.train import parse_losses
    torch.manual_seed(0)
    model = iouaware.build_detector(ConfigDict(bench.MODEL), train_cfg=ConfigDict(bench.TRAIN_CFG),
                                    test_cfg=ConfigDict(bench.TEST_CFG))
    state = model.state_dict()
    synth.e2e_fill_state(state, 7)
    model.load_state_dict(state)
    model = model.cuda().train()
    model.backbone.train_strided = model.neck.train_strided = bool(strided)
    model.bbox_head.train_winograd = True
    assert fuse_inference(model, winograd=True, train=True) > 0
    with _ConvCounter() as cc:
        losses = model(img, metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
        loss, logv = parse_losses(losses)
        loss.backward()
    torch.cuda.synchronize()
    ld = {k: [v.detach().clone() for v in vs] for k, vs in losses.items() if 'loss' in k}
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return ld, loss.detach().clone(), grads, cc.fwd, cc.bwd, sorted(cc.names)


def _rel2(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def test_detector_iteration_convolution_ops_leave_the_framework():
    """the three stride-2 conv2 and P6 / P7: five forward and five backward operators fewer, and
    none left (frozen stem and stage 1 on the inference kernels, every other convolution a node of
    train_fuse.py / winograd_train.py: DESIGN 3.12)"""
    off, on = _iteration(False, 0), _iteration(True, 0)
    print('  aten convolution ops, switches off: %d fwd %d bwd %s | on: %d fwd %d bwd %s'
          % (off[3], off[4], off[5], on[3], on[4], on[5]))
    assert off[3] - on[3] == 5 and off[4] - on[4] == 5
    assert on[3] == 0 and on[4] == 0, on[5]


def test_detector_iteration_switch_on_vs_off():
    """the bounds of test_whole_detector_training_iteration_fused_vs_module, restated: total loss to
    1e-4; every parameter gradient norm-wise within 5e-2 (single ReLU-mask flips), all gradients
    together within 5e-3"""
    (lda, la, ga, *_), (ldb, lb, gb, *_) = _iteration(True, 0), _iteration(False, 0)
    la, lb = float(la), float(lb)
    assert abs(la - lb) <= 1e-4 * abs(lb), (la, lb)
    assert set(lda) == set(ldb)
    for k in ldb:
        for a, b in zip(lda[k], ldb[k]):
            assert abs(float(a) - float(b)) <= 1e-4 * max(abs(float(b)), 1e-3), (k, float(a), float(b))
    assert set(ga) == set(gb)
    worst = max((_rel2(ga[k], gb[k]), k) for k in gb)
    print('  worst parameter gradient, switches on vs off: %.3e at %s' % worst)
    assert worst[0] < 5e-2, worst
    total = torch.cat([g.flatten() for g in ga.values()]), torch.cat([gb[k].flatten() for k in ga])
    print('  all gradients together: %.3e' % _rel2(*total))
    assert _rel2(*total) < 5e-3


def test_detector_iteration_same_bits_twice():
    """both switches on, the framework's `deterministic` flag left off: loss dict and every
    parameter gradient bit-identical in two evaluations"""
    assert torch.backends.cudnn.deterministic is False
    (lda, la, ga, *_), (ldb, lb, gb, *_) = _iteration(True, 0), _iteration(True, 1)
    assert torch.equal(la, lb)
    for k in lda:
        assert all(torch.equal(a, b) for a, b in zip(lda[k], ldb[k])), k
    assert set(ga) == set(gb)
    diff = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not diff, diff[:8]
    assert not any(bool(torch.isnan(g).any()) for g in ga.values())


# ------------------------------------------------------------------ 6. the reference's iteration
def test_training_iteration_vs_the_reference_with_the_switches_on(golden_dir):
    """tests/golden/train_e2e.npz (one training iteration of the reference detector on the CPU, the
    fixture of test_training_iteration_vs_the_reference): loss dict within 1e-4, every parameter's
    gradient norm within 2e-4"""
    import bench
    import iouaware
    from iouaware.config import ConfigDict
    from iouaware.fuse import fuse_inference
    f = np.load(os.path.join(golden_dir, 'train_e2e.npz'))
    ih, iw, ph, pw = [int(v) for v in f['img']]
    B = int(f['batch'])
    img_np = synth.e2e_image(int(f['image_seed']), B, ph, pw, ih, iw)
    assert synth.checksum([img_np]) == int(f['img_checksum'])
    gts, gls = synth.train_targets(int(f['target_seed']), B, ih, iw, max_gt=6)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    metas = [synth.img_meta(ih, iw, ph, pw) for _ in range(B)]
    torch.manual_seed(0)
    model = iouaware.build_detector(ConfigDict(bench.MODEL), train_cfg=ConfigDict(bench.TRAIN_CFG),
                                    test_cfg=ConfigDict(bench.TEST_CFG))
    state = model.state_dict()
    synth.e2e_fill_state(state, int(f['weight_seed']))
    model.load_state_dict(state)
    model = model.cuda().train()
    model.backbone.train_strided = model.neck.train_strided = True
    assert fuse_inference(model, winograd=True, train=True) > 0
    model = model.to(memory_format=torch.channels_last)
    x = _cl(torch.from_numpy(img_np).cuda())
    losses = model(x, metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
    total = sum(sum(v) for k, v in losses.items() if 'loss' in k)
    total.sum().backward()
    for k in ('loss_cls', 'loss_bbox', 'losses_iou'):
        got = np.array([float(v.detach()) for v in losses[k]])
        print('  %s worst deviation %.3e' % (k, float(np.max(np.abs(got - f[k]) / np.maximum(np.abs(f[k]), 1e-3)))))
        assert np.all(np.abs(got - f[k]) <= 1e-4 * np.maximum(np.abs(f[k]), 1e-3)), (k, got, f[k])
    assert abs(float(total.detach().sum()) - float(f['total'])) <= 1e-4 * float(f['total'])
    grads = {k: p.grad for k, p in model.named_parameters()}
    dev = []
    for name, want in zip(f['grad_names'].tolist(), f['grad_norms']):
        assert grads[name] is not None, name
        got = float(grads[name].double().norm())
        dev.append((abs(got - want) / max(want, 1e-12), name))
    print('  worst gradient-norm deviation %.3e at %s (bound 2e-4)' % max(dev))
    assert max(dev)[0] <= 2e-4, max(dev)

"""GPU: `fuse_head_loss` of the FCOS heads (_FCOSHeadBase.forward_loss) -- towers, output convolutions,
point targets and the loss node on the packed channels-last rows with nothing in between, on top of
`train_bf16` and of `train_winograd`; the small heads of tests/test_gpu_fcos_bf16_train.py (64
channels, 2 tower layers, levels 16x24 ... 1x2, batch 2, both head kinds).

  * route: the loss node receives the output convolutions' own tensors (channels-last, the route's
    dtype) and no Scale module runs;
  * fp32 (Winograd) route: loss dict, parameter and feature gradients against the same model with the
    switch off, under the Winograd node's gates (max-relative 1e-4 on the values, relative L2 1e-4 and
    max-relative 2e-4 on the gradients: the towers compute the same bits, so no ReLU mask differs);
  * bf16 route: against the fp64 module, RMS error <= 1.5 x that of the same tree with the switch off
    + 1e-3 of the tensor's maximum, pooled over four draws (the bf16 contract of
    test_gpu_fcos_bf16_train.py; the comparator is the switch-off route);
  * a head the routes do not cover falls back bit for bit; one whole-detector train_step is finite and
    repeatable within the fp32 bound (the loss sums are fp64 atomics: not bit for bit)."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import synth
import synth_fcos_loss as S
from test_gpu_fcos_bf16_train import DRAWS, LEVELS, _deterministic_library, _small_head

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
IMG_H, IMG_W = 64, 96                       # LEVELS at the default strides 4 .. 64


def _cfg():
    from iouaware.config import ConfigDict
    return ConfigDict(dict(gamma=2.0, alpha=0.25))


def _gts(seed):
    gb, gl = S.gts(seed, 2, IMG_H, IMG_W, 3, 8, num_classes=4)
    return gb, gl


def _feats(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, 64, h, w, generator=g) for (h, w) in LEVELS]


def _run(head, feats, gb, gl):
    """forward_loss + backward of the sum -> {name: fp64 CPU tensor} of losses, parameter gradients and
    the feature gradient as one tensor"""
    dev = next(head.parameters()).device
    head.zero_grad()
    xs = [f.to(dev).clone().requires_grad_(True) for f in feats]
    dt = xs[0].dtype
    losses = head.forward_loss(xs, [torch.from_numpy(b).to(dev, dt) for b in gb],
                               [torch.from_numpy(x).to(dev) for x in gl], None, _cfg())
    sum(v.sum() for v in losses.values()).backward()
    res = {k: v.detach().double().cpu() for k, v in losses.items()}
    res.update({n: p.grad.detach().double().cpu() for n, p in head.named_parameters()})
    res['features'] = torch.cat([x.grad.detach().double().cpu().reshape(-1) for x in xs])
    return res, losses


def _set_route(head, route, fuse):
    head.train_bf16, head.train_winograd = route == 'bf16', route == 'winograd'
    head.fuse_head_loss = fuse
    return head


@contextlib.contextmanager
def _spies(head, route):
    """records the loss node's inputs, the outputs of the route's convolution nodes and Scale forwards"""
    from iouaware import conv3x3_bf16_train, fcos_ops, winograd_train
    seen = dict(packed=[], conv=[], scale=[])
    real_packed = fcos_ops.point_head_loss_packed
    mod, name = (conv3x3_bf16_train, 'conv_levels') if route == 'bf16' else (winograd_train, 'wino_conv_levels')
    real_conv = getattr(mod, name)

    def packed(geom, cls_ctr, reg_iou, scales, *a, **k):
        seen['packed'].append((list(cls_ctr), list(reg_iou), list(scales)))
        return real_packed(geom, cls_ctr, reg_iou, scales, *a, **k)

    def conv(*a, **k):
        out = real_conv(*a, **k)
        seen['conv'].extend(out if route == 'winograd' else [t for g in out for t in g])
        return out
    fcos_ops.point_head_loss_packed = packed
    setattr(mod, name, conv)
    hooks = [m.register_forward_hook(lambda *a: seen['scale'].append(1)) for m in head.scales]
    try:
        yield seen
    finally:
        fcos_ops.point_head_loss_packed = real_packed
        setattr(mod, name, real_conv)
        for h in hooks:
            h.remove()


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
@pytest.mark.parametrize('route', ['bf16', 'winograd'])
def test_packed_rows_go_straight_into_the_loss_node(route, iou_branch):
    head = _set_route(_small_head(iou_branch).to(DEV), route, True)
    gb, gl = _gts(61)
    with _spies(head, route) as seen:
        res, losses = _run(head, _feats(9), gb, gl)
    assert list(losses) == ['loss_cls', 'loss_reg', 'loss_centerness'] + (['loss_iou'] if iou_branch else [])
    assert len(seen['packed']) == 1 and not seen['scale'], seen['scale']
    cls_ctr, reg_iou, scales = seen['packed'][0]
    dtype = torch.bfloat16 if route == 'bf16' else torch.float32
    assert len(cls_ctr) == len(reg_iou) == len(scales) == len(LEVELS)
    for t, (h, w) in list(zip(cls_ctr, LEVELS)) + list(zip(reg_iou, LEVELS)):
        assert t.dtype == dtype and t.shape[0] == 2 and tuple(t.shape[2:]) == (h, w)
        assert t.is_contiguous(memory_format=torch.channels_last) and t.shape[1] % 4 == 0
        # the output convolution's own tensor: no slice, no copy, no conversion behind it
        assert any(t is o for o in seen['conv']), 'not a convolution output'
    assert all(s is m.scale for s, m in zip(scales, head.scales))
    for n, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(head.scales[0].scale.grad.abs()) > 0      # (64 x 96 images: positives on the first levels)
    # the switch off: the reference's tuple through loss(), Scale modules and all
    _set_route(head, route, False)
    with _spies(head, route) as seen:
        _run(head, _feats(9), gb, gl)
    assert not seen['packed'] and len(seen['scale']) == len(LEVELS)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _rel2(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_fp32_route_against_the_switch_off(iou_branch):
    head = _small_head(iou_branch).to(DEV)
    gb, gl = _gts(62)
    feats = _feats(10)
    on, _ = _run(_set_route(head, 'winograd', True), feats, gb, gl)
    off, _ = _run(_set_route(head, 'winograd', False), feats, gb, gl)
    assert list(on) == list(off)
    for k in off:
        print('%-34s L2 %.3e  max %.3e' % (k, _rel2(on[k], off[k]), _rel(on[k], off[k])))
        assert on[k].shape == off[k].shape
        if k.startswith('loss_'):
            assert _rel(on[k], off[k]) < 1e-4, k
        else:
            assert _rel2(on[k], off[k]) < 1e-4 and _rel(on[k], off[k]) < 2e-4, k


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_bf16_route_against_fp64(iou_branch):
    sq, top = {}, {}
    for draw in range(DRAWS):
        head = _small_head(iou_branch, seed=7 + draw)
        gb, gl = _gts(63 + draw)
        feats = _feats(20 + draw)
        h64 = copy.deepcopy(head).double()
        h64.fuse_loss = False
        with S.torch_route(cpu_focal=True):
            ref, _ = _run(h64, [f.double() for f in feats], gb, gl)
        dev = copy.deepcopy(head).to(DEV)
        with _spies(dev, 'bf16') as seen:
            got, _ = _run(_set_route(dev, 'bf16', True), feats, gb, gl)
        assert len(seen['packed']) == 1
        cmp_, _ = _run(_set_route(dev, 'bf16', False), feats, gb, gl)
        assert sorted(got) == sorted(ref) == sorted(cmp_)
        for k in ref:
            a = sq.setdefault(k, [0.0, 0.0, 0])
            a[0] += float((got[k] - ref[k]).pow(2).sum())
            a[1] += float((cmp_[k] - ref[k]).pow(2).sum())
            a[2] += ref[k].numel()
            top[k] = max(top.get(k, 0.0), float(ref[k].abs().max()))
    for k in sorted(sq):
        e_got, e_cmp = (sq[k][0] / sq[k][2]) ** 0.5, (sq[k][1] / sq[k][2]) ** 0.5
        print('%-34s max %.3g  switch on %.3g  switch off %.3g  ratio %.2f'
              % (k, top[k], e_got, e_cmp, e_got / max(e_cmp, 1e-30)))
    for k in sorted(sq):
        e_got, e_cmp = (sq[k][0] / sq[k][2]) ** 0.5, (sq[k][1] / sq[k][2]) ** 0.5
        assert e_got <= 1.5 * e_cmp + 1e-3 * top[k], (k, e_got, e_cmp, top[k])


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_a_head_the_routes_do_not_cover_falls_back(iou_branch):
    """48 feature channels: no multiple of 32, the bf16 route does not take it -- forward_loss gives the
    switch-off result bit for bit, through loss(*forward())"""
    from iouaware import conv3x3_bf16_train as T
    head = _small_head(iou_branch, feat_channels=48, num_groups=6).to(DEV)
    gb, gl = _gts(64)
    feats = _feats(11)
    assert not T.fcos_usable([f.to(DEV) for f in feats], head)
    with _deterministic_library():
        with _spies(head, 'bf16') as seen:
            on, _ = _run(_set_route(head, 'bf16', True), feats, gb, gl)
        assert not seen['packed'] and len(seen['scale']) == len(LEVELS)
        off, _ = _run(_set_route(head, 'bf16', False), feats, gb, gl)
    for k in off:
        assert torch.equal(on[k], off[k]), k
    # evaluation mode and gamma != 2 fall back as well
    _set_route(head, 'winograd', True)
    from iouaware.config import ConfigDict
    xs = [f.to(DEV) for f in feats]
    tail = ([torch.from_numpy(b).to(DEV) for b in gb], [torch.from_numpy(x).to(DEV) for x in gl], None)
    with _spies(head, 'winograd') as seen:
        head.forward_loss(xs, *tail, ConfigDict(dict(gamma=1.5, alpha=0.25)))
        head.eval()
        with torch.no_grad():
            head.forward_loss(xs, *tail, _cfg())
        head.train()
    assert not seen['packed']


@pytest.mark.parametrize('route', ['bf16', 'winograd'])
def test_detector_step_is_finite_and_repeatable(route):
    """one train_step of the small IoU-aware FCOS detector with the switch on, twice from one state:
    finite, and the same to the fp32 bound (1e-4 of each tensor's maximum; the loss sums are fp64
    atomics whose order changes from run to run, so the last bits of the normalisers may differ)"""
    from iouaware.train import build_optimizer, train_step
    from test_gpu_fcos import _model
    cfg, model = _model(5)
    model.train()
    _set_route(model.bbox_head, route, True)
    assert model.bbox_head.fuse_head_loss
    B, ph, pw = 2, 128, 160
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(B, 3, ph, pw, device='cuda', generator=g)
    gts, gls = synth.train_targets(11, B, ph, pw, max_gt=5)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    metas = [synth.img_meta(ph, pw, ph, pw) for _ in range(B)]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    runs = []
    with _deterministic_library(), _spies(model.bbox_head, route) as seen:
        for _ in range(2):
            model.load_state_dict(state)
            opt = build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001))
            log = train_step(model, opt, img, metas, gtb, gtl)
            runs.append((log, {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}))
    assert len(seen['packed']) == 2 and not seen['scale']
    (la, ga), (lb, gb_) = runs
    assert all(v == v and abs(v) != float('inf') for v in la.values()), la
    assert any(n.startswith('bbox_head.scales') for n in ga)
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-4 * abs(la[k]), (k, la[k], lb[k])
    for n in ga:
        assert bool(torch.isfinite(ga[n]).all()), n
        assert float((ga[n] - gb_[n]).abs().max()) <= 1e-4 * float(ga[n].abs().max()), n

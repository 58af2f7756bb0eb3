"""GPU: the FCOS heads' training forward on the Winograd tower convolutions and the HIP GroupNorm +
ReLU node (winograd_train.fcos_head_forward) against the module route (`train_winograd = False`:
torch GroupNorm autograd, library convolutions) on one state dict, the reference's training
fixtures (tests/golden/fcos_train.npz, fcos_plain_train.npz) through the new route with hooks that
prove no tower module ran, and the fallback for a head the route does not cover.

Bounds of the route comparison: those of
test_gpu_retina_plain_train.py::test_plain_head_forward_backward_matches_module_path -- outputs
max-relative < 1e-4; gradients relative L2 < 1e-4 and max-relative < 2e-4 where every ReLU is the
identity in both routes ('all_active': GroupNorm beta = 6, so the head is smooth and the two routes
differ by rounding alone).  With ReLUs that switch, single mask flips between two routes whose
pre-activations differ by rounding move individual gradient entries; that variant keeps the loose
bounds of the mirrored test (5e-2 / 1.0) and the 1e-4 bound on the outputs."""
import contextlib
import os

import numpy as np
import pytest
import torch

import synth_fcos

pytestmark = [pytest.mark.gpu, pytest.mark.module_path]
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device('cuda:0')
TOL = 1e-4


@contextlib.contextmanager
def _deterministic_library():
    saved = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _rel2(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _tower_hooks(head, ran):
    """forward hooks on every GroupNorm module and every tower nn.Conv2d of the head"""
    mods = [m for m in head.modules() if isinstance(m, torch.nn.GroupNorm)]
    mods += [m.conv for m in list(head.cls_convs) + list(head.reg_convs)]
    assert len(mods) == 4 * head.stacked_convs
    return [m.register_forward_hook(lambda mod, *a: ran.append(type(mod).__name__)) for m in mods]


def _train_head(iou_branch, strict, **kw):
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    torch.manual_seed(3)
    args = dict(num_classes=81, in_channels=256)
    args.update(kw)
    head = (IoUawareFCOSHead if iou_branch else FCOSHead)(**args).to(DEV).train()
    with torch.no_grad():                      # activations of unit scale through the towers
        for n, p in head.named_parameters():
            if p.dim() == 4:
                p.normal_(0, (2.0 / (9 * p.shape[1])) ** 0.5)
            elif n.endswith('.gn.weight'):
                p.normal_(1.0, 0.1)
            elif n.endswith('.gn.bias'):
                p.fill_(6.0) if strict else p.normal_(0, 0.3)
            elif n.endswith('.scale'):
                p.uniform_(0.8, 1.2)
            else:
                p.normal_(0, 0.1)
        for c in (head.fcos_reg,):             # exp(scale * reg) of moderate size
            c.weight.mul_(0.1)
    return head


@pytest.mark.parametrize('layout', ['nchw', 'channels_last', 'all_active'])
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_head_forward_backward_matches_module_path(iou_branch, layout):
    strict = layout == 'all_active'
    head = _train_head(iou_branch, strict)
    assert head.feat_channels == 256 and head.cls_convs[0].gn.num_groups == 32
    g = torch.Generator(device='cuda').manual_seed(1)
    sizes = synth_fcos.level_shapes(224, 288)
    feats = [torch.randn(2, 256, h, w, device='cuda', generator=g) for (h, w) in sizes]
    if layout == 'channels_last':
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    ups, res = None, {}
    with _deterministic_library():
        for mode in (True, False):
            head.train_winograd = mode
            head.zero_grad()
            xs = [f.clone().requires_grad_(True) for f in feats]
            ran = []
            hooks = _tower_hooks(head, ran)
            outs = head(xs)
            for h in hooks:
                h.remove()
            assert (not ran) == mode, ran
            assert len(outs) == (4 if iou_branch else 3)
            for m, ch in zip(outs, (80, 4, 1, 1)):
                assert len(m) == len(sizes)
                for t, (h, w) in zip(m, sizes):
                    assert tuple(t.shape) == (2, ch, h, w) and t.is_contiguous()
            if ups is None:
                ups = [[torch.randn(t.shape, device='cuda', generator=g) for t in o] for o in outs]
            loss = sum((t * u).sum() for o, us in zip(outs, ups) for t, u in zip(o, us))
            loss.backward()
            res[mode] = ([t.detach() for o in outs for t in o],
                         {n: p.grad.clone() for n, p in head.named_parameters()},
                         [x.grad.contiguous() for x in xs])
    (oa, ga, xa), (ob, gb, xb) = res[True], res[False]
    for a, b in zip(oa, ob):
        assert _rel(a, b) < 1e-4
    tol2, tol = (1e-4, 2e-4) if strict else (5e-2, 1.0)
    assert set(ga) == set(gb) == set(n for n, _ in head.named_parameters())
    for n in gb:
        print(layout, n, _rel2(ga[n], gb[n]), _rel(ga[n], gb[n]))
        assert ga[n].shape == gb[n].shape and _rel2(ga[n], gb[n]) < tol2, (n, _rel2(ga[n], gb[n]))
        assert _rel(ga[n], gb[n]) < tol, n
    for a, b in zip(xa, xb):
        assert _rel2(a, b) < tol2 and _rel(a, b) < tol


def test_frozen_groupnorm_parameters_get_no_gradient():
    """norm_cfg requires_grad=False: the node returns no parameter gradients, everything else trains"""
    head = _train_head(True, False, norm_cfg=dict(type='GN', num_groups=32, requires_grad=False))
    head.train_winograd = True
    sizes = synth_fcos.level_shapes(128, 160)
    feats = [torch.randn(2, 256, h, w, device='cuda') for (h, w) in sizes]
    ran = []
    hooks = _tower_hooks(head, ran)
    outs = head(feats)
    for h in hooks:
        h.remove()
    assert not ran
    sum(t.sum() for o in outs for t in o).backward()
    for n, p in head.named_parameters():
        if '.gn.' in n:
            assert p.grad is None, n
        elif 'centerness' not in n:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, n


@pytest.mark.parametrize('tag', ['iou', 'plain'])
def test_training_fixture_through_the_winograd_route(tag):
    """test_gpu_fcos.py / test_gpu_fcos_plain.py::test_training_step_against_reference (losses 1e-4,
    gradient norms 2e-4 against the reference's arrays) with hooks on the towers: no
    torch.nn.GroupNorm module and no tower nn.Conv2d runs"""
    from iouaware.config import ConfigDict
    if tag == 'iou':
        from test_gpu_fcos import _model
        fixture = 'fcos_train.npz'
    else:
        from test_gpu_fcos_plain import _model
        fixture = 'fcos_plain_train.npz'
    g = np.load(os.path.join(GOLD, fixture), allow_pickle=False)
    img_h, img_w, pad_h, pad_w = (int(v) for v in g['shape'])
    for case in ('pos', 'nopos'):
        cfg, m = _model(int(g['weight_seed']))
        m.train()
        head = m.bbox_head
        head.train_winograd = True
        x = torch.from_numpy(synth_fcos.image(int(g['image_seed']), 2, pad_h, pad_w, img_h, img_w)).to(DEV)
        metas = [dict(ori_shape=(img_h, img_w, 3), img_shape=(img_h, img_w, 3),
                      pad_shape=(pad_h, pad_w, 3), scale_factor=1.0, flip=False)] * 2
        if case == 'pos':
            gb = [g['pos_gt_bboxes_%d' % i] for i in range(2)]
            gl = [g['pos_gt_labels_%d' % i] for i in range(2)]
        else:
            gb = [np.array([[0.5, 0.5, 3.0, 3.0]], np.float32)] * 2
            gl = [np.array([3], np.int64)] * 2
        ran = []
        hooks = _tower_hooks(head, ran)
        outs = head(m.extract_feat(x))
        for h in hooks:
            h.remove()
        assert not ran, ran
        losses = head.loss(*(outs + ([torch.from_numpy(b).to(DEV) for b in gb],
                                     [torch.from_numpy(b).to(DEV) for b in gl], metas,
                                     ConfigDict(cfg.train_cfg))))
        assert len(losses) == (4 if tag == 'iou' else 3)
        for k, v in losses.items():
            ref = g['%s_%s' % (case, k)]
            assert abs(float(v.sum()) - float(ref.sum())) <= TOL * max(1.0, abs(float(ref.sum()))), \
                (case, k, float(v.sum()), float(ref.sum()))
        sum(v.sum() for v in losses.values()).backward()
        named = dict(m.named_parameters())
        for n, ref in zip(g['%s_grad_names' % case], g['%s_grad_norms' % case]):
            p = named[str(n)]
            got = 0.0 if p.grad is None else float(p.grad.norm())
            assert abs(got - ref) <= 2e-4 * max(1.0, ref), (case, str(n), got, float(ref))


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_a_head_the_route_does_not_cover_takes_the_module_route(iou_branch):
    """32 channels in 32 groups (one channel per group: no 16-byte column inside a group), and
    evaluation mode: the modules run, with the results of train_winograd = False"""
    from iouaware import winograd_train
    head = _train_head(iou_branch, False, in_channels=32, feat_channels=32, stacked_convs=2)
    sizes = synth_fcos.level_shapes(128, 160)
    feats = [torch.randn(2, 32, h, w, device='cuda') for (h, w) in sizes]
    assert not winograd_train.fcos_usable(feats, head)
    res = {}
    with _deterministic_library():
        for mode in (True, False):
            head.train_winograd = mode
            head.zero_grad()
            ran = []
            hooks = _tower_hooks(head, ran)
            outs = head(feats)
            for h in hooks:
                h.remove()
            assert len(ran) == len(sizes) * 4 * head.stacked_convs
            sum((t * t).sum() for o in outs for t in o).backward()
            res[mode] = ([t.detach() for o in outs for t in o],
                         {n: p.grad.clone() for n, p in head.named_parameters()})
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    for n in res[False][1]:
        assert _rel(res[True][1][n], res[False][1][n]) < 1e-5, n
    # evaluation mode and no_grad: never the training route
    wide = _train_head(iou_branch, False)
    feats = [torch.randn(2, 256, h, w, device='cuda') for (h, w) in sizes]
    assert winograd_train.fcos_usable(feats, wide)
    with torch.no_grad():
        assert not winograd_train.fcos_usable(feats, wide)
    wide.eval()
    ran = []
    hooks = _tower_hooks(wide, ran)
    wide(feats)
    for h in hooks:
        h.remove()
    assert ran

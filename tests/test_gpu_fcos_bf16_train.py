"""GPU: bf16 training of the FCOS heads (conv3x3_bf16_train.fcos_head_forward: the MFMA convolution
node and the bf16 GroupNorm + ReLU node, `head.train_bf16 = True`) -- both heads against the fp64
module and torch's own bf16 module route, the reference's training fixtures through the route, the
routing of heads it does not cover, frozen GroupNorm parameters and one detector step.

The bf16 contract (README "Parity", tests/test_gpu_conv3x3_bf16_train.py::
test_head_against_fp64_and_torch_bf16): the RMS error against the fp64 module at most 1.5 x that of
torch's bf16 module route + 1e-3 of the tensor's maximum, pooled over four independent draws (RMS and
pooled for the reasons given there: a pre-activation within bf16 rounding of zero falls on either
side of the ReLU mask in any bf16 evaluation)."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

import synth
import synth_fcos

pytestmark = pytest.mark.gpu
BF, CL = torch.bfloat16, torch.channels_last
DEV = torch.device('cuda:0')
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
LEVELS = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
DRAWS = 4


@contextlib.contextmanager
def _deterministic_library():
    saved = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


@contextlib.contextmanager
def _route_calls():
    """counts the calls of the bf16 FCOS route"""
    from iouaware import conv3x3_bf16_train as T
    calls, real = [], T.fcos_head_forward

    def spy(head, feats):
        calls.append(type(head).__name__)
        return real(head, feats)
    T.fcos_head_forward = spy
    try:
        yield calls
    finally:
        T.fcos_head_forward = real


def _tower_hooks(head, ran):
    """forward hooks on every GroupNorm module and every tower nn.Conv2d of the head"""
    mods = [m for m in head.modules() if isinstance(m, torch.nn.GroupNorm)]
    mods += [m.conv for m in list(head.cls_convs) + list(head.reg_convs)]
    assert len(mods) == 4 * head.stacked_convs
    return [m.register_forward_hook(lambda mod, *a: ran.append(type(mod).__name__)) for m in mods]


def _small_head(iou_branch, seed=7, in_channels=64, feat_channels=64, num_groups=8, requires_grad=True):
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    torch.manual_seed(seed)
    head = (IoUawareFCOSHead if iou_branch else FCOSHead)(
        num_classes=5, in_channels=in_channels, feat_channels=feat_channels, stacked_convs=2,
        norm_cfg=dict(type='GN', num_groups=num_groups, requires_grad=requires_grad))
    with torch.no_grad():                      # activations of unit scale through the towers
        for n, p in head.named_parameters():
            if p.dim() == 4:
                p.normal_(0, (2.0 / (9 * p.shape[1])) ** 0.5)
            elif n.endswith('.gn.weight'):
                p.normal_(1.0, 0.1)
            elif n.endswith('.gn.bias'):
                p.normal_(0, 0.3)
            elif n.endswith('.scale'):
                p.uniform_(0.8, 1.2)
            else:
                p.normal_(0, 0.1)
        head.fcos_reg.weight.mul_(0.1)         # exp(scale * reg) of moderate size
    return head.train()


def _run_head(head, feats, ups):
    head.zero_grad()
    xs = [f.clone().requires_grad_(True) for f in feats]
    outs = head(xs)
    flat = [t for o in outs for t in o]
    (sum((t.double() * u.to(t.device).double()).sum() for t, u in zip(flat, ups))).backward()
    res = {'out%d' % i: t.detach().double().cpu() for i, t in enumerate(flat)}
    res.update({n: p.grad.detach().double().cpu() for n, p in head.named_parameters()})
    # the feature gradient as ONE tensor over the levels (the smallest levels hold a handful of terms)
    res['features'] = torch.cat([x.grad.detach().double().cpu().reshape(-1) for x in xs])
    return res, outs


def _kind(name):
    if name.startswith('out') or name == 'features':
        return 'outputs' if name.startswith('out') else 'features'
    if '.gn.' in name:
        return 'GroupNorm parameters'
    if 'convs' in name:
        return 'tower weights'
    return 'output convolutions / scales'


@pytest.mark.parametrize('iou', [False, True], ids=['plain', 'iou'])
def test_head_against_fp64_and_torch_bf16(iou):
    B = 2
    sq, top = {}, {}                       # per tensor: squared errors (route, comparator), count; max |ref|
    for draw in range(DRAWS):
        head = _small_head(iou, seed=7 + draw)
        g = torch.Generator().manual_seed(8 + draw)
        feats = [torch.randn(B, 64, h, w, generator=g) for (h, w) in LEVELS]
        widths = [4, 4, 1] + ([1] if iou else [])
        ups = [torch.randn(B, c, h, w, generator=g) for c in widths for (h, w) in LEVELS]
        # yardstick: the module in fp64 on the CPU; comparator: torch's bf16 module route on the device
        ref, _ = _run_head(copy.deepcopy(head).double(), [f.double() for f in feats], ups)
        cmp_, _ = _run_head(copy.deepcopy(head).cuda().to(BF),
                            [f.cuda().to(BF).contiguous(memory_format=CL) for f in feats], ups)
        dev = copy.deepcopy(head).cuda()
        dev.train_bf16 = True
        ran = []
        hooks = _tower_hooks(dev, ran)
        with _route_calls() as calls:
            got, outs = _run_head(dev, [f.cuda() for f in feats], ups)
        for h in hooks:
            h.remove()
        assert calls and not ran, (calls, ran)
        assert len(outs) == (4 if iou else 3)
        for o, c in zip(outs, widths):
            for t, (h, w) in zip(o, LEVELS):
                assert t.dtype == torch.float32 and t.shape == (B, c, h, w) and t.is_contiguous()
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert got[k].shape == ref[k].shape
            a = sq.setdefault(k, [0.0, 0.0, 0])
            a[0] += float((got[k] - ref[k]).pow(2).sum())
            a[1] += float((cmp_[k] - ref[k]).pow(2).sum())
            a[2] += ref[k].numel()
            top[k] = max(top.get(k, 0.0), float(ref[k].abs().max()))
    ratios = {}
    for k in sorted(sq):
        e_got, e_cmp = (sq[k][0] / sq[k][2]) ** 0.5, (sq[k][1] / sq[k][2]) ** 0.5
        print('%-28s max %.3g  bf16 route %.3g  torch bf16 %.3g  ratio %.2f' % (k, top[k], e_got, e_cmp,
                                                                               e_got / max(e_cmp, 1e-30)))
        ratios.setdefault(_kind(k), []).append(e_got / max(e_cmp, 1e-30))
    for kind in sorted(ratios):
        print('%-30s ratio %.2f .. %.2f' % (kind, min(ratios[kind]), max(ratios[kind])))
    for k in sorted(sq):
        e_got, e_cmp = (sq[k][0] / sq[k][2]) ** 0.5, (sq[k][1] / sq[k][2]) ** 0.5
        assert e_got <= 1.5 * e_cmp + 1e-3 * top[k], (k, e_got, e_cmp, top[k])


@pytest.mark.parametrize('tag', ['iou', 'plain'])
def test_training_fixtures_through_the_bf16_route(tag):
    """the reference's training fixtures (tests/golden/fcos_train.npz, fcos_plain_train.npz): every
    loss as close to the reference's value as the losses on the maps of torch's bf16 module route are
    (the same backbone features, the same fp32 loss)"""
    from iouaware.config import ConfigDict
    if tag == 'iou':
        from test_gpu_fcos import _model
        fixture = 'fcos_train.npz'
    else:
        from test_gpu_fcos_plain import _model
        fixture = 'fcos_plain_train.npz'
    g = np.load(os.path.join(GOLD, fixture), allow_pickle=False)
    img_h, img_w, pad_h, pad_w = (int(v) for v in g['shape'])
    cfg, m = _model(int(g['weight_seed']))
    m.train()
    head = m.bbox_head
    x = torch.from_numpy(synth_fcos.image(int(g['image_seed']), 2, pad_h, pad_w, img_h, img_w)).to(DEV)
    metas = [dict(ori_shape=(img_h, img_w, 3), img_shape=(img_h, img_w, 3),
                  pad_shape=(pad_h, pad_w, 3), scale_factor=1.0, flip=False)] * 2
    with torch.no_grad():
        feats = [f.detach() for f in m.extract_feat(x)]
    cmp_head = copy.deepcopy(head).to(BF)
    for case in ('pos', 'nopos'):
        if case == 'pos':
            gb = [g['pos_gt_bboxes_%d' % i] for i in range(2)]
            gl = [g['pos_gt_labels_%d' % i] for i in range(2)]
        else:
            gb = [np.array([[0.5, 0.5, 3.0, 3.0]], np.float32)] * 2
            gl = [np.array([3], np.int64)] * 2
        tail = ([torch.from_numpy(b).to(DEV) for b in gb], [torch.from_numpy(b).to(DEV) for b in gl], metas,
                ConfigDict(cfg.train_cfg))
        head.train_bf16 = True
        head.zero_grad()
        ran = []
        hooks = _tower_hooks(head, ran)
        with _route_calls() as calls:
            outs = head(feats)
        for h in hooks:
            h.remove()
        assert calls and not ran, (calls, ran)
        losses = head.loss(*(tuple(outs) + tail))
        sum(v.sum() for v in losses.values()).backward()
        for n, p in head.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        head.train_bf16 = False
        with torch.no_grad():
            cmp_outs = cmp_head([f.to(BF).contiguous(memory_format=CL) for f in feats])
            cmp_losses = head.loss(*(tuple([t.float().contiguous() for t in o] for o in cmp_outs) + tail))
        assert len(losses) == (4 if tag == 'iou' else 3) and sorted(losses) == sorted(cmp_losses)
        for k, v in losses.items():
            ref = float(g['%s_%s' % (case, k)].sum())
            b, c = float(v.sum()), float(cmp_losses[k].sum())
            print('%s %s %s: reference %.6g  bf16 route %.6g  torch bf16 %.6g' % (tag, case, k, ref, b, c))
            assert b == b and abs(b) != float('inf')
            assert abs(b - ref) <= 1.5 * abs(c - ref) + 1e-3 * abs(ref), (case, k, ref, b, c)


@pytest.mark.parametrize('kind', ['four_per_group', 'feat48'])
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_a_head_the_route_does_not_cover_takes_the_next_route(iou_branch, kind):
    """4 channels per group (no whole 16-byte bf16 column inside a group) and 48 feature channels (no
    multiple of 32): the modules run, with the results of train_bf16 = False"""
    from iouaware import conv3x3_bf16_train as T
    kw = dict(num_groups=16) if kind == 'four_per_group' else dict(feat_channels=48, num_groups=6)
    head = _small_head(iou_branch, **kw).to(DEV)
    feats = [torch.randn(2, 64, h, w, device='cuda') for (h, w) in LEVELS]
    assert not T.fcos_usable(feats, head)
    res = {}
    with _deterministic_library():
        for mode in (True, False):
            head.train_bf16 = mode
            head.zero_grad()
            ran = []
            hooks = _tower_hooks(head, ran)
            with _route_calls() as calls:
                outs = head(feats)
            for h in hooks:
                h.remove()
            assert not calls and len(ran) == len(LEVELS) * 4 * head.stacked_convs
            sum((t * t).sum() for o in outs for t in o).backward()
            res[mode] = ([t.detach() for o in outs for t in o],
                         {n: p.grad.clone() for n, p in head.named_parameters()})
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    for n in res[False][1]:
        a, b = res[True][1][n], res[False][1][n]
        assert float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) < 1e-5, n


def test_off_by_default_and_only_in_training():
    """train_bf16 = False leaves the parent's behaviour (the tower modules run); no_grad and
    evaluation mode never take the route"""
    from iouaware import conv3x3_bf16_train as T
    head = _small_head(True).to(DEV)
    feats = [torch.randn(2, 64, h, w, device='cuda') for (h, w) in LEVELS]
    assert head.train_bf16 is False and T.fcos_usable(feats, head)
    for setup in ('default', 'no_grad', 'eval'):
        head.train_bf16 = setup != 'default'
        head.train(setup != 'eval')
        ran = []
        hooks = _tower_hooks(head, ran)
        with _route_calls() as calls, (torch.no_grad() if setup == 'no_grad' else contextlib.nullcontext()):
            head(feats)
        for h in hooks:
            h.remove()
        assert not calls and len(ran) == len(LEVELS) * 4 * head.stacked_convs, setup
    with torch.no_grad():
        assert not T.fcos_usable(feats, head)


def test_frozen_groupnorm_parameters_get_no_gradient():
    head = _small_head(True, requires_grad=False).to(DEV)
    head.train_bf16 = True
    feats = [torch.randn(2, 64, h, w, device='cuda') for (h, w) in LEVELS]
    with _route_calls() as calls:
        outs = head(feats)
    assert calls
    sum(t.sum() for o in outs for t in o).backward()
    for n, p in head.named_parameters():
        if '.gn.' in n:
            assert p.grad is None, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, n


def test_tower_gradients_stay_halves_of_one_tensor():
    """between the nodes of the route the two towers' activations and gradients are the channel halves
    of one tensor per level: the convolution backward takes them in one pass and reads the GroupNorm
    node's input gradient where it lies (no copy)"""
    from iouaware import conv3x3_bf16_train as T, fcos_ops
    head = _small_head(False).to(DEV)
    head.train_bf16 = True
    feats = [torch.randn(2, 64, h, w, device='cuda') for (h, w) in LEVELS]
    seen, real = [], T._mask_and_bias_grad
    T._mask_and_bias_grad = lambda dys, ys, gs, n, want_db: (seen.append((n, ys is None, want_db)),
                                                             real(dys, ys, gs, n, want_db))[1]
    try:
        outs = head(feats)
        sum(t.sum() for o in outs for t in o).backward()
    finally:
        T._mask_and_bias_grad = real
    # only the two output convolutions (bias gradients, padded widths) go through the mask / copy pass
    assert len(seen) == 2 and all(want_db for _, _, want_db in seen), seen


@pytest.mark.parametrize('tag', ['iou', 'plain'])
def test_detector_step_is_finite_and_repeatable(tag):
    """one train_step of the FCOS detectors (small image, B = 2) with the bf16 head, twice from one
    state with the framework's convolutions on their deterministic kernels: finite losses, a finite
    gradient for every parameter, the same bits"""
    from iouaware.train import build_optimizer, train_step
    if tag == 'iou':
        from test_gpu_fcos import _model
    else:
        from test_gpu_fcos_plain import _model
    cfg, model = _model(5)
    model.train()
    model.bbox_head.train_bf16 = True
    B, ph, pw = 2, 128, 160
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(B, 3, ph, pw, device='cuda', generator=g)
    gts, gls = synth.train_targets(11, B, ph, pw, max_gt=5)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    metas = [synth.img_meta(ph, pw, ph, pw) for _ in range(B)]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    runs = []
    with _deterministic_library(), _route_calls() as calls:
        for _ in range(2):
            model.load_state_dict(state)
            opt = build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001))
            log = train_step(model, opt, img, metas, gtb, gtl)
            for n, p in model.named_parameters():
                assert p.grad is not None or not p.requires_grad, n
            runs.append((log, {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}))
    assert len(calls) == 2, calls                                          # the bf16 route was taken
    (la, ga), (lb, gb) = runs
    assert any(n.startswith('bbox_head.') for n in ga)
    assert all(v == v and abs(v) != float('inf') for v in la.values()), la
    for n in ga:
        assert bool(torch.isfinite(ga[n]).all()), n
    assert la == lb, (la, lb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n

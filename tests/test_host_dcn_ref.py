"""CPU side of the deformable convolution: the yardstick (tests/dcn_ref.py) pinned against torch's
convolution, shifted convolutions, border probes and gradcheck; the proof that it tells the nearest
wrong operators apart on the very data of tests/test_gpu_deform_conv.py; and the host-side contract
of the feature -- entries declared / bound / exported and refusing bad arguments without a device,
module parameter names and shapes, the `dcn=` backbones' state_dict keys, `fallback_on_stride`, the
mmdet.ops aliases and every refusal by its named error."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dcn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'iouaware.h')
IA_E_ARG = -1
DCN = dict(modulated=False, deformable_groups=1, fallback_on_stride=False)
STAGES = (False, True, True, True)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ 1: the yardstick itself
@pytest.mark.parametrize('stride,padding,dilation', [(1, 1, 1), (2, 1, 1), (1, 2, 2), (2, 0, 1), (3, 2, 2)])
@pytest.mark.parametrize('dg', [1, 2])
def test_zero_offsets_and_unit_mask_are_the_plain_convolution(stride, padding, dilation, dg):
    g = _gen(3)
    x = torch.randn(2, 8, 9, 7, dtype=torch.float64, generator=g)
    w = torch.randn(5, 8, 3, 3, dtype=torch.float64, generator=g)
    b = torch.randn(5, dtype=torch.float64, generator=g)
    Ho, Wo = R.out_hw(9, 7, 3, stride, padding, dilation)
    off = torch.zeros(2, dg * 18, Ho, Wo, dtype=torch.float64)
    ref = F.conv2d(x, w, b, stride, padding, dilation)
    y2 = R.modulated_deform_conv(x, off, torch.ones(2, dg * 9, Ho, Wo, dtype=torch.float64), w, b, stride,
                                 padding, dilation, dg)
    y1 = R.deform_conv(x, off, w, stride, padding, dilation, dg)
    assert y2.shape == ref.shape
    assert float((y2 - ref).abs().max()) <= 1e-12 and float((y1 - (ref - b.view(1, -1, 1, 1))).abs().max()) <= 1e-12


@pytest.mark.parametrize('dy,dx', [(1, 0), (0, -2), (-3, 2), (4, 4)])
@pytest.mark.parametrize('stride,dilation', [(1, 1), (2, 2)])
def test_integer_offsets_are_the_shifted_zero_padded_convolution(dy, dx, stride, dilation):
    g = _gen(5)
    H, W, p = 7, 9, 1
    x = torch.randn(2, 4, H, W, dtype=torch.float64, generator=g)
    w = torch.randn(3, 4, 3, 3, dtype=torch.float64, generator=g)
    Ho, Wo = R.out_hw(H, W, 3, stride, p, dilation)
    off = torch.zeros(2, 18, Ho, Wo, dtype=torch.float64)
    off[:, 0::2], off[:, 1::2] = dy, dx
    m = 5                                          # a zero margin wider than padding + the largest shift
    xb = F.pad(x, (m, m, m, m))
    win = xb[:, :, m - p + dy: m - p + dy + H + 2 * p, m - p + dx: m - p + dx + W + 2 * p]
    ref = F.conv2d(win, w, None, stride, 0, dilation)
    y = R.deform_conv(x, off, w, stride, p, dilation)
    assert y.shape == ref.shape and float((y - ref).abs().max()) <= 1e-12


def test_border_probes():
    """h = -1, -0.5, 0, H-1, H-0.5, H -> 0, half of row 0, row 0, row H-1, half of row H-1, 0; same in w"""
    H, W = 4, 5
    x = torch.arange(1, 1 + 2 * H * W, dtype=torch.float64).view(1, 2, H, W)
    probes = [-1.0, -0.5, 0.0, H - 1.0, H - 0.5, float(H)]
    h = torch.tensor(probes, dtype=torch.float64).view(1, 1, len(probes), 1, 1)
    s = R.sample(x, h, torch.full_like(h, 2.0), 1)[0, :, :, 0, 0]              # (C, probes) at column 2
    want = torch.stack([0 * x[0, :, 0, 2], 0.5 * x[0, :, 0, 2], x[0, :, 0, 2], x[0, :, H - 1, 2],
                        0.5 * x[0, :, H - 1, 2], 0 * x[0, :, 0, 2]], 1)
    assert torch.equal(s, want)
    probes = [-1.0, -0.5, 0.0, W - 1.0, W - 0.5, float(W)]
    w = torch.tensor(probes, dtype=torch.float64).view(1, 1, len(probes), 1, 1)
    s = R.sample(x, torch.full_like(w, 1.0), w, 1)[0, :, :, 0, 0]
    want = torch.stack([0 * x[0, :, 1, 0], 0.5 * x[0, :, 1, 0], x[0, :, 1, 0], x[0, :, 1, W - 1],
                        0.5 * x[0, :, 1, W - 1], 0 * x[0, :, 1, 0]], 1)
    assert torch.equal(s, want)
    # and the variant that drops the rim differs exactly there
    s0 = R.sample(x, h, torch.full_like(h, 2.0), 1, 'border_ge0')[0, :, :, 0, 0]
    assert bool((s0[:, 1] == 0).all()) and bool((s0[:, 4] == 0).all()) and torch.equal(s0[:, 2:4], s[:, 2:4] * 0 + s0[:, 2:4])


@pytest.mark.parametrize('modulated', [False, True])
def test_gradcheck_at_non_integer_positions(modulated):
    d = R.case(8, 2, 3, 5, 4, 1, 1, modulated, seed=2, batch=2)
    args = [d['x'], d['offset'], d['mask'], d['weight'], d['bias']]
    args = [None if a is None else a.double().requires_grad_(True) for a in args]

    def f(*ts):
        it = iter(ts)
        full = [None if a is None else next(it) for a in args]
        return R.modulated_deform_conv(full[0], full[1], full[2], full[3], full[4], 1, 1, 1, 2)
    assert torch.autograd.gradcheck(f, [a for a in args if a is not None], eps=1e-6, atol=1e-7, rtol=1e-5)


def _gpu_cases():
    for (Cc, dg, Co) in R.CHANNELS:
        for (H, W) in R.MAPS:
            for (s, dl) in R.GEOMS:
                for mod in (False, True):
                    yield Cc, dg, Co, H, W, s, dl, mod


def test_the_gpu_data_has_what_the_issue_asks_for():
    for Cc, dg, Co, H, W, s, dl, mod in _gpu_cases():
        d = R.case(Cc, dg, Co, H, W, s, dl, mod)
        off = d['offset']
        assert float(off.abs().max()) < 3 and float(off.min()) < -2 and float(off.max()) > 2
        frac = (off - off.floor()) * 8
        assert bool((frac == frac.round()).all()) and float(frac.min()) >= 1 and float(frac.max()) <= 7
        h, w = R.positions(off, H, W, 3, 3, s, 1, dl, dg)
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        rim = inside & ((h < 0) | (w < 0) | (h > H - 1) | (w > W - 1))
        assert bool(inside.any()) and bool((~inside).any()) and bool(rim.any())


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_the_yardstick_tells_the_nearest_wrong_operators_apart(variant):
    """on every case of the GPU test the variant applies to, the wrong operator misses gate A in y by
    two orders of magnitude at least -- in fp64 and in the fp32 evaluation alike"""
    n = 0
    for Cc, dg, Co, H, W, s, dl, mod in _gpu_cases():
        if (variant == 'tap_major' and dg == 1) or (variant == 'no_mask' and not mod):
            continue
        d = R.case(Cc, dg, Co, H, W, s, dl, mod)
        ref = R.evaluate(d, torch.float64)
        for dt in (torch.float64, torch.float32):
            bad = R.evaluate(d, dt, variant)
            e = R.rel_err(bad['y'], ref['y'])
            assert e > 100 * R.GATE_A, (variant, Cc, dg, H, W, s, dl, mod, e)
        n += 1
    assert n >= 16


def test_fp32_yardstick_is_within_gate_a_of_fp64():
    worst = {}
    for Cc, dg, Co, H, W, s, dl, mod in _gpu_cases():
        d = R.case(Cc, dg, Co, H, W, s, dl, mod)
        ref, f32 = R.evaluate(d, torch.float64), R.evaluate(d, torch.float32)
        for k in R.NAMES:
            if ref[k] is not None:
                worst[k] = max(worst.get(k, 0.0), R.rel_err(f32[k], ref[k]))
    print('fp32 yardstick against fp64, worst over the cases:', {k: '%.2e' % v for k, v in worst.items()})
    assert all(v <= R.GATE_A / 10 for v in worst.values())


def test_relabelling_changes_nothing_in_fp64_and_the_fp32_figure_is_never_zero():
    """evaluate(order=) is the same case: identical to 1e-13 in fp64.  And the figure gate B divides by
    (the largest fp32 error over the orders) is above a quarter of an ulp on every case and quantity"""
    low = {}
    for Cc, dg, Co, H, W, s, dl, mod in _gpu_cases():
        d = R.case(Cc, dg, Co, H, W, s, dl, mod)
        ref = R.evaluate(d, torch.float64)
        if (H, W, s) == (7, 9, 1):
            for o in (1, 2):
                again = R.evaluate(d, torch.float64, order=o)
                assert all(ref[k] is None or R.rel_err(again[k], ref[k]) <= 1e-13 for k in R.NAMES)
        for k, (hi, lo) in R.fp32_figure(d, ref).items():
            low[k] = min(low.get(k, 1.0), hi)
    print('smallest fp32 figure over the cases:', {k: '%.2e' % v for k, v in low.items()})
    assert all(v >= 2.0 ** -26 for v in low.values())


@pytest.mark.parametrize('orders,which', [(2000, 'flagged'), (60, 'all')])
def test_dx_gate_does_not_depend_on_the_order_of_the_atomics(orders, which):
    """dx on the GPU is a sum of fp32 atomics in no fixed order.  Here its fp32 terms (dcn_ref.dx_terms:
    dcol * mask * corner weight, formed as csrc/deform.hip forms them) are added on the CPU in random
    orders other than the ones the figure is taken over (a serial index_add_: the order of the index
    is the order of the adds): 2000 orders of the case on which one yardstick order alone put the GPU
    at 3.6 x, and 60 orders of every case.  Against gate B as tests/test_gpu_deform_conv.py applies
    it (4 x the largest fp32 error over dcn_ref.ORDERS orders) the worst order stays under 3/4 of the
    gate: the outcome of the GPU test does not depend on the order the atomics arrive in."""
    cases = [(8, 1, 5, 7, 9, 1, 1, True)] if which == 'flagged' else list(_gpu_cases())
    worst = 0.0
    for c in cases:
        d = R.case(*c)
        ref = R.evaluate(d, torch.float64)
        fig = R.fp32_figure(d, ref)['dx'][0]
        idx, val, n = R.dx_terms(d, torch.float32)
        exact = torch.zeros(n, dtype=torch.float64).index_add_(0, idx, val.double()).view_as(d['x'])
        assert R.rel_err(exact, ref['dx']) <= 1e-6                      # the terms are dx's terms
        g = torch.Generator().manual_seed(10 ** 6 + orders)            # not fp32_figure's seeds
        for _ in range(orders):
            p = torch.randperm(idx.numel(), generator=g)
            dx = torch.zeros(n).index_add_(0, idx[p], val[p]).view_as(d['x'])
            worst = max(worst, R.rel_err(dx, ref['dx']) / fig)
    print('dx over %d random orders of %d case(s): worst %.2f x the fp32 figure' % (orders, len(cases), worst))
    assert worst <= 0.75 * R.GATE_B


# ------------------------------------------------------------------ 2: entries
NEW = {'ia_deform_im2col3x3_bytes': 7, 'ia_deform_im2col3x3_nhwc': 16, 'ia_deform_col2im3x3_nhwc': 18}


def test_new_entries_are_declared_bound_and_exported():
    from iouaware import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = C.CDLL(_lib.SO_PATH)
    for name, n in NEW.items():
        assert name in _lib.SIGNATURES and hasattr(h, name) and len(_lib.SIGNATURES[name][1]) == n
        decl = re.search(r'\b%s\((.*?)\);' % name, txt, re.S).group(1)
        assert decl.count(',') + 1 == n
    src = open(os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd', 'csrc', 'build.py')).read()
    assert "'deform.hip'" in src


def test_entries_refuse_bad_arguments_without_a_device():
    """every call returns from the argument check: nothing is enqueued, no device is touched"""
    from iouaware import _lib
    lib = _lib.lib()
    buf = (C.c_char * 4096)()
    v = (C.addressof(buf) + 255) // 256 * 256

    def fwd(x=v, off=v, ops_=18, mask=None, mps=0, col=v, B=1, H=7, W=9, Cn=8, s=1, p=1, d=1, dg=1):
        return lib.ia_deform_im2col3x3_nhwc(x, off, ops_, mask, mps, 0, col, B, H, W, Cn, s, p, d, dg, None)

    def bwd(dcol=v, x=v, off=v, ops_=18, mask=None, mps=0, dx=v, do=v, dm=None, B=1, H=7, W=9, Cn=8, s=1, p=1,
            d=1, dg=1):
        return lib.ia_deform_col2im3x3_nhwc(dcol, x, off, ops_, mask, mps, dx, do, dm, B, H, W, Cn, s, p, d, dg, None)
    for f in (fwd, bwd):
        assert f(x=None) == IA_E_ARG and f(off=None) == IA_E_ARG
        assert f(Cn=6) == IA_E_ARG and f(Cn=8, dg=4) == IA_E_ARG and f(Cn=12, dg=2) == IA_E_ARG   # C % (4 dg)
        assert f(s=0) == IA_E_ARG and f(d=0) == IA_E_ARG and f(p=-1) == IA_E_ARG and f(dg=0) == IA_E_ARG
        assert f(B=0) == IA_E_ARG and f(H=0) == IA_E_ARG
        assert f(H=2, W=2, p=0) == IA_E_ARG and f(H=4, W=9, d=3) == IA_E_ARG    # smaller than the dilated kernel
        assert f(ops_=17) == IA_E_ARG and f(mask=v, mps=8) == IA_E_ARG          # rows narrower than dg * 18 / dg * 9
        assert f(x=v + 4) == IA_E_ARG                                           # x not 16-byte aligned
    assert fwd(col=None) == IA_E_ARG and fwd(col=v + 8) == IA_E_ARG
    assert bwd(dcol=None) == IA_E_ARG
    assert bwd(dm=v) == IA_E_ARG                                                # d_mask without a mask
    assert bwd(dx=None, do=None) == IA_E_ARG                                    # nothing asked for
    assert lib.ia_deform_im2col3x3_bytes(3, 7, 9, 8, 2, 1, 1) == 3 * 4 * 5 * 9 * 8 * 4
    assert lib.ia_deform_im2col3x3_bytes(3, 7, 9, 8, 2, 1, 2) == 3 * 3 * 4 * 9 * 8 * 4
    assert lib.ia_deform_im2col3x3_bytes(3, 2, 2, 8, 1, 0, 1) == 0


# ------------------------------------------------------------------ 3: modules
def test_module_parameter_names_shapes_and_initialisation():
    import iouaware
    from iouaware import DeformConv, DeformConvPack, ModulatedDeformConv, ModulatedDeformConvPack
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}     # noqa: E731
    assert shapes(DeformConv(8, 6, 3, padding=1)) == {'weight': (6, 8, 3, 3)}
    assert shapes(ModulatedDeformConv(8, 6, 3, padding=1)) == {'weight': (6, 8, 3, 3), 'bias': (6,)}
    assert shapes(ModulatedDeformConv(8, 6, 3, padding=1, bias=False)) == {'weight': (6, 8, 3, 3)}
    assert shapes(DeformConv(8, 6, 3, groups=2)) == {'weight': (6, 4, 3, 3)}
    assert shapes(DeformConvPack(8, 6, 3, padding=1, deformable_groups=2)) == {
        'weight': (6, 8, 3, 3), 'conv_offset.weight': (36, 8, 3, 3), 'conv_offset.bias': (36,)}
    assert shapes(ModulatedDeformConvPack(8, 6, 3, stride=2, padding=1, deformable_groups=2)) == {
        'weight': (6, 8, 3, 3), 'bias': (6,), 'conv_offset_mask.weight': (54, 8, 3, 3),
        'conv_offset_mask.bias': (54,)}
    with pytest.raises(AssertionError):
        DeformConv(8, 6, 3, bias=True)
    with pytest.raises(AssertionError):
        DeformConv(8, 6, 3, groups=3)
    m = ModulatedDeformConvPack(8, 6, 3, stride=2, padding=1)
    assert (m.stride, m.padding, m.dilation, m.with_bias) == (2, 1, 1, True)          # as given
    assert m.conv_offset_mask.stride == (2, 2) and m.conv_offset_mask.padding == (1, 1)
    assert float(m.conv_offset_mask.weight.detach().abs().sum()) == 0 and float(m.conv_offset_mask.bias.detach().abs().sum()) == 0
    assert float(m.bias.detach().abs().sum()) == 0
    bound = 1.0 / (8 * 9) ** 0.5
    assert 0.5 * bound < float(m.weight.detach().abs().max()) <= bound
    v1 = DeformConvPack(8, 6, 3, stride=2, padding=1, dilation=2)
    assert (v1.stride, v1.padding, v1.dilation) == ((2, 2), (1, 1), (2, 2))           # pairs
    assert float(v1.conv_offset.weight.detach().abs().sum()) == 0 and v1.kernel_size == (3, 3)
    for name in ('DeformConv', 'DeformConvPack', 'ModulatedDeformConv', 'ModulatedDeformConvPack',
                 'deform_conv', 'modulated_deform_conv'):
        assert hasattr(iouaware, name)


def test_compat_aliases():
    import iouaware
    from iouaware import compat
    import importlib
    dc = importlib.import_module('iouaware.deform_conv')
    compat.install()
    import mmdet.ops as mo
    import mmdet.ops.dcn as md
    for name in ('DeformConv', 'DeformConvPack', 'ModulatedDeformConv', 'ModulatedDeformConvPack',
                 'deform_conv', 'modulated_deform_conv'):
        assert getattr(mo, name) is getattr(dc, name) and getattr(md, name) is getattr(dc, name)
        assert getattr(iouaware, name) is getattr(dc, name)


# ------------------------------------------------------------------ 4: backbones
@pytest.mark.parametrize('modulated', [False, True])
def test_resnet50_dcn_state_dict_keys(modulated):
    from iouaware.backbones import ResNet
    from iouaware import DeformConv, ModulatedDeformConv
    plain = ResNet(50)
    net = ResNet(50, dcn=dict(DCN, modulated=modulated), stage_with_dcn=STAGES)
    sd, sp = net.state_dict(), plain.state_dict()
    width = 27 if modulated else 18
    extra = set(sd) - set(sp)
    want = set()
    for stage, blocks in zip((2, 3, 4), (4, 6, 3)):
        planes = 64 * 2 ** (stage - 1)
        for b in range(blocks):
            pre = 'layer%d.%d.' % (stage, b)
            want |= {pre + 'conv2_offset.weight', pre + 'conv2_offset.bias'}
            assert tuple(sd[pre + 'conv2_offset.weight'].shape) == (width, planes, 3, 3)
            assert tuple(sd[pre + 'conv2_offset.bias'].shape) == (width,)
            assert tuple(sd[pre + 'conv2.weight'].shape) == (planes, planes, 3, 3)
            assert pre + 'conv2.bias' not in sd
            blk = getattr(net, 'layer%d' % stage)[b]
            assert type(blk.conv2) is (ModulatedDeformConv if modulated else DeformConv)
            s2 = 2 if b == 0 else 1
            assert blk.conv2_offset.stride == (s2, s2) and blk.conv2_offset.padding == (1, 1)
    assert extra == want and set(sp) <= set(sd)                       # every other key as in the plain net
    assert not any('conv2_offset' in k for k in sd if k.startswith('layer1.'))
    # a reference-named state dict loads
    net.load_state_dict({k: v.clone() + 1 for k, v in sd.items()}, strict=True)
    assert float(net.layer2[0].conv2_offset.bias.detach().min()) > 0.5      # (the default init is small)
    # init_weights zeroes conv2_offset (kaiming would not)
    net.init_weights()
    for m in net.modules():
        if hasattr(m, 'conv2_offset'):
            assert float(m.conv2_offset.weight.detach().abs().sum()) == 0
            assert float(m.conv2_offset.bias.detach().abs().sum()) == 0
            assert float(m.conv2.weight.detach().abs().sum()) > 0


def test_deformable_groups_widths_and_fallback_on_stride():
    from iouaware.backbones import ResNet
    net = ResNet(50, dcn=dict(modulated=True, deformable_groups=4, fallback_on_stride=True), stage_with_dcn=STAGES)
    for stage in (2, 3, 4):
        layer = getattr(net, 'layer%d' % stage)
        assert type(layer[0].conv2) is torch.nn.Conv2d and not hasattr(layer[0], 'conv2_offset')   # the strided block
        assert not layer[0].with_dcn
        for blk in list(layer)[1:]:
            assert blk.with_dcn and blk.with_modulated_dcn and blk.conv2_offset.out_channels == 4 * 27
            assert blk.conv2.deformable_groups == 4
    # a stage whose stride is 1 has no strided block: every block deformable
    net = ResNet(50, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), dcn=dict(DCN, fallback_on_stride=True),
                 stage_with_dcn=STAGES)
    assert net.layer3[0].with_dcn and net.layer3[0].conv2.dilation == (2, 2) and net.layer3[0].conv2_offset.dilation == (2, 2)


def test_detectors_build_with_a_dcn_backbone():
    import json
    import iouaware
    from iouaware.config import ConfigDict
    gold = os.path.join(ROOT, 'tests', 'golden')
    for fixture, key in (('retina_plain_ref.json', None), ('fcos_plain_ref.json', None)):
        with open(os.path.join(gold, fixture)) as fh:
            recs = json.load(fh)
        rec = recs[sorted(recs)[0]]
        rec['model']['pretrained'] = None
        rec['model']['backbone'].update(dcn=dict(DCN), stage_with_dcn=STAGES)
        model = iouaware.build_detector(ConfigDict(rec['model']), train_cfg=ConfigDict(rec['train_cfg']),
                                        test_cfg=ConfigDict(rec['test_cfg']))
        assert model.backbone.layer2[0].with_dcn and not model.backbone.layer1[0].with_dcn


# ------------------------------------------------------------------ 5: refusals
def test_backbone_refusals():
    from iouaware.backbones import ResNet, ResNeXt, Bottleneck
    with pytest.raises(NotImplementedError):
        ResNet(18, dcn=dict(DCN), stage_with_dcn=STAGES)                         # BasicBlock, as in the reference
    with pytest.raises(NotImplementedError, match='groups'):
        ResNeXt(depth=50, groups=32, base_width=4, dcn=dict(DCN), stage_with_dcn=STAGES)
    with pytest.raises(AssertionError):
        ResNet(50, dcn=dict(DCN), stage_with_dcn=(False, True, True))
    with pytest.raises(AssertionError):
        ResNet(50, dcn='v2', stage_with_dcn=STAGES)
    with pytest.raises(AssertionError):
        Bottleneck(64, 16, dcn=dict(DCN), conv_cfg=dict(type='Conv'))
    for kw in (dict(gcb=dict(ratio=1. / 16)), dict(gen_attention=dict(spatial_range=-1))):
        with pytest.raises(NotImplementedError):                                 # exactly as before
            ResNet(50, **kw)
        with pytest.raises(NotImplementedError):
            ResNet(50, dcn=dict(DCN), stage_with_dcn=STAGES, **kw)
    # a bf16 network with DCN blocks is refused at the block, naming dcn
    blk = Bottleneck(64, 16, dcn=dict(DCN)).to(torch.bfloat16)
    with pytest.raises(TypeError, match='dcn'):
        blk(torch.zeros(1, 64, 8, 8, dtype=torch.bfloat16))


def test_op_refusals_by_their_named_errors():
    from iouaware import _lib, deform_conv, modulated_deform_conv, DeformConv, ops
    x, off, w = torch.zeros(1, 8, 7, 9), torch.zeros(1, 18, 7, 9), torch.zeros(5, 8, 3, 3)
    with pytest.raises(_lib.IouAwareLibraryError):                               # CPU tensors: no fallback
        deform_conv(x, off, w, 1, 1)
    with pytest.raises(_lib.IouAwareLibraryError):
        modulated_deform_conv(x, off, torch.zeros(1, 9, 7, 9), w, None, 1, 1)
    with pytest.raises(_lib.IouAwareLibraryError):
        DeformConv(8, 5, 3, padding=1)(x, off)
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.deform_im2col3x3(x.contiguous(memory_format=torch.channels_last), off)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match=str(dt).replace('torch.', '')):
            deform_conv(x.to(dt), off.to(dt), w.to(dt), 1, 1)
    with pytest.raises(NotImplementedError, match='groups'):
        deform_conv(x, off, torch.zeros(6, 4, 3, 3), 1, 1, 1, 2)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        deform_conv(x, torch.zeros(1, 50, 5, 7), torch.zeros(5, 8, 5, 5), 1, 1)
    with pytest.raises(NotImplementedError, match='deformable_groups'):
        deform_conv(x, torch.zeros(1, 72, 7, 9), w, 1, 1, 1, 1, 4)               # 8 % (4 * 4)
    with pytest.raises(NotImplementedError, match='stride'):
        deform_conv(x, off, w, (1, 2), 1)
    with pytest.raises(ValueError, match='offset'):
        deform_conv(x, torch.zeros(1, 18, 7, 8), w, 1, 1)
    with pytest.raises(ValueError, match='mask'):
        modulated_deform_conv(x, off, torch.zeros(1, 18, 7, 9), w, None, 1, 1)

"""GPU: `dcn=` backbones (iouaware/backbones.py) on the deformable convolution kernels -- the module
route, the fused inference route (fuse._dcn_conv2) and training.

R-50, stage_with_dcn = (False, True, True, True), DCN v1 and modulated, batch 2 at 64 x 96.  The
conv2_offset weights are drawn from normal(0, 0.05) and their biases from uniform(-1, 1) first (at
init_weights they are zero and the network would be an ordinary ResNet), BatchNorm runs in eval mode
on non-trivial running statistics and affine parameters (norm3's weight too, which
zero_init_residual would zero).

The fp64 partner is a copy of the module on the CPU in float64 whose deformable conv2 is the
yardstick op (tests/dcn_ref.py).  The training check feeds that copy the upstream gradients the GPU
step delivered at the backbone's outputs (the detector's losses are HIP kernels without a CPU or
fp64 form), so the comparison covers the backbone: everything DCN touches.

Contract: the fp32 one of the project, 1e-4 of the tensor's maximum (dcn_ref.GATE_A)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import dcn_ref as R
import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STAGES = (False, True, True, True)
B, PH, PW = 2, 64, 96


def _randomise(backbone, seed):
    from torch.nn.modules.batchnorm import _BatchNorm
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in backbone.modules():
            if isinstance(m, _BatchNorm):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.weight.copy_(torch.rand(n, generator=g) * 0.5 + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.1)
            if hasattr(m, 'conv2_offset'):
                co = m.conv2_offset
                co.weight.copy_(torch.randn(co.weight.shape, generator=g) * 0.05)
                co.bias.copy_(torch.rand(co.bias.shape, generator=g) * 2 - 1)


def _detector(modulated, train, dg=1):
    import iouaware
    from iouaware.config import ConfigDict
    with open(os.path.join(GOLD, 'retina_plain_ref.json')) as fh:
        rec = json.load(fh)['retinanet_r50_fpn_1x']
    rec['model']['pretrained'] = None
    rec['model']['backbone'].update(dcn=dict(modulated=modulated, deformable_groups=dg, fallback_on_stride=False),
                                    stage_with_dcn=STAGES)
    torch.manual_seed(0)
    model = iouaware.build_detector(ConfigDict(rec['model']), train_cfg=ConfigDict(rec['train_cfg']),
                                    test_cfg=ConfigDict(rec['test_cfg']))
    _randomise(model.backbone, 5 + int(modulated))
    model = model.cuda()
    return model.train() if train else model.eval()


def _fp64_copy(backbone):
    """the module on the CPU in float64, the deformable conv2 of every DCN block -> the yardstick op"""
    ref = copy.deepcopy(backbone).cpu().double()
    n = 0
    for blk in ref.modules():
        if getattr(blk, 'with_dcn', False):
            c2 = blk.conv2
            s, p, d = (v[0] if isinstance(v, tuple) else v for v in (c2.stride, c2.padding, c2.dilation))

            def fwd(x, offset, mask=None, c2=c2, s=s, p=p, d=d):
                return R.modulated_deform_conv(x, offset, mask, c2.weight, None, s, p, d, c2.deformable_groups)
            c2.forward = fwd
            n += 1
    assert n == 13
    return ref


def _img(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, PH, PW, generator=g)


def _share(got, ref):
    return R.rel_err(got, ref)


@pytest.mark.parametrize('modulated,dg', [(False, 1), (True, 1), (True, 4)], ids=['v1', 'v2', 'v2-dg4'])
def test_fused_stages_match_the_module_and_fp64(modulated, dg):
    """dg = 4, modulated: conv2_offset has 108 output channels, a multiple of 4, so at stride 1 it takes
    the Winograd route (`off_wino`); the offsets / mask logits are the first 72 / last 36 channels"""
    from iouaware.fuse import fuse_inference, unfuse_inference
    model = _detector(modulated, train=False, dg=dg)
    bb = model.backbone
    ref64 = _fp64_copy(bb).eval()
    img = _img()
    x = img.cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        plain = bb(x)                                               # module forward, conv2 on the autograd op
        want = ref64(img.double())
        assert fuse_inference(model, winograd=True) > 0
        model = model.to(memory_format=torch.channels_last)
        blk = bb.layer2[1]
        assert 'dcn2' in blk._ia_fused and 'wino2' not in blk._ia_fused and 'im2col2' not in bb.layer2[0]._ia_fused
        assert 'off_im2col' in bb.layer2[0]._ia_fused and 'off_im2col' not in blk._ia_fused
        assert ('off_wino' in blk._ia_fused) == (dg == 4) and 'off_wino' not in bb.layer2[0]._ia_fused
        assert blk.conv2_offset.out_channels == dg * (27 if modulated else 18)
        if dg == 4:
            assert blk._ia_fused['off_wino'].usable(torch.empty(2, 128, 8, 12, device='cuda').contiguous(
                memory_format=torch.channels_last))
        fused = bb(x)
        torch.cuda.synchronize()
        for i in range(4):
            assert fused[i].shape == want[i].shape == plain[i].shape
            e_m, e_r, e_p = _share(fused[i], plain[i]), _share(fused[i], want[i]), _share(plain[i], want[i])
            print('  stage %d  fused vs module %.2e  fused vs fp64 %.2e  module vs fp64 %.2e' % (i + 1, e_m, e_r, e_p))
            assert e_m <= R.GATE_A and e_r <= R.GATE_A and e_p <= R.GATE_A
        # the offsets do something: the same network with conv2_offset zeroed is another function
        unfuse_inference(model)
        assert 'forward' not in bb.layer2[1].__dict__ and not hasattr(bb.layer2[1], '_ia_fused')
        again = bb(x)
        for i in range(4):
            assert _share(again[i], plain[i]) <= 1e-5                # the module forward is back
        for m in bb.modules():
            if hasattr(m, 'conv2_offset'):
                m.conv2_offset.weight.zero_()
                m.conv2_offset.bias.zero_()
        assert _share(bb(x)[3], plain[3]) > 1e-2


def test_retinanet_simple_test_end_to_end():
    from iouaware.fuse import fuse_inference
    model = _detector(True, train=False)
    fuse_inference(model, winograd=True)
    model = model.to(memory_format=torch.channels_last)
    x = _img(4).cuda().contiguous(memory_format=torch.channels_last)
    metas = [synth.img_meta(PH, PW, PH, PW) for _ in range(B)]
    with torch.no_grad():
        results = model.simple_test(x, metas)
    assert len(results) == B
    for per_class in results:
        assert len(per_class) == model.bbox_head.num_classes - 1
        for a in per_class:
            assert isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[1] == 5 and a.dtype == np.float32
            assert np.isfinite(a).all()


@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_train_step_gradients_match_fp64(modulated):
    from iouaware.fuse import fuse_inference
    from iouaware.train import build_optimizer, train_step
    model = _detector(modulated, train=True)
    bb = model.backbone
    ref64 = _fp64_copy(bb).train()                                   # norm_eval: BatchNorm stays in eval mode
    fuse_inference(model, winograd=True, train=True)
    model = model.to(memory_format=torch.channels_last)
    opt = build_optimizer(model, dict(type='SGD', lr=0.0, momentum=0.0, weight_decay=0.0))
    img = _img(6)
    x = img.cuda().contiguous(memory_format=torch.channels_last)
    gts, gls = synth.train_targets(11, B, PH, PW, max_gt=5)
    gtb = [torch.from_numpy(v).cuda() for v in gts]
    gtl = [torch.from_numpy(v).cuda() for v in gls]
    metas = [synth.img_meta(PH, PW, PH, PW) for _ in range(B)]
    outs = []

    def keep(mod, inp, out):
        # hand the neck aliases of the stage outputs: an alias collects what arrives from the neck alone
        # (the stage output itself also receives the next stage's share, which the fp64 run produces itself)
        alias = tuple(t.view_as(t) for t in out)
        for t in alias:
            if t.requires_grad:
                t.retain_grad()
        outs.extend(alias)
        return alias
    h = bb.register_forward_hook(keep)
    masks, hooks = _record_relu_masks(bb)
    log = train_step(model, opt, x, metas, gtb, gtl)
    h.remove()
    for hk in hooks:
        hk.remove()
    torch.cuda.synchronize()
    assert log is not None and np.isfinite(log['loss']), log
    assert any('DeformConv3x3' in type(fn).__name__ for fn in _walk(outs[3].grad_fn))     # the new op ran
    # the fp64 backbone under the same upstream gradients
    flips = _replay_relu_masks(ref64, masks)
    want = ref64(img.double())
    print('  ReLU elements on the other side of zero in fp64: %d of %d' % (flips[0], flips[1]))
    assert flips[0] <= 1e-5 * flips[1]
    pairs = [(w, o.grad.double().cpu()) for w, o in zip(want, outs) if o.grad is not None]
    assert len(pairs) == 3                                           # the neck starts at stage 2
    torch.autograd.backward([w for w, _ in pairs], [g for _, g in pairs])
    got, ref = dict(bb.named_parameters()), dict(ref64.named_parameters())
    errs = {}
    for name in sorted(ref):
        if 'conv2_offset' in name or (name.endswith('conv2.weight') and not name.startswith('layer1.')):
            g = got[name].grad
            assert g is not None and float(g.abs().max()) > 0, name
            errs[name] = R.rel_err(g, ref[name].grad)
            print('  %-32s %.2e' % (name, errs[name]))
    assert len(errs) == 13 * 3
    assert max(errs.values()) <= R.GATE_A, max(errs.items(), key=lambda kv: kv[1])


class _ReplayReLU(torch.autograd.Function):
    """relu(x) whose derivative is the recorded mask"""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return x.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def _record_relu_masks(backbone):
    """the ReLU masks (output > 0) of every trainable bottleneck of the GPU step, per block in call order"""
    masks, hooks = {}, []
    for name, blk in backbone.named_modules():
        if hasattr(blk, 'conv3') and any(p.requires_grad for p in blk.parameters()):
            def rec(mod, inp, out, key=name):
                masks.setdefault(key, []).append((out.detach() > 0).cpu())
            hooks.append(blk.relu.register_forward_hook(rec))
    return masks, hooks


def _replay_relu_masks(ref64, masks):
    """The fp64 run differentiates its ReLUs with the GPU step's masks.  An activation within fp32
    rounding of zero lies on one side in fp32 and possibly on the other in fp64 (and, the framework's
    convolutions adding in another order in every run, not on the same side in two fp32 runs); its
    value is nothing, but its mask switches a whole gradient path on or off -- a tie of the kind the
    operator test keeps out of its data (and tests/test_gpu_wino_fp64.py masks out of its upstream
    gradient).  With the masks replayed no derivative depends on such a tie; the forward values are
    the fp64 run's own.  -> [elements whose fp64 sign differs from the mask, elements]"""
    count = [0, 0]
    blocks = dict(ref64.named_modules())
    for name, ms in masks.items():
        todo = list(ms)

        class Replay(torch.nn.Module):
            def forward(self, x, todo=todo):
                m = todo.pop(0)
                count[0] += int(((x.detach() > 0) != m).sum())
                count[1] += m.numel()
                return _ReplayReLU.apply(x, m.to(x.dtype))
        blocks[name].relu = Replay()
    return count


def _walk(fn, limit=20000):
    seen, stack = set(), [fn]
    while stack and len(seen) < limit:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        yield f
        stack.extend(g for g, _ in f.next_functions)

"""GPU: the bf16 grouped 3x3 convolution of the ResNeXt bottlenecks (csrc/gconv_bf16.hip).

Yardstick: an fp64 F.conv2d of the bf16-rounded input and the bf16-rounded folded weight
(bf16(scale * W), the product in fp32), plus the fp32 bias, ReLU applied.  The kernel accumulates in
fp32 and rounds to bf16 once, so the gate is the one of the project's other bf16 convolutions
(test_gpu_conv3x3_bf16.py, the bf16 stem): element-wise |got - want| <= 2^-8 |want| + 1e-5 max|want|,
on every element of every case.

Shapes are the smallest at which the kernel can go wrong: a wavefront owns 32 channels and walks
a row in tiles of 16 pixels whose neighbours come from DPP shifts and from the tiles left / right."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, groups): Cg = 4 / 8 / 16 / 32 in one supergroup; two supergroups; five (the second workgroup has
# three idle wavefronts)
WIDTHS = [(32, 8), (32, 4), (32, 2), (32, 1), (64, 2), (160, 5)]
# single pixel | the tile edges of the neighbour exchange and a last partial tile | stride 2 with odd
# and even extents
SIZES = [(1, 1), (2, 15), (3, 16), (3, 17), (5, 33), (7, 11), (8, 16)]
B = 2       # the last row of image 0 lies next to the first row of image 1


def _gate(got, want):
    err = (got.double() - want).abs()
    tol = 2.0 ** -8 * want.abs() + 1e-5 * float(want.abs().max())
    return bool((err <= tol).all()), float((err - tol).max())


@functools.lru_cache(maxsize=None)
def _case(C, groups, stride, H, W):
    """inputs, packed weights and the fp64 result WITHOUT bias / ReLU (shared, never written to)"""
    from iouaware import ops
    cg = C // groups
    g = torch.Generator(device='cuda').manual_seed(1000 * C + 100 * groups + 10 * H + W + stride)
    x = torch.randn(B, C, H, W, device='cuda', generator=g).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w = torch.randn(C, cg, 3, 3, device='cuda', generator=g) * (2.0 / (9 * cg)) ** 0.5
    scale = torch.rand(C, device='cuda', generator=g) + 0.5
    bias = torch.randn(C, device='cuda', generator=g)
    folded = (w * scale.view(-1, 1, 1, 1)).to(torch.bfloat16)           # fp32 product, one rounding
    wp = ops.pack_grouped_weight_bf16(w, scale)
    want = F.conv2d(x.double(), folded.double(), None, stride, 1, 1, groups)
    return x, folded, bias, wp, want


@pytest.mark.parametrize('hw', SIZES)
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C,groups', WIDTHS)
def test_grouped_conv3x3_bf16_matches_fp64_convolution(C, groups, stride, hw):
    from iouaware import ops
    H, W = hw
    x, _, bias, wp, conv = _case(C, groups, stride, H, W)
    for relu in (False, True):
        for b in (None, bias):
            got = ops.grouped_conv3x3_bf16(x, wp, b, groups, stride, relu=relu)
            assert got.dtype == torch.bfloat16 and got.shape == conv.shape
            assert got.is_contiguous(memory_format=torch.channels_last)
            want = conv if b is None else conv + b.double().view(1, -1, 1, 1)
            if relu:
                want = want.clamp(min=0)
            ok, over = _gate(got, want)
            print('C %d groups %d stride %d %dx%d relu %d bias %d: worst error - tolerance %.3e'
                  % (C, groups, stride, H, W, relu, b is not None, over))
            assert ok, (relu, b is not None, over)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C,groups', WIDTHS)
def test_no_leakage_between_groups(C, groups, stride):
    """input non-zero in the channels of ONE group, no bias, no ReLU: every output channel outside
    that group is exactly 0.0 (the zero blocks of the dense 32 x 32 matrices are zeros, and the
    wavefronts of the other supergroups see zeros only)"""
    from iouaware import ops
    cg = C // groups
    H, W = 3, 17
    x0, _, _, wp, _ = _case(C, groups, stride, H, W)
    _, folded, _, _, _ = _case(C, groups, stride, H, W)
    for gi in sorted({0, groups // 2, groups - 1}):
        x = torch.zeros_like(x0)
        x[:, gi * cg:(gi + 1) * cg] = x0[:, gi * cg:(gi + 1) * cg]
        got = ops.grouped_conv3x3_bf16(x, wp, None, groups, stride)
        outside = torch.ones(C, dtype=torch.bool, device='cuda')
        outside[gi * cg:(gi + 1) * cg] = False
        assert bool((got[:, outside] == 0.0).all()), (gi, float(got[:, outside].abs().max()))
        # and the group itself carries its result (the test is not about an all-zero output)
        want = F.conv2d(x.double(), folded.double(), None, stride, 1, 1, groups)
        assert float(want[:, ~outside].abs().max()) > 0.1
        ok, over = _gate(got, want)
        assert ok, (gi, over)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C,groups', WIDTHS)
def test_single_tap_weights_match_the_shifted_input(C, groups, stride):
    """the weights of ONE tap only (no scale, bias, ReLU) against that tap written out in fp64: the
    zero-padded input shifted by (ky, kx), subsampled, times the tap's per-group matrix.  A swapped
    tap moves the image, a swapped channel mixes it: both miss this."""
    from iouaware import ops
    cg = C // groups
    H, W = 5, 33
    x, folded, _, _, _ = _case(C, groups, stride, H, W)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xpad = F.pad(x.double(), (1, 1, 1, 1))
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(C, cg, 3, 3, device='cuda')
            w[:, :, ky, kx] = folded[:, :, ky, kx].float()              # bf16 values: packing is exact
            got = ops.grouped_conv3x3_bf16(x, ops.pack_grouped_weight_bf16(w), None, groups, stride)
            xs = xpad[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            want = torch.einsum('bgihw,goi->bgohw', xs.reshape(B, groups, cg, Ho, Wo),
                                w[:, :, ky, kx].double().view(groups, cg, cg)).reshape(B, C, Ho, Wo)
            ok, over = _gate(got, want)
            assert ok, (ky, kx, over)


@pytest.mark.parametrize('stride', [1, 2])
def test_second_launch_gives_the_same_bits(stride):
    from iouaware import ops
    x, _, bias, wp, _ = _case(160, 5, stride, 5, 33)
    first = ops.grouped_conv3x3_bf16(x, wp, bias, 5, stride, relu=True)
    again = ops.grouped_conv3x3_bf16(x, wp, bias, 5, stride, relu=True)
    assert torch.equal(first.view(torch.int16), again.view(torch.int16))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C,groups', WIDTHS)
def test_not_worse_than_the_library(C, groups, stride):
    """RMS error against the fp64 yardstick <= 1.2 x that of torch's own bf16 grouped F.conv2d + 1e-6
    (the factor of test_gpu_conv3x3_bf16.py).  On the 5 x 33 map: 2 x 165 x C >= 10 560 outputs, so
    that an RMS of rounding errors (relative spread ~ 1 / sqrt(2 n)) is known to about a percent."""
    from iouaware import ops
    x, folded, bias, wp, conv = _case(C, groups, stride, 5, 33)
    wcl = folded.contiguous(memory_format=torch.channels_last)
    for b in (None, bias):
        got = ops.grouped_conv3x3_bf16(x, wp, b, groups, stride, relu=True)
        eager = F.conv2d(x, wcl, None if b is None else b.to(torch.bfloat16), stride, 1, 1, groups).clamp(min=0)
        want = (conv if b is None else conv + b.double().view(1, -1, 1, 1)).clamp(min=0)
        e_mine = float((got.double() - want).pow(2).mean().sqrt())
        e_eager = float((eager.double() - want).pow(2).mean().sqrt())
        print('C %d groups %d stride %d bias %d: rms error %.3e, library %.3e'
              % (C, groups, stride, b is not None, e_mine, e_eager))
        assert e_mine <= 1.2 * e_eager + 1e-6, (e_mine, e_eager)


def test_ops_reject_what_the_kernel_does_not_cover():
    from iouaware import ops, _lib
    cl = torch.channels_last
    wp = ops.pack_grouped_weight_bf16(torch.zeros(64, 8, 3, 3, device='cuda'))
    assert wp.is_cuda and wp.dtype == torch.bfloat16
    x = torch.zeros(1, 64, 4, 4, device='cuda', dtype=torch.bfloat16).contiguous(memory_format=cl)
    with pytest.raises(ValueError):
        ops.grouped_conv3x3_bf16(x.float(), wp, None, 8)
    with pytest.raises(ValueError):
        ops.grouped_conv3x3_bf16(x.contiguous(), wp, None, 8)
    with pytest.raises(ValueError):
        ops.grouped_conv3x3_bf16(x, wp, None, 32)                     # 2 channels per group
    with pytest.raises(ValueError):
        ops.grouped_conv3x3_bf16(x, wp[:-8], None, 8)                 # not the packed size of 64 channels
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.grouped_conv3x3_bf16(x, wp, None, 8, stride=3)


# ------------------------------------------------------------------ the route in a whole network
def _stage_outputs(m, x):
    feats = m.backbone(x)
    pyr = m.neck(feats)
    head = m.bbox_head(pyr)
    return ([('C%d' % (i + 2), t) for i, t in enumerate(feats)] +
            [('P%d' % (i + 3), t) for i, t in enumerate(pyr)] +
            [('%s%d' % (n, i + 3), t) for n, ts in zip(('cls', 'reg', 'iou'), head)
             for i, t in enumerate(ts)])


def test_resnext50_bf16_network_takes_the_route(monkeypatch):
    """ResNeXt-50 32x4d IoU-aware RetinaNet, trained-like weights rounded to bf16, fused
    (winograd=True), channels-last bf16.  Every stage output (C2-C5, P3-P7, the 15 head outputs)
    under the contract of the config-3 test: RMS-relative error against the fp32 modules on the
    same rounded weights <= 1.5 x torch's own bf16 modules + 1e-3.  And the grouped convolution of
    each of the 16 bottlenecks ran on ops.grouped_conv3x3_bf16, once."""
    import copy
    import bench
    import iouaware
    import synth
    from iouaware import ops
    from iouaware.config import ConfigDict
    from iouaware.fuse import fuse_inference
    cfg = ConfigDict(bench.MODEL)
    cfg.backbone.update(dict(type='ResNeXt', depth=50, groups=32, base_width=4))
    torch.manual_seed(0)
    m = iouaware.build_detector(cfg, train_cfg=None, test_cfg=ConfigDict(bench.TEST_CFG)).eval()
    with torch.no_grad():
        synth.e2e_fill_state(m.state_dict(), 11)
        m = m.cuda()
        for p_ in m.parameters():
            p_.copy_(p_.to(torch.bfloat16).float())
        for b_ in m.buffers():
            if b_.dtype == torch.float32:
                b_.copy_(b_.to(torch.bfloat16).float())
    x = torch.from_numpy(synth.e2e_image(9, 2, 128, 160, 128, 160)).cuda().to(torch.bfloat16).float()
    calls = []
    real = ops.grouped_conv3x3_bf16

    def counted(xx, *a, **k):
        calls.append(tuple(xx.shape))
        return real(xx, *a, **k)
    monkeypatch.setattr(ops, 'grouped_conv3x3_bf16', counted)
    with torch.no_grad():
        ref = _stage_outputs(m, x)
        eager = copy.deepcopy(m).to(torch.bfloat16)
        eag = _stage_outputs(eager, x.to(torch.bfloat16))
        del eager
        assert not calls                                      # the plain modules do not come here
        fuse_inference(m, winograd=True)
        mb = m.to(memory_format=torch.channels_last).to(torch.bfloat16)
        out = _stage_outputs(mb, x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
    assert len(calls) == 16, calls
    assert sorted({c[1] for c in calls}) == [128, 256, 512, 1024]

    def rms_rel(a, r):
        return float((a.float() - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp(min=1e-12))
    assert len(ref) == len(eag) == len(out) == 4 + 5 + 15
    for (name, r), (_, e), (_, o) in zip(ref, eag, out):
        assert o.dtype == torch.bfloat16
        e_eager, e_fused = rms_rel(e, r), rms_rel(o, r)
        line = '%-5s fused %.2e  torch-bf16 %.2e' % (name, e_fused, e_eager)
        print(line)
        assert e_fused <= 1.5 * e_eager + 1e-3, line

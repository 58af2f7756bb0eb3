"""CPU: the opt-in grouped 3x3 training route (iouaware/train_fuse.py: grouped_conv3x3_train on
csrc/gconv.hip / csrc/gconv_bwd.hip) -- off by default, its C entry points declared, bound and
exported, every unsupported argument refused before a device is touched, and the test yardstick
(tests/gconv_ref.py) consistent with itself: the grouped evaluation equals the per-group one, the
gather restatement of the input gradient equals autograd, and its nearest wrong variants miss
gate A by a wide margin on the inputs the GPU tests use."""
import ctypes

import pytest
import torch

import gconv_ref as G
import wino_ref as R
from test_capi_symbols import declared_functions

ENTRIES = ('ia_grouped_conv3x3_pack_dev', 'ia_grouped_conv3x3_bwd_data_nhwc',
           'ia_grouped_conv3x3_bwd_weight_workspace_bytes', 'ia_grouped_conv3x3_bwd_weight_nhwc')
IA_E_ARG = -1


def test_entries_are_declared_bound_and_exported():
    from iouaware import _lib
    names = declared_functions()
    _lib.lib()                                     # builds the library when it is missing
    h = ctypes.CDLL(_lib.SO_PATH)
    for e in ENTRIES:
        assert e in names and e in _lib.SIGNATURES and hasattr(h, e), e


def test_switch_exists_and_is_off_by_default():
    from iouaware.backbones import ResNet, ResNeXt, Bottleneck
    from iouaware.fuse import fuse_inference, unfuse_inference
    assert ResNet.train_gconv is False and ResNeXt.train_gconv is False
    net = ResNeXt(depth=50, groups=32, base_width=4)
    assert net.train_gconv is False
    for on in (False, True):
        net.train_gconv = on
        fuse_inference(net, winograd=True, train=True)
        blocks = [m for m in net.modules() if isinstance(m, Bottleneck)]
        assert blocks and all(b._ia_train_gconv is on for b in blocks)
        unfuse_inference(net)
        assert not any(hasattr(b, '_ia_train_gconv') for b in blocks)
    assert ResNet.train_gconv is False


def _buffers():
    """host memory standing in for device pointers: an argument error is found before any of it
    is looked at.  16-byte aligned base addresses."""
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 15) & ~15
    return raw, [ctypes.c_void_p(base + 1024 * k) for k in range(4)]


def test_bad_arguments_are_refused_without_a_device():
    from iouaware import _lib
    L = _lib.lib()
    raw, (p0, p1, p2, p3) = _buffers()
    null = ctypes.c_void_p(0)
    off = ctypes.c_void_p(p0.value + 4)            # 4-byte, not 16-byte aligned
    B, H, W = 1, 4, 4
    # 12 channels per group (C = 48, 4 groups); stride 3; NULL; misaligned
    assert L.ia_grouped_conv3x3_pack_dev(p0, null, 48, 4, 0, p1, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_pack_dev(null, null, 32, 4, 0, p1, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_pack_dev(p0, null, 32, 4, 0, null, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_pack_dev(p0, null, 32, 4, 3, p1, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_pack_dev(p0, null, 32, 4, -1, p1, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_pack_dev(p0, null, 24, 3, 0, p1, null) == IA_E_ARG     # C % 16
    for stride in (1, 2):
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(p0, p1, p2, B, H, W, 48, 4, stride, null) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(null, p1, p2, B, H, W, 32, 4, stride, null) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(p0, null, p2, B, H, W, 32, 4, stride, null) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(p0, p1, null, B, H, W, 32, 4, stride, null) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(off, p1, p2, B, H, W, 32, 4, stride, null) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(p0, p1, off, B, H, W, 32, 4, stride, null) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_data_nhwc(p0, p1, p2, 0, H, W, 32, 4, stride, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_bwd_data_nhwc(p0, p1, p2, B, H, W, 32, 4, 3, null) == IA_E_ARG
    for stride in (1, 2):
        need = L.ia_grouped_conv3x3_bwd_weight_workspace_bytes(B, H, W, 32, 4, stride)
        assert need > 0 and need % (32 * 16 * 9 * 4) == 0
        args = (B, H, W, 32, 4, stride, null)
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, p1, p2, p3, need - 1, *args) == IA_E_ARG   # one byte short
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(null, p1, p2, p3, need, *args) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, null, p2, p3, need, *args) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, p1, null, p3, need, *args) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, p1, p2, null, need, *args) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(off, p1, p2, p3, need, *args) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, off, p2, p3, need, *args) == IA_E_ARG
        assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, p1, p2, p3, need, B, H, W, 48, 4, stride, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_bwd_weight_nhwc(p0, p1, p2, p3, 1 << 20, B, H, W, 32, 4, 3, null) == IA_E_ARG
    assert L.ia_grouped_conv3x3_bwd_weight_workspace_bytes(B, H, W, 48, 4, 1) == 0
    assert L.ia_grouped_conv3x3_bwd_weight_workspace_bytes(B, H, W, 32, 4, 3) == 0
    assert bytes(raw) == bytes(4096)               # nothing written


def test_front_end_refuses_cpu_tensors_and_wrong_shapes():
    from iouaware import ops, _lib
    cl = torch.channels_last
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.pack_grouped_weight_dev(torch.zeros(32, 8, 3, 3))
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.grouped_conv3x3_bwd_data(torch.zeros(1, 32, 4, 4).contiguous(memory_format=cl), torch.zeros(1), 4, 1, (4, 4))
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.grouped_conv3x3_bwd_weight(torch.zeros(1, 32, 4, 4).contiguous(memory_format=cl),
                                       torch.zeros(1, 32, 4, 4).contiguous(memory_format=cl), 4, 1)


def test_module_side_conditions():
    import torch.nn as nn
    from iouaware.train_fuse import grouped_conv_ok as ok
    assert ok(nn.Conv2d(128, 128, 3, padding=1, groups=32, bias=False)) is True
    assert ok(nn.Conv2d(128, 128, 3, stride=2, padding=1, groups=32, bias=False)) is True
    assert ok(nn.Conv2d(96, 96, 3, padding=1, groups=3, bias=False)) is True              # 32 per group
    assert ok(nn.Conv2d(128, 128, 3, padding=1, groups=1, bias=False)) is False
    assert ok(nn.Conv2d(96, 96, 3, padding=1, groups=8, bias=False)) is False             # 12 per group
    assert ok(nn.Conv2d(128, 128, 3, stride=3, padding=1, groups=32, bias=False)) is False
    assert ok(nn.Conv2d(128, 128, 3, padding=1, groups=32, bias=True)) is False
    assert ok(nn.Conv2d(128, 256, 3, padding=1, groups=32, bias=False)) is False
    assert ok(nn.Conv2d(128, 128, 3, padding=2, dilation=2, groups=32, bias=False)) is False
    assert ok(nn.Conv2d(160, 160, 3, padding=1, groups=5, bias=False)) is True
    assert ok(nn.Conv2d(32, 32, 3, padding=1, groups=1, bias=False)) is False


# ------------------------------------------------------------------ the yardstick
CASES = [(s, cg, H, W) for s in (1, 2) for cg in (4, 16) for (H, W) in ((7, 11), (6, 32), (1, 1))]


def _data(stride, cg, H, W, groups=2, B=2):
    g = torch.Generator().manual_seed(1000 * stride + 100 * cg + 10 * H + W)
    C = cg * groups
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(C, cg, 3, 3, generator=g, dtype=torch.float64) * (1.0 / (9 * cg)) ** 0.5
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    dy = torch.randn(B, C, G.out_size(H, stride), G.out_size(W, stride), generator=g, dtype=torch.float64)
    return x, w, b, dy, groups


@pytest.mark.parametrize('stride,cg,H,W', CASES)
def test_grouped_evaluation_equals_the_per_group_one(stride, cg, H, W):
    x, w, b, dy, groups = _data(stride, cg, H, W)
    a, c = G.conv(x, w, b, stride, groups), G.conv_per_group(x, w, b, stride, groups)
    assert float((a - c).abs().max()) <= 1e-12 * max(float(c.abs().max()), 1.0)


@pytest.mark.parametrize('stride,cg,H,W', CASES)
def test_gather_restatement_and_adjoint_weight_equal_autograd(stride, cg, H, W):
    x, w, b, dy, groups = _data(stride, cg, H, W)
    ref = G.conv_train(x, w, b, dy, stride, groups, False)
    dx = G.input_grad(dy, w, stride, groups, H, W)
    assert float((dx - ref['dx']).abs().max()) <= 1e-12 * max(float(ref['dx'].abs().max()), 1.0)
    if stride == 1:      # the forward convolution on the flipped and transposed weight
        dx2 = G.conv(dy, G.adjoint_weight(w, groups), None, 1, groups)
        assert float((dx2 - ref['dx']).abs().max()) <= 1e-12 * float(ref['dx'].abs().max())
    assert torch.equal(G.adjoint_weight(G.adjoint_weight(w, groups), groups), w)


def test_the_mask_comes_from_the_given_output():
    x, w, b, dy, groups = _data(1, 4, 7, 11)
    own = G.conv_train(x, w, b, dy, 1, groups, True)
    same = G.conv_train(x, w, b, dy, 1, groups, True, mask=own['y'] > 0)
    assert all(torch.equal(own[k], same[k]) for k in own)
    none = G.conv_train(x, w, b, dy, 1, groups, True, mask=torch.zeros_like(own['y'], dtype=torch.bool))
    assert float(none['dx'].abs().max()) == 0.0 and float(none['dW'].abs().max()) == 0.0


@pytest.mark.parametrize('stride,cg,H,W', [c for c in CASES if c[2:] != (1, 1)])
def test_wrong_variants_miss_gate_a_by_a_wide_margin(stride, cg, H, W):
    """taps not flipped, group block not transposed, and (stride 2, an even edge) terms clamped
    instead of masked: each at least 100 x gate A away from the input gradient on these inputs"""
    x, w, b, dy, groups = _data(stride, cg, H, W)
    ref = G.conv_train(x, w, b, dy, stride, groups, False)['dx']
    wrong = dict(flip=G.input_grad(dy, w, stride, groups, H, W, flip=False),
                 transpose=G.input_grad(dy, w, stride, groups, H, W, transpose=False))
    if stride == 2 and (H % 2 == 0 or W % 2 == 0):
        wrong['clamp'] = G.input_grad(dy, w, stride, groups, H, W, clamp=True)
    assert stride == 1 or (H, W) != (6, 32) or 'clamp' in wrong
    for name, t in wrong.items():
        e = R.rel_err(t, ref)
        assert e >= 100 * R.GATE_A, (name, e)

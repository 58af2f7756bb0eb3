"""CPU: the opt-in strided 3x3 training route (iouaware/train_fuse.py: conv3x3_strided on
csrc/im2col.hip's k_im2col3x3 / k_col2im3x3) -- off by default, its C entry point declared and
exported, the front-end refusing CPU tensors and wrong shapes, the module-side conditions turning
the node down so that the convolution keeps the route it has today, and the test yardstick's
col2im agreeing with autograd."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv3s_ref as S
from test_capi_symbols import declared_functions


def test_both_switches_exist_and_are_off_by_default():
    from iouaware.backbones import ResNet
    from iouaware.fpn import FPN
    assert ResNet.train_strided is False and FPN.train_strided is False
    assert ResNet(50).train_strided is False
    fpn = FPN([8, 16], 8, 4, add_extra_convs=True)
    assert fpn.train_strided is False
    fpn.train_strided = True                      # per model, settable after construction
    assert FPN.train_strided is False


def test_col2im_entry_is_declared_bound_and_exported():
    from iouaware import _lib
    assert 'ia_col2im3x3_nhwc' in declared_functions()
    assert 'ia_col2im3x3_nhwc' in _lib.SIGNATURES
    _lib.lib()                                     # builds the library when it is missing
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), 'ia_col2im3x3_nhwc')


def test_col2im_refuses_cpu_tensors_and_wrong_shapes():
    from iouaware import ops, _lib
    dcol = torch.zeros(3 * 4 * 5, 9 * 8)
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.col2im3x3(dcol, 3, 7, 9, 8, 2)
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.im2col3x3(torch.zeros(1, 4, 3, 3), 2)
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.conv3x3_dcol(torch.zeros(1, 4, 3, 3), torch.zeros(36, 4))


def test_fuse_reads_the_backbone_switch_for_its_bottlenecks():
    from iouaware.backbones import ResNet, Bottleneck
    from iouaware.fuse import fuse_inference, unfuse_inference
    for on in (False, True):
        net = ResNet(50)
        net.train_strided = on
        fuse_inference(net, winograd=True, train=True)
        blocks = [m for m in net.modules() if isinstance(m, Bottleneck)]
        assert blocks and all(b._ia_train_strided is on for b in blocks)
        unfuse_inference(net)
        assert not any(hasattr(b, '_ia_train_strided') for b in blocks)


def test_convolutions_the_node_does_not_cover_are_turned_down():
    from iouaware import train_fuse
    ok = train_fuse.strided_conv_ok
    assert ok(nn.Conv2d(8, 12, 3, stride=2, padding=1)) is True
    assert ok(nn.Conv2d(8, 12, 3, stride=2, padding=1, bias=False)) is True
    assert ok(nn.Conv2d(6, 12, 3, stride=2, padding=1)) is False               # Cin % 4
    assert ok(nn.Conv2d(8, 16, 3, stride=2, padding=1, groups=2)) is False     # grouped
    assert ok(nn.Conv2d(8, 12, 3, stride=2, padding=2, dilation=2)) is False   # dilated
    assert ok(nn.Conv2d(8, 12, 3, stride=1, padding=1)) is False               # the Winograd node's
    assert ok(nn.Conv2d(8, 12, 3, stride=(2, 1), padding=1)) is False
    assert ok(nn.Conv2d(8, 12, 3, stride=2, padding=0)) is False
    assert ok(nn.Conv2d(8, 12, 1, stride=2)) is False
    assert ok(nn.Conv2d(8, 12, 3, stride=2, padding=1).double()) is False


@pytest.mark.parametrize('cin,kw', [(6, {}), (8, dict(groups=2)), (8, dict(dilation=2, padding=2))])
def test_an_uncovered_extra_level_keeps_its_module_with_the_switch_on(cin, kw):
    """train_fuse._extra_conv on a ConvModule the node does not take (and, here, CPU features): the
    module's own forward, bit for bit"""
    from iouaware import train_fuse
    from iouaware.fpn import FPN
    from iouaware.layers import ConvModule
    torch.manual_seed(3)
    fpn = FPN([8, 8], 8, 4, add_extra_convs=True)
    fpn.train_strided = True
    fc = ConvModule(cin, 8, 3, stride=2, **dict(dict(padding=1), **kw), activation=None)
    x = torch.randn(2, cin, 7, 9)
    assert torch.equal(train_fuse._extra_conv(fpn, fc, x), fc(x))
    covered = fpn.fpn_convs[-1]                   # P7, 8 -> 8, 3x3 / 2: covered, but x is on the CPU
    x = torch.randn(2, 8, 7, 9)
    assert train_fuse.strided_conv_ok(covered.conv)
    assert torch.equal(train_fuse._extra_conv(fpn, covered, x), covered(x))


@pytest.mark.parametrize('stride,H,W', [(2, 7, 9), (2, 8, 6), (2, 1, 1), (2, 2, 3), (1, 5, 4), (3, 8, 8),
                                        (4, 9, 9)])
def test_yardstick_col2im_is_the_adjoint_of_the_convolution(stride, H, W):
    """dx = col2im(g . w_kn^T) and dW = col^T . g against F.conv2d autograd in fp64 (the formulas of
    the node, evaluated by the test helper's restatement)"""
    g = torch.Generator().manual_seed(stride * 100 + H * 10 + W)
    B, cin, cout = 2, 4, 3
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    Ho, Wo = S.out_size(H, stride), S.out_size(W, stride)
    dy = torch.randn(B, cout, Ho, Wo, generator=g, dtype=torch.float64)
    ref = S.conv_train(x, w, None, dy, stride, False)
    w_kn = w.permute(2, 3, 1, 0).reshape(9 * cin, cout)
    g2 = dy.permute(0, 2, 3, 1).reshape(-1, cout)
    dcol = (g2 @ w_kn.t()).float()
    dx = S.col2im(dcol, B, H, W, cin, stride).permute(0, 3, 1, 2)
    assert float((dx.double() - ref['dx']).abs().max()) <= 1e-5 * max(float(ref['dx'].abs().max()), 1.0)
    if stride == 4:
        assert bool((dx[:, :, 2::4, :] == 0).all())          # rows no tap reads
    col = F.unfold(x, 3, padding=1, stride=stride)            # (B, cin * 9, P): row c * 9 + tap
    col = col.view(B, cin, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(-1, 9 * cin)
    dW = (col.t() @ g2).view(3, 3, cin, cout).permute(3, 2, 0, 1)
    assert float((dW - ref['dW']).abs().max()) <= 1e-10 * max(float(ref['dW'].abs().max()), 1.0)

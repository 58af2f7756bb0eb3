"""Host: tests/gn_ref.py is GroupNorm + ReLU and its autograd (fp64 against F.group_norm: 1e-12),
the gates the GPU test of the training node applies (tests/test_gpu_groupnorm_train.py)

    gate A  max|got - ref| / max|ref| <= 1e-4                         the project's contract
    gate B  the same figure <= max(4 x that of the fp32 helper, 2^-22)

separate a correct fp32 evaluation from structural faults (a chunk of pixels lost from the group
sums, the parameter gradients of one level instead of all), and the host side of
winograd_train.fcos_usable refuses what the kernels do not cover.  If a bar is loosened until a
fault passes, this file fails."""
import pytest
import torch
import torch.nn.functional as F

import gn_ref as R

SIZES = [(20, 28), (10, 14), (5, 7)]


def _data(seed, batch, ch, sizes, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(batch, ch, h, w, generator=g) for (h, w) in sizes]
    if shift:
        xs = [x * 0.007 + 0.007 * shift for x in xs]
    ups = [torch.randn(batch, ch, h, w, generator=g) for (h, w) in sizes]
    gamma = torch.rand(ch, generator=g) + 0.5
    beta = torch.randn(ch, generator=g) * 0.3
    return xs, ups, gamma, beta


def _autograd64(xs, ups, gamma, beta, groups, relu):
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    x64 = [x.double().requires_grad_(True) for x in xs]
    ys = [F.group_norm(x, groups, gm, bt, 1e-5) for x in x64]
    if relu:
        ys = [y.relu() for y in ys]
    sum((y * u.double()).sum() for y, u in zip(ys, ups)).backward()
    return [y.detach() for y in ys], [x.grad for x in x64], gm.grad, bt.grad


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('shift', [0.0, 200.0])
def test_fp64_helper_is_group_norm_and_its_autograd(relu, shift):
    xs, ups, gamma, beta = _data(0, 3, 32, SIZES + [(1, 1)], shift)
    ys64, dx64, dg64, db64 = _autograd64(xs, ups, gamma, beta, 8, relu)
    ys = R.forward(xs, gamma, beta, 8, relu=relu)
    dxs, dg, db = R.backward(xs, ups, gamma, beta, 8, relu=relu)
    for got, ref in zip(ys + dxs + [dg, db], ys64 + dx64 + [dg64, db64]):
        assert got.shape == ref.shape
        if float(ref.abs().max()) == 0.0:            # the 1x1 level: xh = 0, dx = 0
            assert float(got.abs().max()) <= 1e-12
        else:
            assert R.rel_err(got, ref) <= 1e-12


def _passes(got, ref, helper):
    e, e32 = R.rel_err(got, ref), R.rel_err(helper, ref)
    return e <= R.GATE_A and e <= R.gate_b(e32)


def test_gates_pass_fp32_and_fail_structural_faults():
    xs, ups, gamma, beta = _data(1, 2, 64, SIZES)
    ups, dropped = R.safe_upstream(xs, ups, gamma, beta, 8)
    assert dropped <= 0.005
    ref = R.backward(xs, ups, gamma, beta, 8)
    h32 = R.backward(xs, ups, gamma, beta, 8, dtype=torch.float32)
    # a correct fp32 evaluation in another order of operations (channels-last memory) passes
    cl = [x.contiguous(memory_format=torch.channels_last) for x in xs]
    ok = R.backward(cl, [u.contiguous(memory_format=torch.channels_last) for u in ups], gamma, beta, 8,
                    dtype=torch.float32)
    for l in range(len(xs)):
        assert _passes(ok[0][l], ref[0][l], h32[0][l])
    assert _passes(ok[1], ref[1], h32[1]) and _passes(ok[2], ref[2], h32[2])
    # a lost chunk: the group means of every level with more than one chunk are off
    lost = R.backward(xs, ups, gamma, beta, 8, dtype=torch.float32, fault='lost_chunk')
    assert not any(_passes(lost[0][l], ref[0][l], h32[0][l]) for l in range(len(xs)))
    # per-level instead of all-levels parameter gradients
    lvl = R.backward(xs, ups, gamma, beta, 8, dtype=torch.float32, fault='level_dgamma')
    assert not _passes(lvl[1], ref[1], h32[1]) and not _passes(lvl[2], ref[2], h32[2])
    assert R.rel_err(lvl[1], ref[1]) > R.GATE_A and R.rel_err(lost[0][0], ref[0][0]) > R.GATE_A


def test_safe_upstream_leaves_out_little():
    xs, ups, gamma, beta = _data(2, 2, 64, SIZES)
    safe, dropped = R.safe_upstream(xs, ups, gamma, beta, 8)
    assert 0.0 < dropped <= 0.005
    pres = R.forward(xs, gamma, beta, 8, pre=True)
    for p, u, s in zip(pres, ups, safe):
        far = p.abs() > 1e-4 * p.abs().max()
        assert torch.equal(s[far], u[far]) and not s[~far].any()


# ------------------------------------------------------------------ the head's switch, host side
def _head(iou_branch=True, **kw):
    from iouaware.fcos_head import FCOSHead, IoUawareFCOSHead
    args = dict(num_classes=81, in_channels=64, feat_channels=64, stacked_convs=2,
                norm_cfg=dict(type='GN', num_groups=16, requires_grad=True))
    args.update(kw)
    return (IoUawareFCOSHead if iou_branch else FCOSHead)(**args)


@pytest.mark.parametrize('iou_branch', [True, False])
def test_fcos_usable_host_logic(iou_branch):
    from iouaware import winograd_train as T
    sizes = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
    assert _head(iou_branch).train_winograd is False          # opt-in until measured faster
    assert T.fcos_head_supported(_head(iou_branch), sizes, 2)
    assert T.fcos_head_supported(_head(iou_branch, feat_channels=256, in_channels=256,
                                       norm_cfg=dict(type='GN', num_groups=32)), sizes, 4)
    # 32 channels in 32 groups: one channel per group, no 16-byte column inside a group
    assert not T.fcos_head_supported(_head(iou_branch, in_channels=32, feat_channels=32,
                                           norm_cfg=dict(type='GN', num_groups=32)), sizes, 2)
    # 96 channels: not 4 * 2^k
    assert not T.fcos_head_supported(_head(iou_branch, feat_channels=96,
                                           norm_cfg=dict(type='GN', num_groups=8)), sizes, 2)
    # towers with bias and without norm
    assert not T.fcos_head_supported(_head(iou_branch, norm_cfg=None), sizes, 2)
    # BatchNorm towers, an output convolution that is not 3x3, channels not a multiple of 4
    assert not T.fcos_head_supported(_head(iou_branch, norm_cfg=dict(type='BN')), sizes, 2)
    h = _head(iou_branch)
    h.fcos_reg = torch.nn.Conv2d(64, 4, 1)
    assert not T.fcos_head_supported(h, sizes, 2)
    assert not T.fcos_head_supported(_head(iou_branch, in_channels=66), sizes, 2)
    # more levels than scales
    assert not T.fcos_head_supported(_head(iou_branch), sizes + [(1, 1)], 2)
    # features on the host, or without autograd: the module route
    h = _head(iou_branch).train()
    feats = [torch.zeros(2, 64, hh, ww) for (hh, ww) in sizes]
    assert not T.fcos_usable(feats, h)
    outs = h(feats)
    assert len(outs) == (4 if iou_branch else 3) and 'Wino' not in type(outs[0][0].grad_fn).__name__


def test_groupnorm_relu_refuses_before_the_device():
    from iouaware import fcos_ops
    x = torch.zeros((1, 64, 4, 4)).contiguous(memory_format=torch.channels_last)
    g, b = torch.ones(64), torch.zeros(64)
    for bad in ([x], [x.double()], [x.contiguous()], []):
        with pytest.raises(ValueError):
            fcos_ops.groupnorm_relu(bad, g, b, 16)


def test_new_size_queries_on_the_host():
    import ctypes
    from iouaware import _lib, fcos_ops
    sizes = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
    g = fcos_ops.winograd._wino_geom(sizes, 4)
    L = _lib.lib()
    rows = 4 * sum((h * w + 255) // 256 for (h, w) in sizes)
    assert L.ia_groupnorm_saved_bytes(ctypes.byref(g), 256, 32) == (5 * 4 * 32 * 16 + 255) // 256 * 256
    assert L.ia_groupnorm_bwd_workspace_bytes(ctypes.byref(g), 256, 32) == rows * (32 + 256) * 16
    for ch, gr in ((256, 48), (384, 32), (32, 32), (2048, 32)):
        assert L.ia_groupnorm_saved_bytes(ctypes.byref(g), ch, gr) == 0
        assert L.ia_groupnorm_bwd_workspace_bytes(ctypes.byref(g), ch, gr) == 0
    assert fcos_ops.groupnorm_supported(sizes, 4, 256, 32)
    assert not fcos_ops.groupnorm_supported(sizes, 4, 32, 32)

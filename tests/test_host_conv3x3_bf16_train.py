"""CPU: the opt-in bf16 training route of the RetinaNet heads (iouaware/conv3x3_bf16_train.py) -- off by
default, its C entry points declared, the weight-gradient size query, and `usable` turning the
route down (CPU features, channel counts the MFMA kernels do not take) so that the module forward
runs unchanged."""
import ctypes as C

import torch

import synth
from test_capi_symbols import declared_functions
from test_host_targets import HEAD_KW

ENTRIES = ('ia_conv3x3_bf16_wgrad_workspace_bytes', 'ia_conv3x3_bf16_wgrad_plan',
           'ia_conv3x3_bf16_wgrad_levels', 'ia_conv3x3_bf16_pack_f32',
           'ia_relu_bwd_bias_grad_bf16_workspace_bytes', 'ia_relu_bwd_bias_grad_bf16')


def _heads(**kw):
    from iouaware.head import RetinaHead, IoUawareRetinaHead
    kw = dict(dict(HEAD_KW, num_classes=5, in_channels=32, feat_channels=32, stacked_convs=2), **kw)
    return [cls(**kw) for cls in (RetinaHead, IoUawareRetinaHead)]


def test_the_route_is_off_by_default():
    from iouaware.head import RetinaHead, IoUawareRetinaHead
    assert RetinaHead.train_bf16 is False and IoUawareRetinaHead.train_bf16 is False
    for head in _heads():
        assert head.train_bf16 is False


def test_entry_points_are_declared_and_bound():
    from iouaware import _lib
    names = declared_functions()
    for name in ENTRIES:
        assert name in names and name in _lib.SIGNATURES


def _desc(cin, cout, sizes, batch=2, groups=1):
    from iouaware import _lib
    d = _lib.Conv3x3Desc()
    d.num_levels, d.batch, d.groups = len(sizes), batch, groups
    d.cin, d.cout, d.x_stride, d.y_stride = cin, cout, cin, cout
    for l, (h, w) in enumerate(sizes):
        d.H[l], d.W[l] = h, w
    return d


def test_wgrad_workspace_query():
    from iouaware import _lib
    lib = _lib.lib()
    sizes = synth.level_shapes(64, 96)
    assert len(sizes) == 5
    assert lib.ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(_desc(48, 64, sizes))) == 0
    d = _desc(32, 720, sizes)
    nbytes = lib.ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(d))
    t, st, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert lib.ia_conv3x3_bf16_wgrad_plan(C.byref(d), C.byref(t), C.byref(st), C.byref(n)) == 0
    # one fp32 partial result per slice; the slices cover the tile list
    assert nbytes == n.value * 9 * 720 * 32 * 4 and nbytes > 0
    assert (n.value - 1) * st.value < t.value <= n.value * st.value
    assert lib.ia_conv3x3_bf16_wgrad_plan(C.byref(_desc(48, 64, sizes)), None, None, None) == -1      # IA_E_ARG
    assert lib.ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(_desc(32, 64, sizes, groups=3))) == 0
    assert lib.ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(_desc(32, 0, sizes))) == 0
    assert lib.ia_relu_bwd_bias_grad_bf16_workspace_bytes(0, 64) == 0
    assert lib.ia_relu_bwd_bias_grad_bf16_workspace_bytes(100, 45) > 0


def test_unusable_inputs_fall_through_to_the_module_forward():
    from iouaware import conv3x3_bf16_train
    sizes = synth.level_shapes(64, 96)
    for head in _heads():
        head.train()
        g = torch.Generator().manual_seed(2)
        feats = [torch.randn(2, 32, h, w, generator=g) for (h, w) in sizes]
        assert conv3x3_bf16_train.usable(feats, head) is False           # CPU features
        ref = head(feats)
        head.train_bf16 = True
        got = head(feats)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            for x, y in zip(a, b):
                assert x.dtype == torch.float32 and torch.equal(x, y)
    for head in _heads(feat_channels=48):
        head.train()
        head.train_bf16 = True
        feats = [torch.zeros(1, 32, h, w) for (h, w) in sizes]
        assert conv3x3_bf16_train.usable(feats, head) is False
        # the module side alone (no device needed): 48 feature channels are turned down, 32 are not
        assert conv3x3_bf16_train.head_supported(head, sizes, 1) is False
        assert head(feats)[0][0].shape[1] == head.num_anchors * head.cls_out_channels
    for head in _heads():
        assert conv3x3_bf16_train.head_supported(head, sizes, 2) is True

"""GPU: bf16 training of the RetinaNet heads -- the MFMA weight-gradient kernel
(csrc/conv3x3_bf16_bwd.hip), the fp32 -> packed bf16 weight entry, the bf16 ReLU-backward / bias
gradient, the autograd node (iouaware/conv3x3_bf16_train.py), the head route and one detector step.

Yardstick: tests/conv3_ref.py, torch autograd of F.conv2d in fp64 on the CPU on the operands the
kernels see (x, w, dy rounded to bf16).  Gates:
  * fp32 results (dW, db): the project's tests/wino_ref.py gates -- within GATE_A = 1e-4 of the maximum
    and at most GATE_B = 4 x the error of the same autograd in fp32 on the CPU;
  * bf16 results (dx): the forward kernel's bound, |err| <= 2^-8 |want| + 2e-3 * 2^-8 * max|want| (the same
    kernel on the adjoint weight, one rounding);
  * the head: error against the fp64 module <= 1.5 x the error of torch's own bf16 module route
    + 1e-3 of the tensor's maximum (README, "Parity").
"""
import functools
import json
import os

import pytest
import torch

import conv3_ref as R
import synth
import wino_ref as WR

pytestmark = pytest.mark.gpu
BF, CL = torch.bfloat16, torch.channels_last
LEVELS = [(28, 40), (14, 20), (7, 10), (1, 2), (1, 1)]
HERE = os.path.dirname(os.path.abspath(__file__))


def _pad32(n):
    return (n + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def _wgrad_case(cin, cout, groups, sizes, batch, dense_dy):
    """inputs on the CPU (bf16 values) and the fp64 / fp32 weight gradients, computed once.
    x: the channel halves of a 2 * cin-wide activation; dy: half zeros, like behind a ReLU; the
    channel slices [g * P, g * P + cout) of a groups * P-wide tensor (P = cout rounded up to 32), or
    -- dense_dy -- a dense tensor of cout channels (an odd pixel stride for an odd cout)"""
    g = torch.Generator().manual_seed(1000 * cin + cout + groups)
    P = cout if dense_dy else _pad32(cout)
    acts = [torch.randn(batch, 2 * cin, h, w, generator=g).to(BF).contiguous(memory_format=CL) for (h, w) in sizes]
    dys = [(torch.randn(batch, groups * P, h, w, generator=g) * (torch.rand(batch, groups * P, h, w, generator=g) > 0.5))
           .to(BF).contiguous(memory_format=CL) for (h, w) in sizes]
    xs = [[a[:, k * cin:(k + 1) * cin] for a in acts] for k in range(groups)]
    ds = [[d[:, k * P:k * P + cout] for d in dys] for k in range(groups)]
    w = torch.zeros(groups * cout, cin, 3, 3)
    ref = R.conv_grads_groups(xs, w, ds, torch.float64, want=('dw',))['dw']
    helper = R.conv_grads_groups(xs, w, ds, torch.float32, want=('dw',))['dw']
    return acts, dys, P, ref, helper


def _dev_slices(acts, dys, cin, cout, groups, P):
    acts = [a.cuda().contiguous(memory_format=CL) for a in acts]
    dys = [d.cuda().contiguous(memory_format=CL) for d in dys]
    xs = [[a[:, k * cin:(k + 1) * cin] for a in acts] for k in range(groups)]
    ds = [[d[:, k * P:k * P + cout] for d in dys] for k in range(groups)]
    return xs, ds


# ------------------------------------------------------------------ 1: weight gradient against fp64
@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('cin,cout', [(32, 64), (64, 80), (32, 45), (96, 720)])
def test_wgrad_against_fp64(cin, cout, groups):
    from iouaware import ops
    acts, dys, P, ref, helper = _wgrad_case(cin, cout, groups, tuple(LEVELS), 3, False)
    xs, ds = _dev_slices(acts, dys, cin, cout, groups, P)
    dw = ops.conv3x3_bf16_wgrad_levels(xs, ds, cin, cout)
    assert dw.shape == (groups * cout, cin, 3, 3) and dw.dtype == torch.float32
    e, h, ratio = WR.gates(dw, helper, ref)
    print('wgrad %d->%d x%d: err %.3g  fp32 helper %.3g  ratio %.2f' % (cin, cout, groups, e, h, ratio))
    assert e <= WR.GATE_A and ratio <= WR.GATE_B


@pytest.mark.parametrize('cin,cout', [(32, 45), (64, 80)])
def test_wgrad_single_level_dense_dy(cin, cout):
    """one level (13, 21), one image, dy a dense tensor of cout channels: pixel stride 45 (element
    loads) and 80 (16-byte loads)"""
    from iouaware import ops
    acts, dys, P, ref, helper = _wgrad_case(cin, cout, 1, ((13, 21),), 1, True)
    xs, ds = _dev_slices(acts, dys, cin, cout, 1, P)
    assert ds[0][0].stride(3) == cout
    dw = ops.conv3x3_bf16_wgrad_levels(xs, ds, cin, cout)
    e, h, ratio = WR.gates(dw, helper, ref)
    print('wgrad single level %d->%d: err %.3g  fp32 helper %.3g  ratio %.2f' % (cin, cout, e, h, ratio))
    assert e <= WR.GATE_A and ratio <= WR.GATE_B


# ------------------------------------------------------------------ 2: workspace and determinism
def test_wgrad_workspace_and_determinism():
    from iouaware import ops, _lib
    sizes, batch, cin, cout = ((13, 21), (7, 10), (1, 1)), 3, 32, 64
    acts, dys, P, ref, helper = _wgrad_case(cin, cout, 1, sizes, batch, False)
    xs, ds = _dev_slices(acts, dys, cin, cout, 1, P)
    tiles, slice_tiles, slices = ops.conv3x3_bf16_wgrad_plan(xs, ds, cin, cout)
    # K spans at least three split-K slices and the last one is partial
    assert slices >= 3 and tiles % slice_tiles != 0 and (slices - 1) * slice_tiles < tiles < slices * slice_tiles
    import ctypes as C
    nbytes = _lib.lib().ia_conv3x3_bf16_wgrad_workspace_bytes(C.byref(ops._wgrad_desc(xs, ds, cin, cout)))
    assert nbytes == slices * 9 * cout * cin * 4
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    a = ops.conv3x3_bf16_wgrad_levels(xs, ds, cin, cout, workspace=ws)
    ws.view(torch.float32).fill_(float('nan'))
    b = ops.conv3x3_bf16_wgrad_levels(xs, ds, cin, cout, workspace=ws)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    e, h, ratio = WR.gates(a, helper, ref)
    assert e <= WR.GATE_A and ratio <= WR.GATE_B
    small = torch.zeros(nbytes - 16, dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.conv3x3_bf16_wgrad_levels(xs, ds, cin, cout, workspace=small)


# ------------------------------------------------------------------ 3: input gradient, adjoint pack
@pytest.mark.parametrize('cout', [80, 720])
def test_dx_against_fp64_and_adjoint_pack(cout):
    from iouaware import ops, conv3x3_bf16_train as T
    cin, batch, sizes = 32, 2, [(14, 20), (7, 10), (1, 2)]
    g = torch.Generator().manual_seed(cout)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    xs = [torch.randn(batch, cin, h, wd, generator=g).to(BF) for (h, wd) in sizes]
    dys = [torch.randn(batch, cout, h, wd, generator=g).to(BF) for (h, wd) in sizes]
    want = R.conv_grads(xs, w.to(BF), dys, torch.float64, want=('dx',))['dx']
    wd = w.cuda()
    xd = [x.cuda().contiguous(memory_format=CL).requires_grad_(True) for x in xs]
    ys = T.conv_levels([xd], wd, None, relu=False)[0]
    assert all(y.shape == (batch, cout, h, w_) and y.dtype == BF for y, (h, w_) in zip(ys, sizes))
    dx = torch.autograd.grad(ys, xd, [d.cuda() for d in dys])
    for got, ref in zip(dx, want):
        assert got.dtype == BF and got.shape == ref.shape
        err = (got.double().cpu() - ref).abs()
        assert bool((err <= R.bf16_bound(ref)).all()), (float(err.max()), float(ref.abs().max()))
    # the one-launch fp32 entry against a cast, a transpose, a flip, a zero pad and the bf16 entry
    P = _pad32(cout)
    wt = torch.zeros(cin, P, 3, 3, dtype=BF, device='cuda')
    wt[:, :cout] = wd.to(BF).flip(2, 3).transpose(0, 1)
    a, b = ops.conv3x3_bf16_pack(wd, adjoint=True), ops.conv3x3_bf16_pack(wt)
    assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
    a, b = ops.conv3x3_bf16_pack(wd), ops.conv3x3_bf16_pack(wd.to(BF))
    assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------ 4: mask and bias gradient
@pytest.mark.parametrize('n,wide', [(64, 96), (45, 45), (45, 64), (720, 736)])
@pytest.mark.parametrize('masked', [True, False])
def test_relu_bwd_bias_grad_bf16(n, wide, masked):
    from iouaware import ops
    B, H, W = 3, 28, 40
    g = torch.Generator(device='cuda').manual_seed(n + wide)
    dy = torch.randn(B, n, H, W, device='cuda', generator=g).to(BF).contiguous(memory_format=CL)
    y = None
    if masked:
        y = torch.randn(B, wide, H, W, device='cuda', generator=g).to(BF).contiguous(memory_format=CL)[:, :n]
        flat = y.permute(0, 2, 3, 1)
        flat[0, 0, :5] = 0.0                   # y == +0 and y == -0 are masked
        flat[0, 1, :5] = -0.0
        assert bool((y[0, :, 1, :5].view(torch.int16) == -32768).all())
    out = torch.zeros(B, wide, H, W, dtype=BF, device='cuda').contiguous(memory_format=CL)
    gg, db = ops.relu_bwd_bias_grad_bf16(dy, y, bias_grad=True, out=out[:, :n])
    want_g = dy * (y > 0) if masked else dy
    assert torch.equal(gg.contiguous().view(torch.int16), want_g.contiguous().view(torch.int16))
    assert not bool(out[:, n:].any())           # the padding channels of the wider tensor are not touched
    ref = want_g.double().cpu().sum((0, 2, 3))
    helper = want_g.float().cpu().sum((0, 2, 3))
    e, h, ratio = WR.gates(db.cpu(), helper, ref)
    print('db n=%d stride %d masked=%s: err %.3g  fp32 helper %.3g  ratio %.2f' % (n, wide, masked, e, h, ratio))
    assert db.dtype == torch.float32 and db.shape == (n,)
    assert e <= WR.GATE_A and ratio <= WR.GATE_B
    # a new output tensor; no bias gradient; nothing to do
    g2, none = ops.relu_bwd_bias_grad_bf16(dy, y, bias_grad=False)
    assert none is None and torch.equal(g2.view(torch.int16), want_g.contiguous(memory_format=CL).view(torch.int16))
    if not masked:
        assert g2 is dy


# ------------------------------------------------------------------ 5: the node
def _node_reference(xs_groups, w, dys_groups, ys_groups, relu):
    """fp64 / fp32 gradients with the ReLU mask taken from the node's own (stored) outputs"""
    gs = [[(d.double().cpu() * ((y.detach().double().cpu() > 0) if relu else 1.0)) for d, y in zip(ds, ys)]
          for ds, ys in zip(dys_groups, ys_groups)]
    wb = w.to(BF)
    ref = R.conv_grads_groups(xs_groups, wb, gs, torch.float64)
    helper = R.conv_grads_groups(xs_groups, wb, gs, torch.float32, want=('dw', 'db'))
    return ref, helper


@pytest.mark.parametrize('relu,bias', [(True, True), (False, False)])
def test_node_two_groups(relu, bias):
    """two towers on their own inputs (channel halves of one activation); the reg tower's input does
    not require grad: its gradient is None"""
    from iouaware import conv3x3_bf16_train as T
    cin, cout, batch, sizes = 32, 64, 2, [(14, 20), (7, 10), (1, 1)]
    g = torch.Generator(device='cuda').manual_seed(5)
    w = (torch.randn(2 * cout, cin, 3, 3, device='cuda', generator=g) * 0.08).requires_grad_(True)
    b = (torch.randn(2 * cout, device='cuda', generator=g) * 0.1).requires_grad_(True) if bias else None
    acts = [torch.randn(batch, 2 * cin, h, wd, device='cuda', generator=g).to(BF).contiguous(memory_format=CL)
            for (h, wd) in sizes]
    # (both groups with the pixel stride 2 * cin: the cls half of one activation that requires grad,
    # the reg half of another that does not)
    leaf = [a.clone(memory_format=torch.preserve_format).requires_grad_(True) for a in acts]
    xa = [a[:, :cin] for a in leaf]
    xb = [a[:, cin:] for a in acts]
    ys = T.conv_levels([xa, xb], w, b, relu=relu)
    assert len(ys) == 2 and all(y.shape == (batch, cout, h, wd) for k in range(2) for y, (h, wd) in zip(ys[k], sizes))
    flat = [y for k in range(2) for y in ys[k]]
    dys = [torch.randn(y.shape, device='cuda', generator=g).to(BF) for y in flat]
    leaves = [w] + ([b] if bias else []) + xa
    seen, real_bwd = {}, T._Bf16ConvLevels.backward

    def spy(ctx, *gs):
        seen['out'] = real_bwd(ctx, *gs)
        return seen['out']
    T._Bf16ConvLevels.backward = staticmethod(spy)
    try:
        grads = list(torch.autograd.grad(flat, leaves, dys))
    finally:
        T._Bf16ConvLevels.backward = staticmethod(real_bwd)
    L = len(sizes)
    ref, helper = _node_reference([xa, xb], w, [dys[:L], dys[L:]], ys, relu)
    dw = grads.pop(0)
    e, h, ratio = WR.gates(dw, helper['dw'], ref['dw'])
    print('node dW relu=%s: err %.3g helper %.3g ratio %.2f' % (relu, e, h, ratio))
    assert dw.dtype == torch.float32 and e <= WR.GATE_A and ratio <= WR.GATE_B
    if bias:
        db = grads.pop(0)
        e, h, ratio = WR.gates(db, helper['db'], ref['db'])
        assert db.dtype == torch.float32 and e <= WR.GATE_A and ratio <= WR.GATE_B
    for got, want in zip(grads, ref['dx'][0]):
        err = (got.double().cpu() - want).abs()
        assert got.dtype == BF and bool((err <= R.bf16_bound(want)).all()), float(err.max())
    # inputs that do not require grad get None ...
    assert all(o is not None for o in seen['out'][4:4 + L]) and all(o is None for o in seen['out'][4 + L:])
    # ... and when no input requires grad there is no input-gradient launch at all
    from iouaware import ops
    ys2 = T.conv_levels([[a.detach() for a in xa], xb], w, b, relu=relu)
    calls, real = [], ops.conv3x3_bf16_levels
    ops.conv3x3_bf16_levels = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        torch.autograd.grad([y for k in range(2) for y in ys2[k]], [w], dys)
    finally:
        ops.conv3x3_bf16_levels = real
    assert calls == []


def test_node_shared_input_sums_both_towers():
    from iouaware import conv3x3_bf16_train as T
    cin, cout, batch, sizes = 32, 32, 2, [(14, 20), (7, 10)]
    g = torch.Generator(device='cuda').manual_seed(6)
    w = (torch.randn(2 * cout, cin, 3, 3, device='cuda', generator=g) * 0.08).requires_grad_(True)
    b = (torch.randn(2 * cout, device='cuda', generator=g) * 0.1).requires_grad_(True)
    xs = [torch.randn(batch, cin, h, wd, device='cuda', generator=g).to(BF).contiguous(memory_format=CL)
          .requires_grad_(True) for (h, wd) in sizes]
    ys = T.conv_levels([xs, xs], w, b, relu=True)
    flat = [y for k in range(2) for y in ys[k]]
    dys = [torch.randn(y.shape, device='cuda', generator=g).to(BF) for y in flat]
    grads = list(torch.autograd.grad(flat, [w, b] + xs, dys))
    L = len(sizes)
    ref, helper = _node_reference([xs, xs], w, [dys[:L], dys[L:]], ys, True)
    e, h, ratio = WR.gates(grads[0], helper['dw'], ref['dw'])
    assert e <= WR.GATE_A and ratio <= WR.GATE_B
    e, h, ratio = WR.gates(grads[1], helper['db'], ref['db'])
    assert e <= WR.GATE_A and ratio <= WR.GATE_B
    for got, wa, wb in zip(grads[2:], ref['dx'][0], ref['dx'][1]):
        want = wa + wb
        err = (got.double().cpu() - want).abs()
        assert bool((err <= R.bf16_bound(want)).all()), float(err.max())


def test_bias_grad_launches_do_not_depend_on_allocator_placement():
    """levels share one mask / bias-gradient launch only as views of ONE storage.  Two separately
    allocated gradients that happen to lie side by side (an upstream node's per-level results) must
    take the launches they take anywhere else: the strips of the column sums, and with them the
    bits of db, would otherwise follow the allocator from run to run."""
    from iouaware import ops, conv3x3_bf16_train as T
    n, shape = 64, (1, 64, 2, 2)                       # 4 rows x 128 bytes = one 512-byte allocation
    for _ in range(64):                                # two allocations that ARE neighbours (the usual case;
        keep = [torch.empty(shape, dtype=BF, device='cuda', memory_format=CL).normal_() for _ in range(2)]
        if keep[1].data_ptr() == keep[0].data_ptr() + 512:   # if the allocator never obliges, the rest still holds)
            break
    calls, real = [], ops.relu_bwd_bias_grad_bf16_rows
    ops.relu_bwd_bias_grad_bf16_rows = lambda *a: (calls.append(a[5]), real(*a))[1]
    try:
        flat = T._alloc_levels(keep, n)                # views of one storage: one launch
        db_a = T._mask_and_bias_grad(keep, None, flat, n, True)
        assert calls == [4, 4], calls                  # dy: two storages -> two launches of 4 rows
        both = torch.cat([k.permute(0, 2, 3, 1).reshape(-1, n) for k in keep])
        views = [both[4 * i:4 * i + 4].view(1, 2, 2, n).permute(0, 3, 1, 2) for i in range(2)]
        del calls[:]
        db_b = T._mask_and_bias_grad(views, None, flat, n, True)
        assert calls == [8], calls                     # one storage, consecutive: one launch of 8 rows
    finally:
        ops.relu_bwd_bias_grad_bf16_rows = real
    want = both.double().sum(0)
    for db in (db_a, db_b):
        assert float((db.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ------------------------------------------------------------------ 6: the heads
DRAWS = 4


def _small_head(cls, seed=7):
    from test_host_targets import HEAD_KW
    torch.manual_seed(seed)
    head = cls(**dict(HEAD_KW, num_classes=5, in_channels=32, feat_channels=32, stacked_convs=2))
    with torch.no_grad():
        for p in head.parameters():
            p.normal_(0, 0.05)
    return head.train()


def _run_head(head, feats, ups):
    head.zero_grad()
    xs = [f.clone().requires_grad_(True) for f in feats]
    outs = head(xs)
    flat = [t for o in outs for t in o]
    loss = sum((t.double() * u.to(t.device).double()).sum() for t, u in zip(flat, ups)) if ups else None
    if loss is not None:
        loss.backward()
    res = {'out%d' % i: t.detach().double().cpu() for i, t in enumerate(flat)}
    if loss is not None:
        res.update({n: p.grad.detach().double().cpu() for n, p in head.named_parameters()})
        # the feature gradient as ONE tensor over the levels: P6 / P7 have two / one pixel per image here,
        # a level's whole gradient is a handful of terms there and one flipped ReLU element (see
        # test_head_against_fp64_and_torch_bf16) is its entire error in whichever route it hits
        res['features'] = torch.cat([x.grad.detach().double().cpu().reshape(-1) for x in xs])
    return res, outs


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize('iou', [False, True])
def test_head_against_fp64_and_torch_bf16(iou):
    """Outputs and every parameter / feature gradient of the head on the bf16 route against the fp64
    module, judged by the project's bf16 contract (README "Parity", tests/test_gpu_e2e.py): the RMS
    error at most 1.5 x that of torch's own bf16 module route + 1e-3 of the tensor's maximum.
    RMS, not the largest element, for the reason the Winograd head test is norm-wise: a tower
    pre-activation within bf16 rounding of zero falls on either side of the ReLU mask in ANY bf16
    evaluation, the comparator included, and one flipped element moves a gradient by a whole term of
    its sum (258 pixels here: 4-6 on gradients whose maximum is 23, in both routes alike), so the
    largest element says which elements the draw put next to zero, not how the route computes.
    For the same reason the RMS is pooled over DRAWS independent draws of the issue's case (weights,
    features, cotangents): a tower gradient's error is a few dozen such events per draw, and which
    route they hit harder varies from draw to draw (ratio of the two RMS errors over 20 draws on one
    MI355X: 0.3 - 1.6 per tensor, mean 0.93); four draws halve that spread."""
    import copy
    from iouaware.head import RetinaHead, IoUawareRetinaHead
    from iouaware.config import ConfigDict
    from test_host_targets import TRAIN_CFG
    sizes, B = synth.level_shapes(64, 96), 2
    sq, top = {}, {}                       # per tensor: squared errors (route, comparator), count; max |ref|
    for draw in range(DRAWS):
        head = _small_head(IoUawareRetinaHead if iou else RetinaHead, seed=7 + draw)
        g = torch.Generator().manual_seed(8 + draw)
        feats = [torch.randn(B, 32, h, w, generator=g) for (h, w) in sizes]
        widths = [head.num_anchors * head.cls_out_channels, head.num_anchors * 4] + ([head.num_anchors] if iou else [])
        ups = [torch.randn(B, c, h, w, generator=g) for c in widths for (h, w) in sizes]
        # yardstick: the module in fp64 on the CPU; comparator: torch's bf16 module route on the device
        ref, _ = _run_head(copy.deepcopy(head).double(), [f.double() for f in feats], ups)
        cmp_head = copy.deepcopy(head).cuda().to(BF)
        cmp_, _ = _run_head(cmp_head, [f.cuda().to(BF).contiguous(memory_format=CL) for f in feats], ups)
        dev = copy.deepcopy(head).cuda()
        dev.train_bf16 = True
        got, outs = _run_head(dev, [f.cuda() for f in feats], ups)
        assert 'Bf16ConvLevels' in type(outs[0][0].grad_fn).__name__
        assert len(outs) == (3 if iou else 2)
        for o, c in zip(outs, widths):
            for t, (h, w) in zip(o, sizes):
                assert t.dtype == BF and t.shape == (B, c, h, w)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert got[k].shape == ref[k].shape
            a = sq.setdefault(k, [0.0, 0.0, 0])
            a[0] += float((got[k] - ref[k]).pow(2).sum())
            a[1] += float((cmp_[k] - ref[k]).pow(2).sum())
            a[2] += ref[k].numel()
            top[k] = max(top.get(k, 0.0), float(ref[k].abs().max()))
    for k in sorted(sq):
        e_got, e_cmp = (sq[k][0] / sq[k][2]) ** 0.5, (sq[k][1] / sq[k][2]) ** 0.5
        print('%-28s max %.3g  bf16 route %.3g  torch bf16 %.3g' % (k, top[k], e_got, e_cmp))
        assert e_got <= 1.5 * e_cmp + 1e-3 * top[k], (k, e_got, e_cmp, top[k])
    # ---- one loss evaluation with device targets: keys and shapes of the fp32 route, finite, and as close
    # to the fp32 route as torch's bf16 module route is (the same gate)
    gts, gls = synth.train_targets(11, B, 64, 96, max_gt=4)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda().clamp(max=4) for x in gls]
    metas = [synth.img_meta(64, 96, 64, 96) for _ in range(B)]
    cfg = ConfigDict(TRAIN_CFG)

    def losses(h, xs):
        o = h(xs)
        return h.loss(*o, gtb, gtl, metas, cfg)
    fp32 = copy.deepcopy(head).cuda()
    la = losses(fp32, [f.cuda() for f in feats])
    lb = losses(dev, [f.cuda() for f in feats])
    lc = losses(cmp_head, [f.cuda().to(BF).contiguous(memory_format=CL) for f in feats])
    assert sorted(la) == sorted(lb)
    for k in la:
        assert len(la[k]) == len(lb[k])
        for a, b, c in zip(la[k], lb[k], lc[k]):
            a, b, c = float(a), float(b), float(c)
            print('%s fp32 %.6g  bf16 route %.6g  torch bf16 %.6g' % (k, a, b, c))
            assert lb[k][0].shape == la[k][0].shape and b == b and abs(b) != float('inf')
            assert abs(b - a) <= 1.5 * abs(c - a) + 1e-3 * abs(a), (k, a, b, c)


# ------------------------------------------------------------------ 7: the detector
def test_detector_step_is_finite_and_repeatable():
    """one train_step of retinanet_r50_fpn_1x (small image, B = 2) with the bf16 head: every parameter
    gets a finite gradient, and a second step from the same state gives the same bits.  The
    framework's own convolutions (backbone, neck) are asked for their deterministic kernels for
    the duration: without that the P6 / P7 features differ from run to run on this stack, with the
    bf16 head and without (the library picks an atomics-based kernel for the stride-2 convolutions)."""
    import iouaware
    from iouaware.config import ConfigDict
    from iouaware.train import build_optimizer, train_step
    with open(os.path.join(HERE, 'golden', 'retina_plain_ref.json')) as fh:
        rec = json.load(fh)['retinanet_r50_fpn_1x']
    rec['model']['pretrained'] = None
    torch.manual_seed(0)
    model = iouaware.build_detector(ConfigDict(rec['model']), train_cfg=ConfigDict(rec['train_cfg']),
                                    test_cfg=ConfigDict(rec['test_cfg'])).cuda().train()
    model.bbox_head.train_bf16 = True
    B, ph, pw = 2, 128, 160
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(B, 3, ph, pw, device='cuda', generator=g)
    gts, gls = synth.train_targets(11, B, ph, pw, max_gt=5)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    metas = [synth.img_meta(ph, pw, ph, pw) for _ in range(B)]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    seen, real = [], type(model.bbox_head).forward

    def spy(self, feats):
        outs = real(self, feats)
        seen.append(type(outs[0][0].grad_fn).__name__)
        return outs
    runs = []
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    type(model.bbox_head).forward = spy
    try:
        for _ in range(2):
            model.load_state_dict(state)
            opt = build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001))
            log = train_step(model, opt, img, metas, gtb, gtl)
            for n, p in model.named_parameters():
                assert p.grad is not None or not p.requires_grad, n
            runs.append((log, {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}))
    finally:
        torch.backends.cudnn.deterministic = was
        type(model.bbox_head).forward = real
    assert seen and all('Bf16ConvLevels' in s for s in seen), seen        # the bf16 route was taken
    (la, ga), (lb, gb) = runs
    assert any(n.startswith('bbox_head.') for n in ga)
    assert all(v == v and abs(v) != float('inf') for v in la.values()), la
    for n in ga:
        assert bool(torch.isfinite(ga[n]).all()), n
    assert la == lb, (la, lb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n

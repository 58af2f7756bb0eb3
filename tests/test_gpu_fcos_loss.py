"""GPU: the FCOS training kernels (csrc/pointloss.hip) -- point targets bit for bit against the
torch evaluation on the CPU and the reference's arrays, the all-levels loss node and its gradients
against the torch `_loss` body in fp64, the reference fixture tests/golden/fcos_loss.npz
(tests/golden/make_golden_fcos_loss.py), the heads' switch and the entries' return codes.

Error bound of the loss comparisons (losses and every gradient tensor, error relative to the
tensor's max-abs in the fp64 yardstick): <= 1e-4, the project's fp32 contract, AND
<= 4 x the error of the fp32 torch route on the same inputs on the device, with a floor of 2^-22
for what the torch route gets exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synth_fcos_loss as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device('cuda:0')
TOL = 1e-4
FLOOR = 2.0 ** -22
SMALL_SIZES = S.synth_fcos.level_shapes(128, 160)


def _dev(xs, grad=False):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad) for x in xs]


def _geom(sizes):
    from iouaware import fcos_ops
    return fcos_ops.PointGeometry(sizes, S.STRIDES, S.C)


def _gpu_targets(sizes, gb, gl):
    from iouaware import fcos_ops
    lab, tgt, counts = fcos_ops.point_targets(_geom(sizes), _dev(gb), _dev(gl), S.RANGES)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in lab], [t.cpu().numpy() for t in tgt], counts.cpu().numpy()


def _cpu_targets(sizes, gb, gl):
    """the project's torch fcos_target on the CPU in fp32, per level (B, N_l[, 4])"""
    head = S.make_head(False, False)
    pts = head.get_points(sizes, torch.float32, 'cpu')
    lab, tgt = head.fcos_target(pts, [torch.from_numpy(b) for b in gb], [torch.from_numpy(x) for x in gl])
    B = len(gb)
    return [t.numpy().reshape(B, -1) for t in lab], [t.numpy().reshape(B, -1, 4) for t in tgt]


def _same_targets(got, ref, what):
    for l, (a, b) in enumerate(zip(got[0], ref[0])):
        assert a.dtype == np.int64 and np.array_equal(a, b), '%s: labels of level %d differ' % (what, l)
    for l, (a, b) in enumerate(zip(got[1], ref[1])):
        assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            '%s: bbox_targets of level %d differ in %d entries' % (
                what, l, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def _check_targets(sizes, gb, gl, unique_areas=True):
    if unique_areas:
        S.check_conditions(sizes, gb, gl)
    lab, tgt, counts = _gpu_targets(sizes, gb, gl)
    _same_targets((lab, tgt), _cpu_targets(sizes, gb, gl), 'against torch on the CPU')
    assert counts.dtype == np.int32
    assert np.array_equal(counts, sum((a > 0).sum(1) for a in lab))
    return lab, tgt


# ------------------------------------------------------------------ 1. targets, bit for bit
def _special(name):
    ih, iw = 120, 150
    if name == 'one_gt':
        return S.gts(51, 3, ih, iw, 1, 1)
    if name == 'gt512':
        gb, gl = S.gts(52, 2, ih, iw, 512, 512)
        return [gb[0], gb[1][:5]], [gl[0], gl[1][:5]]
    if name == 'batch16':
        return S.gts(53, 16, ih, iw, 1, 6)
    if name == 'edge':
        # x1 = 36 passes through the level-0 points x = 36: left == 0 there, not inside
        return ([np.array([[36.0, 10.5, 90.25, 60.5]], np.float32)], [np.array([7], np.int64)])
    if name == 'range_end':
        # level-0 point (36, 20) in the first box: right = 64 = the end of (-1, 64);
        # level-1 point (40, 40) in the second: right = 64 = the start of (64, 128)
        return ([np.array([[30.5, 10.5, 100.0, 30.5], [20.5, 33.5, 104.0, 46.5]], np.float32)],
                [np.array([11, 12], np.int64)])
    if name == 'nowhere':
        return ([np.array([[0.5, 0.5, 3.0, 3.0]], np.float32), S.gts(54, 1, ih, iw, 2, 2)[0][0]],
                [np.array([3], np.int64), np.array([4, 5], np.int64)])
    raise KeyError(name)


@pytest.mark.parametrize('name', ['main', 'small', 'one_gt', 'gt512', 'batch16', 'edge', 'range_end',
                                  'nowhere'])
def test_targets_bit_for_bit_against_torch_on_the_cpu(name):
    if name in ('main', 'small'):
        sizes, gb, gl, _ = S.case_inputs(S.MAIN if name == 'main' else S.SMALL)
        pos = S.check_conditions(sizes, gb, gl, 50 if name == 'main' else 0)
        print(name, 'positives per level', pos)
    else:
        sizes, (gb, gl) = SMALL_SIZES, _special(name)
    lab, tgt = _check_targets(sizes, gb, gl)
    W0, W1 = sizes[0][1], sizes[1][1]
    if name == 'edge':
        col = lab[0].reshape(-1, W0)[:, 4]                 # the points x = 36
        assert (tgt[0].reshape(-1, W0, 4)[:, 4, 0] == 0).all() and (col == 0).all()
        assert (lab[0] == 7).any()
    if name == 'range_end':
        assert tgt[0][0, 2 * W0 + 4, 2] == 64 and lab[0][0, 2 * W0 + 4] == 11
        assert tgt[1][0, 2 * W1 + 2, 2] == 64 and lab[1][0, 2 * W1 + 2] == 12
    if name == 'nowhere':
        assert all((a[0] == 0).all() for a in lab)         # image 0: no point inside its gt
        assert any((a[1] > 0).any() for a in lab)
    if name == 'gt512':
        assert gb[0].shape[0] == 512


def test_targets_equal_area_tie_takes_the_lowest_index():
    """two gts of one fp32 area: the lowest index wins (numpy's argmin; torch leaves it open)"""
    boxes = np.array([[10.5, 10.5, 60.5, 50.5], [20.5, 10.5, 70.5, 50.5], [15.5, 12.5, 40.5, 30.5]],
                     np.float32)
    for order, labels in (((0, 1, 2), (5, 9, 2)), ((1, 0, 2), (9, 5, 2)), ((2, 1, 0), (2, 9, 5))):
        gb = [boxes[list(order)]]
        gl = [np.array(labels, np.int64)]
        area = (gb[0][:, 2] - gb[0][:, 0] + np.float32(1)) * (gb[0][:, 3] - gb[0][:, 1] + np.float32(1))
        assert len(np.unique(area)) == 2
        lab, tgt, _ = _gpu_targets(SMALL_SIZES, gb, gl)
        ref = S.np_targets(SMALL_SIZES, gb, gl)
        _same_targets((lab, tgt), ref, 'against numpy')
        first = labels[min(order.index(0), order.index(1))]
        both = {5, 9} - {first}
        # the points in both big boxes and outside the small one carry the first of the two
        assert (lab[0] == first).any() and (lab[0] == both.pop()).any()


def test_targets_against_the_reference_fixture():
    g = np.load(os.path.join(GOLD, 'fcos_loss.npz'))
    for k, case in enumerate((S.SMALL, S.MAIN1)):
        sizes, gb, gl, _ = S.case_inputs(case)
        lab, tgt, _ = _gpu_targets(sizes, gb, gl)
        B = len(gb)
        ref = ([g['labels_%d_%d' % (k, l)].reshape(B, -1) for l in range(len(sizes))],
               [g['bbox_targets_%d_%d' % (k, l)].reshape(B, -1, 4) for l in range(len(sizes))])
        _same_targets((lab, tgt), ref, 'against the reference, case %d' % k)


def test_targets_of_an_image_do_not_depend_on_the_batch():
    sizes, gb, gl, _ = S.case_inputs(S.MAIN)
    lab, tgt, counts = _gpu_targets(sizes, gb, gl)
    for b in (0, 2):
        l1, t1, c1 = _gpu_targets(sizes, gb[b:b + 1], gl[b:b + 1])
        _same_targets((l1, t1), ([a[b:b + 1] for a in lab], [a[b:b + 1] for a in tgt]), 'image %d alone' % b)
        assert c1[0] == counts[b]


# ------------------------------------------------------------------ 2. loss and gradients
KEYS = ('loss_cls', 'loss_reg', 'loss_centerness', 'loss_iou')
KINDS = ('cls', 'reg', 'ctr', 'iou')


def _grads_of(losses, outs, which):
    """{grad_of: {kind: [L numpy arrays]}} of a loss dict with respect to the head outputs"""
    flat = [t for m in outs for t in m]
    L = len(outs[0])
    res = {}
    for w in which:
        tgt = sum(v.sum() for v in losses.values()) if w == 'sum' else losses[w].sum()
        gs = torch.autograd.grad(tgt, flat, allow_unused=True, retain_graph=True)
        gs = [np.zeros(tuple(t.shape)) if g is None else g.detach().cpu().numpy() for g, t in zip(gs, flat)]
        res[w] = {k: gs[i * L:(i + 1) * L] for i, k in enumerate(KINDS[:len(outs)])}
    return res


def _route(kind, iou_branch, outs_np, gb, gl, attach=True, gamma=2.0, alpha=0.25):
    """losses {key: float} and gradients of one evaluation.  kind: 'fp64' (the torch body in fp64 on
    the CPU: the yardstick), 'torch' (the same body in fp32 on the device, the HIP focal op),
    'fused' (the HIP node)"""
    from iouaware import fcos_ops
    n = 4 if iou_branch else 3
    which = list(KEYS[:n]) + ['sum']
    if kind == 'fp64':
        outs = [[torch.from_numpy(x).double().requires_grad_(True) for x in m] for m in outs_np[:n]]
        head = S.make_head(iou_branch, False)
        with S.torch_route(cpu_focal=True, detach_iou_target=not attach):
            losses = S.head_loss(head, outs, [torch.from_numpy(b).double() for b in gb],
                                 [torch.from_numpy(x) for x in gl], gamma, alpha)
    elif kind == 'torch':
        outs = [_dev(m, True) for m in outs_np[:n]]
        head = S.make_head(iou_branch, False)
        with S.torch_route(detach_iou_target=not attach):
            losses = S.head_loss(head, outs, _dev(gb), _dev(gl), gamma, alpha)
    else:
        outs = [_dev(m, True) for m in outs_np[:n]]
        sizes = [tuple(x.shape[-2:]) for x in outs_np[0]]
        geom = _geom(sizes)
        lab, tgt, counts = fcos_ops.point_targets(geom, _dev(gb), _dev(gl), S.RANGES)
        losses = fcos_ops.point_head_loss(geom, outs[0], outs[1], outs[2], outs[3] if iou_branch else None,
                                          lab, tgt, counts, gamma, alpha, attach_iou_target=attach)
    assert list(losses) == list(KEYS[:n])
    vals = {k: float(v.detach().double().sum()) for k, v in losses.items()}
    return vals, _grads_of(losses, outs, which)


def _judge(tag, got, ref32, ref64, scale):
    """the bound of this module on one quantity; prints the observed errors"""
    if scale == 0.0:
        assert not np.any(got), '%s: the yardstick is zero everywhere, the result is not' % tag
        return 0.0
    e = float(np.abs(np.asarray(got, np.float64) - ref64).max()) / scale
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) / scale
    print('%-46s fused %.3e  torch fp32 %.3e  ratio %.2f' % (tag, e, e32, e / max(e32, 1e-30)))
    assert e <= TOL, '%s: error %.3e above %.0e' % (tag, e, TOL)
    assert e <= max(4.0 * e32, FLOOR), '%s: error %.3e above 4 x the torch route (%.3e)' % (tag, e, e32)
    return e


# (IoU branch, attach_iou_target): the flag only exists with the branch
@pytest.mark.parametrize('iou_branch,attach', [(True, True), (True, False), (False, True)],
                         ids=['iou-attached', 'iou-detached', 'plain'])
@pytest.mark.parametrize('case', [S.SMALL, S.MAIN], ids=['small', 'main'])
def test_loss_and_gradients_against_fp64(case, iou_branch, attach):
    sizes, gb, gl, outs = S.case_inputs(case)
    lab, tgt = S.np_targets(sizes, gb, gl)
    assert S.edge_ties(sizes, lab, tgt, outs[1]) == 0
    S.check_conditions(sizes, gb, gl, 50 if case is S.MAIN else 0)
    v64, g64 = _route('fp64', iou_branch, outs, gb, gl, attach)
    v32, g32 = _route('torch', iou_branch, outs, gb, gl, attach)
    vf, gf = _route('fused', iou_branch, outs, gb, gl, attach)
    head = '%s/%s/%s' % (case[0], 'iou' if iou_branch else 'plain', 'attached' if attach else 'detached')
    for k in v64:
        _judge('%s %s' % (head, k), vf[k], v32[k], v64[k], abs(v64[k]))
    for w in g64:
        for kind in g64[w]:
            for l in range(len(sizes)):
                ref = g64[w][kind][l]
                _judge('%s d %s / d %s[%d]' % (head, w, kind, l), gf[w][kind][l], g32[w][kind][l], ref,
                       float(np.abs(ref).max()))
    if iou_branch:
        reach = max(float(np.abs(x).max()) for x in gf['loss_iou']['reg'])
        assert (reach > 0) == attach, 'loss_iou -> bbox_pred: %g with attach_iou_target = %s' % (reach, attach)


# ------------------------------------------------------------------ 3. no positives
def _nopos_gts():
    """the `nopos` gts of fcos_train.npz (make_golden_fcos.gen_train): between the points of every level"""
    return [np.array([[0.5, 0.5, 3.0, 3.0]], np.float32)] * 2, [np.array([3], np.int64)] * 2


@pytest.mark.parametrize('iou_branch', [True, False])
@pytest.mark.parametrize('mixed', [False, True])
def test_no_positives(iou_branch, mixed):
    sizes, gb1, gl1, outs = S.case_inputs(S.SMALL)
    gb, gl = _nopos_gts()
    if mixed:                                      # one image with positives next to one without
        gb, gl = [gb1[0], gb[1]], [gl1[0], gl[1]]
    lab, _ = S.np_targets(sizes, gb, gl)
    npos = [int(sum((a[b] > 0).sum() for a in lab)) for b in range(2)]
    assert npos[1] == 0 and (npos[0] > 0) == mixed
    v64, g64 = _route('fp64', iou_branch, outs, gb, gl)
    v32, g32 = _route('torch', iou_branch, outs, gb, gl)
    vf, gf = _route('fused', iou_branch, outs, gb, gl)
    tag = 'nopos%s/%s' % ('+pos' if mixed else '', 'iou' if iou_branch else 'plain')
    _judge('%s loss_cls' % tag, vf['loss_cls'], v32['loss_cls'], v64['loss_cls'], abs(v64['loss_cls']))
    for l in range(len(sizes)):
        ref = g64['sum']['cls'][l]
        _judge('%s d sum / d cls[%d]' % (tag, l), gf['sum']['cls'][l], g32['sum']['cls'][l], ref,
               float(np.abs(ref).max()))
    if not mixed:
        # the yardstick's loss_cls is the sum over (0 + B): the focal sum divided by B
        for k in list(vf)[1:]:
            assert vf[k] == 0.0 and v64[k] == 0.0, (k, vf[k])
        for w in gf:
            for kind in KINDS[1:4 if iou_branch else 3]:
                assert all(not np.any(x) for x in gf[w][kind]), (w, kind)
    else:
        for k in list(vf)[1:]:
            _judge('%s %s' % (tag, k), vf[k], v32[k], v64[k], abs(v64[k]))
        for kind in KINDS[1:4 if iou_branch else 3]:
            for l in range(len(sizes)):
                ref = g64['sum'][kind][l]
                assert not np.any(gf['sum'][kind][l][1])              # the image without positives
                _judge('%s d sum / d %s[%d]' % (tag, kind, l), gf['sum'][kind][l], g32['sum'][kind][l], ref,
                       float(np.abs(ref).max()))


# ------------------------------------------------------------------ 4. reference fixture
@pytest.mark.parametrize('tag', ['iou', 'plain'])
def test_loss_against_the_reference_fixture(tag):
    g = np.load(os.path.join(GOLD, 'fcos_loss.npz'))
    for k, case in enumerate((S.SMALL, S.MAIN1)):
        sizes, gb, gl, outs = S.case_inputs(case)
        vf, gf = _route('fused', tag == 'iou', outs, gb, gl, gamma=float(g['gamma']), alpha=float(g['alpha']))
        ref = g['loss_%s_%d' % (tag, k)]
        for key, r in zip(KEYS, ref):
            print('fixture %s case %d %s: %.7g (reference %.7g)' % (tag, k, key, vf[key], r))
            assert abs(vf[key] - r) <= TOL * max(1.0, abs(r)), (tag, k, key, vf[key], r)
        for kind in KINDS[:len(ref)]:
            for l in range(len(sizes)):
                idx = g['g_%s_%d_%s_%d_idx' % (tag, k, kind, l)]
                r = g['g_%s_%d_%s_%d' % (tag, k, kind, l)].astype(np.float64)
                got = gf['sum'][kind][l].reshape(-1)[idx]
                scale = float(np.abs(r).max())
                if scale == 0.0:
                    assert not np.any(got)
                else:
                    err = float(np.abs(got - r).max()) / scale
                    assert err <= 2e-4, (tag, k, kind, l, err)


# ------------------------------------------------------------------ 5. the head
def _head_run(head, feats, gb, gl, gamma=2.0, channels_last=False):
    """loss() of a head on features -> (loss dict, {parameter name: gradient of the sum})"""
    outs = head(feats)
    if channels_last:
        outs = tuple([t.contiguous(memory_format=torch.channels_last) for t in m] for m in outs)
    losses = S.head_loss(head, outs, gb, gl, gamma)
    names = [n for n, p in head.named_parameters()]
    gs = torch.autograd.grad(sum(v.sum() for v in losses.values()), [p for _, p in head.named_parameters()],
                             allow_unused=True)
    return losses, {n: (None if g is None else g.detach().double().cpu().numpy()) for n, g in zip(names, gs)}


@pytest.mark.parametrize('iou_branch', [True, False])
def test_head_loss_fused_against_torch_route(iou_branch, monkeypatch):
    from iouaware import fcos_ops
    sizes, gb, gl, _ = S.case_inputs(S.SMALL)
    torch.manual_seed(5)
    head = S.make_head(iou_branch, True)
    for p in head.parameters():
        if p.dim() == 4:
            torch.nn.init.normal_(p, std=0.05)
    rs = np.random.RandomState(6)
    feats_np = [rs.standard_normal((2, 32, h, w)).astype(np.float32) for (h, w) in sizes]
    # yardstick: the same module in fp64 on the CPU, torch route with the one-hot focal formula
    import copy
    h64 = copy.deepcopy(head).double()
    h64.fuse_loss = False
    with S.torch_route(cpu_focal=True):
        l64, p64 = _head_run(h64, [torch.from_numpy(f).double() for f in feats_np],
                             [torch.from_numpy(b).double() for b in gb], [torch.from_numpy(x) for x in gl])
    head = head.to(DEV)
    feats, dgb, dgl = _dev(feats_np), _dev(gb), _dev(gl)
    calls = {'nonzero': 0, 'fused': 0}
    real_nonzero, real_fused = torch.Tensor.nonzero, fcos_ops.point_head_loss

    def counting_nonzero(self, *a, **k):
        calls['nonzero'] += 1
        return real_nonzero(self, *a, **k)

    def counting_fused(*a, **k):
        calls['fused'] += 1
        return real_fused(*a, **k)
    monkeypatch.setattr(torch.Tensor, 'nonzero', counting_nonzero)
    monkeypatch.setattr(fcos_ops, 'point_head_loss', counting_fused)
    head.fuse_loss = True
    lf, pf = _head_run(head, feats, dgb, dgl)
    assert calls == {'nonzero': 0, 'fused': 1}, calls
    head.fuse_loss = False
    lt, pt = _head_run(head, feats, dgb, dgl)
    assert calls['nonzero'] >= 1 and calls['fused'] == 1, calls
    assert list(lf) == list(lt) == list(l64) == list(KEYS[:4 if iou_branch else 3])
    tag = 'head/%s' % ('iou' if iou_branch else 'plain')
    for k in lf:
        assert tuple(lf[k].shape) == tuple(lt[k].shape) == (1,)
        r = float(l64[k].detach().sum())
        _judge('%s %s' % (tag, k), float(lf[k].sum()), float(lt[k].sum()), r, abs(r))
    for n in p64:
        if p64[n] is None:
            assert pf[n] is None or not np.any(pf[n])
            continue
        _judge('%s d sum / d %s' % (tag, n), pf[n], pt[n], p64[n], float(np.abs(p64[n]).max()))
    # what the node does not cover takes the torch route, with the same result as fuse_loss = False
    head.fuse_loss = True
    for kw in (dict(gamma=1.5), dict(channels_last=True)):
        before = dict(calls)
        la, _ = _head_run(head, feats, dgb, dgl, **kw)
        assert calls['fused'] == before['fused'] and calls['nonzero'] > before['nonzero'], (kw, calls)
        head.fuse_loss = False
        lb, _ = _head_run(head, feats, dgb, dgl, **kw)
        head.fuse_loss = True
        for k in la:
            a, b = float(la[k].sum()), float(lb[k].sum())
            assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (kw, k, a, b)


# ------------------------------------------------------------------ 6. return codes
def test_return_codes():
    from iouaware import _lib, fcos_ops
    L = _lib.lib()
    sizes, gb, gl, outs_np = S.case_inputs(S.SMALL)
    geom = _geom(sizes)
    B = 2
    outs = [_dev(m) for m in outs_np]
    dgb, dgl = _dev(gb), _dev(gl)
    lab, tgt, counts = fcos_ops.point_targets(geom, dgb, dgl, S.RANGES)
    gp = (C.c_void_p * B)(*[t.data_ptr() for t in dgb])
    lp = (C.c_void_p * B)(*[t.data_ptr() for t in dgl])
    rr = (C.c_float * 10)(*[float(v) for r in S.RANGES for v in r])
    labels = torch.empty(B * geom.N, dtype=torch.int64, device=DEV)
    bt = torch.empty(B * geom.N * 4, dtype=torch.float32, device=DEV)
    cnt = torch.empty(B, dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def targets(g=geom, ng=(len(gb[0]), len(gb[1])), batch=B, boxes=gp):
        return L.ia_point_targets_ptrs(g.ref(), boxes, lp, (C.c_int32 * len(ng))(*ng), batch, rr, ptr(labels),
                                       ptr(bt), None, ptr(cnt), None)
    bad_levels = _geom(sizes)
    bad_levels.struct.num_levels = 0
    assert targets() == 0
    assert targets(g=bad_levels) == -1
    assert targets(ng=(0, 1)) == -1 and targets(ng=(513, 1)) == -1
    assert targets(batch=0) == -1 and targets(batch=17, ng=(1,) * 17) == -1
    assert targets(boxes=None) == -1
    assert L.ia_point_packed_labels_elems(bad_levels.ref(), B) == 0
    assert L.ia_point_head_loss_workspace_bytes(bad_levels.ref(), B) == 0
    assert L.ia_point_head_loss_workspace_bytes(geom.ref(), 0) == 0

    nbytes = L.ia_point_head_loss_workspace_bytes(geom.ref(), B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    res = torch.full((6,), -7.0, device=DEV)
    gin = torch.ones(4, device=DEV)
    grads = [[torch.full_like(t, -7.0) for t in m] for m in outs]

    def ptrs(maps, iou='all'):
        p = _lib.PointLevelPtrs()
        for l in range(geom.L):
            p.cls[l], p.reg[l], p.ctr[l] = (m[l].data_ptr() for m in maps[:3])
            if iou == 'all' or (iou == 'mixed' and l % 2 == 0):
                p.iou[l] = maps[3][l].data_ptr()
        return p
    pt = _lib.PointTargets()
    for l in range(geom.L):
        pt.labels[l], pt.bbox_targets[l] = lab[l].data_ptr(), tgt[l].data_ptr()

    def fwd(g=geom, p=None, cfg=(2.0, 0.25, 1, 0), w=ws, n=nbytes, t=pt, batch=B):
        p = ptrs(outs) if p is None else p
        return L.ia_point_head_loss_fwd(g.ref(), C.byref(p), batch, C.byref(t), C.byref(_lib.PointLossCfg(*cfg)),
                                        ptr(w) if w is not None else None, n, ptr(res), None)

    def bwd(g=geom, p=None, gr=None, cfg=(2.0, 0.25, 1, 0), batch=B):
        p = ptrs(outs) if p is None else p
        gr = ptrs(grads) if gr is None else gr
        return L.ia_point_head_loss_bwd(g.ref(), C.byref(p), batch, C.byref(pt), C.byref(_lib.PointLossCfg(*cfg)),
                                        ptr(ws), ptr(res), ptr(gin), C.byref(gr), None)
    no_labels = _lib.PointTargets()
    for call in (lambda: fwd(g=bad_levels), lambda: fwd(batch=0), lambda: fwd(p=ptrs(outs, 'mixed')),
                 lambda: fwd(cfg=(1.5, 0.25, 1, 0)), lambda: fwd(w=None), lambda: fwd(t=no_labels),
                 lambda: bwd(g=bad_levels), lambda: bwd(batch=0), lambda: bwd(p=ptrs(outs, 'mixed')),
                 lambda: bwd(gr=ptrs(grads, 'none')), lambda: bwd(gr=ptrs(grads, 'mixed')),
                 lambda: bwd(cfg=(1.5, 0.25, 1, 0))):
        assert call() == -1
    assert fwd(n=nbytes - 1) == -2
    torch.cuda.synchronize()
    # nothing was launched: result and gradient buffers are as they were
    assert bool((res == -7.0).all()) and all(bool((t == -7.0).all()) for m in grads for t in m)
    # and the good calls work, with and without the IoU branch, packing the labels themselves
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    with_pack = res.clone()
    v, _ = _route('fused', True, outs_np, gb, gl)
    assert np.allclose(with_pack[:4].cpu().numpy(), [v[k] for k in KEYS], rtol=1e-6, atol=0)
    assert all(bool((t != -7.0).all()) for m in grads for t in m)
    assert fwd(p=ptrs(outs, 'none')) == 0
    torch.cuda.synchronize()
    assert float(res[3]) == 0.0 and np.allclose(res[:3].cpu().numpy(), with_pack[:3].cpu().numpy(), rtol=1e-6)

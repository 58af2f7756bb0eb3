"""GPU (MI355X): the IoU-balanced losses on the all-levels head-loss node (csrc/headloss.hip, BAL_CLS /
BAL_LOC instances; ops.head_loss(eta=, delta=); IoUawareRetinaHead.fuse_balanced).

Bounds.  Node against the per-level kernels of csrc/loss.hip on the same targets: losses 1e-6, gradients
1e-6 of their scale, as test_all_levels_loss_node_equals_per_level_kernels (both sides fp32 element math on
the hardware transcendentals, fp64 sums).  Node against the reference (tests/golden/losses_balanced.npz):
1e-4 on the losses, 2e-4 of the gradient scale, as test_head_loss_iou_balanced_vs_reference; norm_l against
S1 / (S2 + 1e-6) of the oracle's fp64 sums: 1e-5.  Channels-last against NCHW: 1e-6; bf16 against fp32 on
the bf16-rounded inputs: 1e-6 on the losses and equal bf16 gradients, as
test_all_levels_loss_node_torch_targets_and_bf16."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synth
import gpu_util as G

pytestmark = pytest.mark.gpu

ETA, DELTA, LW_BBOX = 1.5, 1.5, 3.049
KEYS = ('loss_cls', 'loss_bbox', 'losses_iou')
IA_E_ARG = -1


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from iouaware import ops as o
    return o


@pytest.fixture(scope='module')
def fx(golden_dir):
    f = np.load(os.path.join(golden_dir, 'losses_small.npz'))
    ih, iw, ph, pw = [int(v) for v in f['img']]
    B = int(f['batch'])
    cls, reg, iou = synth.head_outputs(int(f['seed']), B, ph, pw, str(f['kind']))
    return f, cls, reg, iou, B, (ph, pw)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def _head(kind='both'):
    """IoUawareRetinaHead with the balanced classification loss, localisation loss, or both"""
    from iouaware.head import IoUawareRetinaHead
    from test_host_targets import HEAD_KW
    kw = dict(HEAD_KW)
    if kind in ('cls', 'both'):
        kw['loss_cls'] = dict(type='IOUbalancedSigmoidFocalLoss', use_sigmoid=True, gamma=2.0,
                              alpha=0.25, eta=ETA, loss_weight=1.0)
    if kind in ('loc', 'both'):
        kw['loss_bbox'] = dict(type='IoUbalancedSmoothL1Loss', beta=0.11, delta=DELTA, loss_weight=LW_BBOX)
    return IoUawareRetinaHead(**kw).cuda()


def _inputs(fx, dtype=torch.float32):
    f, cls, reg, iou, B, (ph, pw) = fx
    ih, iw = int(f['img'][0]), int(f['img'][1])
    metas = [synth.img_meta(ih, iw, ph, pw) for _ in range(B)]
    gts = [torch.from_numpy(f['gt_bboxes_%d' % b]).cuda() for b in range(B)]
    gls = [torch.from_numpy(f['gt_labels_%d' % b]).cuda() for b in range(B)]
    mk = lambda xs: [t.requires_grad_(True) for t in G.to_dev(xs, dtype)]     # noqa: E731
    return metas, gts, gls, mk(cls), mk(reg), mk(iou)


def _weighted_backward(losses):
    """upstream gradients that differ per loss and level"""
    w = torch.arange(1, 16, device='cuda', dtype=torch.float32).reshape(3, 5) * 0.25
    sum(w[k, l] * losses[key][l] for k, key in enumerate(KEYS) for l in range(5)).sum().backward()


def _grads_close(xs, ys, tol=1e-6):
    for l, (x, y) in enumerate(zip(xs, ys)):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert float((x - y).abs().max()) <= tol * max(float(y.abs().max()), 1e-30), l


# ------------------------------------------------------------------ 1: the node is taken
def test_node_taken_only_with_fuse_balanced(ops, fx):
    from test_host_targets import TRAIN_CFG
    for fuse in (True, False):
        head = _head()
        assert head.fuse_balanced is False and type(head).fuse_balanced is False
        head.fuse_balanced = fuse
        metas, gts, gls, c, r, i = _inputs(fx)
        losses = head.loss(c, r, i, gts, gls, metas, TRAIN_CFG)
        for k in KEYS:
            assert isinstance(losses[k], ops.LevelLosses) == fuse, k
            if fuse:
                assert losses[k].total.shape == (1,)
    f = fx[0]
    metas, gts, gls, c, r, i = _inputs(fx)
    geom = head.geometry([tuple(t.shape[-2:]) for t in c], -1)
    t = _fixture_targets(fx, geom)
    out = ops.head_loss(geom, c, r, i, *t, avg_factor=float(f['num_total_pos']), eta=1.5, delta=1.5)
    assert out['loss_cls'].norm.shape == (5,) and all(np.isfinite(float(x.detach())) for k in KEYS for x in out[k])
    plain = ops.head_loss(geom, c, r, i, *t, avg_factor=float(f['num_total_pos']))
    assert plain['loss_cls'].norm is None
    assert all(rel(float(a.detach()), float(b.detach())) < 1e-6 for a, b in zip(out['losses_iou'], plain['losses_iou']))
    # (the balanced class loss VALUE is S0 + S1 * S2 / (S2 + 1e-6), the plain one up to the 1e-6: the IoU
    # weights move its gradient, not its value)
    assert all(rel(float(a), float(b)) < 1e-5 for a, b in zip(out['loss_cls'], plain['loss_cls']))
    assert any(float(a) < float(b) for a, b in zip(out['loss_bbox'], plain['loss_bbox']))     # iou^delta <= 1


def _fixture_targets(fx, geom):
    f, B = fx[0], fx[4]
    out = ([], [], [], [])
    for l, (h, w) in enumerate(geom.featmap_sizes):
        n_l = h * w * synth.A
        out[0].append(torch.from_numpy(f['labels_%d' % l]).cuda().reshape(B, n_l))
        out[1].append(torch.from_numpy(f['label_weights_%d' % l]).cuda().reshape(B, n_l))
        out[2].append(torch.from_numpy(f['bbox_targets_%d' % l]).cuda().reshape(B, n_l, 4))
        out[3].append(torch.from_numpy(f['bbox_weights_%d' % l]).cuda().reshape(B, n_l, 4))
    return out


# ------------------------------------------------------------------ 2: node against the per-level kernels
@pytest.mark.parametrize('attach', [True, False])
@pytest.mark.parametrize('kind', ['cls', 'loc', 'both'])
def test_node_equals_per_level_kernels(ops, fx, kind, attach):
    from test_host_targets import TRAIN_CFG
    outs = []
    for fuse in (True, False):
        head = _head(kind)
        head.fuse_balanced, head.attach_iou_target = fuse, attach
        metas, gts, gls, c, r, i = _inputs(fx)
        losses = head.loss(c, r, i, gts, gls, metas, TRAIN_CFG)
        assert isinstance(losses['loss_cls'], ops.LevelLosses) == fuse
        _weighted_backward(losses)
        outs.append((losses, [t.grad for t in c], [t.grad for t in r], [t.grad for t in i]))
    (la, ca, ra, ia_), (lb, cb, rb, ib) = outs
    for k in la:
        for x, y in zip(la[k], lb[k]):
            assert x.shape == (1,) and rel(float(x), float(y)) < 1e-6, (k, float(x), float(y))
        assert rel(float(la[k].total), sum(float(v) for v in lb[k])) < 1e-6
    _grads_close(ca, cb)
    _grads_close(ra, rb)
    _grads_close(ia_, ib)


# ------------------------------------------------------------------ 3: node against the reference
def test_node_vs_reference_and_norm_vs_oracle(ops, oracle_lib, fx, golden_dir):
    from test_host_targets import TRAIN_CFG
    f, cls, reg, iou, B, (ph, pw) = fx
    fb = np.load(os.path.join(golden_dir, 'losses_balanced.npz'))
    assert float(fb['eta']) == ETA and float(fb['delta']) == DELTA
    head = _head()
    head.fuse_balanced = True
    metas, gts, gls, c, r, i = _inputs(fx)
    losses = head.loss(c, r, i, gts, gls, metas, TRAIN_CFG)
    assert isinstance(losses['loss_cls'], ops.LevelLosses)
    for k in losses:
        got = np.array([float(x) for x in losses[k]])
        assert np.all(np.abs(got - fb[k]) <= 1e-4 * np.maximum(np.abs(fb[k]), 1e-6)), (k, got, fb[k])
    sum(v.total for v in losses.values()).sum().backward()
    for l in range(5):
        for key, g in (('g_cls_%d' % l, c[l].grad), ('g_reg_%d' % l, r[l].grad),
                       ('g_iou_%d' % l, i[l].grad)):
            want = fb[key].astype(np.float64)
            got = g.cpu().numpy().reshape(-1)[fb[key + '_idx']].astype(np.float64)
            assert np.abs(got - want).max() <= 2e-4 * max(np.abs(want).max(), 1e-30), key
    norm = losses['loss_cls'].norm.cpu().numpy()
    base = oracle_lib.head_base_anchors(synth.STRIDES)
    for l in range(5):
        bt, bw = f['bbox_targets_%d' % l].reshape(-1, 4), f['bbox_weights_%d' % l].reshape(-1, 4)
        _, tgt, _, _ = oracle_lib.iou_bce(reg[l], iou[l], bt, bw, base[l], synth.STRIDES[l])
        _, _, sums = oracle_lib.focal_loss_balanced(cls[l], f['labels_%d' % l].reshape(-1),
                                                    f['label_weights_%d' % l].reshape(-1), tgt, synth.A,
                                                    2.0, 0.25, ETA)
        want = sums[1] / (sums[2] + 1e-6)
        assert abs(float(norm[l]) - want) <= 1e-5 * max(abs(want), 1e-30), (l, float(norm[l]), want)


# ------------------------------------------------------------------ 4: channels-last, bf16
def _cl(ts):
    return [t.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in ts]


@pytest.mark.parametrize('fused', [False, True])
def test_channels_last_node_equals_nchw_node(ops, fx, fused):
    """reg / iou as their own channels-last tensors, and (fused) as slices of one 48-channel row whose
    gradient comes back as one tensor with exact zeros in the padding channels (grad_rows_start_at_reg)"""
    from test_host_targets import TRAIN_CFG
    head = _head()
    head.fuse_balanced = True
    metas, gts, gls, c, r, i = _inputs(fx)

    def run(c_, r_, i_):
        losses = head.loss(c_, r_, i_, gts, gls, metas, TRAIN_CFG)
        assert isinstance(losses['loss_cls'], ops.LevelLosses)
        _weighted_backward(losses)
        return losses
    la = run(c, r, i)
    c2 = _cl(c)
    n_reg, n_iou = r[0].shape[1], i[0].shape[1]
    geom = head.geometry([tuple(t.shape[-2:]) for t in c], -1)
    if fused:
        bases = []
        for rr, ii in zip(r, i):
            pad = torch.randn(rr.shape[0], 3, *rr.shape[2:], device='cuda')
            bases.append(torch.cat([rr.detach(), ii.detach(), pad], 1)
                         .contiguous(memory_format=torch.channels_last).requires_grad_(True))
        assert bases[0].shape[1] == 48
        r2 = [b[:, :n_reg] for b in bases]
        i2 = [b[:, n_reg:n_reg + n_iou] for b in bases]
        assert ops._nhwc_route(geom, c2, r2, i2)[0] is not None
    else:
        r2, i2 = _cl(r), _cl(i)
        assert ops._nhwc_route(geom, c2, r2, i2) is not None
    lb = run(c2, r2, i2)
    for k in la:
        for x, y in zip(la[k], lb[k]):
            assert rel(float(x), float(y)) < 1e-6, k
    assert torch.allclose(la['loss_cls'].norm, lb['loss_cls'].norm, rtol=1e-6, atol=0)
    _grads_close([t.grad for t in c2], [t.grad for t in c])
    for l in range(5):
        assert c2[l].grad.is_contiguous(memory_format=torch.channels_last)
        if fused:
            g = bases[l].grad
            assert g.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(g[:, :n_reg], r[l].grad) and torch.equal(g[:, n_reg:n_reg + n_iou], i[l].grad), l
            assert float(g[:, n_reg + n_iou:].abs().max()) == 0.0
        else:
            assert torch.equal(r2[l].grad, r[l].grad) and torch.equal(i2[l].grad, i[l].grad), l


def test_bf16_node_equals_fp32_node_on_rounded_inputs(ops, fx):
    f = fx[0]
    head = _head()
    _, _, _, cb, rb, ib = _inputs(fx, torch.bfloat16)
    geom = head.geometry([tuple(t.shape[-2:]) for t in cb], -1)
    t = _fixture_targets(fx, geom)
    avg = float(f['num_total_pos'])
    cf, rf, if_ = [[x.detach().float().requires_grad_(True) for x in xs] for xs in (cb, rb, ib)]
    kw = dict(avg_factor=avg, eta=ETA, delta=DELTA, loss_weight_bbox=LW_BBOX)
    a = ops.head_loss(geom, cb, rb, ib, *t, **kw)
    b = ops.head_loss(geom, cf, rf, if_, *t, **kw)
    sum(v.total for v in a.values()).sum().backward()
    sum(v.total for v in b.values()).sum().backward()
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert rel(float(x), float(y)) < 1e-6          # same (bf16-exact) inputs
    for xs, ys in ((cb, cf), (rb, rf), (ib, if_)):
        for x, y in zip(xs, ys):
            assert x.grad.dtype == torch.bfloat16
            assert torch.equal(x.grad, y.grad.to(torch.bfloat16))


# ------------------------------------------------------------------ 5: small hand-made case
class _Small:
    """synth.level_shapes(64, 96): 96, 24, 6, 2, 1 positions (the vector path on the first two levels, the
    scalar path on the rest), B = 2.  Every level's class range is split into chunks of CCHUNK = 8 classes
    (fill_levels: 9 wavefronts per image and level, far below its target), and the positives carry the labels
    1, CCHUNK, CCHUNK + 1 and C; level 4 has no positive.  DISJOINT (image, level, position, anchor), a
    positive of level 0, is predicted ten anchor widths to the right of its target: IoU 0.  The logit of BIG, a
    positive of level 2, is 65 (> 60)."""
    CCHUNK = 8

    def __init__(self, ops):
        self.sizes = sizes = synth.level_shapes(64, 96)
        assert [h * w for h, w in sizes] == [96, 24, 6, 2, 1]
        self.B = B = 2
        A, Cn = synth.A, synth.C
        self.geom = ops.HeadGeometry(sizes, synth.STRIDES, G.product_base_anchors(), Cn, softmax=False,
                                     iou_branch=True)
        rs = np.random.RandomState(11)
        self.cls = [(rs.standard_normal((B, A * Cn, h, w)) * 2 - 3).astype(np.float32) for h, w in sizes]
        self.reg = [(rs.standard_normal((B, A * 4, h, w)) * 0.2).astype(np.float32) for h, w in sizes]
        self.iou = [rs.standard_normal((B, A, h, w)).astype(np.float32) for h, w in sizes]
        lab = [np.zeros((B, h * w, A), np.int64) for h, w in sizes]
        lw = [np.ones((B, h * w, A), np.float32) for h, w in sizes]
        picks = (1, self.CCHUNK, self.CCHUNK + 1, Cn)
        self.pos = []                       # (image, level, position, anchor, label)
        k = 0
        for l, (h, w) in enumerate(sizes[:4]):
            for b in range(B):
                for p in sorted(set([0, (h * w) // 2, h * w - 1, 5 % (h * w)])):
                    for an in ((2 + k) % A, (7 + k) % A):
                        if lab[l][b, p, an] == 0:
                            lab[l][b, p, an] = picks[k % 4]
                            self.pos.append((b, l, p, an, picks[k % 4]))
                            k += 1
        self.DISJOINT = [q[:4] for q in self.pos if q[1] == 0][3]
        self.BIG = [q[:4] for q in self.pos if q[1] == 2][2]
        assert set(q[4] for q in self.pos if q[1] == 0) == set(picks)      # level 0: every chunk edge
        lw[0][1, 7, :] = 0.0                # an ignored position
        self.bt = [np.zeros((B, h * w, A, 4), np.float32) for h, w in sizes]
        self.bw = [np.zeros((B, h * w, A, 4), np.float32) for h, w in sizes]
        for (b, l, p, an, _) in self.pos:
            self.bt[l][b, p, an] = rs.standard_normal(4) * 0.1
            self.bw[l][b, p, an] = 1.0
        b, l, p, an = self.DISJOINT
        h, w = sizes[l]
        self.bt[l][b, p, an] = 0.0
        self.reg[l][b, an * 4:an * 4 + 4, p // w, p % w] = (10.0, 0.0, 0.0, 0.0)   # dx = 10 widths (stds = 1)
        b, l, p, an = self.BIG
        h, w = sizes[l]
        assert lab[l][b, p, an] > 0
        self.cls[l][b, an * Cn + lab[l][b, p, an] - 1, p // w, p % w] = 65.0
        dev = lambda xs, shp: [torch.from_numpy(x.reshape(B, -1, *shp)).cuda() for x in xs]   # noqa: E731
        self.lab = lab
        self.targets = (dev(lab, ()), dev(lw, ()), dev(self.bt, (4,)), dev(self.bw, (4,)))
        self.avg = 7.0

    def maps(self):
        return [[t.requires_grad_(True) for t in G.to_dev(xs)] for xs in (self.cls, self.reg, self.iou)]

    def per_level(self, ops, c, r, i, attach):
        """the per-level route of IoUawareRetinaHead.loss_single on these targets"""
        labels, lw, bt, bw = self.targets
        out = {k: [] for k in KEYS}
        ious = []
        for l in range(5):
            li, t = ops.iou_bce_sum(r[l], i[l], bt[l], bw[l], self.geom, l, attach, return_iou=True)
            ious.append(t)
            out['losses_iou'].append(li * (1.0 / self.avg))
            out['loss_bbox'].append(ops.smooth_l1_balanced_sum(r[l], bt[l], bw[l], t, synth.A, 0.11, DELTA)
                                    * (LW_BBOX / self.avg))
            out['loss_cls'].append(ops.focal_loss_balanced_sum(c[l], labels[l], lw[l], t, synth.A, 2.0, 0.25,
                                                               ETA) * (1.0 / self.avg))
        return out, ious


@pytest.mark.parametrize('channels_last', [False, True])
def test_small_hand_made_case(ops, channels_last):
    s = _Small(ops)
    A, Cn = synth.A, synth.C
    c, r, i = s.maps()
    want, ious = s.per_level(ops, c, r, i, True)
    _weighted_backward(want)
    c2, r2, i2 = s.maps()
    if channels_last:
        c2, r2, i2 = _cl(c2), _cl(r2), _cl(i2)
    got = ops.head_loss(s.geom, c2, r2, i2, *s.targets, avg_factor=s.avg, loss_weight_bbox=LW_BBOX,
                        attach_iou_target=True, exact_large_logits=True, eta=ETA, delta=DELTA,
                        channels_last=channels_last)
    _weighted_backward(got)
    for k in KEYS:
        for l in range(5):
            x, y = float(got[k][l]), float(want[k][l])
            assert np.isfinite(x) and rel(x, y) < 1e-6, (k, l, x, y)
    for xs, ys in ((c2, c), (r2, r), (i2, i)):
        for x in xs:
            assert bool(torch.isfinite(x.grad).all())
        _grads_close([x.grad for x in xs], [y.grad for y in ys])
    # a level without positives: norm 0, a finite loss, and the level's labels are all 0
    norm = got['loss_cls'].norm.cpu().numpy()
    assert int(s.lab[4].max()) == 0 and float(norm[4]) == 0.0 and float(got['loss_cls'][4]) > 0
    assert all(np.isfinite(norm[l]) and float(norm[l]) > 0.0 for l in range(4))
    # the disjoint positive: IoU target exactly 0, and from the balanced factors its class gradient and
    # the gradient of its four deltas are exactly 0 (the attached IoU target adds +-0 there: no overlap)
    b, l, p, an = s.DISJOINT
    h, w = s.sizes[l]
    assert float(ious[l].reshape(s.B, h * w, A)[b, p, an]) == 0.0
    lab = int(s.lab[l][b, p, an])
    assert float(c2[l].grad[b, an * Cn + lab - 1, p // w, p % w]) == 0.0
    assert bool((r2[l].grad[b, an * 4:an * 4 + 4, p // w, p % w] == 0.0).all())
    # ... while its neighbours in the class row keep their negative-form gradient
    assert float(c2[l].grad[b, an * Cn + lab % Cn, p // w, p % w]) != 0.0


# ------------------------------------------------------------------ 6: return codes
class _Abi:
    """the four C entries on one small level set (B = 1, five live positive anchors on level 0), valid
    device buffers throughout; the same values in both layouts"""

    def __init__(self):
        from iouaware import _lib, ops
        self._lib, self.ops, self.lib = _lib, ops, _lib.lib()
        self.sizes = sizes = synth.level_shapes(64, 96)
        self.B, self.A, self.Cn, self.L = 1, synth.A, synth.C, len(sizes)
        B, A, Cn, L = self.B, self.A, self.Cn, self.L
        base = G.product_base_anchors()
        self.geoms = {ib: ops.HeadGeometry(sizes, synth.STRIDES, base, Cn, softmax=False, iou_branch=ib)
                      for ib in (False, True)}
        gen = torch.Generator(device='cuda').manual_seed(5)
        rnd = lambda ch, sc: [torch.randn(B, h, w, ch, device='cuda', generator=gen) * sc   # noqa: E731
                              for h, w in sizes]                   # (B, H, W, ch): pixel rows
        self.nhwc = (rnd(A * Cn, 1.0), rnd(A * 4, 0.2), rnd(A, 1.0))
        self.nchw = [[t.permute(0, 3, 1, 2).contiguous() for t in ts] for ts in self.nhwc]
        n = lambda h, w: h * w * A                                 # noqa: E731
        self.t = ([torch.zeros(B, n(h, w), dtype=torch.int64, device='cuda') for h, w in sizes],
                  [torch.ones(B, n(h, w), device='cuda') for h, w in sizes],
                  [torch.zeros(B, n(h, w), 4, device='cuda') for h, w in sizes],
                  [torch.zeros(B, n(h, w), 4, device='cuda') for h, w in sizes])
        self.t[0][0][0, :5] = torch.tensor([1, 8, 9, 80, 40], device='cuda')
        self.t[3][0][0, :5] = 1.0
        self.t[2][0][0, :5] = 0.3
        self.ht = _lib.HeadTargets()
        for l in range(L):
            self.ht.labels[l], self.ht.label_weights[l] = self.t[0][l].data_ptr(), self.t[1][l].data_ptr()
            self.ht.bbox_targets[l], self.ht.bbox_weights[l] = self.t[2][l].data_ptr(), self.t[3][l].data_ptr()
        self.ht.avg_factor = 1.0
        self.gin = torch.arange(1, 3 * L + 4, device='cuda', dtype=torch.float32) * 0.25
        bal = self.cfg(1, 1)
        self.nbytes = {
            'plain': self.lib.ia_head_loss_workspace_bytes(self.geoms[True].ref(), B),
            'bal': self.lib.ia_head_loss_workspace_bytes_cfg(self.geoms[True].ref(), B, C.byref(bal))}
        self.ws = torch.zeros(self.nbytes['bal'], dtype=torch.uint8, device='cuda')
        self.res = torch.zeros(4 * L + 4, device='cuda')
        self.grads = None

    def cfg(self, bal_cls, bal_loc, eta=ETA, delta=DELTA):
        return self._lib.HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, 0, eta, delta, bal_cls, bal_loc)

    def _ptrs(self, maps, with_iou, nhwc):
        p, st = self._lib.LevelPtrs(), self._lib.LevelPixStrides()
        for l in range(self.L):
            p.cls[l], p.reg[l] = maps[0][l].data_ptr(), maps[1][l].data_ptr()
            p.iou[l] = maps[2][l].data_ptr() if with_iou else None
            if nhwc:
                st.cls[l], st.reg[l], st.iou[l] = (maps[k][l].shape[-1] for k in range(3))
        return p, st

    def new_grads(self, nhwc, fill):
        self.grads = [[torch.full_like(t, fill) for t in ts] for ts in (self.nhwc if nhwc else self.nchw)]
        return self.grads

    def call(self, entry, hc, with_iou=True, nbytes=None, fill=7.25):
        """entry: fwd | bwd | fwd_nhwc | bwd_nhwc -> return code (bwd: fresh gradient maps in self.grads)"""
        nhwc = entry.endswith('nhwc')
        g = self.geoms[with_iou].ref()
        p, st = self._ptrs(self.nhwc if nhwc else self.nchw, with_iou, nhwc)
        nbytes = self.nbytes['bal'] if nbytes is None else nbytes
        ptr, s = self.ops._ptr, self.ops._stream()
        if entry == 'fwd':
            return self.lib.ia_head_loss_fwd(g, C.byref(p), self._lib.IA_F32, self.B, C.byref(self.ht),
                                             C.byref(hc), ptr(self.ws), nbytes, ptr(self.res), s)
        if entry == 'fwd_nhwc':
            return self.lib.ia_head_loss_fwd_nhwc(g, C.byref(p), C.byref(st), self.B, C.byref(self.ht),
                                                  C.byref(hc), ptr(self.ws), nbytes, ptr(self.res), s)
        gp, gst = self._ptrs(self.new_grads(nhwc, fill), with_iou, nhwc)
        if entry == 'bwd':
            return self.lib.ia_head_loss_bwd(g, C.byref(p), self._lib.IA_F32, self.B, C.byref(self.ht),
                                             C.byref(hc), ptr(self.ws), ptr(self.res), ptr(self.gin),
                                             C.byref(gp), s)
        return self.lib.ia_head_loss_bwd_nhwc(g, C.byref(p), C.byref(st), self.B, C.byref(self.ht),
                                              C.byref(hc), ptr(self.res), ptr(self.gin), C.byref(gp),
                                              C.byref(gst), s)


ENTRIES = ('fwd', 'bwd', 'fwd_nhwc', 'bwd_nhwc')


@pytest.mark.parametrize('entry', ENTRIES)
def test_refusals_are_ia_e_arg_and_touch_nothing(entry):
    s = _Abi()
    fwd = 'fwd_nhwc' if entry.endswith('nhwc') else 'fwd'
    assert s.call(fwd, s.cfg(1, 1)) == 0                 # a valid balanced forward call first
    torch.cuda.synchronize()
    assert float(s.res[3 * s.L + 4]) > 0.0               # norm of level 0, behind the plain result
    bad = [
        (s.cfg(1, 0), False), (s.cfg(0, 1), False), (s.cfg(1, 1), False),        # no IoU branch
        (s.cfg(1, 0, eta=0.0), True), (s.cfg(1, 1, eta=-1.0), True),
        (s.cfg(0, 1, delta=0.0), True), (s.cfg(1, 1, delta=-0.5), True),
        (s.cfg(1, 1, eta=float('nan')), True), (s.cfg(1, 1, delta=float('nan')), True)]
    sizes = [None] * len(bad)
    if entry == 'fwd':                                   # a workspace sized for the plain loss
        assert s.nbytes['bal'] == s.nbytes['plain'] + 8 * 2 * s.L * s._lib.IA_LOSS_SLOTS
        bad += [(s.cfg(1, 1), True), (s.cfg(1, 0), True)]
        sizes += [s.nbytes['plain'], s.nbytes['bal'] - 1]
    elif entry == 'fwd_nhwc':
        bad += [(s.cfg(1, 1), True), (s.cfg(1, 0), True)]
        sizes += [8 * 3 * s.L * s._lib.IA_LOSS_SLOTS, 8 * 5 * s.L * s._lib.IA_LOSS_SLOTS - 1]
    for (hc, with_iou), nbytes in zip(bad, sizes):
        s.ws.fill_(0xA5)
        res = s.res.clone()
        rc = s.call(entry, hc, with_iou=with_iou, nbytes=nbytes)
        torch.cuda.synchronize()
        assert rc == IA_E_ARG, (hc.eta, hc.delta, hc.balanced_cls, hc.balanced_loc, with_iou, nbytes)
        assert bool((s.ws == 0xA5).all()) and torch.equal(s.res.view(torch.int32), res.view(torch.int32))
        if s.grads is not None:
            assert all(bool((t == 7.25).all()) for ts in s.grads for t in ts)
    if entry.startswith('fwd'):                          # loc alone needs no more than the plain size
        plain = s.nbytes['plain'] if entry == 'fwd' else 8 * 3 * s.L * s._lib.IA_LOSS_SLOTS
        assert s.call(entry, s.cfg(0, 1), nbytes=plain) == 0
        torch.cuda.synchronize()


@pytest.mark.parametrize('nhwc', [False, True])
def test_flags_zero_give_the_bits_of_the_old_struct_values(nhwc):
    """both flags 0 (whatever eta / delta hold): result and gradients carry the bits of a call with the eight
    old fields alone; and the 8-positional construction still works"""
    s = _Abi()
    fwd, bwd = ('fwd_nhwc', 'bwd_nhwc') if nhwc else ('fwd', 'bwd')
    outs = []
    for hc in (s._lib.HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, 0), s.cfg(0, 0, eta=1.5, delta=2.5)):
        s.res.fill_(-3.0)
        assert s.call(fwd, hc, nbytes=s.nbytes['plain']) == 0
        assert s.call(bwd, hc) == 0
        torch.cuda.synchronize()
        assert bool((s.res[3 * s.L + 4:] == -3.0).all())          # the plain result is 3L + 4 floats
        outs.append((s.res.clone(), s.grads))
    (ra, ga), (rb, gb) = outs
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert float(ra[0]) > 0 and float(ga[1][0].abs().max()) > 0
    for xs, ys in zip(ga, gb):
        for x, y in zip(xs, ys):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))

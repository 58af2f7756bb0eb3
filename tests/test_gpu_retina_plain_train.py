"""GPU: training plain RetinaNet (RetinaHead) on the fused routes -- the all-levels head loss
without the IoU term (csrc/headloss.hip, IA_CLS_SIGMOID_NOIOU: k_box_ml / k_box_nhwc IOU = false)
against the per-level kernels, the oracle at full size, the channels-last route, bf16, and the
reference's RetinaHead.loss (tests/golden/retina_plain_train.npz, written by
tests/golden/make_golden_retina_plain_train.py); the argument checks of the four entries; and the
Winograd training head for a head without `retina_iou` against the module path.  Tolerances are
those of the same comparisons on the IoU-aware head (tests/test_gpu_losses.py,
tests/test_gpu_winograd_train.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import synth
import gpu_util as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
IA_E_ARG = -1                        # include/iouaware.h
KEYS = ('loss_cls', 'loss_bbox')


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def _head(**kw):
    from iouaware.head import RetinaHead
    from test_host_targets import HEAD_KW
    return RetinaHead(**dict(HEAD_KW, **kw)).cuda()


def _case(k, dtype=torch.float32):
    """fixture case k -> (fixture, head, metas, gt boxes, gt labels, cls leaves, reg leaves)"""
    f = np.load(os.path.join(GOLD, 'retina_plain_train.npz'))
    seed, B, ph, pw, ih, iw = [int(v) for v in f['case_%d' % k]]
    cls, reg, _ = synth.head_outputs(seed, B, ph, pw, 'A')
    metas = [synth.img_meta(ih, iw, ph, pw) for _ in range(B)]
    gts = [torch.from_numpy(f['gt_bboxes_%d_%d' % (k, b)]).cuda() for b in range(B)]
    gls = [torch.from_numpy(f['gt_labels_%d_%d' % (k, b)]).cuda() for b in range(B)]
    mk = lambda xs: [t.requires_grad_(True) for t in G.to_dev(xs, dtype)]     # noqa: E731
    return f, _head(), metas, gts, gls, mk(cls), mk(reg)


def _weighted(losses):
    """upstream gradients that differ per loss and level"""
    w = torch.arange(1, 11, device='cuda', dtype=torch.float32).reshape(2, 5) * 0.25
    return sum(w[k, l] * losses[key][l] for k, key in enumerate(KEYS) for l in range(5)).sum()


def _close(x, y, tol=1e-6):
    return x.shape == y.shape and float((x - y).abs().max()) <= tol * max(float(y.abs().max()), 1e-30)


# ------------------------------------------------------------------ 6: fused node == per-level kernels
def test_plain_loss_node_equals_per_level_kernels():
    from iouaware import ops
    from test_host_targets import TRAIN_CFG
    outs = []
    for fuse in (True, False):
        _, head, metas, gts, gls, c, r = _case(0)
        head.fuse_levels = fuse
        losses = head.loss(c, r, gts, gls, metas, TRAIN_CFG)
        assert sorted(losses) == ['loss_bbox', 'loss_cls']           # no 'losses_iou'
        for k in KEYS:
            assert isinstance(losses[k], ops.LevelLosses) == fuse and len(losses[k]) == 5
        _weighted(losses).backward()
        outs.append((losses, [t.grad for t in c], [t.grad for t in r]))
    (la, ca, ra), (lb, cb, rb) = outs
    for k in KEYS:
        for x, y in zip(la[k], lb[k]):
            print(k, float(x), float(y))
            assert x.shape == (1,) and rel(float(x), float(y)) < 1e-6, k
        assert rel(float(la[k].total), sum(float(v) for v in lb[k])) < 1e-6
    assert sum(float(v) > 0 for v in la['loss_bbox']) >= 3
    for name, xs, ys in (('cls', ca, cb), ('reg', ra, rb)):
        for l, (x, y) in enumerate(zip(xs, ys)):
            assert _close(x, y) and x.dtype == y.dtype, (name, l)


# ------------------------------------------------------------------ 7: full size against the oracle
def _random_targets(geom, B, seed=5):
    rs = np.random.RandomState(seed)
    labels, lw, bt, bw = [], [], [], []
    for (h, w) in geom.featmap_sizes:
        n = h * w * synth.A
        lab = np.zeros((B, n), np.int64)
        pos = rs.rand(B, n) < 0.004
        lab[pos] = rs.randint(1, 81, int(pos.sum()))
        wgt = (rs.rand(B, n) > 0.05).astype(np.float32)          # 5 % ignored
        labels.append(lab); lw.append(wgt)
        bt.append((rs.standard_normal((B, n, 4)) * 0.2 * pos[..., None]).astype(np.float32))
        bw.append(np.repeat(pos[..., None].astype(np.float32), 4, -1))
    return labels, lw, bt, bw


@pytest.mark.parametrize('nhwc', [False, True])
def test_plain_loss_full_size_vs_oracle(oracle_lib, nhwc):
    """800x1344, batch 2: per-level sums and gradients against the oracle's focal / smooth-L1; the
    box gradient is the smooth-L1 gradient alone"""
    from iouaware import ops
    ph, pw, B = 800, 1344, 2
    head = _head()
    geom = head.geometry(synth.level_shapes(ph, pw), -1)
    cls, reg, _ = synth.head_outputs(31, B, ph, pw, 'A')
    labels, lw, bt, bw = _random_targets(geom, B)
    dev = lambda xs: [torch.from_numpy(x).cuda() for x in xs]    # noqa: E731
    c = [t.requires_grad_(True) for t in G.to_dev(cls)]
    r = [t.requires_grad_(True) for t in G.to_dev(reg)]
    if nhwc:
        c, r = _cl(c), _cl(r)
    avg = 37.0
    out = ops.head_loss(geom, c, r, None, dev(labels), dev(lw), dev(bt), dev(bw), avg_factor=avg,
                        channels_last=nhwc)
    assert sorted(out) == ['loss_bbox', 'loss_cls']
    sum(v.total for v in out.values()).sum().backward()
    for l in range(geom.L):
        so, go = oracle_lib.focal_loss(cls[l], labels[l], lw[l], synth.A, 2.0, 0.25,
                                       gscale=1.0 / avg)
        s1, g1 = oracle_lib.smooth_l1(reg[l], bt[l], bw[l], synth.A, 0.11, gscale=1.0 / avg)
        print(l, float(out['loss_cls'][l]), so / avg, float(out['loss_bbox'][l]), s1 / avg)
        assert rel(float(out['loss_cls'][l]), so / avg) < 1e-5, l
        g = c[l].grad.cpu().numpy()
        assert np.abs(g - go).max() <= 1e-5 * np.abs(go).max(), l
        assert rel(float(out['loss_bbox'][l]), s1 / avg) < 1e-5, l
        gr = r[l].grad.cpu().numpy()
        assert np.abs(gr - g1).max() <= 1e-6 * max(np.abs(g1).max(), 1e-30), l


# ------------------------------------------------------------------ 8: channels-last route
def _cl(ts):
    return [t.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in ts]


@pytest.mark.parametrize('pad', [None, 4, 68])
def test_plain_channels_last_route_equals_nchw_route(pad):
    """pad None: reg is its own channels-last tensor.  pad 4 / 68: reg is the leading slice of a
    wider tensor with random values behind it; the gradient arrives as ONE tensor of the wider
    shape with exact zeros in the padding (written by the kernel up to 64 channels, by a host fill
    beyond)."""
    from iouaware import ops
    from test_host_targets import TRAIN_CFG
    _, head, metas, gts, gls, c, r = _case(0)
    la = head.loss(c, r, gts, gls, metas, TRAIN_CFG)               # NCHW route
    _weighted(la).backward()
    c2 = _cl(c)
    n_reg = r[0].shape[1]
    geom = head.geometry([tuple(t.shape[-2:]) for t in c], -1)
    if pad is None:
        r2 = _cl(r)
        assert ops._nhwc_route(geom, c2, r2, None)[0] is None
    else:
        bases = [torch.cat([rr.detach(), torch.randn(rr.shape[0], pad, *rr.shape[2:], device='cuda')], 1)
                 .contiguous(memory_format=torch.channels_last).requires_grad_(True) for rr in r]
        r2 = [b[:, :n_reg] for b in bases]
        assert ops._nhwc_route(geom, c2, r2, None)[0] is not None
    lb = head.loss(c2, r2, gts, gls, metas, TRAIN_CFG)
    assert sorted(lb) == ['loss_bbox', 'loss_cls'] and isinstance(lb['loss_cls'], ops.LevelLosses)
    _weighted(lb).backward()
    for k in KEYS:
        for x, y in zip(la[k], lb[k]):
            assert rel(float(x), float(y)) < 1e-6, k
    for l in range(5):
        assert _close(c2[l].grad, c[l].grad), l
        assert c2[l].grad.is_contiguous(memory_format=torch.channels_last)
        if pad is None:
            assert _close(r2[l].grad, r[l].grad), l
        else:
            g = bases[l].grad
            assert g.shape == bases[l].shape and g.is_contiguous(memory_format=torch.channels_last)
            assert _close(g[:, :n_reg], r[l].grad), l
            assert float(g[:, n_reg:].abs().max()) == 0.0


# ------------------------------------------------------------------ 9: bf16 head outputs
def test_plain_loss_node_bf16_and_host_normaliser():
    from iouaware import ops
    from iouaware.targets import anchor_target
    from test_host_targets import TRAIN_CFG
    f, head, metas, gts, gls, c, r = _case(0)
    sizes = [tuple(t.shape[-2:]) for t in c]
    anchors, flags = head.get_anchors(sizes, metas, device='cuda')
    t = anchor_target(anchors, flags, gts, metas, head.target_means, head.target_stds, TRAIN_CFG,
                      gt_labels_list=gls, label_channels=80, sampling=False)
    geom = head.geometry(sizes, -1)
    out = ops.head_loss(geom, c, r, None, t[0], t[1], t[2], t[3], avg_factor=t[4])
    out2 = ops.head_loss(geom, c, r, None, t[0], t[1], t[2], t[3],
                         avg_factor=torch.tensor([float(t[4])], device='cuda'))
    assert all(float(a) == float(b) for k in out for a, b in zip(out[k], out2[k]))
    _, _, _, _, _, cb, rb = _case(0, torch.bfloat16)
    cf = [x.detach().float().requires_grad_(True) for x in cb]
    rf = [x.detach().float().requires_grad_(True) for x in rb]
    a = ops.head_loss(geom, cb, rb, None, t[0], t[1], t[2], t[3], avg_factor=t[4])
    b = ops.head_loss(geom, cf, rf, None, t[0], t[1], t[2], t[3], avg_factor=t[4])
    sum(v.total for v in a.values()).sum().backward()
    sum(v.total for v in b.values()).sum().backward()
    for k in KEYS:
        for x, y in zip(a[k], b[k]):
            assert rel(float(x), float(y)) < 1e-6          # same (bf16-exact) inputs
    for xs, ys in ((cb, cf), (rb, rf)):
        for x, y in zip(xs, ys):
            assert x.grad.dtype == torch.bfloat16
            assert torch.equal(x.grad, y.grad.to(torch.bfloat16))


# ------------------------------------------------------------------ 10: the reference fixture
@pytest.mark.parametrize('device_targets', [True, False])
@pytest.mark.parametrize('case', [0, 1])
def test_plain_head_loss_against_reference_fixture(case, device_targets):
    """RetinaHead.loss on the fixture inputs, targets from the HIP assigner and from the torch
    path: per-level losses 1e-4 relative, recorded gradient entries 2e-4 of their scale,
    parse_losses total 1e-4"""
    from iouaware import ops
    from iouaware.train import parse_losses
    from test_host_targets import TRAIN_CFG
    f, head, metas, gts, gls, c, r = _case(case)
    if not device_targets:
        head._device_targets_ok = lambda *a: False
    losses = head.loss(c, r, gts, gls, metas, TRAIN_CFG)
    assert sorted(losses) == ['loss_bbox', 'loss_cls']
    assert isinstance(losses['loss_cls'], ops.LevelLosses)
    for k in KEYS:
        want = f['%s_%d' % (k, case)]
        got = np.array([float(x) for x in losses[k]])
        print(case, device_targets, k, got, want)
        assert np.all(np.abs(got - want) <= 1e-4 * np.maximum(np.abs(want), 1e-6)), k
    loss, log_vars = parse_losses(losses)
    want = float(f['loss_cls_%d' % case].sum() + f['loss_bbox_%d' % case].sum())
    assert rel(float(loss), want) < 1e-4
    assert sorted(log_vars) == ['loss', 'loss_bbox', 'loss_cls']
    loss.backward()
    for l in range(5):
        for nm, ts in (('cls', c), ('reg', r)):
            key = 'g_%s_%d_%d' % (nm, case, l)
            want = f[key].astype(np.float64)
            got = ts[l].grad.cpu().numpy().reshape(-1)[f[key + '_idx']].astype(np.float64)
            err = np.abs(got - want).max()
            print(key, err, np.abs(want).max())
            assert err <= 2e-4 * max(np.abs(want).max(), 1e-30), key


# ------------------------------------------------------------------ 11: argument checks
def test_head_loss_entries_check_the_iou_pointers_and_the_kind():
    """return codes only, valid device buffers throughout: the no-IoU kind with an IoU pointer, the
    IoU-aware kind without one, and both softmax kinds are IA_E_ARG for all four entries; the
    matching combinations succeed"""
    from iouaware import _lib, ops
    sizes = synth.level_shapes(64, 96)
    B, A, Cn, L = 1, synth.A, synth.C, len(sizes)
    base = G.product_base_anchors()
    geoms = {(sm, ib): ops.HeadGeometry(sizes, synth.STRIDES, base, Cn, softmax=sm, iou_branch=ib)
             for sm in (False, True) for ib in (False, True)}
    cl = torch.channels_last
    z = lambda ch: [torch.zeros(B, ch, h, w, device='cuda').contiguous(memory_format=cl)   # noqa: E731
                    for h, w in sizes]
    # channels-last buffers for the nhwc entries (key True), NCHW ones for the others
    maps = {True: (z(A * Cn), z(A * 4), z(A)),
            False: tuple([t.contiguous() for t in x] for x in (z(A * Cn), z(A * 4), z(A)))}
    grads = {k: tuple([torch.empty_like(t) for t in x] for x in v) for k, v in maps.items()}
    labels = [torch.zeros(B, h * w * A, dtype=torch.int64, device='cuda') for h, w in sizes]
    lw = [torch.ones(B, h * w * A, device='cuda') for h, w in sizes]
    bt = [torch.zeros(B, h * w * A, 4, device='cuda') for h, w in sizes]
    bw = [torch.zeros(B, h * w * A, 4, device='cuda') for h, w in sizes]
    bw[0][0, :5] = 1.0                                            # five live anchors on level 0
    bt[0][0, :5] = 0.3
    ht = _lib.HeadTargets()
    for l in range(L):
        ht.labels[l], ht.label_weights[l] = labels[l].data_ptr(), lw[l].data_ptr()
        ht.bbox_targets[l], ht.bbox_weights[l] = bt[l].data_ptr(), bw[l].data_ptr()
    ht.avg_factor = 1.0
    hc = _lib.HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, 0)
    res = torch.zeros(3 * L + 4, device='cuda')
    gin = torch.ones(3 * L + 3, device='cuda')
    lib = _lib.lib()
    nbytes = lib.ia_head_loss_workspace_bytes(geoms[(False, True)].ref(), B)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')

    def ptrs(ts, with_iou, nhwc):
        p, st = _lib.LevelPtrs(), _lib.LevelPixStrides()
        for l in range(L):
            p.cls[l], p.reg[l] = ts[0][l].data_ptr(), ts[1][l].data_ptr()
            st.cls[l], st.reg[l], st.iou[l] = A * Cn, A * 4, A
            p.iou[l] = ts[2][l].data_ptr() if with_iou else None
        return p, st

    def call(entry, geom, with_iou, grad_iou=None):
        grad_iou = with_iou if grad_iou is None else grad_iou
        nhwc = entry.endswith('nhwc')
        p, st = ptrs(maps[nhwc], with_iou, nhwc)
        gp, gst = ptrs(grads[nhwc], grad_iou, nhwc)
        s = ops._stream()
        g = geom.ref()
        if entry == 'fwd':
            return lib.ia_head_loss_fwd(g, C.byref(p), _lib.IA_F32, B, C.byref(ht), C.byref(hc),
                                        ops._ptr(ws), nbytes, ops._ptr(res), s)
        if entry == 'bwd':
            return lib.ia_head_loss_bwd(g, C.byref(p), _lib.IA_F32, B, C.byref(ht), C.byref(hc),
                                        ops._ptr(ws), ops._ptr(res), ops._ptr(gin), C.byref(gp), s)
        if entry == 'fwd_nhwc':
            return lib.ia_head_loss_fwd_nhwc(g, C.byref(p), C.byref(st), B, C.byref(ht), C.byref(hc),
                                             ops._ptr(ws), nbytes, ops._ptr(res), s)
        return lib.ia_head_loss_bwd_nhwc(g, C.byref(p), C.byref(st), B, C.byref(ht), C.byref(hc),
                                         ops._ptr(res), ops._ptr(gin), C.byref(gp), C.byref(gst), s)

    for entry in ('fwd', 'bwd', 'fwd_nhwc', 'bwd_nhwc'):
        plain, aware = geoms[(False, False)], geoms[(False, True)]
        assert call(entry, plain, True) == IA_E_ARG, entry        # IoU map given to the no-IoU kind
        assert call(entry, aware, False) == IA_E_ARG, entry       # IoU map missing for the IoU-aware kind
        if entry.startswith('bwd'):                               # the gradient pointers likewise
            assert call(entry, plain, False, grad_iou=True) == IA_E_ARG, entry
            assert call(entry, aware, True, grad_iou=False) == IA_E_ARG, entry
        for ib in (False, True):                                  # softmax kinds: no fused loss
            assert call(entry, geoms[(True, ib)], ib) == IA_E_ARG, (entry, ib)
    # the matching combinations succeed (forward before backward), and the result vector keeps
    # its 3L + 4 layout: with the no-IoU kind the losses_iou entries and their total are 0.0f
    for with_iou in (True, False):
        for pair in (('fwd', 'bwd'), ('fwd_nhwc', 'bwd_nhwc')):
            res.fill_(-1.0)
            for entry in pair:
                assert call(entry, geoms[(False, with_iou)], with_iou) == 0, (entry, with_iou)
            torch.cuda.synchronize()
            out = res.cpu().numpy()
            assert out[L] > 0 and out[3 * L + 1] == out[L:2 * L].sum()          # loss_bbox, level 0
            assert out[3 * L + 3] == 1.0                                           # avg_factor
            if with_iou:
                assert out[2 * L] > 0 and out[3 * L + 2] > 0
            else:
                assert (out[2 * L:3 * L] == 0.0).all() and out[3 * L + 2] == 0.0


class _Abi:
    """the set-up of the test above for the C-ABI tests below: one level set, B = 1, five live
    anchors on level 0, valid device buffers throughout; here the head outputs are channels-last
    with random box deltas and IoU logits, and the upstream gradients differ per entry"""

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
        self.maps = (rnd(A * Cn, 1.0), rnd(A * 4, 0.2), rnd(A, 1.0))
        self.g_cls = self.rows(A * Cn, 0.0)
        n = lambda h, w: h * w * A                                 # noqa: E731
        self.t = ([torch.zeros(B, n(h, w), dtype=torch.int64, device='cuda') for h, w in sizes],
                  [torch.ones(B, n(h, w), device='cuda') for h, w in sizes],
                  [torch.zeros(B, n(h, w), 4, device='cuda') for h, w in sizes],
                  [torch.zeros(B, n(h, w), 4, device='cuda') for h, w in sizes])
        self.t[3][0][0, :5] = 1.0                                  # five live anchors on level 0
        self.t[2][0][0, :5] = 0.3
        self.ht = _lib.HeadTargets()
        for l in range(L):
            self.ht.labels[l], self.ht.label_weights[l] = self.t[0][l].data_ptr(), self.t[1][l].data_ptr()
            self.ht.bbox_targets[l], self.ht.bbox_weights[l] = self.t[2][l].data_ptr(), self.t[3][l].data_ptr()
        self.ht.avg_factor = 1.0
        self.res = torch.zeros(3 * L + 4, device='cuda')
        self.gin = torch.arange(1, 3 * L + 4, device='cuda', dtype=torch.float32) * 0.25
        self.nbytes = self.lib.ia_head_loss_workspace_bytes(self.geoms[True].ref(), B)
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device='cuda')

    def rows(self, width, fill):
        """per level one buffer of pixel rows of `width` floats"""
        return [torch.full((self.B, h, w, width), fill, device='cuda') for h, w in self.sizes]

    def _ptrs(self, cls, reg, iou):
        """lists of (pointer, pixel stride) per level; iou = None: no IoU maps"""
        p, st = self._lib.LevelPtrs(), self._lib.LevelPixStrides()
        for l in range(self.L):
            (p.cls[l], st.cls[l]), (p.reg[l], st.reg[l]) = cls[l], reg[l]
            if iou is not None:
                p.iou[l], st.iou[l] = iou[l]
        return p, st

    def _inputs(self, with_iou):
        at = lambda ts: [(t.data_ptr(), t.shape[-1]) for t in ts]   # noqa: E731
        return self._ptrs(at(self.maps[0]), at(self.maps[1]), at(self.maps[2]) if with_iou else None)

    def _cfg(self, flag=0):
        return self._lib.HeadLossCfg(2.0, 0.25, 1.0, 0.11, 1.0, 1, 0, flag)

    def fwd_nhwc(self, with_iou):
        p, st = self._inputs(with_iou)
        hc = self._cfg()
        return self.lib.ia_head_loss_fwd_nhwc(self.geoms[with_iou].ref(), C.byref(p), C.byref(st), self.B,
                                              C.byref(self.ht), C.byref(hc), self.ops._ptr(self.ws),
                                              self.nbytes, self.ops._ptr(self.res), self.ops._stream())

    def fwd(self, with_iou):
        """the NCHW entry on the same values"""
        nchw = [[t.permute(0, 3, 1, 2).contiguous() for t in ts] for ts in self.maps]
        p = self._lib.LevelPtrs()
        for l in range(self.L):
            p.cls[l], p.reg[l] = nchw[0][l].data_ptr(), nchw[1][l].data_ptr()
            p.iou[l] = nchw[2][l].data_ptr() if with_iou else None
        hc = self._cfg()
        return self.lib.ia_head_loss_fwd(self.geoms[with_iou].ref(), C.byref(p), self._lib.IA_F32, self.B,
                                         C.byref(self.ht), C.byref(hc), self.ops._ptr(self.ws),
                                         self.nbytes, self.ops._ptr(self.res), self.ops._stream())

    def bwd_nhwc(self, flag, reg, iou):
        """reg / iou: the gradient maps as lists of (pointer, pixel stride); iou = None: no-IoU kind"""
        with_iou = iou is not None
        p, st = self._inputs(with_iou)
        gp, gst = self._ptrs([(t.data_ptr(), t.shape[-1]) for t in self.g_cls], reg, iou)
        hc = self._cfg(flag)
        return self.lib.ia_head_loss_bwd_nhwc(self.geoms[with_iou].ref(), C.byref(p), C.byref(st), self.B,
                                              C.byref(self.ht), C.byref(hc), self.ops._ptr(self.res),
                                              self.ops._ptr(self.gin), C.byref(gp), C.byref(gst),
                                              self.ops._stream())


SENTINEL = 7.25


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize('with_iou', [True, False])
def test_bwd_nhwc_grad_rows_start_at_reg_contradictions_and_padding(with_iou):
    """cfg->grad_rows_start_at_reg set: a gradient row that contradicts it is IA_E_ARG (checked
    before memory is touched) -- iou not at reg + 4A, unequal strides, more than 64 channels
    behind reg | iou (behind reg for the no-IoU kind); the matching row returns 0, its padding
    channels read back exactly 0.0f and its reg | iou channels carry the bits of the call with
    separate gradient tensors.  Rows: 5A + 3 floats with the IoU branch; without it 4A + 4, the
    narrowest padded row the entry takes -- 4A + 3 floats is no multiple of 16 bytes, which the
    entry refuses for every reg stride (include/iouaware.h: strides 16-byte aligned)."""
    s = _Abi()
    A = s.A
    used = 5 * A if with_iou else 4 * A
    assert s.fwd_nhwc(with_iou) == 0

    def call(width, iou_off=4 * A, iou_stride_plus=0):
        rows = s.rows(width, SENTINEL)
        reg = [(t.data_ptr(), width) for t in rows]
        iou = [(t.data_ptr() + 4 * iou_off, width + iou_stride_plus) for t in rows] if with_iou else None
        return s.bwd_nhwc(1, reg, iou), rows

    if with_iou:
        assert call(used + 3, iou_off=4 * A + 1)[0] == IA_E_ARG       # grads.iou != grads.reg + 4A
        assert call(used + 3, iou_stride_plus=4)[0] == IA_E_ARG       # strides differ
        assert call(used + 67)[0] == IA_E_ARG                         # 67 channels behind reg | iou
        width = used + 3
    else:
        assert call(used + 68)[0] == IA_E_ARG                         # 68 channels behind reg
        assert call(used + 3)[0] == IA_E_ARG                          # 39 floats: not 16-byte rows
        width = used + 4
    rc, rows = call(width)
    assert rc == 0
    g_reg, g_iou = s.rows(4 * A, SENTINEL), s.rows(A, SENTINEL)       # the call without the flag
    assert s.bwd_nhwc(0, [(t.data_ptr(), 4 * A) for t in g_reg],
                      [(t.data_ptr(), A) for t in g_iou] if with_iou else None) == 0
    torch.cuda.synchronize()
    assert float(g_reg[0].abs().max()) > 0
    for l in range(s.L):
        assert _same_bits(rows[l][..., used:], torch.zeros_like(rows[l][..., used:])), l
        assert _same_bits(rows[l][..., :4 * A], g_reg[l]), l
        if with_iou:
            assert _same_bits(rows[l][..., 4 * A:used], g_iou[l]), l


def test_bwd_nhwc_without_the_flag_writes_the_reg_and_iou_slices_alone():
    """cfg->grad_rows_start_at_reg clear, gradient rows [X (4) | reg | iou | pad (3)] filled with a
    sentinel: after the call X and pad of every pixel still hold it, and reg | iou carry the bits
    of the call with separate gradient tensors"""
    s = _Abi()
    A = s.A
    assert s.fwd_nhwc(True) == 0
    g_reg, g_iou = s.rows(4 * A, SENTINEL), s.rows(A, SENTINEL)
    assert s.bwd_nhwc(0, [(t.data_ptr(), 4 * A) for t in g_reg], [(t.data_ptr(), A) for t in g_iou]) == 0
    width = 4 + 5 * A + 3
    rows = s.rows(width, SENTINEL)
    assert s.bwd_nhwc(0, [(t.data_ptr() + 4 * 4, width) for t in rows],
                      [(t.data_ptr() + 4 * (4 + 4 * A), width) for t in rows]) == 0
    torch.cuda.synchronize()
    assert float(g_reg[0].abs().max()) > 0 and float(g_iou[0].abs().max()) > 0
    for l in range(s.L):
        r = rows[l]
        assert bool((r[..., :4] == SENTINEL).all()) and bool((r[..., 4 + 5 * A:] == SENTINEL).all()), l
        assert _same_bits(r[..., 4:4 + 4 * A], g_reg[l]) and _same_bits(r[..., 4 + 4 * A:4 + 5 * A], g_iou[l]), l


@pytest.mark.parametrize('entry', ['fwd', 'fwd_nhwc'])
def test_forward_entries_refuse_a_missing_normaliser_before_any_launch(entry):
    """counts = NULL, avg_factor_dev = NULL, avg_factor = 0: IA_E_ARG, and nothing was enqueued --
    workspace and result still hold the bytes they were filled with"""
    s = _Abi()
    s.ht.avg_factor = 0.0
    s.ws.fill_(0xA5)
    s.res.view(torch.uint8).fill_(0xA5)
    assert getattr(s, entry)(True) == IA_E_ARG
    torch.cuda.synchronize()
    assert bool((s.ws == 0xA5).all()) and bool((s.res.view(torch.uint8) == 0xA5).all())


# ------------------------------------------------------------------ 12: Winograd training head
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _rel2(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _train_head():
    torch.manual_seed(3)
    head = _head().train()
    with torch.no_grad():                      # activations of unit scale through the towers
        for p in head.parameters():
            if p.dim() == 4:
                p.normal_(0, (2.0 / (9 * p.shape[1])) ** 0.5)
            else:
                p.normal_(0, 0.1)
    return head


@pytest.mark.module_path
@pytest.mark.parametrize('layout', ['nchw', 'channels_last', 'all_active'])
def test_plain_head_forward_backward_matches_module_path(layout):
    """tests/test_gpu_winograd_train.py::test_head_forward_backward_matches_module_path for the head
    without `retina_iou`: train_winograd True against False on one state dict"""
    head = _train_head()
    strict = layout == 'all_active'
    if strict:
        # tower biases large enough that no pre-activation is ever negative: every ReLU is the
        # identity in both paths, the head is linear, and gradients must agree element-wise
        with torch.no_grad():
            for m in list(head.cls_convs) + list(head.reg_convs):
                m.conv.weight.mul_(0.2)
                m.conv.bias.fill_(6.0)
    g = torch.Generator(device='cuda').manual_seed(1)
    sizes = synth.level_shapes(224, 288)
    feats = [torch.randn(2, 256, h, w, device='cuda', generator=g) for (h, w) in sizes]
    if layout == 'channels_last':
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    ups = None
    res = {}
    for mode in (True, False):
        head.train_winograd = mode
        head.zero_grad()
        xs = [f.clone().requires_grad_(True) for f in feats]
        outs = head(xs)
        assert len(outs) == 2
        cls, reg = outs
        assert ('WinoConvLevels' in type(cls[0].grad_fn).__name__) == mode
        if ups is None:
            ups = [[torch.randn(t.shape, device='cuda', generator=g) for t in o] for o in (cls, reg)]
        loss = sum((t * u).sum() for o, us in zip((cls, reg), ups) for t, u in zip(o, us))
        loss.backward()
        res[mode] = ([t.detach().contiguous() for o in (cls, reg) for t in o],
                     {n: p.grad.clone() for n, p in head.named_parameters()},
                     [x.grad.contiguous() for x in xs])
    (oa, ga, xa), (ob, gb, xb) = res[True], res[False]
    assert [tuple(t.shape) for t in oa] == [tuple(t.shape) for t in ob]
    for a, b in zip(oa, ob):
        assert _rel(a, b) < 1e-4
    # (the bounds and their reason: the IoU-aware test this one mirrors)
    tol2, tol = (1e-4, 2e-4) if strict else (5e-2, 1.0)
    for n in gb:
        print(layout, n, _rel2(ga[n], gb[n]), _rel(ga[n], gb[n]))
        assert ga[n].shape == gb[n].shape and _rel2(ga[n], gb[n]) < tol2, (n, _rel2(ga[n], gb[n]))
        assert _rel(ga[n], gb[n]) < tol, n
    for a, b in zip(xa, xb):
        assert _rel2(a, b) < tol2


@pytest.mark.module_path
def test_plain_training_iteration_same_losses_and_grads():
    """the whole plain detector (retinanet_r50_fpn_1x settings, small image), one iteration with and
    without the Winograd training head: loss 1e-5 relative, gradient norms 1e-2"""
    import iouaware
    from iouaware import ops
    from iouaware.config import ConfigDict
    from iouaware.train import parse_losses
    with open(os.path.join(GOLD, 'retina_plain_ref.json')) as fh:
        rec = json.load(fh)['retinanet_r50_fpn_1x']
    rec['model']['pretrained'] = None
    torch.manual_seed(0)
    model = iouaware.build_detector(ConfigDict(rec['model']), train_cfg=ConfigDict(rec['train_cfg']),
                                    test_cfg=ConfigDict(rec['test_cfg'])).cuda().train()
    B, ph, pw = 2, 256, 320
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(B, 3, ph, pw, device='cuda', generator=g)
    gts, gls = synth.train_targets(11, B, ph, pw, max_gt=5)
    gtb = [torch.from_numpy(x).cuda() for x in gts]
    gtl = [torch.from_numpy(x).cuda() for x in gls]
    metas = [synth.img_meta(ph, pw, ph, pw) for _ in range(B)]
    out = {}
    for mode in (True, False):
        model.bbox_head.train_winograd = mode
        model.zero_grad()
        losses = model(img, metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
        assert sorted(losses) == ['loss_bbox', 'loss_cls']
        assert isinstance(losses['loss_cls'], ops.LevelLosses)       # the fused node, both routes
        loss, lv = parse_losses(losses)
        loss.backward()
        out[mode] = (float(loss), {n: p.grad.clone() for n, p in model.named_parameters()
                                   if p.grad is not None})
    (la, ga), (lb, gb) = out[True], out[False]
    print('loss', la, lb)
    assert abs(la - lb) <= 1e-5 * abs(lb)
    assert set(ga) == set(gb)
    for n in gb:
        assert _rel2(ga[n], gb[n]) < 1e-2, (n, _rel2(ga[n], gb[n]))

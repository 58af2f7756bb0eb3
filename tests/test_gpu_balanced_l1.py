"""GPU (MI355X): BalancedL1Loss on the anchor heads -- the per-level kernels (csrc/loss.hip,
k_smooth_l1<.., LOC = 1> behind ia_balanced_l1_fwd / _bwd), the all-levels node (csrc/headloss.hip,
k_box_ml / k_box_nhwc with LOC = 1 behind the ia_head_loss_*_box entries), the loss module on both heads
and one training step per route -- against tests/balanced_l1_ref.py (float64 torch autograd) and the
reference's recorded numbers (tests/golden/balanced_l1.npz, make_golden_balanced_l1.py).

The edge data is built here (numpy, from seeds) and shared with tests/test_host_balanced_l1.py:
  levels (bl_level): maps 2 x 3 (one tile) and 17 x 19 (a partial second tile), B = 2, A = 9, random
    deltas, about half the anchors with weight 0, and planted among them the anchors of bl_specs():
    |pred - target| in {0, beta, both fp32 neighbours of beta, 1e-4, 3, 1e4} in both signs, the weights
    (1, 0.5, 0, 2) and a weight-0 anchor with a large prediction;
  node (node_data): the same on synth.level_shapes(64, 96) = 96, 24, 6, 2 and 1 positions -- level
    boundaries fall inside one block, blocks with and without a live anchor;
  beta in {0.11, 1.0}, (alpha, gamma) in {(0.5, 1.5), (0.25, 1.0)}.
check_coverage asserts that live elements fall in both branches and exactly on the knee.

Bars.
  * weight-0 elements and pred == target: gradient == 0; every output finite;
  * the *_box entries with NULL and with kind 0: torch.equal to the old entries (results and gradients);
  * against the yardstick: gradients max(4 x E_ref, 1e-5 |g| + 1e-6 max|g|), sums max(4 x E_ref, 1e-5)
    relative -- the floors of the focal kernels in tests/test_gpu_loss_edges.py, which also use the
    hardware log; a measured error above FOCAL_FINDING (2.5e-5) is a finding, not a bar to raise;
  * bf16 maps: grad_within of that file, the fp32 bar plus one bf16 rounding;
  * node against the per-level kernels, channels-last against NCHW: 1e-6 (test_gpu_retina_plain_train.py);
  * with the IoU term the bar of the box gradient is the sum of the bars of its two parts (the
    BalancedL1 bar above, and box_bar('g_box') of test_gpu_loss_edges.py for the part through the target);
  * the reference fixture: losses 1e-4, gradient entries 2e-4 of their scale (retina_plain_train.npz).

E_ref -- a plain float32 torch evaluation of the same expression against the yardstick, on the edge
data (tests/test_host_balanced_l1.py prints and asserts this table; worst over both levels, the node's
five levels, fp32 and bf16-rounded inputs; gradients as a share of the tensor's maximum, sums relative):
    beta   (alpha, gamma)   gradient     sum
    0.11   (0.5, 1.5)       1.3e-7       1.1e-7
    0.11   (0.25, 1.0)      1.9e-7       1.3e-7
    1.0    (0.5, 1.5)       1.0e-7       1.1e-7
    1.0    (0.25, 1.0)      9.2e-8       1.4e-7
  4 x these stay below the floors, which therefore are the bars: 1e-5 |g| + 1e-6 max|g|, sums 1e-5.

Measured on an MI355X (this file, fp32 maps, worst over the same set and both (alpha, gamma); what
note() prints, and what the module's last step holds against FOCAL_FINDING):
                                   beta 0.11            beta 1.0
    per-level g, of max            8.1e-8               8.6e-8
    per-level sum, relative        4.0e-8               1.1e-7
    node g_reg, of max             1.2e-7               2.3e-7      (with the IoU term: + the part through the target)
    node loss_bbox, relative       6.0e-8               1.1e-7
  all below E_ref x 4 and two orders below FOCAL_FINDING; a bf16 gradient differs by its one rounding
  (up to 3.0e-3 of the maximum here), which grad_within allows and nothing more.
"""
import os

import numpy as np
import pytest
import torch

import balanced_l1_ref as BL
import loss_ref as R
import synth
from test_gpu_loss_edges import (FOCAL_FINDING, SETS, _next, bf16_round, box_bar, finite, grad_within, np32,
                                 rel, share_of_max)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
B, A = 2, synth.A
BETAS = (0.11, 1.0)
AGS = ((0.5, 1.5), (0.25, 1.0))
LEVELS = {'2x3': (2, 3), '17x19': (17, 19)}
NODE_PAD = (64, 96)                      # synth.level_shapes -> 96, 24, 6, 2, 1 positions
NODE_SET = 'stds'                        # target means / stds of the node's IoU decode
GS = 0.375

# (beta, (alpha, gamma)) -> (gradient error as a share of the tensor's maximum, relative error of the sum):
# float32 torch against the yardstick, CPU (tests/test_host_balanced_l1.py asserts it)
E_REF = {
    (0.11, (0.5, 1.5)): (1.3e-7, 1.1e-7),
    (0.11, (0.25, 1.0)): (1.9e-7, 1.3e-7),
    (1.0, (0.5, 1.5)): (1.0e-7, 1.1e-7),
    (1.0, (0.25, 1.0)): (9.2e-8, 1.4e-7),
}


def bars(beta, ag):
    """-> (share of max allowed beside the floor 1e-5 |g| + 1e-6 max|g|, relative bar of the sum)"""
    eg, es = E_REF[(beta, ag)]
    assert eg <= FOCAL_FINDING and es <= FOCAL_FINDING
    return 4.0 * eg, max(4.0 * es, 1e-5)


def grad_ok(got, ref, beta, ag, bf16=False):
    share, _ = bars(beta, ag)
    return grad_within(got, ref, 1e-6, 1e-5, bf16) or grad_within(got, ref, share, 0.0, bf16)


# ------------------------------------------------------------------ data
def bl_specs(beta):
    """-> list of (name, pred(4), weights(4)); the target of a planted anchor is 0, so |pred - target| is
    the stored number itself"""
    b = np.float32(beta)
    up, dn = _next(b, 1), _next(b, -1)
    one, z = (1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0)
    return [('weights', (b, -b, 3.0, up), (1.0, 0.5, 0.0, 2.0)),
            ('knee_a', (-up, -dn, dn, up), one),
            ('knee_b', (b, -b, dn, -dn), one),
            ('small', (0.0, 1e-4, -1e-4, 0.0), one),
            ('far', (3.0, -3.0, 1e4, -1e4), one),
            ('mixed', (-1e-4, 1e4, -b, 0.0), (2.0, 0.5, 1.0, 1.0)),
            ('w0', (1e4, -3e4, b, 0.05), z)]                   # weight 0, a large prediction: gradient 0


_CACHE = {}


def bl_level(h, w, beta, seed, rot=0, bf16=False):
    """-> dict(reg (B, A*4, h, w), iou (B, A, h, w), bt / bw (B, h*w*A, 4), slots {spec name: (b, p, a)}),
    float32; read-only, cached"""
    key = (h, w, beta, seed, rot, bf16)
    if key in _CACHE:
        return _CACHE[key]
    rs = np.random.RandomState(seed)
    HW = h * w
    N = B * HW * A
    pred = (rs.standard_normal((N, 4)) * 0.25).astype(np.float32)
    tgt = (rs.standard_normal((N, 4)) * 0.25).astype(np.float32)
    xl = (rs.standard_normal(N) * 1.5).astype(np.float32)
    wgt = np.repeat((rs.rand(N) < 0.5).astype(np.float32)[:, None], 4, 1)
    specs = bl_specs(beta)
    nS = len(specs)
    step = max(N // nS, 1)
    if step > 1 and step % A == 0:
        step -= 1                                  # walk through the anchors of a position too
    slots = {}
    for k in range(min(nS, N)):
        name, p4, w4 = specs[(k + rot) % nS]
        n = k * step
        pred[n], tgt[n], wgt[n] = np.asarray(p4, np.float32), 0.0, w4
        slots[name] = (n // (HW * A), (n // A) % HW, n % A)
    if bf16:
        pred, tgt, xl = bf16_round(pred), bf16_round(tgt), bf16_round(xl)
    reg = np.ascontiguousarray(pred.reshape(B, h, w, A * 4).transpose(0, 3, 1, 2))
    iou = np.ascontiguousarray(xl.reshape(B, h, w, A).transpose(0, 3, 1, 2))
    out = dict(reg=reg, iou=iou, bt=tgt.reshape(B, HW * A, 4), bw=wgt.reshape(B, HW * A, 4), slots=slots,
               hw=(h, w))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = out
    return out


def _rows(d):
    """(N, 4) |pred - target| and weights of a level, in fp32 as the kernels form them"""
    h, w = d['hw']
    pred = d['reg'].transpose(0, 2, 3, 1).reshape(-1, 4)
    return np.abs(pred - d['bt'].reshape(-1, 4)), d['bw'].reshape(-1, 4)


def check_coverage(levels, beta, bf16=False):
    """live elements fall in both branches and exactly on the knee (and on both fp32 neighbours of it);
    about half the anchors weigh 0; pred == target occurs on a live element.  bf16-rounded maps: the
    neighbours do not exist, and the knee itself only where beta is a bf16 number"""
    knee = not bf16 or float(np.float32(beta)) == float(bf16_round(np.float32([beta]))[0])
    diff = np.concatenate([_rows(d)[0] for d in levels])
    wgt = np.concatenate([_rows(d)[1] for d in levels])
    live = wgt != 0
    b = np.float32(beta)
    assert (live & (diff < b)).any() and (live & (diff > b)).any()
    assert (live & (diff == 0)).any()
    if knee:
        assert (live & (diff == b)).any()
    if not bf16:
        assert (live & (diff == _next(b, 1))).any() and (live & (diff == _next(b, -1))).any()
    dead = (wgt == 0).all(1).mean()
    assert 0.25 < dead < 0.75, dead


def weight0_mask(d, anchors=False):
    """(B, A*4, h, w) bool: coordinates whose weight is 0 (anchors: of anchors whose four weights are 0 --
    the part of the gradient through the IoU target weighs all four coordinates by the first weight)"""
    h, w = d['hw']
    z = d['bw'] == 0
    if anchors:
        z = np.broadcast_to(z.all(-1, keepdims=True), z.shape)
    return np.ascontiguousarray(z.reshape(B, h, w, A * 4).transpose(0, 3, 1, 2))


def equal_mask(d):
    """(B, A*4, h, w) bool: pred == target"""
    h, w = d['hw']
    tg = d['bt'].reshape(B, h, w, A * 4).transpose(0, 3, 1, 2)
    return d['reg'] == tg


def node_data(beta, bf16=False):
    """-> (sizes, levels, cls, labels, label weights): the planted anchors spread over five levels"""
    sizes = synth.level_shapes(*NODE_PAD)
    levels = [bl_level(h, w, beta, 40 + l, rot=2 * l, bf16=bf16) for l, (h, w) in enumerate(sizes)]
    rs = np.random.RandomState(9)
    cls, labels, lw = [], [], []
    for (h, w) in sizes:
        n = h * w * A
        x = (rs.standard_normal((B, A * synth.C, h, w)) * 2.0 - 6.0).astype(np.float32)
        cls.append(bf16_round(x) if bf16 else x)
        lab = np.zeros((B, n), np.int64)
        pos = rs.rand(B, n) < 0.1
        lab[pos] = rs.randint(1, synth.C + 1, int(pos.sum()))
        labels.append(lab)
        lw.append((rs.rand(B, n) > 0.1).astype(np.float32))
    return sizes, levels, cls, labels, lw


# ------------------------------------------------------------------ GPU tests
gpu = pytest.mark.gpu
WORST = {}


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))
    print('%-44s %.3g' % (key, err))


@pytest.fixture(scope='module', autouse=True)
def worst_errors_are_no_finding():
    """after the module's tests: every fp32 error note() collected in this run stays below FOCAL_FINDING (a
    bf16 entry holds that map's one rounding, which grad_within has judged element by element)"""
    yield
    for key, err in sorted(WORST.items()):
        assert key.startswith('bf16 ') or err <= FOCAL_FINDING, (key, err)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from iouaware import ops as o
    return o


def _dev(a, bf16=False):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def _geom(ops, iou_branch=True, set_name=NODE_SET):
    import gpu_util as G
    means, stds = SETS[set_name]
    base = G.product_base_anchors()
    geom = ops.HeadGeometry(synth.level_shapes(*NODE_PAD), synth.STRIDES, base, synth.C, means=means, stds=stds,
                            iou_branch=iou_branch)
    return geom, base


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('ag', AGS, ids=['a.5g1.5', 'a.25g1'])
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('level', sorted(LEVELS))
def test_per_level_kernels_edges(ops, level, beta, ag, bf16):
    """ia_balanced_l1_fwd / _bwd: sum and gradient against the yardstick, the exact zeros, a gradient
    written for every element"""
    h, w = LEVELS[level]
    d = bl_level(h, w, beta, 11, bf16=bf16)
    check_coverage([d], beta, bf16)
    alpha, gamma = ag
    ref = BL.balanced_l1(d['reg'], d['bt'], d['bw'], A, beta, alpha, gamma, GS)
    r = _dev(d['reg'], bf16).requires_grad_(True)
    loss = ops.balanced_l1_sum(r, _dev(d['bt']), _dev(d['bw']), A, beta, alpha, gamma)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    (loss * GS).sum().backward()
    torch.cuda.synchronize()
    g, loss = np32(r.grad), loss.detach()
    assert r.grad.dtype == r.dtype and finite(g, float(loss))
    es, eg = rel(float(loss), ref['sum']), share_of_max(g, ref['grad'])
    tag = 'bf16 ' if bf16 else ''
    note('%sper-level beta %g ag %s sum (rel)' % (tag, beta, ag), es)
    note('%sper-level beta %g ag %s g (of max)' % (tag, beta, ag), eg)
    assert es <= bars(beta, ag)[1]
    assert grad_ok(g, ref['grad'], beta, ag, bf16)
    assert bool((g[weight0_mask(d)] == 0.0).all()) and bool((g[equal_mask(d)] == 0.0).all())
    assert weight0_mask(d).any() and (equal_mask(d) & ~weight0_mask(d)).any()
    # the module form on (N, 4) rows: the same kernels with B = N, A = 1, HW = 1
    from iouaware.losses import BalancedL1Loss
    mod = BalancedL1Loss(alpha=alpha, gamma=gamma, beta=beta, loss_weight=2.0)
    rows = _dev(d['reg'], bf16).permute(0, 2, 3, 1).reshape(-1, 4)
    out = mod(rows, _dev(d['bt']).reshape(-1, 4).to(rows.dtype), _dev(d['bw']).reshape(-1, 4), avg_factor=7.0)
    assert out.shape == (1,) and rel(float(out), 2.0 * ref['sum'] / 7.0) <= bars(beta, ag)[1]
    lvl = mod.forward_level(_dev(d['reg'], bf16), _dev(d['bt']), _dev(d['bw']), A, 7.0)
    assert rel(float(lvl), float(out)) <= 1e-6


def _run_node(ops, beta, layout, iou_branch, box_loss, bf16=False, attach=True, eta=None, pad=None,
              weights=None):
    """the all-levels node on node_data(beta) -> dict(losses {key: [L floats]}, g_cls, g_reg, g_iou (fp32
    numpy per level, NCHW order), g_pad).  layout: 'nchw' | 'nhwc'; pad: reg (| iou) as the leading slice
    of a row with `pad` more channels (channels-last only)"""
    sizes, levels, cls, labels, lw = node_data(beta, bf16)
    geom, _ = _geom(ops, iou_branch)
    cl = layout == 'nhwc'

    def leaf(x):
        t = _dev(x, bf16)
        if cl:
            t = t.contiguous(memory_format=torch.channels_last)
        return t.requires_grad_(True)
    c = [leaf(x) for x in cls]
    bases = None
    if pad is None:
        r = [leaf(d['reg']) for d in levels]
        i = [leaf(d['iou']) for d in levels] if iou_branch else None
    else:
        gen = torch.Generator(device='cuda').manual_seed(3)
        bases = []
        for d in levels:
            parts = [_dev(d['reg'])] + ([_dev(d['iou'])] if iou_branch else [])
            parts.append(torch.randn(B, pad, *d['hw'], device='cuda', generator=gen))
            bases.append(torch.cat(parts, 1).contiguous(memory_format=torch.channels_last).requires_grad_(True))
        r = [b[:, :4 * A] for b in bases]
        i = [b[:, 4 * A:5 * A] for b in bases] if iou_branch else None
        assert ops._nhwc_route(geom, c, r, i)[0] is not None
    out = ops.head_loss(geom, c, r, i, [_dev(x) for x in labels], [_dev(x) for x in lw],
                        [_dev(d['bt']) for d in levels], [_dev(d['bw']) for d in levels], avg_factor=13.0,
                        gamma=2.0, alpha=0.25, beta=beta, loss_weight_bbox=1.0, attach_iou_target=attach,
                        channels_last=cl, eta=eta, box_loss=box_loss)
    L = len(sizes)
    if weights is None:
        total = sum(v.total for v in out.values()).sum()
    else:                                           # upstream gradients that differ per loss and level
        total = sum(weights[k][l] * v[l] for k, v in enumerate(out.values()) for l in range(L)).sum()
    total.backward()
    torch.cuda.synchronize()
    res = dict(losses={k: [float(x.detach()) for x in v] for k, v in out.items()},
               raw={k: torch.cat([x.detach().reshape(1) for x in v]) for k, v in out.items()},
               g_cls=[t.grad for t in c])
    if bases is None:
        res['g_reg'] = [t.grad for t in r]
        res['g_iou'] = [t.grad for t in i] if iou_branch else None
        res['g_pad'] = None
    else:
        res['g_reg'] = [b.grad[:, :4 * A] for b in bases]
        res['g_iou'] = [b.grad[:, 4 * A:5 * A] for b in bases] if iou_branch else None
        res['g_pad'] = [b.grad[:, (5 if iou_branch else 4) * A:] for b in bases]
    return res


class _OldEntries(object):
    """the library with every ia_head_loss_*_box entry routed to the entry WITHOUT the box argument
    (which must be NULL): what ran before the choice existed"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not (name.startswith('ia_head_loss_') and name.endswith('_box')):
            return fn
        old = getattr(self._lib, name[:-len('_box')])

        def call(*a):
            assert a[6] is None, 'the old entries have no localisation-loss choice'
            return old(*(a[:6] + a[7:]))
        return call


@gpu
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou_aware', 'noiou'])
@pytest.mark.parametrize('layout,bf16', [('nchw', False), ('nchw', True), ('nhwc', False)],
                         ids=['nchw-fp32', 'nchw-bf16', 'channels_last'])
def test_null_and_kind0_are_the_old_entries(ops, monkeypatch, layout, bf16, iou_branch):
    """the *_box entries with box = NULL and with kind IA_BOX_SMOOTH_L1 return results and gradients
    torch.equal to ia_head_loss_fwd / _bwd(_nhwc)"""
    from iouaware import _lib
    import ctypes as C
    real = _lib.lib()
    runs = {}
    runs['null'] = _run_node(ops, 0.11, layout, iou_branch, None, bf16)
    with monkeypatch.context() as m:
        m.setattr(_lib, 'lib', lambda: _OldEntries(real))
        runs['old'] = _run_node(ops, 0.11, layout, iou_branch, None, bf16)
    with monkeypatch.context() as m:
        # alpha / gamma of a kind-0 struct are not looked at
        m.setattr(ops, '_box_loss_cfg', lambda box: _lib.BoxLossCfg(C.sizeof(_lib.BoxLossCfg),
                                                                    _lib.IA_BOX_SMOOTH_L1, -1.0, 0.0))
        runs['kind0'] = _run_node(ops, 0.11, layout, iou_branch, None, bf16)
    old = runs['old']
    assert sum(v > 0 for v in old['losses']['loss_bbox']) >= 3
    for name in ('null', 'kind0'):
        got = runs[name]
        assert sorted(got['raw']) == sorted(old['raw'])
        for k in old['raw']:
            assert torch.equal(got['raw'][k], old['raw'][k]), (name, k)
        for key in ('g_cls', 'g_reg') + (('g_iou',) if iou_branch else ()):
            for l, (x, y) in enumerate(zip(got[key], old[key])):
                assert x.dtype == y.dtype and torch.equal(x, y), (name, key, l)


def _node_refs(beta, ag, levels, base, iou_branch, attach, bf16=False):
    """per level: yardstick sums and gradients of the node's box part, gscale = 1 / 13"""
    means, stds = SETS[NODE_SET]
    out = []
    for l, d in enumerate(levels):
        rb = BL.balanced_l1(d['reg'], d['bt'], d['bw'], A, beta, ag[0], ag[1], 1.0 / 13.0)
        ri = None
        if iou_branch:
            ri = R.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base[l], synth.STRIDES[l], means, stds,
                           1.0 / 13.0, attach)
        out.append((rb, ri))
    return out


def _check_node_against_yardstick(ops, got, beta, ag, iou_branch, attach, tag, bf16=False):
    import gpu_util as G
    sizes, levels, cls, labels, lw = node_data(beta, bf16)
    refs = _node_refs(beta, ag, levels, G.product_base_anchors(), iou_branch, attach, bf16)
    share, sum_bar = bars(beta, ag)
    for l, (d, (rb, ri)) in enumerate(zip(levels, refs)):
        gr = np32(got['g_reg'][l])
        lb = got['losses']['loss_bbox'][l]
        assert finite(gr, lb), l
        es = rel(lb, rb['sum'] / 13.0) if rb['sum'] else abs(lb)
        note('%s beta %g ag %s sum (rel)' % (tag, beta, ag), es)
        assert es <= sum_bar, (l, lb, rb['sum'] / 13.0)
        want = rb['grad']
        extra = 0.0
        if iou_branch and attach:
            # the bar of a sum of two parts: the sum of their bars
            want = want + ri['g_box']
            extra = box_bar('g_box') * float(ri['g_box'].abs().max())
        note('%s beta %g ag %s g_reg (of max)' % (tag, beta, ag), share_of_max(gr, want))
        w64 = np.asarray(want, np.float64)
        tol = np.maximum(share * np.abs(w64).max(), 1e-5 * np.abs(w64) + 1e-6 * np.abs(w64).max()) + extra
        if bf16:
            from test_gpu_loss_edges import _to_bf16
            ok = (gr >= _to_bf16(w64 - tol, -np.inf)) & (gr <= _to_bf16(w64 + tol, np.inf))
        else:
            ok = np.abs(gr - w64) <= tol
        assert bool(ok.all()), (l, float(np.abs(gr - w64).max()), float(tol.min()))
        through = iou_branch and attach             # a gradient through the IoU target on every coordinate
        assert bool((gr[weight0_mask(d, anchors=through)] == 0.0).all()), l
        if not through:
            assert bool((gr[equal_mask(d)] == 0.0).all()), l
        if iou_branch:
            gi = np32(got['g_iou'][l])
            assert finite(gi) and grad_within(gi, ri['g_iou'], box_bar('g_iou'), bf16=bf16), l
            assert rel(got['losses']['losses_iou'][l], ri['sum'] / 13.0) <= box_bar('iou_sum'), l


@gpu
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou_aware', 'noiou'])
@pytest.mark.parametrize('layout,bf16', [('nchw', False), ('nchw', True), ('nhwc', False)],
                         ids=['nchw-fp32', 'nchw-bf16', 'channels_last'])
@pytest.mark.parametrize('ag', AGS, ids=['a.5g1.5', 'a.25g1'])
@pytest.mark.parametrize('beta', BETAS)
def test_node_edges(ops, beta, ag, layout, bf16, iou_branch):
    """the node with kind 1 against the yardstick, both layouts, with and without the IoU term (the box
    gradient = BalancedL1 + the part through the attached target); focal results are those of kind 0"""
    sizes, levels, *_ = node_data(beta, bf16)
    check_coverage(levels, beta, bf16)
    seen = set()
    for d in levels:
        seen |= set(d['slots'])
    assert seen == set(n for n, *_ in bl_specs(beta))
    got = _run_node(ops, beta, layout, iou_branch, ('balanced_l1',) + ag, bf16)
    assert sorted(got['losses']) == (['loss_bbox', 'loss_cls', 'losses_iou'] if iou_branch
                                     else ['loss_bbox', 'loss_cls'])
    tag = ('bf16 ' if bf16 else '') + 'node %s %s' % (layout, 'iou' if iou_branch else 'noiou')
    _check_node_against_yardstick(ops, got, beta, ag, iou_branch, True, tag, bf16)
    plain = _run_node(ops, beta, layout, iou_branch, None, bf16)
    assert torch.equal(got['raw']['loss_cls'], plain['raw']['loss_cls'])
    for x, y in zip(got['g_cls'], plain['g_cls']):
        assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_iou_aware_detached_target_and_balanced_cls(ops, layout):
    """target detached: the box gradient is the BalancedL1 gradient alone; balanced_cls together with
    kind 1 runs, its box part unchanged"""
    beta, ag = 0.11, AGS[0]
    box = ('balanced_l1',) + ag
    det = _run_node(ops, beta, layout, True, box, attach=False)
    _check_node_against_yardstick(ops, det, beta, ag, True, False, 'node %s detached' % layout)
    att = _run_node(ops, beta, layout, True, box)
    assert any(not torch.equal(x, y) for x, y in zip(att['g_reg'], det['g_reg']))
    bal = _run_node(ops, beta, layout, True, box, eta=1.5)
    assert finite(*[np32(t) for t in bal['g_cls'] + bal['g_reg'] + bal['g_iou']], *bal['losses']['loss_cls'])
    assert torch.equal(bal['raw']['loss_bbox'], att['raw']['loss_bbox'])
    assert torch.equal(bal['raw']['losses_iou'], att['raw']['losses_iou'])
    for x, y in zip(bal['g_reg'], att['g_reg']):
        assert torch.equal(x, y)
    assert not torch.equal(bal['raw']['loss_cls'], att['raw']['loss_cls'])
    with pytest.raises(ValueError):                              # kind 1 with the IoU-balanced weighting
        sizes, levels, cls, labels, lw = node_data(beta)
        ops.head_loss(_geom(ops)[0], [_dev(x) for x in cls], [_dev(d['reg']) for d in levels],
                      [_dev(d['iou']) for d in levels], [_dev(x) for x in labels], [_dev(x) for x in lw],
                      [_dev(d['bt']) for d in levels], [_dev(d['bw']) for d in levels], avg_factor=13.0,
                      beta=beta, delta=1.5, box_loss=box)


def _close(x, y, tol=1e-6):
    return x.shape == y.shape and float((x.float() - y.float()).abs().max()) <= \
        tol * max(float(y.float().abs().max()), 1e-30)


@gpu
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou_aware', 'noiou'])
def test_node_equals_per_level_kernels_and_layouts_agree(ops, iou_branch):
    """the node equals the per-level kernels within 1e-6 (different upstream gradients per level);
    channels-last equals NCHW with reg as its own tensor, as the leading slice of a 40-channel (no IoU)
    / 48-channel row and of a 104-channel row; with grad_rows_start_at_reg the trailing channels are exact
    zeros"""
    beta, ag = 0.11, AGS[0]
    box = ('balanced_l1',) + ag
    L = 5
    wts = torch.arange(1, 3 * L + 1, device='cuda', dtype=torch.float32).reshape(3, L) * 0.25
    a = _run_node(ops, beta, 'nchw', iou_branch, box, weights=wts)
    sizes, levels, *_ = node_data(beta)
    for l, d in enumerate(levels):
        r = _dev(d['reg']).requires_grad_(True)
        s = ops.balanced_l1_sum(r, _dev(d['bt']), _dev(d['bw']), A, beta, *ag) * (1.0 / 13.0)
        assert rel(float(s.detach()), a['losses']['loss_bbox'][l]) < 1e-6 or float(s.detach()) == a['losses']['loss_bbox'][l]
        total = s * wts[1, l]
        if iou_branch:                               # + the part through the attached IoU target
            i = _dev(d['iou']).requires_grad_(True)
            li = ops.iou_bce_sum(r, i, _dev(d['bt']), _dev(d['bw']), _geom(ops)[0], l, True) * (1.0 / 13.0)
            assert rel(float(li.detach()), a['losses']['losses_iou'][l]) < 1e-6
            total = total + li * wts[2, l]
        total.sum().backward()
        assert _close(a['g_reg'][l], r.grad), l
        if iou_branch:
            assert _close(a['g_iou'][l], i.grad), l
    # A = 9: 4 A = 36, 5 A = 45; 40 / 48-channel rows (alignment padding) and 104-channel rows
    used = (5 if iou_branch else 4) * A
    for pad in (None, (48 if iou_branch else 40) - used, 104 - used):
        b = _run_node(ops, beta, 'nhwc', iou_branch, box, pad=pad, weights=wts)
        for k in a['losses']:
            for x, y in zip(a['losses'][k], b['losses'][k]):
                assert rel(x, y) < 1e-6 or x == y, (pad, k)
        for key in ('g_cls', 'g_reg') + (('g_iou',) if iou_branch else ()):
            for l, (x, y) in enumerate(zip(b[key], a[key])):
                assert _close(x, y), (pad, key, l)
        if pad is not None:
            # (up to 64 trailing channels the kernel writes the zeros itself, grad_rows_start_at_reg; the
            # 104-channel row without the IoU slice has 68, cleared by the node's host fill)
            for g in b['g_pad']:
                assert g.shape[1] == pad and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------ heads and the reference fixture
KEYS = ('loss_cls', 'loss_bbox', 'losses_iou')
BL_CFG = dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5, beta=0.11, loss_weight=1.0)


def _head(iou_branch, **kw):
    from iouaware.head import IoUawareRetinaHead, RetinaHead
    from test_host_targets import HEAD_KW
    cls = IoUawareRetinaHead if iou_branch else RetinaHead
    return cls(**dict(HEAD_KW, loss_bbox=dict(BL_CFG), **kw)).cuda()


def _case(k, iou_branch):
    import gpu_util as G
    f = np.load(os.path.join(GOLD, 'balanced_l1.npz'))
    seed, Bn, ph, pw, ih, iw = [int(v) for v in f['case_%d' % k]]
    cls, reg, iou = synth.head_outputs(seed, Bn, ph, pw, 'A')
    metas = [synth.img_meta(ih, iw, ph, pw) for _ in range(Bn)]
    gts = [torch.from_numpy(f['gt_bboxes_%d_%d' % (k, b)]).cuda() for b in range(Bn)]
    gls = [torch.from_numpy(f['gt_labels_%d_%d' % (k, b)]).cuda() for b in range(Bn)]
    mk = lambda xs: [t.requires_grad_(True) for t in G.to_dev(xs)]     # noqa: E731
    maps = [mk(cls), mk(reg)] + ([mk(iou)] if iou_branch else [])
    return f, _head(iou_branch), metas, gts, gls, maps


@gpu
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou_aware', 'plain'])
def test_head_loss_on_the_node_equals_the_per_level_route(ops, iou_branch):
    from test_host_targets import TRAIN_CFG
    outs = []
    for fuse in (True, False):
        _, head, metas, gts, gls, maps = _case(0, iou_branch)
        assert type(head.loss_bbox).__name__ == 'BalancedL1Loss'
        head.fuse_levels = fuse
        assert bool(head._fused_loss_ok(maps[0])) == fuse
        losses = head.loss(*maps, gts, gls, metas, TRAIN_CFG)
        keys = KEYS[:len(maps)]
        assert sorted(losses) == sorted(keys)
        assert isinstance(losses['loss_bbox'], ops.LevelLosses) == fuse
        w = torch.arange(1, 16, device='cuda', dtype=torch.float32).reshape(3, 5) * 0.25
        sum(w[k, l] * losses[key][l] for k, key in enumerate(keys) for l in range(5)).sum().backward()
        outs.append((losses, [[t.grad for t in m] for m in maps]))
    (la, ga), (lb, gb) = outs
    for k in la:
        for x, y in zip(la[k], lb[k]):
            print(k, float(x), float(y))
            assert x.shape == (1,) and (rel(float(x), float(y)) < 1e-6 or float(x) == float(y)), k
    assert sum(float(v) > 0 for v in la['loss_bbox']) >= 3
    for xs, ys in zip(ga, gb):
        for l, (x, y) in enumerate(zip(xs, ys)):
            assert _close(x, y) and x.dtype == y.dtype, l


@gpu
@pytest.mark.parametrize('device_targets', [True, False])
@pytest.mark.parametrize('case', [0, 1])
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou_aware', 'plain'])
def test_head_loss_against_the_reference_fixture(ops, iou_branch, case, device_targets):
    """both heads with BalancedL1Loss(0.5, 1.5, 0.11) on the fixture inputs, targets from the HIP assigner
    and from the torch path: per-level losses 1e-4 relative, recorded gradient entries 2e-4 of their scale"""
    from test_host_targets import TRAIN_CFG
    f, head, metas, gts, gls, maps = _case(case, iou_branch)
    tag = 'iou' if iou_branch else 'plain'
    if not device_targets:
        head._device_targets_ok = lambda *a: False
    losses = head.loss(*maps, gts, gls, metas, TRAIN_CFG)
    assert isinstance(losses['loss_bbox'], ops.LevelLosses)
    for k in KEYS[:len(maps)]:
        want = f['%s_%s_%d' % (tag, k, case)]
        got = np.array([float(x) for x in losses[k]])
        print(tag, case, device_targets, k, got, want)
        assert np.all(np.abs(got - want) <= 1e-4 * np.maximum(np.abs(want), 1e-6)), k
    sum(sum(v) for v in losses.values()).sum().backward()
    for l in range(5):
        for nm, ts in zip(('cls', 'reg', 'iou'), maps):
            key = '%s_g_%s_%d_%d' % (tag, nm, case, l)
            want = f[key].astype(np.float64)
            got = ts[l].grad.cpu().numpy().reshape(-1)[f[key + '_idx']].astype(np.float64)
            err = np.abs(got - want).max()
            print(key, err, np.abs(want).max())
            assert err <= 2e-4 * max(np.abs(want).max(), 1e-30), key


@gpu
@pytest.mark.parametrize('beta_i', [0, 1])
def test_device_reproduces_the_reference_element_list(ops, beta_i):
    """the reference's weighted_balanced_l1_loss on the planted element list, through the module's (N, 4)
    form: sum 1e-5 relative (the bar of the sums above), gradients 1e-5 |g| + 1e-6 max|g|"""
    from iouaware.losses import BalancedL1Loss
    f = np.load(os.path.join(GOLD, 'balanced_l1.npz'))
    beta = float(f['betas'][beta_i])
    pred, weight = f['el_pred_%d' % beta_i], f['el_weight_%d' % beta_i]
    assert pred.size % 4 == 0
    p = _dev(pred).reshape(-1, 4).requires_grad_(True)
    mod = BalancedL1Loss(alpha=float(f['alpha']), gamma=float(f['gamma']), beta=beta)
    s = mod(p, torch.zeros_like(p), _dev(weight).reshape(-1, 4), avg_factor=1.0)
    s.sum().backward()
    g = np32(p.grad).reshape(-1)
    s = s.detach()
    print(float(s), float(f['el_sum_%d' % beta_i]), np.abs(g - f['el_grad_%d' % beta_i]).max())
    assert rel(float(s), float(f['el_sum_%d' % beta_i])) <= 1e-5
    assert grad_within(g, f['el_grad_%d' % beta_i], 1e-6, 1e-5)
    assert bool((g[(weight == 0) | (pred == 0)] == 0.0).all())


ROUTES = {'module': dict(train_winograd=False, train_bf16=False),
          'winograd': dict(train_winograd=True, train_bf16=False),
          'bf16': dict(train_winograd=True, train_bf16=True)}


@gpu
@pytest.mark.parametrize('route', sorted(ROUTES))
@pytest.mark.parametrize('config', ['retinanet_r50_fpn_1x', 'iou_aware_retinanet_r50_fpn_1x_4gpu'])
def test_one_training_step_with_the_loss_switched_in(config, route):
    """one train_step at 64 x 96 on each training route of both heads: finite losses, a gradient for every
    trainable parameter, the node (not the per-level route) carrying the loss"""
    import json
    import iouaware
    from iouaware import ops as O
    from iouaware.config import ConfigDict
    from iouaware.train import build_optimizer, train_step
    name = 'retina_plain_ref.json' if config.startswith('retinanet') else 'ref_configs.json'
    with open(os.path.join(GOLD, name)) as fh:
        rec = json.load(fh)[config]
    rec['model']['pretrained'] = None
    rec['model']['bbox_head']['loss_bbox'] = dict(BL_CFG)
    torch.manual_seed(0)
    model = iouaware.build_detector(ConfigDict(rec['model']), train_cfg=ConfigDict(rec['train_cfg']),
                                    test_cfg=ConfigDict(rec['test_cfg'])).cuda().train()
    head = model.bbox_head
    assert type(head.loss_bbox).__name__ == 'BalancedL1Loss'
    for k, v in ROUTES[route].items():
        setattr(head, k, v)
    Bn, ph, pw = 2, NODE_PAD[0], NODE_PAD[1]
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(Bn, 3, ph, pw, device='cuda', generator=g)
    gts, gls = synth.train_targets(11, Bn, ph, pw, max_gt=3)
    metas = [synth.img_meta(ph, pw, ph, pw) for _ in range(Bn)]
    seen, real = [], O.head_loss

    def spy(*a, **kw):
        seen.append(kw.get('box_loss'))
        return real(*a, **kw)
    O.head_loss = spy
    try:
        opt = build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001))
        log = train_step(model, opt, img, metas, [torch.from_numpy(x).cuda() for x in gts],
                         [torch.from_numpy(x).cuda() for x in gls])
    finally:
        O.head_loss = real
    assert seen == [('balanced_l1', 0.5, 1.5)], seen
    assert 'loss_bbox' in log and all(v == v and abs(v) != float('inf') for v in log.values()), log
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n

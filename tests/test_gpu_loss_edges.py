"""GPU (MI355X): the anchor-head loss kernels at their edges, against tests/loss_ref.py (float64
torch autograd) -- csrc/loss.hip (k_focal, k_smooth_l1, k_iou_bce, fp32 and bf16 maps, plain and
IoU-balanced) and the all-levels node of csrc/headloss.hip (NCHW and channels-last).

The data is built here (numpy, from seeds) and shared with tests/test_host_loss_ref.py, which
holds the CPU oracle to the same yardstick on the same inputs:

  box / IoU / smooth-L1 levels (box_level): random anchors, about half of them with weight 0,
    and planted among them the anchors of box_specs() -- prediction == target, two tied
    coordinates, nested boxes, disjoint boxes, deltas beyond / exactly at the max_ratio clamp,
    a target beyond the clamp, IoU logits +-40 / +-95, |pred - target| at beta and its fp32
    neighbours, unequal weights (1, 0.5, 0, 2), a weight-0 anchor -- for the (means, stds) sets
    of SETS.  'distinct' has four different stds: in the other three (identity, and the
    (0.1, 0.1, 0.2, 0.2) of real configurations with and without means) stds[2] == stds[3] and
    stds[0] == stds[1], so a swapped index would not show.
  focal levels (focal_level): logits 0, +-40, +-95, +-110 on positive and on negative elements,
    labels on the first and the last class and on both sides of every class-chunk boundary of
    the launch, one position with label weight 0; C in {80, 11, 1}, H*W in {1, 2, 6, 24, 272, 323}
    (scalar path / vector path, one tile / a partial second tile), gamma in {2, 1, 1.5, 3, 0.5}.

Bars.
  * every output is finite wherever the yardstick is (it is everywhere: asserted on the CPU);
    no element is left out of any comparison;
  * "exactly 0" / "exactly 1" (IoU of equal boxes, gradient of a clamped delta, of disjoint boxes,
    of a weight-0 anchor): ==;
  * IoU targets, g_iou, g_box, smooth-L1: bit-identical to the oracle (same exact-math path), and
    against the yardstick 4 x the oracle-against-yardstick error below, at least 1e-6 of the
    tensor's maximum (sums: relative);
  * focal (hardware exp / log / rcp): max(existing gamma = 2 bar, 4 x the error measured on the
    GPU below); gradients 1e-5 |g| + 1e-6 max|g|, sums 1e-5 relative;
  * a bf16 gradient: the fp32 bar plus one bf16 rounding -- it must be the bf16 rounding of a number
    within the fp32 bar of the yardstick (grad_within; one such rounding is up to 2^-8 of the value,
    not 2^-9: bf16 keeps 8 significant bits), and bit-identical to the oracle's value rounded once.

Oracle against yardstick, CPU (tests/test_host_loss_ref.py prints and asserts this table: worst
over the four sets, both levels, the node's five levels, fp32 and bf16-rounded inputs; they are
BOX_MEASURED below, and the fp32 rounding of box corners near 200 px):
    iou targets, absolute      9.7e-7      smooth-L1 sum, relative         1.9e-8
    iou-bce sum, relative      1.2e-7      smooth-L1 g, of max             4.8e-8
    g_iou, of max              9.4e-7      balanced smooth-L1 sum          2.2e-8
    g_box, of max              8.6e-7      balanced smooth-L1 g, of max    1.3e-7
    g_reg = smooth-L1 + g_box  8.0e-7
    focal, gamma 2 / 1 / 1.5 / 3 / 0.5:  g 6.3e-7 / 3.5e-7 / 4.8e-7 / 9.7e-7 / 1.9e-7 of max,
                                         sums 1.5e-8 .. 2.5e-8

Measured on an MI355X, fp32 maps, worst over the whole set (FOCAL_MEASURED below):
                          gamma 2     1        1.5      3        0.5
    k_focal g, of max     3.9e-7   2.9e-7   3.6e-7   5.2e-7   2.8e-7
    k_focal sum, rel      8.0e-8   6.1e-8   9.4e-8   7.9e-8   6.8e-8
  4 x these stay below the gamma = 2 floor, which therefore is the bar for every gamma.
  k_iou_bce / k_smooth_l1 / the node: the oracle's bits; against the yardstick iou targets 7.6e-7,
  g_iou 6.9e-7, g_box 8.6e-7, node g_reg 3.7e-7, node g_iou 4.2e-7.
  Before the fix of focal_elem's general-gamma branch (pt == 0 once exp(-|x|) flushes, |x| > 87.3)
  the gradients at gamma = 1 and gamma = 0.5 held NaN on this set; gamma = 2, 1.5, 3 passed.
"""
import numpy as np
import pytest
import torch

import loss_ref as R
import synth

B, A = 2, synth.A
BETA = 0.11
MAX_RATIO = np.float32(4.135166556742356)

SETS = {
    'identity': ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)),
    'stds': ((0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)),
    'means': ((0.05, -0.02, 0.1, -0.1), (0.1, 0.1, 0.2, 0.2)),
    'distinct': ((0.05, -0.02, 0.1, -0.1), (0.1, 0.15, 0.2, 0.25)),
}
# (h, w, index into synth.STRIDES): one tile of 256 positions; two tiles, odd sizes
BOX_LEVELS = {'2x3': (2, 3, 0), '17x19': (17, 19, 0)}
NODE_PAD = (64, 96)                      # synth.level_shapes -> 96, 24, 6, 2, 1 positions

# the bars of the exact-math outputs: 4 x oracle-against-yardstick (table above), floor 1e-6
BOX_MEASURED = dict(iou=9.7e-7, iou_sum=1.2e-7, g_iou=9.4e-7, g_box=8.6e-7, sl1_sum=1.9e-8,
                    sl1_grad=4.8e-8, sl1b_sum=2.2e-8, sl1b_grad=1.3e-7, g_reg=8.0e-7)


def box_bar(key):
    return max(4.0 * BOX_MEASURED[key], 1e-6)


GAMMAS = (2.0, 1.0, 1.5, 3.0, 0.5)
ALPHA = 0.25
ETAS = (1.5, 1.0)
FOCAL_LOGITS = (0.0, 40.0, -40.0, 95.0, -95.0, 110.0, -110.0)
FOCAL_HW = {1: (1, 1), 2: (1, 2), 6: (2, 3), 24: (4, 6), 272: (16, 17), 323: (17, 19)}
FOCAL_C = (80, 11, 1)
# gamma -> (gradient error as a share of the tensor's maximum, relative error of the sum), GPU
FOCAL_MEASURED = {2.0: (3.9e-7, 8.0e-8), 1.0: (2.9e-7, 6.1e-8), 1.5: (3.6e-7, 9.4e-8), 3.0: (5.2e-7, 7.9e-8),
                  0.5: (2.8e-7, 6.8e-8)}
FOCAL_FINDING = 2.5e-5                  # a measured error above this is a finding, not a bar


def focal_bars(gamma):
    """-> (share of max allowed beside the floor 1e-5 |g| + 1e-6 max, relative bar of the sum)"""
    mg, ms = FOCAL_MEASURED[gamma]
    assert mg <= FOCAL_FINDING and ms <= FOCAL_FINDING
    return 4.0 * mg, max(4.0 * ms, 1e-5)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def _next(v, n):
    v = np.float32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return v


# ------------------------------------------------------------------ box / IoU / smooth-L1 data
def box_specs(means, stds):
    """-> list of (name, pred(4), target(4), iou logit, weights(4), raw).  raw = False: pred /
    target are the deltas AFTER `* std + mean` (what the decode sees), stored as (v - mean) / std
    so that the boxes are the same in every set; raw = True: the stored values themselves."""
    identity = tuple(stds) == (1.0, 1.0, 1.0, 1.0) and tuple(means) == (0.0, 0.0, 0.0, 0.0)
    one = (1.0, 1.0, 1.0, 1.0)
    S = []

    def add(name, pred, tgt, xl, w=one, raw=False):
        S.append((name, tuple(pred), tuple(tgt), float(xl), tuple(w), raw))
    e = (0.13, -0.21, 0.3, -0.17)
    add('equal', e, e, 0.9)                                            # IoU 1, box gradient 0
    add('tie_x', (0.1, 0.2, 0.25, 0.1), (0.1, -0.1, 0.25, 0.3), -0.8)  # x1 and x2 tie, y free
    add('pred_inside', (0.02, -0.03, -0.5, -0.4), (0.0, 0.0, 0.2, 0.1), 1.3)
    add('target_inside', (0.0, 0.0, 0.2, 0.1), (0.02, -0.03, -0.5, -0.4), -1.1)
    add('aside', (10.0, 0.1, 0.0, 0.1), (0.05, 0.0, 0.1, -0.1), 1.7)    # IoU 0, box gradient 0
    # dw clamped at +max_ratio (62.5 anchor widths wide); the left edge lies inside the target
    # and y overlaps partly, so dx, dy, dh keep a gradient
    add('dw_over', (30.95, 0.3, 5.0, 0.1), (0.1, 0.1, 0.2, 0.2), 0.7)
    # dh clamped at -max_ratio (0.016 anchor heights); centred on the target's upper edge
    add('dh_under', (0.3, 0.1 - 0.5 * np.exp(0.2), 0.1, -5.0), (0.1, 0.1, 0.2, 0.2), -0.6)
    # exactly at the bound the gradient passes; representable only with identity means / stds
    add('dw_at_clamp', (0.05, 0.1, float(MAX_RATIO) if identity else 0.9 * float(MAX_RATIO), 0.1),
        (0.0, 0.0, 0.2, 0.1), 0.8)
    add('target_over', (0.1, 0.05, 0.3, 0.1), (0.0, 0.1, 6.0, 0.2), 0.5)
    for xl in (40.0, -40.0, 95.0, -95.0):
        add('xl%+d' % xl, (0.1, -0.05, 0.15, 0.1), (0.0, 0.05, -0.1, 0.2), xl)
    b, z = np.float32(BETA), (0.0, 0.0, 0.0, 0.0)
    add('sl1_weights', (b, -b, 3.0, _next(b, 1)), z, 0.3, (1.0, 0.5, 0.0, 2.0), True)
    add('sl1_b', (-_next(b, 1), -_next(b, -1), _next(b, 2), _next(b, -2)), z, -0.3, one, True)
    add('sl1_c', (-_next(b, 2), -_next(b, -2), 0.0, 3.0), z, 0.2, one, True)
    add('sl1_d', (-3.0, _next(b, -1), b, -b), z, -0.2, one, True)
    add('sl1_w0', (3.0, -3.0, b, 0.05), z, 0.4, z, True)               # weight 0: gradient 0
    return S


_BOX_CACHE = {}


def box_level(h, w, set_name, seed, rot=0, bf16=False):
    """-> dict(reg (B, A*4, h, w), iou (B, A, h, w), bt / bw (B, h*w*A, 4), anchor_iou (B, h*w*A),
    slots {spec name: (b, p, a)}), float32; read-only, cached."""
    key = (h, w, set_name, seed, rot, bf16)
    if key in _BOX_CACHE:
        return _BOX_CACHE[key]
    means, stds = SETS[set_name]
    m64, s64 = np.asarray(means, np.float64), np.asarray(stds, np.float64)
    rs = np.random.RandomState(seed)
    HW = h * w
    N = B * HW * A
    pred = ((rs.standard_normal((N, 4)) * 0.25 - m64) / s64).astype(np.float32)
    tgt = ((rs.standard_normal((N, 4)) * 0.25 - m64) / s64).astype(np.float32)
    xl = (rs.standard_normal(N) * 1.5).astype(np.float32)
    wgt = np.repeat((rs.rand(N) < 0.5).astype(np.float32)[:, None], 4, 1)
    aiou = rs.uniform(0.05, 0.95, N).astype(np.float32)
    specs = box_specs(means, stds)
    nS = len(specs)
    step = max(N // nS, 1)
    if step > 1 and step % A == 0:
        step -= 1                                  # walk through the anchors of a position too
    slots = {}
    edge_iou = (0.0, 1e-30, 0.5, 1.0)
    for k in range(min(nS, N)):
        name, p4, t4, x, w4, raw = specs[(k + rot) % nS]
        n = k * step
        if raw:
            pred[n], tgt[n] = np.asarray(p4, np.float32), np.asarray(t4, np.float32)
        else:
            # equal deltas are stored equal: one expression for both
            pred[n] = ((np.asarray(p4, np.float64) - m64) / s64).astype(np.float32)
            tgt[n] = ((np.asarray(t4, np.float64) - m64) / s64).astype(np.float32)
        xl[n], wgt[n] = x, w4
        aiou[n] = edge_iou[k % 4]                  # the IoU-balanced smooth-L1's anchor IoU
        slots[name] = (n // (HW * A), (n // A) % HW, n % A)
    if bf16:
        pred, tgt, xl = bf16_round(pred), bf16_round(tgt), bf16_round(xl)
    reg = np.ascontiguousarray(pred.reshape(B, h, w, A * 4).transpose(0, 3, 1, 2))
    iou = np.ascontiguousarray(xl.reshape(B, h, w, A).transpose(0, 3, 1, 2))
    out = dict(reg=reg, iou=iou, bt=tgt.reshape(B, HW * A, 4), bw=wgt.reshape(B, HW * A, 4),
               anchor_iou=aiou.reshape(B, HW * A), slots=slots, hw=(h, w))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _BOX_CACHE[key] = out
    return out


def slot_views(d, name, g_box=None, g_iou=None, iou=None):
    """the planted anchor's entries of (B, A*4, h, w) / (B, A, h, w) / (B, N) outputs"""
    b, p, a = d['slots'][name]
    h, w = d['hw']
    y, x = p // w, p % w
    out = []
    if g_box is not None:
        out.append(np.asarray(g_box)[b, 4 * a:4 * a + 4, y, x])
    if g_iou is not None:
        out.append(np.asarray(g_iou)[b, a, y, x])
    if iou is not None:
        out.append(np.asarray(iou).reshape(B, -1)[b, p * A + a])
    return out[0] if len(out) == 1 else out


def weight0_mask(d):
    """(B, A*4, h, w) bool: coordinates of anchors whose four weights are 0"""
    h, w = d['hw']
    z = (d['bw'] == 0).all(-1).reshape(B, h, w, A, 1)
    return np.ascontiguousarray(np.broadcast_to(z, (B, h, w, A, 4)).reshape(B, h, w, A * 4)
                                .transpose(0, 3, 1, 2))


def check_box_exact(d, set_name, iou, g_box, g_iou, fp32, zero_tol=0.0):
    """the == statements of the edge set on one implementation's outputs (zero_tol: the float64
    yardstick's own rounding, as a share of max|g_box|)"""
    s = d['slots']
    gmax = np.abs(np.asarray(g_box, np.float64)).max()

    def zero(v):
        return bool((np.abs(np.asarray(v, np.float64)) <= zero_tol * gmax).all())
    if 'equal' in s:
        assert slot_views(d, 'equal', iou=iou) == 1.0
        assert zero(slot_views(d, 'equal', g_box=g_box))
    if 'aside' in s:
        assert slot_views(d, 'aside', iou=iou) == 0.0
        assert zero(slot_views(d, 'aside', g_box=g_box))
    for name, k in (('dw_over', 2), ('dh_under', 3)):
        if name in s:
            g = slot_views(d, name, g_box=g_box)
            assert g[k] == 0.0, (name, g)
            if fp32:
                assert all(g[j] != 0.0 for j in range(4) if j != k), (name, g)
    if 'dw_at_clamp' in s and set_name == 'identity' and fp32:
        assert slot_views(d, 'dw_at_clamp', g_box=g_box)[2] != 0.0
    assert bool((np.asarray(g_box)[weight0_mask(d)] == 0.0).all())
    assert bool((np.asarray(g_iou)[weight0_mask(d)[:, ::4]] == 0.0).all())


# ------------------------------------------------------------------ focal data
def focal_cchunk(batch, num_anchors, C, HW):
    """classes per wavefront, as launch_focal of csrc/loss.hip picks them"""
    blocks = batch * num_anchors * ((HW + 255) // 256)
    split = max((2048 + blocks - 1) // blocks, 1)
    split = min(split, (C + 7) // 8)
    return ((C + split - 1) // split + 7) // 8 * 8


def focal_labels(C, HW):
    """first and last class, and both sides of every chunk boundary"""
    ch = focal_cchunk(B, A, C, HW)
    labs = [1, C]
    for k in range(1, (C + ch - 1) // ch):
        labs += [k * ch, k * ch + 1]
    return sorted(set(v for v in labs if 1 <= v <= C))


_FOCAL_CACHE = {}


def focal_level(HW, C, bf16=False):
    """-> dict(cls (B, A*C, h, w), labels (B, HW*A) int64, lw, anchor_iou (B, HW*A)); cached."""
    key = (HW, C, bf16)
    if key in _FOCAL_CACHE:
        return _FOCAL_CACHE[key]
    h, w = FOCAL_HW[HW]
    rs = np.random.RandomState(1000 * C + HW)
    N = B * HW * A
    x = (rs.standard_normal((N, C)) * 2.0 - 3.0).astype(np.float32)
    labels = np.zeros(N, np.int64)
    lw = np.ones(N, np.float32)
    aiou = rs.uniform(0.05, 0.95, N).astype(np.float32)
    dead = slice((HW + HW // 2) * A, (HW + HW // 2 + 1) * A)    # image 1, position HW // 2
    lw[dead] = 0.0
    labs, rot = focal_labels(C, HW), HW + C
    nl = len(labs)
    on_pos, on_neg, used = set(), set(), set()
    j = 0
    for n in range(N):
        live = lw[n] != 0.0
        if n % 2 == 0:                                          # every other anchor is positive
            labels[n] = labs[j % nl]
            v = FOCAL_LOGITS[(j + j // nl + rot) % 7]
            x[n, labels[n] - 1] = v
            aiou[n] = (0.0, 0.5, 1.0)[j % 3]
            if live:
                on_pos.add(v)
                used.add(int(labels[n]))
            j += 1
        c = (5 * n + 2) % C
        if c != labels[n] - 1:
            v = FOCAL_LOGITS[(n // 2 + n + rot + 3) % 7]
            x[n, c] = v
            if live:
                on_neg.add(v)
    if HW >= 6:                                                 # enough anchors for all of it
        assert on_pos == set(FOCAL_LOGITS) and used == set(labs), (HW, C)
        assert on_neg == set(FOCAL_LOGITS) or C == 1, (HW, C)
    if bf16:
        x = bf16_round(x)
    cls = np.ascontiguousarray(x.reshape(B, h, w, A * C).transpose(0, 3, 1, 2))
    out = dict(cls=cls, labels=labels.reshape(B, HW * A), lw=lw.reshape(B, HW * A),
               anchor_iou=aiou.reshape(B, HW * A))
    for v in out.values():
        v.setflags(write=False)
    _FOCAL_CACHE[key] = out
    return out


# ------------------------------------------------------------------ comparisons
WORST = {}


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))
    print('%-28s %.3g' % (key, err))


def finite(*arrs):
    return all(bool(np.isfinite(np.asarray(a, np.float64)).all()) for a in arrs)


def share_of_max(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def _to_bf16(a, toward):
    """float64 -> bf16 (as float64), through the fp32 neighbour on the `toward` side so that the
    two roundings cannot land past a correctly rounded fp32 value's"""
    a32 = np.nextafter(np.asarray(a, np.float64).astype(np.float32), np.float32(toward), dtype=np.float32)
    return torch.from_numpy(a32).to(torch.bfloat16).to(torch.float64).numpy()


def grad_within(got, ref, share, rel_elem=0.0, bf16=False):
    """every element: |got - ref| <= tol = share * max|ref| + rel_elem * |ref|.
    bf16: the gradient was rounded to bf16 once on its way back -- `got` must be what that rounding
    makes of SOME number within tol of ref, rd(ref - tol) <= got <= rd(ref + tol) (rounding is
    monotonic).  That is "the fp32 bar plus one bf16 rounding" without an allowance of its own: one
    such rounding moves a number by up to 2^-8 of its size (bf16 keeps 8 significant bits), e.g.
    2.0079e-3 -> 2.0142e-3, 3.1e-3 relative, so a flat 2^-9 |ref| would fail a correctly rounded
    gradient, and 2^-8 |ref| would accept more than one rounding can do."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    tol = share * np.abs(ref).max() + rel_elem * np.abs(ref)
    if bf16:
        return bool(((got >= _to_bf16(ref - tol, -np.inf)) & (got <= _to_bf16(ref + tol, np.inf))).all())
    return bool((np.abs(got - ref) <= tol).all())


def np32(t):
    return t.detach().float().cpu().numpy()


# ------------------------------------------------------------------ GPU tests
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from iouaware import ops as o
    return o


def _level_geom(ops, level, set_name):
    import gpu_util as G
    import oracle
    h, w, li = BOX_LEVELS[level]
    base = G.product_base_anchors()
    base_o = oracle.head_base_anchors(synth.STRIDES)
    assert np.array_equal(base, base_o)
    means, stds = SETS[set_name]
    geom = ops.HeadGeometry([(h, w)], [synth.STRIDES[li]], base[li:li + 1], synth.C, means=means,
                            stds=stds)
    return geom, base_o[li], synth.STRIDES[li]


def _dev(a, bf16=False):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def _same_as_oracle(got, want, bf16):
    """bit for bit (+0 == -0); a bf16 gradient: the oracle's fp32 value rounded once"""
    import gpu_util as G
    if bf16:
        return torch.equal(got.detach().cpu(), torch.from_numpy(want).to(torch.bfloat16))
    return G.same_bits(np32(got), want)


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('level', sorted(BOX_LEVELS))
@pytest.mark.parametrize('set_name', sorted(SETS))
def test_iou_bce_edges(ops, oracle_lib, set_name, level, bf16):
    """k_iou_bce: IoU targets, sum, g_iou, g_box (attached and detached)"""
    h, w, _ = BOX_LEVELS[level]
    d = box_level(h, w, set_name, 11, bf16=bf16)
    geom, base, stride = _level_geom(ops, level, set_name)
    means, stds = SETS[set_name]
    gs = 0.375
    bt, bw = _dev(d['bt']), _dev(d['bw'])
    ref = R.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base, stride, means, stds, gs, True)
    so, tgt_o, gi_o, gb_o = oracle_lib.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base, stride,
                                               means, stds, gscale=gs)
    r = _dev(d['reg'], bf16).requires_grad_(True)
    i = _dev(d['iou'], bf16).requires_grad_(True)
    loss, tgt = ops.iou_bce_sum(r, i, bt, bw, geom, 0, True, return_iou=True)
    (loss * gs).sum().backward()
    t2, s2 = ops.iou_targets(r.detach(), i.detach(), bt, bw, geom, 0)
    torch.cuda.synchronize()
    tgt, gi, gb = np32(tgt), np32(i.grad), np32(r.grad)
    assert finite(tgt, gi, gb, float(loss), float(s2))
    assert torch.equal(t2.cpu(), torch.from_numpy(tgt)) and rel(float(s2), float(loss)) < 1e-6
    tag = 'bf16 ' if bf16 else ''
    e_t = np.abs(tgt.astype(np.float64).reshape(B, -1) - ref['iou'].numpy()).max()
    e_s = rel(float(loss), ref['sum'])
    note(tag + 'iou targets (abs)', e_t)
    note(tag + 'iou-bce sum (rel)', e_s)
    note(tag + 'g_iou (of max)', share_of_max(gi, ref['g_iou']))
    note(tag + 'g_box (of max)', share_of_max(gb, ref['g_box']))
    assert e_t <= box_bar('iou') and e_s <= box_bar('iou_sum')
    assert grad_within(gi, ref['g_iou'], box_bar('g_iou'), bf16=bf16)
    assert grad_within(gb, ref['g_box'], box_bar('g_box'), bf16=bf16)
    # the exact-math path: the oracle's bits
    import gpu_util as G
    assert G.same_bits(tgt, tgt_o)
    assert rel(float(loss), so) < 1e-6
    assert _same_as_oracle(i.grad, gi_o, bf16) and _same_as_oracle(r.grad, gb_o, bf16)
    check_box_exact(d, set_name, tgt, gb, gi, not bf16)
    # detached target: no box gradient, the same g_iou
    r2 = _dev(d['reg'], bf16).requires_grad_(True)
    i2 = _dev(d['iou'], bf16).requires_grad_(True)
    (ops.iou_bce_sum(r2, i2, bt, bw, geom, 0, False) * gs).sum().backward()
    assert r2.grad is None and torch.equal(i2.grad, i.grad)
    refd = R.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base, stride, means, stds, gs, False)
    assert refd['g_box'] is None and grad_within(np32(i2.grad), refd['g_iou'], box_bar('g_iou'), bf16=bf16)


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('level', sorted(BOX_LEVELS))
def test_smooth_l1_edges(ops, oracle_lib, level, bf16):
    """k_smooth_l1 at |pred - target| = beta and its neighbours, with four different weights, and
    its IoU-balanced form at anchor IoU 0, 1e-30, 0.5, 1"""
    h, w, _ = BOX_LEVELS[level]
    d = box_level(h, w, 'distinct', 11, bf16=bf16)
    gs = 0.375
    bt, bw, ai = _dev(d['bt']), _dev(d['bw']), _dev(d['anchor_iou'])
    tag = 'bf16 ' if bf16 else ''
    w0 = weight0_mask(d)
    for delta in (None, 1.5, 0.5, 1.0):
        r = _dev(d['reg'], bf16).requires_grad_(True)
        if delta is None:
            loss = ops.smooth_l1_sum(r, bt, bw, A, BETA)
            ref = R.smooth_l1(d['reg'], d['bt'], d['bw'], A, BETA, gs)
            so, go = oracle_lib.smooth_l1(d['reg'], d['bt'], d['bw'], A, BETA, gscale=gs)
            ks, kg, name = 'sl1_sum', 'sl1_grad', 'smooth-L1'
        else:
            loss = ops.smooth_l1_balanced_sum(r, bt, bw, ai, A, BETA, delta)
            ref = R.smooth_l1(d['reg'], d['bt'], d['bw'], A, BETA, gs, d['anchor_iou'], delta)
            so, go = oracle_lib.smooth_l1_balanced(d['reg'], d['bt'], d['bw'], d['anchor_iou'], A,
                                                   BETA, delta, gscale=gs)
            ks, kg, name = 'sl1b_sum', 'sl1b_grad', 'balanced smooth-L1'
        (loss * gs).sum().backward()
        torch.cuda.synchronize()
        g = np32(r.grad)
        assert finite(g, float(loss))
        note(tag + name + ' sum (rel)', rel(float(loss), ref['sum']))
        note(tag + name + ' g (of max)', share_of_max(g, ref['grad']))
        assert rel(float(loss), ref['sum']) <= box_bar(ks), delta
        assert grad_within(g, ref['grad'], box_bar(kg), bf16=bf16), delta
        assert rel(float(loss), so) < 1e-6 and _same_as_oracle(r.grad, go, bf16), delta
        assert bool((g[w0] == 0.0).all())
        assert bool((slot_views(d, 'sl1_w0', g_box=g) == 0.0).all())
        assert slot_views(d, 'sl1_weights', g_box=g)[2] == 0.0          # weight (1, 0.5, 0, 2)


def _focal_case(ops, f, gamma, bf16, eta):
    """one (level, gamma, eta) through the per-level entry -> (sum, grad fp32 numpy)"""
    c = _dev(f['cls'], bf16).requires_grad_(True)
    lab, lw = _dev(f['labels']), _dev(f['lw'])
    if eta is None:
        loss = ops.focal_loss_sum(c, lab, lw, A, gamma, ALPHA)
    else:
        loss = ops.focal_loss_balanced_sum(c, lab, lw, _dev(f['anchor_iou']), A, gamma, ALPHA, eta)
    (loss * 0.375).sum().backward()
    return float(loss.detach()), np32(c.grad)


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('gamma', GAMMAS)
def test_focal_edges(ops, gamma, bf16):
    """k_focal, GAMMA2 and general gamma, plain and IoU-balanced, on saturating logits"""
    share, sum_bar = focal_bars(gamma)
    worst_g = worst_s = 0.0
    for C in FOCAL_C:
        for HW in sorted(FOCAL_HW):
            f = focal_level(HW, C, bf16)
            h, w = FOCAL_HW[HW]
            for eta in (None,) + ETAS:
                ref = R.focal(f['cls'], f['labels'], f['lw'], A, gamma, ALPHA, 0.375,
                              None if eta is None else f['anchor_iou'], eta)
                assert finite(ref['grad'].numpy(), ref['sum'])
                s, g = _focal_case(ops, f, gamma, bf16, eta)
                torch.cuda.synchronize()
                where = (gamma, C, HW, eta)
                assert finite(g, s), where
                es, eg = rel(s, ref['sum']), share_of_max(g, ref['grad'])
                worst_g, worst_s = max(worst_g, eg), max(worst_s, es)
                ok = grad_within(g, ref['grad'], 1e-6, 1e-5, bf16) or grad_within(g, ref['grad'], share, 0.0, bf16)
                if es > sum_bar or not ok:
                    print('focal %s: sum %.3g (bar %.3g), grad %.3g of max' % (where, es, sum_bar, eg))
                assert es <= sum_bar and ok, where
                dead = (f['lw'] == 0).reshape(B, h, w, A, 1)       # label weight 0: gradient exactly 0
                dead = np.broadcast_to(dead, (B, h, w, A, C)).reshape(B, h, w, A * C).transpose(0, 3, 1, 2)
                assert dead.any() and bool((g[dead] == 0.0).all()), where
    tag = 'bf16 ' if bf16 else ''
    note(tag + 'focal gamma %g g (of max)' % gamma, worst_g)
    note(tag + 'focal gamma %g sum (rel)' % gamma, worst_s)


NODE_SETS = ('stds', 'means', 'distinct')


def node_data(set_name):
    sizes = synth.level_shapes(*NODE_PAD)
    levels = [box_level(h, w, set_name, 20 + l, rot=5 * l) for l, (h, w) in enumerate(sizes)]
    rs = np.random.RandomState(7)
    cls, labels, lw = [], [], []
    for (h, w) in sizes:
        n = h * w * A
        cls.append((rs.standard_normal((B, A * synth.C, h, w)) * 2.0 - 6.0).astype(np.float32))
        lab = np.zeros((B, n), np.int64)
        pos = rs.rand(B, n) < 0.1
        lab[pos] = rs.randint(1, synth.C + 1, int(pos.sum()))
        labels.append(lab)
        lw.append((rs.rand(B, n) > 0.1).astype(np.float32))
    return sizes, levels, cls, labels, lw


@gpu
@pytest.mark.parametrize('channels_last', [False, True], ids=['nchw', 'channels_last'])
@pytest.mark.parametrize('set_name', NODE_SETS)
def test_head_loss_node_edges(ops, set_name, channels_last):
    """the all-levels node (k_box_ml / k_box_nhwc, k_focal_ml / k_focal_nhwc) on the box edge set
    spread over five levels, against the yardstick alone (the per-level kernels run the same
    device functions)"""
    import gpu_util as G
    means, stds = SETS[set_name]
    sizes, levels, cls, labels, lw = node_data(set_name)
    geom, base = G.geometry(NODE_PAD[0], NODE_PAD[1], -1, means, stds)
    assert geom.featmap_sizes == [tuple(s) for s in sizes]
    avg = 13.0

    def maps(xs):
        ts = [_dev(x) for x in xs]
        if channels_last:
            ts = [t.contiguous(memory_format=torch.channels_last) for t in ts]
        return [t.requires_grad_(True) for t in ts]
    c, r, i = maps(cls), maps([d['reg'] for d in levels]), maps([d['iou'] for d in levels])
    out = ops.head_loss(geom, c, r, i, [_dev(x) for x in labels], [_dev(x) for x in lw],
                        [_dev(d['bt']) for d in levels], [_dev(d['bw']) for d in levels],
                        avg_factor=avg, gamma=2.0, alpha=ALPHA, beta=BETA, exact_large_logits=True,
                        channels_last=channels_last)
    sum(v.total for v in out.values()).sum().backward()
    torch.cuda.synchronize()
    seen = set()
    for l, d in enumerate(levels):
        stride = synth.STRIDES[l]
        rb = R.iou_bce(d['reg'], d['iou'], d['bt'], d['bw'], base[l], stride, means, stds, 1.0 / avg)
        rs = R.smooth_l1(d['reg'], d['bt'], d['bw'], A, BETA, 1.0 / avg)
        rf = R.focal(cls[l], labels[l], lw[l], A, 2.0, ALPHA, 1.0 / avg)
        gc, gr, gi = np32(c[l].grad), np32(r[l].grad), np32(i[l].grad)
        lc, lb, li = (float(out[k][l]) for k in ('loss_cls', 'loss_bbox', 'losses_iou'))
        assert finite(gc, gr, gi, lc, lb, li), l
        g_reg = rs['grad'] + rb['g_box']
        note('node smooth-L1 sum (rel)', rel(lb, rs['sum'] / avg))
        note('node iou-bce sum (rel)', rel(li, rb['sum'] / avg))
        note('node g_reg (of max)', share_of_max(gr, g_reg))
        note('node g_iou (of max)', share_of_max(gi, rb['g_iou']))
        assert rel(lb, rs['sum'] / avg) <= box_bar('sl1_sum'), l
        assert rel(li, rb['sum'] / avg) <= box_bar('iou_sum'), l
        assert grad_within(gr, g_reg, box_bar('g_reg')), l
        assert grad_within(gi, rb['g_iou'], box_bar('g_iou')), l
        assert rel(lc, rf['sum'] / avg) <= 1e-5, l
        assert grad_within(gc, rf['grad'], 1e-6, 1e-5), l
        # the == statements; the smooth-L1 part of an anchor's gradient is taken off in float64
        # only where it is 0 anyway (prediction == target) or known exactly
        s = d['slots']
        seen |= set(s)
        w0 = weight0_mask(d)
        assert bool((gr[w0] == 0.0).all()) and bool((gi[w0[:, ::4]] == 0.0).all()), l
        if 'equal' in s:
            assert bool((slot_views(d, 'equal', g_box=gr) == 0.0).all()), l
        if 'sl1_w0' in s:
            assert bool((slot_views(d, 'sl1_w0', g_box=gr) == 0.0).all()), l
    assert seen == set(n for n, *_ in box_specs(means, stds))

"""GPU (MI355X): the FCOS heads' loss kernels at their edges, against tests/point_loss_ref.py (float64
torch autograd, per positive point) -- k_point_box / k_point_box_nhwc / k_point_finalize /
k_point_scale_finalize of csrc/pointloss.hip and the A = 1, unit-weight instances of k_focal_ml /
k_focal_nhwc, through fcos_ops.point_head_loss (NCHW), fcos_ops.point_head_loss_packed (raw rows,
exp(scale x) inside) and the distance form of ia_point_head_loss_*_nhwc.

The data is built here (numpy, from seeds) and shared with tests/test_host_point_loss_ref.py, which
holds the yardstick to the head's torch body and asserts the conditions below on the CPU.

  geometries  'g128' = level_shapes(128, 160): 16x20 (two tiles of 256, the second partial), 8x10, 4x5,
              2x3, 1x2; 'odd': 17x19, 9x10, 5x5, 3x3, 1x2 (no H*W a multiple of 4: the scalar label
              path on every level); batch 2.
  gt boxes    on a 1/8 px grid, reaching outside the padded image (the two coarsest levels need target
              distances above 256 and 512), positives on every level, labels 1 and C among them.
  specs       planted on the positives of every level round-robin (the last positive of a level and
              one slot of the rotation keep random values): `equal` d = t; `tie_x` / `tie_y` two tied coordinates, the
              others at 0.5 t and 2 t; `near_tie` d = t +- 2^-12 on one coordinate; `pred_inside` 0.5 t;
              `target_inside` 2 t; `mixed` (0.5, 2, 2, 0.5) t; `zero` one or all four distances 0 (raw:
              scale x = -110, where expf_ flushes); `huge` d = 2^20 t; `sat` centerness / IoU logits
              from 0, +-40, +-95, +-110 with the class logits of FOCAL_LOGITS on the labelled and on
              another class (every third negative point carries one too).  Located, not planted:
              `centre` (t.x == t.z, t.y == t.w: c == 1), `corner` (a target distance of 1/8: c near 0),
              `raw_tie` (a target distance of exactly 1, met by d = 1 / x = 0).
              In the raw form d = exp(scale x) cannot be put on t: there the tied coordinates of
              `equal`, `tie_*`, `near_tie` sit at 33/32 t (`equal` is then the group `near_equal`),
              and `raw_tie`, `zero` are the exact ones.  bf16 rows: the inputs are rounded first and the
              yardstick sees the rounded values; a tie survives where t is a bf16 number, `equal`
              elsewhere joins `near_equal`.
  single      a batch whose only positive is one point of the last level (n = 1), random or `equal`;
              its second image has no positive.

Metric: per element, relative to the max-abs of the yardstick inside the same spec group, output kind
and level (at least 2^-100: below that an fp32 result has no relative precision left).
Bars.
  * exact (==): the gradient of every non-positive point (the whole image without positives, a level
    without positives), the rows' padding channels as +0 bits, d scale_l of a level without
    positives, the box gradient of `equal` and, through the single-positive batch, u == 1 of `equal`
    (loss_reg == 0);
  * box-kernel outputs (exact-math helpers): max(4 x E_cpu32, 1e-6), E_cpu32 = the error of the head's
    torch body in fp32 on the CPU against the yardstick, per form, kind and group (E_CPU32 below;
    test_host_point_loss_ref.py measures and asserts it); d scale_l: the same bar times sum |g d x|;
  * the loss scalars: relative, max(4 x E_cpu32, 2^-22); loss_cls and the class gradients: the bars
    of test_gpu_loss_edges.focal_bars(2.0) (hardware exp2 / log2 / rcp);
  * a bf16 gradient: the bf16 rounding of a number within the fp32 bar (grad_within);
  * exact_large_logits = 0 documents logits <= 60 (kXMax of csrc/headloss.hip) as its domain: it runs on
    the class maps clipped there, exact_large_logits = 1 on the full set.

Measured on an MI355X, fp32 maps and rows, worst over the whole set in the metric above (MEASURED_GPU
below; in brackets the group, and E_cpu32 of that entry):
                     distance form                        raw form
    d reg            1.1e-6 (tie_y, 2.4e-6)               3.0e-6 (tie_x, 5.7e-5)
    d ctr            5.4e-7 (pred_inside, 5.4e-7)         4.3e-7 (mixed, 8.0e-7)
    d iou            4.9e-7 (mixed, 4.2e-7)               5.7e-7 (tie_y, 9.5e-7)
    d scale          --                                   2.3e-7 of sum |g d x| (1.4e-7)
    d cls, of max    4.2e-7                               4.2e-7
    loss_cls / reg / centerness / iou, relative
                     3.7e-8 / 4.8e-8 / 4.5e-8 / 4.6e-8    7.3e-8 / 6.9e-7 / 8.5e-8 / 2.6e-7
  bf16 rows: every gradient inside grad_within (3.8e-3 of the group's maximum at most: one bf16 rounding),
  losses 2.6e-8 .. 7.0e-8.  No entry is above 25 x its E_cpu32.  The two large E_cpu32 entries (tie_y of the
  distance form, tie_x of the raw form) are groups of one positive per level on which the two parts of
  d / du, -c / (u sum c) and -iou_p / n, nearly cancel under the upstream (1.3, 2.0): the group's maximum is
  small against the rounding of its parts, in the fp32 torch body as in the kernels.
  The box gradient of `equal` is exactly 0 and loss_reg of the single `equal` positive exactly 0 in every run.
  On the parent's kernels (strict > / <: the target's side takes a tie) 31 of the then 40 cases failed, in the
  groups that hold a tie and in no other: `equal`, `tie_x`, `tie_y`, `raw_tie` everywhere, and in the bf16
  distance rows `near_tie`, `near_equal` and one `sat` positive of the odd geometry, whose rounded distances
  land on a (bf16) target distance; relative errors 0.18 .. 1.1, and the `equal` gradient of the order 1e-4 instead of 0.
"""
import functools

import numpy as np
import pytest
import torch

import point_loss_ref as R
import synth_fcos_loss as S
from test_gpu_loss_edges import FOCAL_LOGITS, focal_bars, grad_within

gpu = pytest.mark.gpu
B = 2
C = S.C
UP = (0.7, 1.3, -0.5, 2.0)                  # upstream gradients of (cls, reg, centerness, iou)
GEOMS = {'g128': S.synth_fcos.level_shapes(128, 160), 'odd': [(17, 19), (9, 10), (5, 5), (3, 3), (1, 2)]}
NL = 5
SCALES = np.array([0.5, 1.0, 2.3, 1.0, 0.5], np.float32)
SAT = (0.0, 40.0, -40.0, 95.0, -95.0, 110.0, -110.0)
assert tuple(FOCAL_LOGITS) == SAT
ROT = ('equal', 'tie_x', 'sat0', 'tie_y', 'near_tie', 'sat1', 'pred_inside', 'target_inside', 'sat2', 'mixed',
       'zero1', 'sat3', 'zero4', 'huge', 'sat4', 'random', 'sat5', 'equal', 'sat6', 'near_tie', 'tie_y', 'zero1')
TIE_FAMILY = ('equal', 'tie_x', 'tie_y', 'near_tie')
KEYS = R.KEYS
FLOOR = 2.0 ** -22
TINY = 2.0 ** -100
XMAX0 = 60.0                                # the domain of exact_large_logits = 0


def _gts(single):
    f = lambda rows: np.array(rows, np.float32)   # noqa: E731
    if single:
        # (64, 64) of the last level alone: left = 524.5; every finer level's point inside is out of range
        return [f([[-460.5, 40.25, 100.125, 90.5]]), f([[0.5, 0.5, 3.0, 3.0]])], \
               [np.array([C], np.int64), np.array([3], np.int64)]
    g0 = f([[-500.125, -300.5, 700.25, 400.375],       # level 4
            [-250.5, -200.25, 200.125, 180.75],         # level 3
            [-100.5, -90.25, 150.125, 125.5],           # level 2
            [10.125, 5.5, 140.25, 100.375],             # level 1
            [20.125, 30.25, 75.5, 80.375],              # level 0
            [87.5, 34.75, 112.5, 53.25],                # centred on the level-0 point (100, 44)
            [99.875, 60.5, 130.25, 85.125],             # left = 1/8 at the level-0 points x = 100
            [11.0, 50.5, 40.25, 75.125]])               # left = 1 at the level-0 points x = 12
    l0 = np.array([C, 1, 40, 7, 3, C, 2, 1], np.int64)
    g1 = f([[-400.25, -520.5, 300.125, 200.75],
            [-150.125, -280.5, 230.25, 150.375],
            [-60.5, -130.25, 170.125, 140.5],
            [30.5, 20.125, 150.25, 127.875],
            [60.125, 40.5, 110.25, 95.625],
            [3.0, 2.5, 30.375, 28.125],                 # top = 1.5, left = 1 at the level-0 point (4, 4)
            [118.25, 8.125, 150.5, 36.75]])
    l1 = np.array([1, C, 41, 8, 4, 79, 17], np.int64)
    return [g0, g1], [l0, l1]


def _spec_distances(spec, t, rnd, j, raw):
    """the planted distances (float64) of one positive: t its target, rnd its random distances"""
    tie = 33.0 / 32.0 if raw else 1.0       # the raw form cannot sit on t: beside it instead
    if spec == 'equal':
        return t * tie
    if spec == 'tie_x':
        return t * np.array([tie, 0.5, tie, 2.0])
    if spec == 'tie_y':
        return t * np.array([0.5, tie, 2.0, tie])
    if spec == 'near_tie':
        d = t * np.roll(np.array([tie, 0.5, 2.0, 0.75]), j % 4)
        if not raw:
            d[j % 4] += (1.0 if (j // 4) % 2 else -1.0) * 2.0 ** -12
        return d
    if spec == 'pred_inside':
        return t * 0.5
    if spec == 'target_inside':
        return t * 2.0
    if spec == 'mixed':
        return t * np.array([0.5, 2.0, 2.0, 0.5])
    if spec == 'zero1':
        d = rnd.copy()
        d[j % 4] = 0.0
        return d
    if spec == 'zero4':
        return np.zeros(4)
    if spec == 'huge':
        return t * 2.0 ** 20
    return rnd.copy()


def group_of(spec):
    return spec.rstrip('0123456789')


@functools.lru_cache(maxsize=None)
def edge_case(geom, raw=False, bf16=False, single=None):
    """-> dict: sizes, gb, gl, labels / targets (np_targets), outs = (cls, reg, ctr, iou) per-level NCHW
    fp32 arrays (reg: distances, or raw x with `scales`), scales or None, spec {(l, b, p): name},
    groups {name: [(l, b, p)]}.  single: None | 'random' | 'equal'.  Read-only, cached."""
    sizes = GEOMS[geom]
    gb, gl = _gts(single is not None)
    labels, targets = S.np_targets(sizes, gb, gl)
    seed = 700 + 10 * sorted(GEOMS).index(geom) + (1 if raw else 0)
    cls, reg, ctr, iou = S.synth_fcos.head_outputs(seed, B, sizes)
    rnd = [x.astype(np.float64) for x in reg]
    if raw:                                 # every point's x, so that exp(scale x) is the random distance
        reg = [(np.log(d) / float(s)).astype(np.float32) for d, s in zip(rnd, SCALES)]
    spec, nneg = {}, 0
    for l, (h, w) in enumerate(sizes):
        s = float(SCALES[l])
        bs, ps = np.nonzero(labels[l] > 0)
        for j, (b, p) in enumerate(zip(bs, ps)):
            t = targets[l][b, p].astype(np.float64)
            y, x = p // w, p % w
            if single is not None:
                name = single
            elif t[0] == t[2] and t[1] == t[3]:
                name = 'centre'
            elif t.min() == 0.125:
                name = 'corner'
            elif (t == 1.0).any():
                name = 'raw_tie'
            elif j == len(bs) - 1:
                name = 'random'
            else:
                name = ROT[(j + 5 * l + 3 * sorted(GEOMS).index(geom)) % len(ROT)]
            d = _spec_distances(name, t, rnd[l][b, :, y, x], j, raw)
            if name == 'raw_tie':
                d[t == 1.0] = 1.0
            if raw:
                with np.errstate(divide='ignore'):
                    v = np.where(d > 0, np.log(np.maximum(d, 1e-300)) / s, -110.0 / s)
            else:
                v = d
                assert (v.astype(np.float32) == v).all(), (name, v)
            reg[l][b, :, y, x] = v.astype(np.float32)
            if name.startswith('sat'):
                k = int(name[3:])
                ctr[l][b, 0, y, x], iou[l][b, 0, y, x] = SAT[k], SAT[(k + 3) % 7]
                lab = int(labels[l][b, p])
                cls[l][b, lab - 1, y, x] = SAT[k]
                cls[l][b, (lab + 5) % C, y, x] = SAT[(k + 2) % 7]
            spec[(l, int(b), int(p))] = name
        for b, p in zip(*np.nonzero(labels[l] == 0)):
            if nneg % 3 == 0:
                cls[l][b, (7 * nneg) % C, p // w, p % w] = SAT[(nneg // 3) % 7]
            nneg += 1
    outs = (cls, reg, ctr, iou)
    if bf16:
        outs = tuple([torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy() for x in m] for m in outs)
    # groups from the data: `equal` means four ties (else `near_equal`)
    groups = {}
    for (l, b, p), name in spec.items():
        g = group_of(name)
        if g == 'equal':
            w = sizes[l][1]
            d = outs[1][l][b, :, p // w, p % w]
            if raw or not (d == targets[l][b, p]).all():
                g = 'near_equal'
        groups.setdefault(g, []).append((l, b, p))
    for m in outs:
        for x in m:
            x.setflags(write=False)
    return dict(geom=geom, raw=raw, bf16=bf16, single=single, sizes=sizes, gb=gb, gl=gl, labels=labels,
                targets=targets, outs=outs, scales=SCALES if raw else None, spec=spec, groups=groups)


ALL_CASES = [(g, raw, bf16, None) for g in sorted(GEOMS) for raw in (False, True) for bf16 in (False, True)] + \
            [('g128', raw, False, s) for raw in (False, True) for s in ('random', 'equal')]
MODES = ((True, True), (True, False), (False, True))       # (IoU branch, attach_iou_target)


def clipped(case):
    """the class maps inside the domain of exact_large_logits = 0"""
    c = dict(case)
    c['outs'] = ([np.minimum(x, np.float32(XMAX0)) for x in case['outs'][0]],) + tuple(case['outs'][1:])
    return c


_YARD = {}


def yardstick(case, with_iou, attach, clip=False):
    """-> losses {key: float}, grads {key: {kind: [L] maps | 'scale': (L,)}}, pos, raw result; cached"""
    key = (case['geom'], case['raw'], case['bf16'], case['single'], with_iou, attach, clip)
    if key not in _YARD:
        c = clipped(case) if clip else case
        _YARD[key] = R.yardstick_maps(c['sizes'], c['labels'], c['targets'], c['outs'], c['scales'], attach,
                                      with_iou)
    return _YARD[key]


def torch_body(case, with_iou, attach, dtype):
    """the head's torch `_loss` body on the CPU in `dtype` (one-hot focal formula), exp(scale x) inside
    the graph for the raw form -> losses, grads as `yardstick`"""
    n = 4 if with_iou else 3
    leaves = [[torch.from_numpy(np.array(x)).to(dtype).requires_grad_(True) for x in m] for m in case['outs'][:n]]
    sc = None
    outs = list(leaves)
    if case['raw']:
        sc = [torch.tensor([float(s)], dtype=dtype, requires_grad=True) for s in SCALES]
        outs[1] = [(s * x).exp() for s, x in zip(sc, leaves[1])]
    head = S.make_head(with_iou, False)
    with S.torch_route(cpu_focal=True, detach_iou_target=not attach):
        losses = S.head_loss(head, outs, [torch.from_numpy(b).to(dtype) for b in case['gb']],
                             [torch.from_numpy(x) for x in case['gl']])
    flat = [t for m in leaves for t in m] + (sc or [])
    grads = {}
    for k, v in losses.items():
        gs = torch.autograd.grad(v.sum(), flat, allow_unused=True, retain_graph=True)
        gs = [np.zeros(tuple(t.shape)) if g is None else g.detach().double().numpy() for g, t in zip(gs, flat)]
        grads[k] = {kind: gs[i * NL:(i + 1) * NL] for i, kind in enumerate(('cls', 'reg', 'ctr', 'iou')[:n])}
        if sc:
            grads[k]['scale'] = np.array([float(g.sum()) for g in gs[n * NL:]])
    return {k: float(v.detach().double().sum()) for k, v in losses.items()}, grads


# ------------------------------------------------------------------ the per-element metric
def group_values(case, maps, kind, name, l):
    """the (n, ch) entries of one kind's level map at the positives of a group, or None"""
    idx = [(b, p) for (ll, b, p) in case['groups'].get(name, ()) if ll == l]
    if not idx:
        return None
    m = np.asarray(maps[kind][l], np.float64)
    m = m.reshape(m.shape[0], m.shape[1], -1)
    b, p = np.array(idx).T
    return m[b, :, p]


def group_errors(case, got, ref, kinds):
    """-> {(kind, group): worst over the levels of max |got - ref| / max(max |ref|, 2^-100) inside
    (group, kind, level)}.  ('reg', 'equal') is left out: it is an exact statement."""
    out = {}
    for kind in kinds:
        for name in case['groups']:
            if (kind, name) == ('reg', 'equal'):
                continue
            for l in range(NL):
                r = group_values(case, ref, kind, name, l)
                if r is None:
                    continue
                g = group_values(case, got, kind, name, l)
                e = float(np.abs(g - r).max() / max(np.abs(r).max(), TINY))
                out[(kind, name)] = max(out.get((kind, name), 0.0), e)
    return out


def scale_terms(case, ref_grads):
    """sum |g d x| per level: (the yardstick's raw-reg gradient) * x / scale_l, absolute values summed"""
    return np.array([float(np.abs(ref_grads['reg'][l] * case['outs'][1][l].astype(np.float64)).sum()) /
                     float(SCALES[l]) for l in range(NL)])


def form(case):
    return 'raw' if case['raw'] else 'dist'


# E_cpu32: the head's torch body in fp32 on the CPU against the yardstick, worst over the geometries, the
# levels, the three (IoU branch, attach) modes, fp32 and bf16-rounded inputs and the single-positive
# batches (tests/test_host_point_loss_ref.py::test_e_cpu32_table prints and asserts it)
E_CPU32 = {
    ('dist', 'ctr', 'centre'): 1.4e-7,
    ('dist', 'ctr', 'corner'): 7.8e-8,
    ('dist', 'ctr', 'equal'): 5.2e-7,
    ('dist', 'ctr', 'huge'): 1.9e-7,
    ('dist', 'ctr', 'mixed'): 1.4e-7,
    ('dist', 'ctr', 'near_equal'): 1.3e-6,
    ('dist', 'ctr', 'near_tie'): 1.4e-7,
    ('dist', 'ctr', 'pred_inside'): 5.4e-7,
    ('dist', 'ctr', 'random'): 2.4e-7,
    ('dist', 'ctr', 'raw_tie'): 1.3e-7,
    ('dist', 'ctr', 'sat'): 8.4e-8,
    ('dist', 'ctr', 'target_inside'): 1.2e-7,
    ('dist', 'ctr', 'tie_x'): 3.9e-7,
    ('dist', 'ctr', 'tie_y'): 2.0e-7,
    ('dist', 'ctr', 'zero'): 4.4e-7,
    ('dist', 'iou', 'centre'): 1.1e-7,
    ('dist', 'iou', 'corner'): 9.0e-8,
    ('dist', 'iou', 'equal'): 1.6e-7,
    ('dist', 'iou', 'huge'): 1.2e-7,
    ('dist', 'iou', 'mixed'): 4.2e-7,
    ('dist', 'iou', 'near_equal'): 7.9e-7,
    ('dist', 'iou', 'near_tie'): 2.5e-7,
    ('dist', 'iou', 'pred_inside'): 1.7e-7,
    ('dist', 'iou', 'random'): 2.7e-7,
    ('dist', 'iou', 'raw_tie'): 1.5e-7,
    ('dist', 'iou', 'sat'): 1.8e-7,
    ('dist', 'iou', 'target_inside'): 1.7e-7,
    ('dist', 'iou', 'tie_x'): 3.7e-7,
    ('dist', 'iou', 'tie_y'): 4.9e-7,
    ('dist', 'iou', 'zero'): 1.4e-7,
    ('dist', 'reg', 'centre'): 1.3e-7,
    ('dist', 'reg', 'corner'): 3.1e-7,
    ('dist', 'reg', 'huge'): 1.7e-7,
    ('dist', 'reg', 'mixed'): 6.0e-7,
    ('dist', 'reg', 'near_equal'): 2.3e-7,
    ('dist', 'reg', 'near_tie'): 2.7e-7,
    ('dist', 'reg', 'pred_inside'): 2.3e-7,
    ('dist', 'reg', 'random'): 5.6e-7,
    ('dist', 'reg', 'raw_tie'): 2.6e-7,
    ('dist', 'reg', 'sat'): 4.4e-7,
    ('dist', 'reg', 'target_inside'): 1.4e-7,
    ('dist', 'reg', 'tie_x'): 1.8e-7,
    ('dist', 'reg', 'tie_y'): 2.4e-6,
    ('dist', 'reg', 'zero'): 2.3e-7,
    ('raw', 'ctr', 'centre'): 7.3e-8,
    ('raw', 'ctr', 'corner'): 9.6e-8,
    ('raw', 'ctr', 'huge'): 1.6e-7,
    ('raw', 'ctr', 'mixed'): 8.0e-7,
    ('raw', 'ctr', 'near_equal'): 1.8e-7,
    ('raw', 'ctr', 'near_tie'): 1.5e-7,
    ('raw', 'ctr', 'pred_inside'): 1.4e-7,
    ('raw', 'ctr', 'random'): 3.7e-7,
    ('raw', 'ctr', 'raw_tie'): 1.2e-7,
    ('raw', 'ctr', 'sat'): 8.4e-8,
    ('raw', 'ctr', 'target_inside'): 1.6e-7,
    ('raw', 'ctr', 'tie_x'): 1.6e-7,
    ('raw', 'ctr', 'tie_y'): 4.1e-7,
    ('raw', 'ctr', 'zero'): 4.1e-7,
    ('raw', 'iou', 'centre'): 1.1e-7,
    ('raw', 'iou', 'corner'): 9.3e-8,
    ('raw', 'iou', 'huge'): 8.1e-8,
    ('raw', 'iou', 'mixed'): 9.1e-7,
    ('raw', 'iou', 'near_equal'): 6.8e-7,
    ('raw', 'iou', 'near_tie'): 4.7e-7,
    ('raw', 'iou', 'pred_inside'): 3.3e-7,
    ('raw', 'iou', 'random'): 3.1e-7,
    ('raw', 'iou', 'raw_tie'): 1.6e-7,
    ('raw', 'iou', 'sat'): 2.1e-7,
    ('raw', 'iou', 'target_inside'): 2.2e-7,
    ('raw', 'iou', 'tie_x'): 3.6e-7,
    ('raw', 'iou', 'tie_y'): 9.5e-7,
    ('raw', 'iou', 'zero'): 1.8e-7,
    ('raw', 'reg', 'centre'): 1.6e-7,
    ('raw', 'reg', 'corner'): 3.7e-7,
    ('raw', 'reg', 'huge'): 4.8e-7,
    ('raw', 'reg', 'mixed'): 6.8e-7,
    ('raw', 'reg', 'near_equal'): 3.3e-7,
    ('raw', 'reg', 'near_tie'): 5.0e-7,
    ('raw', 'reg', 'pred_inside'): 3.4e-7,
    ('raw', 'reg', 'random'): 2.6e-7,
    ('raw', 'reg', 'raw_tie'): 2.5e-7,
    ('raw', 'reg', 'sat'): 3.7e-7,
    ('raw', 'reg', 'target_inside'): 2.3e-7,
    ('raw', 'reg', 'tie_x'): 5.7e-5,
    ('raw', 'reg', 'tie_y'): 4.8e-7,
    ('raw', 'reg', 'zero'): 4.3e-7,
    ('raw', 'scale', 'all'): 1.4e-7,
}
E_CPU32_LOSS = {
    ('dist', 'loss_centerness'): 7.0e-8,
    ('dist', 'loss_cls'): 7.9e-8,
    ('dist', 'loss_iou'): 1.2e-7,
    ('dist', 'loss_reg'): 6.8e-8,
    ('raw', 'loss_centerness'): 9.4e-8,
    ('raw', 'loss_cls'): 7.0e-8,
    ('raw', 'loss_iou'): 4.5e-7,
    ('raw', 'loss_reg'): 7.0e-7,
}

MEASURED_GPU = {('dist', 'reg'): 1.1e-6, ('dist', 'ctr'): 5.4e-7, ('dist', 'iou'): 4.9e-7, ('raw', 'reg'): 3.0e-6,
                ('raw', 'ctr'): 4.3e-7, ('raw', 'iou'): 5.7e-7, ('raw', 'scale'): 2.3e-7, ('dist', 'cls'): 4.2e-7,
                ('raw', 'cls'): 4.2e-7, ('dist', 'loss'): 4.8e-8, ('raw', 'loss'): 6.9e-7}


def bar(form_, kind, name):
    return max(4.0 * E_CPU32.get((form_, kind, name), 0.0), 1e-6)


def loss_bar(form_, key):
    return max(4.0 * E_CPU32_LOSS.get((form_, key), 0.0), FLOOR)


WORST = {}


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))


@pytest.fixture(scope='module', autouse=True)
def _table():
    yield
    if WORST:
        print('\nworst observed per kind')
        for k in sorted(WORST):
            print('    %-44s %.3g' % (k, WORST[k]))


# ------------------------------------------------------------------ GPU side
DEV = 'cuda:0'


def _dev(xs):
    return [torch.from_numpy(np.array(x)).to(DEV) for x in xs]


def _gpu_targets(case):
    from iouaware import fcos_ops
    geom = fcos_ops.PointGeometry(case['sizes'], S.STRIDES, C)
    assert fcos_ops.point_loss_supported(geom, B)
    lab, tgt, counts = fcos_ops.point_targets(geom, _dev(case['gb']), _dev(case['gl']), S.RANGES)
    for l in range(NL):                     # the yardstick's targets are the kernels' targets
        assert np.array_equal(lab[l].cpu().numpy(), case['labels'][l])
        assert np.array_equal(tgt[l].cpu().numpy().view(np.uint32), case['targets'][l].view(np.uint32))
    return geom, lab, tgt, counts


def _within(got, ref, tol, bf16):
    m = float(np.abs(ref).max())
    if m == 0.0:                            # one bf16 rounding moves a number by up to 2^-8 of its size
        return bool((np.abs(got) <= tol * (1.0 + 2.0 ** -8 if bf16 else 1.0)).all())
    return grad_within(got, ref, tol / m, 0.0, bf16)


def judge(tag, case, with_iou, attach, losses, maps, bf16=False, clip=False):
    """losses {key: float} and gradient maps {kind: [L] (B, ch, H, W)} (+ 'scale') of one node run
    with upstream UP against the yardstick: every bar of the module docstring"""
    v64, g64, pos, _ = yardstick(case, with_iou, attach, clip)
    ref = R.combine(g64, UP)
    f = ('bf16 ' if bf16 else '') + form(case)
    kinds = ('reg', 'ctr', 'iou')[:3 if with_iou else 2]
    fails = []
    n = len(pos['b'])
    for k in v64:
        got = losses[k]
        assert np.isfinite(got), (tag, k)
        if n == 0 and k != 'loss_cls':
            assert got == 0.0
            continue
        e = abs(got - v64[k]) / max(abs(v64[k]), 1e-300) if v64[k] != 0.0 else abs(got)
        note('%s %s (rel)' % (f, k), e)
        lim = focal_bars(2.0)[1] if k == 'loss_cls' else loss_bar(form(case), k)
        if e > lim:
            fails.append('%s %s: %.3g above %.3g' % (tag, k, e, lim))
    share, _ = focal_bars(2.0)
    for l in range(NL):
        g, r = np.asarray(maps['cls'][l], np.float64), ref['cls'][l]
        assert np.isfinite(g).all(), (tag, 'cls', l)
        note('%s d cls (of max)' % f, np.abs(g - r).max() / np.abs(r).max())
        if not (grad_within(g, r, 1e-6, 1e-5, bf16) or grad_within(g, r, share, 0.0, bf16)):
            fails.append('%s d cls[%d]: %.3g of max' % (tag, l, np.abs(g - r).max() / np.abs(r).max()))
    for kind in kinds:
        for l, (h, w) in enumerate(case['sizes']):
            g = np.asarray(maps[kind][l], np.float64)
            assert np.isfinite(g).all(), (tag, kind, l)
            neg = np.broadcast_to((case['labels'][l] == 0).reshape(B, 1, h, w), g.shape)
            assert bool((g[neg] == 0.0).all()), '%s d %s[%d]: a non-positive point has a gradient' % (tag, kind, l)
            seen = 0
            for name in case['groups']:
                r = group_values(case, ref, kind, name, l)
                if r is None:
                    continue
                gg = group_values(case, maps, kind, name, l)
                seen += len(r)
                if (kind, name) == ('reg', 'equal'):
                    if not bool((gg == 0.0).all()):
                        fails.append('%s d reg[%d] equal: %s, not 0' % (tag, l, gg.ravel()[:4]))
                    continue
                scale = max(float(np.abs(r).max()), TINY)
                e = float(np.abs(gg - r).max()) / scale
                note('%s d %s %s' % (f, kind, name), e)
                lim = bar(form(case), kind, name)
                if not _within(gg, r, lim * scale, bf16):
                    fails.append('%s d %s[%d] %s: %.3g above %.3g' % (tag, kind, l, name, e, lim))
            assert seen == int((case['labels'][l] > 0).sum()), 'a positive was left out'
    if case['raw']:
        terms = scale_terms(case, ref)
        for l in range(NL):
            got = float(maps['scale'][l])
            if not (case['labels'][l] > 0).any():
                assert got == 0.0 and ref['scale'][l] == 0.0, (tag, l, got)
                continue
            e = abs(got - ref['scale'][l]) / terms[l]
            note('raw d scale (of sum |g d x|)', e)
            if e > bar('raw', 'scale', 'all'):
                fails.append('%s d scale[%d]: %.3g above %.3g' % (tag, l, e, bar('raw', 'scale', 'all')))
    if case['single'] == 'equal' and not case['raw']:
        assert losses['loss_reg'] == 0.0, 'u of `equal` is not exactly 1'
    assert not fails, '\n'.join(fails)


NCHW_CASES = [c for c in ALL_CASES if not c[1] and not c[2]]


@gpu
@pytest.mark.parametrize('big', [1, 0], ids=['exact_large', 'clipped'])
@pytest.mark.parametrize('with_iou,attach', MODES, ids=['iou-attached', 'iou-detached', 'plain'])
@pytest.mark.parametrize('cid', NCHW_CASES, ids=lambda c: '%s%s' % (c[0], '-single-' + c[3] if c[3] else ''))
def test_nchw_node(cid, with_iou, attach, big):
    """fcos_ops.point_head_loss on the distance form, upstream UP"""
    from iouaware import fcos_ops
    case = edge_case(*cid)
    run = clipped(case) if not big else case
    geom, lab, tgt, counts = _gpu_targets(case)
    n = 4 if with_iou else 3
    outs = [[t.requires_grad_(True) for t in _dev(m)] for m in run['outs'][:n]]
    losses = fcos_ops.point_head_loss(geom, outs[0], outs[1], outs[2], outs[3] if with_iou else None, lab, tgt,
                                      counts, 2.0, 0.25, attach_iou_target=attach, exact_large_logits=bool(big))
    assert list(losses) == list(KEYS[:n])
    flat = [t for m in outs for t in m]
    gs = torch.autograd.grad(sum(u * v.sum() for u, v in zip(UP, losses.values())), flat)
    torch.cuda.synchronize()
    maps = {kind: [g.double().cpu().numpy() for g in gs[i * NL:(i + 1) * NL]]
            for i, kind in enumerate(('cls', 'reg', 'ctr', 'iou')[:n])}
    judge('nchw/%s/%s' % (cid[0], cid[3]), case, with_iou, attach, {k: float(v.detach()) for k, v in losses.items()},
          maps, clip=not big)


ROW_WIDTHS = {'f32': (torch.float32, 84, 8), 'bf16': (torch.bfloat16, 96, 32), 'f32-tight': (torch.float32, 88, 4)}


def _row_params(raw):
    out = []
    for c in ALL_CASES:
        if c[1] != raw:
            continue
        for rows in ('bf16',) if c[2] else ('f32', 'f32-tight'):
            for with_iou in (True, False):
                if (rows == 'f32-tight' and with_iou) or (rows == 'f32' and not with_iou and not c[3]):
                    continue                            # a 4-wide reg row has no IoU channel; fp32 plain: there
                out.append(pytest.param(c, rows, with_iou, id='%s%s-%s-%s' % (
                    c[0], '-single-' + c[3] if c[3] else '', rows, 'iou' if with_iou else 'plain')))
    return out


def _padding_is_plus_zero(rows, real):
    bits = torch.int16 if rows.dtype == torch.bfloat16 else torch.int32
    return rows.shape[-1] == real or not bool(rows[..., real:].contiguous().view(bits).any())


@gpu
@pytest.mark.parametrize('cid,rows,with_iou', _row_params(True))
def test_packed_rows_raw(cid, rows, with_iou):
    """fcos_ops.point_head_loss_packed: raw regression rows, scales 0.5 / 1 / 2.3 per level"""
    import gpu_util as G
    from iouaware import fcos_ops
    case = edge_case(*cid)
    dtype, wc, wr = ROW_WIDTHS[rows]
    geom, lab, tgt, counts = _gpu_targets(case)
    cc, ri = G.point_rows(case['outs'], with_iou, dtype, wc, wr, C)
    cc = [t.permute(0, 3, 1, 2).requires_grad_(True) for t in cc]
    ri = [t.permute(0, 3, 1, 2).requires_grad_(True) for t in ri]
    sc = [torch.tensor([float(s)], device=DEV, requires_grad=True) for s in SCALES]
    losses = fcos_ops.point_head_loss_packed(geom, cc, ri, sc, lab, tgt, counts, 2.0, 0.25, attach_iou_target=True,
                                             exact_large_logits=True, with_iou=with_iou)
    gs = torch.autograd.grad(sum(u * v.sum() for u, v in zip(UP, losses.values())), cc + ri + sc)
    torch.cuda.synchronize()
    g_cc = [g.permute(0, 2, 3, 1) for g in gs[:NL]]
    g_ri = [g.permute(0, 2, 3, 1) for g in gs[NL:2 * NL]]
    for l in range(NL):
        assert g_cc[l].dtype == dtype and g_ri[l].dtype == dtype
        assert _padding_is_plus_zero(g_cc[l], C + 1) and _padding_is_plus_zero(g_ri[l], 5 if with_iou else 4), l
    maps = G.point_row_maps((g_cc, g_ri, torch.cat([g.reshape(1) for g in gs[2 * NL:]])), with_iou, C)
    judge('packed/%s/%s/%s' % (cid[0], cid[3], rows), case, with_iou, True,
          {k: float(v.detach()) for k, v in losses.items()}, maps, bf16=dtype == torch.bfloat16)


@gpu
@pytest.mark.parametrize('cid,rows,with_iou', _row_params(False))
def test_distance_rows(cid, rows, with_iou):
    """ia_point_head_loss_*_nhwc with reg_scale NULL: the rows hold the distances"""
    import gpu_util as G
    case = edge_case(*cid)
    dtype, wc, wr = ROW_WIDTHS[rows]
    _gpu_targets(case)
    node = G.PointRowsNode(case['sizes'], S.STRIDES, C, S.RANGES, case['gb'], case['gl'], with_iou, case['outs'],
                           dtype, wc, wr, None, cfg=(2.0, 0.25, 1, 1))
    res, grads = node.run_upstream(UP)
    for l in range(NL):
        assert _padding_is_plus_zero(grads[0][l], C + 1) and _padding_is_plus_zero(grads[1][l], 5 if with_iou else 4), l
    maps = G.point_row_maps(grads, with_iou, C)
    judge('rows/%s/%s/%s' % (cid[0], cid[3], rows), case, with_iou, True,
          {k: float(res[i]) for i, k in enumerate(KEYS[:4 if with_iou else 3])}, maps, bf16=dtype == torch.bfloat16)

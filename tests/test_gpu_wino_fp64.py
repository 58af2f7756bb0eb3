"""GPU (MI355X): the Winograd F(4x4,3x3) transforms (csrc/wino.hip) and the training node
`winograd_train.wino_conv_levels` against an fp64 yardstick (tests/wino_ref.py).

1. Transforms, element by element.  `ia_wino_input_transform`, `ia_wino_grad_output_transform` and
   `ia_wino_output_transform` against their fp64 definitions under a DERIVED bound.  With
   u = 2^-24 and the library built with -ffp-contract=off, the longest chain of roundings through
   one 1-D pass is 3 (recounted against wino.hip; multiplications by 2, 4, 8 are exact):
     bt6  o[0] = (4 d0 - 5 d2) + d4     5 d2 | the difference | + d4          3   (o[5] alike)
          o[1] = (d3 + d4) - 4 (d1 + d2)  the sums | the difference            2   (o[2..4] alike)
     at6  o[0] = (m0 + s12) + s34       s12 | + m0 | + s34                     3
          o[3] = (d12 + 8 d34) + m5     d34 | + d12 | + m5                     3   (o[1], o[2]: 2)
     a6   o[3] = t02 + t13              t02, t13 | the sum                     2
   Two passes give (1 + u)^6 - 1 on the absolute-value product, the bias one more rounding: 7u.
   Hence, componentwise and evaluated in fp64,
     |got - ref| <= 8u (|B^T| |d| |B|)     resp.  8u (|A| |dy| |A^T|),  8u (|A^T| |M| |A| + |bias|)
   and for the pre-activation relu?(x s + t), two roundings, 2u (|x s| + |t|) pushed through
   |B^T| . |B| on top (ReLU is 1-Lipschitz).  Where the bound is 0 the result must be exactly 0.
   Outputs are pre-filled with NaN and followed by a NaN guard: every element is written, nothing
   behind the buffer and no destination channel outside the segments is.

2. The node against fp64 autograd (`F.conv2d` on .double() copies, on the GPU): every y_l, dx_l,
   dW, db as max|got - ref| / max|ref| through
     gate A  <= 1e-4 (the project's contract), and
     gate B  <= 4 x the same figure of the fp32 helper (tests/wino_ref.py, evaluated on the CPU:
             independent code and an independent GEMM) on the same tensors; why 4 and not the 2
             it started at is written next to wino_ref.GATE_B,
   at the training configuration (batch 4, five levels of 800 x 1344, T = 5 720 tiles), the
   backbone's single-level shapes and odd geometries; with ReLU element-wise (upstream gradient
   zeroed where the fp64 pre-activation is within gate A's tolerance of zero, so no mask flip can
   move a gradient).  tests/test_host_wino_ref.py shows on the CPU that 16-bit GEMM operands fail
   gate B and structural faults fail gate A; two sensitivity tests repeat that through the HIP
   route.

Measured on an MI355X (HIP error / fp32-helper error, ratio), full-size cases:
                                       y                 dx                dW                db
  five levels b4 256->256   1.71e-5/9.10e-6 1.88  1.81e-5/8.94e-6 2.02  9.53e-6/7.17e-6 1.33  1.47e-7/1.57e-7 0.93
  five levels b4 256->720   1.72e-5/1.19e-5 1.44  2.47e-5/9.28e-6 2.66  1.31e-5/6.26e-6 2.09  1.59e-7/1.50e-7 1.07
  five levels b4 256->48    1.43e-5/8.89e-6 1.61  7.79e-6/8.94e-6 0.87  9.76e-6/6.24e-6 1.57  -
  the same, 256->256 + ReLU 1.57e-5/8.90e-6 1.76  1.81e-5/1.17e-5 1.55  9.77e-6/5.90e-6 1.66  1.59e-7/2.03e-7 0.78
  64 @ 200x336, batch 4     7.94e-6/7.60e-6 1.04  8.91e-6/8.34e-6 1.07  1.12e-5/8.40e-6 1.33  2.28e-7/1.61e-7 1.42
  128 @ 100x168             1.05e-5/1.01e-5 1.05  1.00e-5/1.07e-5 0.94  1.28e-5/5.67e-6 2.25  1.60e-7/1.88e-7 0.85
  256 @ 50x84               1.27e-5/9.21e-6 1.38  1.32e-5/8.38e-6 1.57  1.66e-5/6.63e-6 2.50  1.39e-7/1.02e-7 1.36
  512 @ 25x42               2.25e-5/8.49e-6 2.66  1.97e-5/9.92e-6 1.99  1.04e-5/7.16e-6 1.45  1.53e-7/1.43e-7 1.06
Worst ratio over all cases: y 2.66, dx 2.66, dW 2.50, db 2.39 (12 -> 4 channels on levels smaller
than a tile: 1.4e-7 against 5.7e-8, both at the last bit).  Before the weight-gradient reduction
was cut into slices (winograd_train.weight_grad_product) dW stood at 2.56e-5 / 4.33e-5 / 2.48e-5
(3.6 / 6.9 / 4.0 x) in the first three rows and 2.55e-5 (4.5 x) at 128 @ 100x168.  Sensitivity,
256->48 at five levels: gemm_tn operands cut to 16 bits dW 1.88e-4 (30 x), last tile lost
1.04e-2.  Transforms: the worst |error| / bound over the 106 cases is 0.47.  The file runs in
about 12 s.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import wino_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')
GUARD = 4096

TRAIN5 = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]      # 800 x 1344, strides 8 .. 128
THREE = [(37, 53), (19, 27), (5, 3)]
# name -> (batch, sizes).  tail13 / tail177: T is a multiple neither of 8 (the XCD remap) nor of
# any tiles-per-wavefront count (64, 21, 7, 5, 4, 2): the last wavefront is partly filled
LEVELS = {
    'train5': (4, TRAIN5),
    'one': (2, [(200, 336)]),
    'three': (2, THREE),
    'unit': (1, [(1, 1)]),
    'odd': (3, [(3, 2), (1, 7)]),
    'tail13': (1, [(9, 13), (3, 2)]),
    'tail177': (1, THREE),
}
CHANNELS = [4, 12, 36, 48, 64, 128, 256, 260, 512, 720]


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _plan(key):
    from iouaware import winograd as W
    batch, sizes = LEVELS[key]
    plan = W._Plan(sizes, batch, torch.device('cuda'))
    assert plan.T == R.tile_count(sizes, batch)
    return plan, batch, sizes


def _guarded(shape):
    """NaN-filled contiguous tensor of `shape` with a NaN guard behind it"""
    n = math.prod(shape)
    flat = torch.full((n + GUARD,), NAN, device='cuda')
    return flat[:n].view(*shape), flat[n:]


def _guarded_cl(batch, c, h, w):
    """the same for a channels-last (batch, c, h, w) activation"""
    t, guard = _guarded((batch, h, w, c))
    return t.permute(0, 3, 1, 2), guard


def _where_tile(key, flat, shape, groups=1):
    """flat index into (groups * 36, T, Cg) -> readable position"""
    batch, sizes = LEVELS[key]
    k, rem = divmod(int(flat), shape[1] * shape[2])
    t, c = divmod(rem, shape[2])
    l, b, ty, tx = R.tile_index(sizes, batch, t)
    return 'matrix %d (group %d, k %d) tile %d = level %d image %d tile (%d, %d), channel %d' % (
        k, k // 36, k % 36, t, l, b, ty, tx, (k // 36) * shape[2] + c)


def _check_tiles(key, got, ref, bound, guard, groups=1):
    assert got.shape == ref.shape
    assert not bool(torch.isnan(got).any()), 'elements never written: first at ' + _where_tile(
        key, torch.isnan(got).flatten().nonzero()[0], got.shape, groups)
    assert bool(torch.isnan(guard).all()), 'written behind the buffer'
    err = (got.double() - ref).abs()
    bad = err > bound
    worst = float((err / bound.clamp(min=1e-300)).max())
    print('  %s %s: worst |err| / bound %.3f (bound = 8u |.|), max|err| %.2e of max|ref| %.2e'
          % (key, tuple(got.shape), worst, float(err.max()), float(ref.abs().max())))
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError('outside the bound at %s: got %r ref %r bound %r' % (
            _where_tile(key, i, got.shape, groups), float(got.flatten()[i]), float(ref.flatten()[i]),
            float(bound.flatten()[i])))
    zero = bound == 0
    assert bool((got[zero] == 0).all())


# ------------------------------------------------------------------ 1a. input transform
_PRE = {
    'none': None,
    'shift': (False, False), 'shift_relu': (False, True),
    'scale_shift': (True, False), 'scale_shift_relu': (True, True),
}
_IN_CASES = (
    [(c, 'three', 1, 'none') for c in CHANNELS]
    + [(c, k, 1, 'none') for k in ('train5', 'one', 'unit', 'odd', 'tail13', 'tail177') for c in (256, 48)]
    + [(36, 'tail177', 1, 'none'), (64, 'tail13', 1, 'none'), (128, 'one', 1, 'scale_shift_relu'),
       (64, 'one', 1, 'scale_shift_relu'), (512, 'odd', 1, 'shift_relu')]
    + [(64, 'three', 2, 'none'), (72, 'tail177', 2, 'none'), (512, 'three', 2, 'none'),
       (512, 'train5', 2, 'none'), (64, 'odd', 2, 'scale_shift_relu'), (520, 'tail13', 2, 'shift')]
    + [(c, k, 1, p) for p in ('shift', 'shift_relu', 'scale_shift', 'scale_shift_relu')
       for (c, k) in ((64, 'three'), (256, 'odd'), (36, 'tail13'))]
)


@pytest.mark.parametrize('channels,key,groups,pre', _IN_CASES)
def test_input_transform_elementwise_vs_fp64(channels, key, groups, pre):
    from iouaware import winograd as W
    plan, batch, sizes = _plan(key)
    g = _gen(channels * 7 + groups)
    xs = [_cl(torch.randn(batch, channels, h, w, device='cuda', generator=g)) for (h, w) in sizes]
    p = p64 = None
    e_pre = None
    if _PRE[pre] is not None:
        scaled, relu = _PRE[pre]
        s = torch.randn(channels, device='cuda', generator=g) if scaled else None      # both signs
        t = torch.randn(channels, device='cuda', generator=g)
        p = (s, t, relu)
        p64 = (None if s is None else s.double(), t.double(), relu)
        xs64 = [x.double() if s is None else x.double() * s.double().view(1, -1, 1, 1) for x in xs]
        e_pre = [2 * U * (x.abs() + t.double().abs().view(1, -1, 1, 1)) for x in xs64]
    out, guard = _guarded((groups * 36, plan.T, channels // groups))
    W.input_transform(plan, xs, groups, out, p)
    torch.cuda.synchronize()
    ref = R.input_transform(xs, torch.float64, pre=p64, groups=groups)
    d_abs = [R.pre_activation(x.double(), p64).abs() for x in xs]
    bound = 8 * U * R.input_transform(d_abs, torch.float64, groups=groups, absolute=True)
    if e_pre is not None:
        bound = bound + R.input_transform(e_pre, torch.float64, groups=groups, absolute=True)
    _check_tiles(key, out, ref, bound, guard, groups)


# ------------------------------------------------------------------ 1b. gradient-of-output transform
@pytest.mark.parametrize('channels,key', [(c, 'three') for c in CHANNELS]
                         + [(c, k) for k in ('train5', 'one', 'unit', 'odd', 'tail13', 'tail177')
                            for c in (256, 48)] + [(36, 'tail177'), (720, 'train5'), (4, 'odd')])
def test_grad_output_transform_elementwise_vs_fp64(channels, key):
    from iouaware import winograd_train as WT
    plan, batch, sizes = _plan(key)
    g = _gen(channels * 11 + 1)
    dys = [_cl(torch.randn(batch, channels, h, w, device='cuda', generator=g)) for (h, w) in sizes]
    out, guard = _guarded((36, plan.T, channels))
    WT.grad_output_transform(plan, dys, out)
    torch.cuda.synchronize()
    ref = R.grad_output_transform(dys, torch.float64)
    bound = 8 * U * R.grad_output_transform([d.abs() for d in dys], torch.float64, absolute=True)
    _check_tiles(key, out, ref, bound, guard)


# ------------------------------------------------------------------ 1c. output transform
def _segs(name, channels):
    """-> list of (c0, n, destination channels, dst_offset, destination id); segments that name
    the same destination id write into one tensor"""
    if name == 'same':
        return [(0, channels, channels, 0, 0)]
    if name == 'head':                 # reg | iou | padding: 36 + 9 of 48, the 9-channel one unaligned
        assert channels == 48
        return [(0, 36, 36, 0, 0), (36, 9, 9, 0, 1)]
    if name == 'offset':               # a slice of the product into the middle of a wider tensor
        return [(16, channels - 32, channels + 16, 8, 0)]
    if name == 'offset_odd':           # neither the offset nor the destination width 16-byte aligned
        return [(0, channels, channels + 13, 6, 0)]
    if name == 'four':                 # aligned, offset, a 3-channel one, a gap (channel 159), aligned
        assert channels == 256
        return [(0, 100, 100, 0, 0), (100, 56, 60, 4, 1), (156, 3, 3, 0, 2), (160, 96, 96, 0, 3)]
    if name == 'two_into_one':         # two segments side by side in one destination, swapped
        return [(0, channels // 2, channels, channels // 2, 0), (channels // 2, channels // 2, channels, 0, 0)]
    raise KeyError(name)


_OUT_CASES = (
    [(c, 'three', 1, i % 2 == 0, i % 3 != 0, 'same') for i, c in enumerate(CHANNELS)]
    + [(256, k, 1, True, True, 'same') for k in ('train5', 'one', 'unit', 'odd', 'tail13', 'tail177')]
    + [(48, k, 1, True, False, 'head') for k in ('train5', 'three', 'unit', 'odd', 'tail13', 'tail177')]
    + [(48, 'three', 1, False, True, 'head'), (36, 'tail177', 1, False, False, 'same')]
    + [(64, 'three', 1, True, False, 'offset'), (64, 'odd', 1, True, True, 'offset_odd'),
       (256, 'three', 1, False, False, 'offset'), (260, 'tail13', 1, True, False, 'offset_odd'),
       (256, 'three', 1, True, True, 'four'), (256, 'odd', 1, False, False, 'four'),
       (128, 'tail177', 1, True, False, 'two_into_one')]
    + [(64, 'three', 2, True, True, 'same'), (512, 'three', 2, True, True, 'same'),
       (512, 'train5', 2, True, True, 'same'), (72, 'tail177', 2, False, False, 'same'),
       (64, 'odd', 2, True, False, 'offset_odd')]
)


@pytest.mark.parametrize('channels,key,groups,bias,relu,segs', _OUT_CASES)
def test_output_transform_elementwise_vs_fp64(channels, key, groups, bias, relu, segs):
    from iouaware import winograd as W
    plan, batch, sizes = _plan(key)
    g = _gen(channels * 13 + groups)
    m = torch.randn(groups * 36, plan.T, channels // groups, device='cuda', generator=g)
    b = torch.randn(channels, device='cuda', generator=g) if bias else None
    spec = _segs(segs, channels)
    dsts = {}
    for (c0, n, cd, off, did) in spec:
        if did not in dsts:
            dsts[did] = [_guarded_cl(batch, cd, h, w) for (h, w) in sizes]
    W.output_transform(plan, m, channels, groups, b, relu,
                       [(c0, n, [t for t, _ in dsts[did]], off) for (c0, n, cd, off, did) in spec])
    torch.cuda.synchronize()
    ref = R.output_transform(m.double(), sizes, batch, None if b is None else b.double(), relu, groups)
    bound = R.output_transform(m.double().abs(), sizes, batch, None if b is None else b.double(),
                               False, groups, absolute=True)
    worst = 0.0
    for did, tensors in dsts.items():
        for l, (t, guard) in enumerate(tensors):
            assert bool(torch.isnan(guard).all()), 'written behind destination %d level %d' % (did, l)
            written = torch.zeros(t.shape[1], dtype=torch.bool, device='cuda')
            for (c0, n, cd, off, d2) in spec:
                if d2 != did:
                    continue
                written[off:off + n] = True
                got = t[:, off:off + n]
                assert not bool(torch.isnan(got).any()), \
                    'pixels never written: destination %d level %d' % (did, l)
                err = (got.double() - ref[l][:, c0:c0 + n]).abs()
                bnd = 8 * U * bound[l][:, c0:c0 + n]
                worst = max(worst, float((err / bnd.clamp(min=1e-300)).max()))
                bad = err > bnd
                if bool(bad.any()):
                    bi, ci, yi, xi = [int(v) for v in bad.nonzero()[0]]
                    raise AssertionError(
                        'outside the bound: level %d image %d pixel (%d, %d) = tile (%d, %d), product '
                        'channel %d -> destination %d channel %d: got %r ref %r bound %r' % (
                            l, bi, yi, xi, yi // 4, xi // 4, c0 + ci, did, off + ci,
                            float(got[bi, ci, yi, xi]), float(ref[l][bi, c0 + ci, yi, xi]),
                            float(bnd[bi, ci, yi, xi])))
            assert bool(torch.isnan(t[:, ~written]).all()), \
                'a channel outside the segments was written: destination %d level %d' % (did, l)
    print('  %s %d ch, %s: worst |err| / bound %.3f' % (key, channels, segs, worst))


# ------------------------------------------------------------------ 2. the node against fp64 autograd
def _report(tag, name, got, helper, ref, rep):
    if isinstance(got, (list, tuple)):
        for l, (a, h, r) in enumerate(zip(got, helper, ref)):
            assert a.shape == r.shape
            print('    %s %s[%d] %s: HIP %.2e helper %.2e' % (tag, name, l, tuple(r.shape),
                                                            R.rel_err(a, r), R.rel_err(h, r)))
    else:
        assert got.shape == ref.shape
    e, h, ratio = R.gates(got, helper, ref)
    print('  %s %-3s HIP %.2e  fp32 helper %.2e  ratio %.2f' % (tag, name, e, h, ratio))
    rep[name] = (e, h, ratio)


def _assert_gates(rep):
    for name, (e, h, ratio) in rep.items():
        assert e <= R.GATE_A, 'gate A: %s %.3e' % (name, e)
        assert ratio <= R.GATE_B, 'gate B: %s HIP %.3e vs helper %.3e = %.2f x' % (name, e, h, ratio)


def _data(cin, cout, batch, sizes, seed):
    g = _gen(seed)
    w = torch.randn(cout, cin, 3, 3, device='cuda', generator=g) * (1.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, device='cuda', generator=g) * 0.1
    xs = [torch.randn(batch, cin, h, ww, device='cuda', generator=g) for (h, ww) in sizes]
    ups = [torch.randn(batch, cout, h, ww, device='cuda', generator=g) for (h, ww) in sizes]
    return w, b, xs, ups


@functools.lru_cache(maxsize=1)
def _yardsticks(cin, cout, key, bias, relu, seed=0):
    """data, the fp64 autograd reference (GPU) and the fp32 helper's results (CPU) of one case"""
    batch, sizes = LEVELS[key] if isinstance(key, str) else key
    w, b, xs, ups = _data(cin, cout, batch, list(sizes), seed + cin + cout)
    if not bias:
        b = None
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if bias else None
    x64 = [x.double().requires_grad_(True) for x in xs]
    z64 = [F.conv2d(x, w64, b64, padding=1) for x in x64]
    if relu:
        # delta = gate A's own forward tolerance: a forward that passes gate A cannot put an
        # element with |z64| >= delta on the other side of the mask
        keep = [z.detach().abs() >= R.GATE_A * z.detach().abs().max() for z in z64]
        ups = [u * k for u, k in zip(ups, keep)]
        share = sum(int((~k).sum()) for k in keep) / float(sum(k.numel() for k in keep))
        print('  ReLU: %.4f %% of the upstream gradient zeroed (|z64| < 1e-4 max|z64|)' % (100 * share))
        assert share <= 0.002
        y64 = [z.clamp(min=0) for z in z64]
    else:
        y64 = z64
    torch.autograd.backward([(y * u.double()).sum() for y, u in zip(y64, ups)])
    ref = dict(y=[y.detach() for y in y64], dx=[x.grad for x in x64], dW=w64.grad,
               db=b64.grad if bias else None)
    del z64, y64
    wc, bc = w.cpu(), (b.cpu() if bias else None)
    xc, uc = [x.cpu() for x in xs], [u.cpu() for u in ups]
    yh, v = R.conv_fwd(xc, wc, bc, torch.float32, relu=relu, keep_v=True)
    gh = [u * (y > 0) for u, y in zip(uc, yh)] if relu else uc
    helper = dict(y=yh, dx=R.conv_dx(gh, wc, torch.float32), dW=R.conv_dw(v, gh, torch.float32),
                  db=R.conv_db(gh, torch.float32) if bias else None)
    return w, b, xs, ups, ref, helper


def _node(tag, cin, cout, key, bias=True, relu=False, layout='nchw', w_cl=False,
          freeze=(), seed=0):
    """one forward + backward of the node; -> {quantity: (HIP error, helper error, ratio)}"""
    from iouaware.winograd_train import wino_conv_levels
    w, b, xs, ups, ref, helper = _yardsticks(cin, cout, key, bias, relu, seed)
    wp = (_cl(w) if w_cl else w.clone()).requires_grad_('w' not in freeze)
    bp = b.clone().requires_grad_('b' not in freeze) if bias else None
    xin = [(_cl(x) if layout == 'channels_last' else x.clone()).requires_grad_('x' not in freeze)
           for x in xs]
    ys = wino_conv_levels(xin, wp, bp, relu=relu)
    if 'w' in freeze:
        # a frozen weight: no V kept for the weight gradient (only the weight and, with ReLU, y)
        assert len(ys[0].grad_fn.saved_tensors) == 1 + (len(xs) if relu else 0)
    wanted = [t for t in [wp, bp] + xin if t is not None and t.requires_grad]
    grads = list(torch.autograd.grad([(y * u).sum() for y, u in zip(ys, ups)], wanted))
    torch.cuda.synchronize()
    rep = {}
    _report(tag, 'y', [y.detach() for y in ys], helper['y'], ref['y'], rep)
    if 'w' not in freeze:
        dw = grads.pop(0)
        assert dw.stride() == wp.stride()                 # the weight's own memory format
        _report(tag, 'dW', dw, helper['dW'], ref['dW'], rep)
    if bias and 'b' not in freeze:
        _report(tag, 'db', grads.pop(0), helper['db'], ref['db'], rep)
    if 'x' not in freeze:
        _report(tag, 'dx', grads, helper['dx'], ref['dx'], rep)
    return rep


_FULL = [(256, 256), (256, 720), (256, 48)]


@pytest.mark.parametrize('cin,cout', _FULL)
def test_node_training_levels_batch4_vs_fp64(cin, cout):
    """the head's convolutions at the training configuration: T = 5 720 tiles per matrix"""
    _assert_gates(_node('train5 %d->%d' % (cin, cout), cin, cout, 'train5', bias=cout != 48))


# ------------------------------------------------------------------ sensitivity through the HIP route
def test_gate_b_fails_when_gemm_tn_sees_16_bit_operands(monkeypatch):
    """the failure mode gate B exists for: the Winograd-domain weight-gradient product from
    operands with 16 significand bits (a 2-term bf16 split).  Python-side only."""
    from iouaware import ops
    orig = ops.gemm_tn
    monkeypatch.setattr(ops, 'gemm_tn', lambda g, x: orig(R.cut_mantissa(g, 16), R.cut_mantissa(x, 16)))
    rep = _node('train5 256->48, gemm_tn operands cut', 256, 48, 'train5', bias=False)
    e, h, ratio = rep['dW']
    assert ratio > R.GATE_B_MAX
    assert rep['dx'][2] <= R.GATE_B and rep['y'][2] <= R.GATE_B      # nothing else moved


def test_gate_a_fails_when_the_last_tile_is_lost(monkeypatch):
    """one tile of 5 720 missing from the weight-gradient reduction.  Python-side only."""
    from iouaware import ops
    orig = ops.gemm_tn

    def lossy(g, x):                # g = V, as (36, T, Cin) or cut into slices of the tile list
        g = g.clone()
        g.view(36, -1, g.shape[2])[:, -1] = 0
        return orig(g, x)
    monkeypatch.setattr(ops, 'gemm_tn', lossy)
    rep = _node('train5 256->48, last tile of V zeroed', 256, 48, 'train5', bias=False)
    assert rep['dW'][0] > R.GATE_A


def test_node_training_levels_relu_elementwise_vs_fp64():
    """a tower convolution with its ReLU at full size, gradients element-wise (masked upstream)"""
    _assert_gates(_node('train5 256->256 relu', 256, 256, 'train5', relu=True,
                        layout='channels_last', seed=1))


@pytest.mark.parametrize('c,h,w', [(64, 200, 336), (128, 100, 168), (256, 50, 84), (512, 25, 42)])
def test_node_backbone_single_level_vs_fp64(c, h, w):
    """the bottleneck conv2 shapes of an 800 x 1344 batch of 4 (packed lane maps at 64 / 128)"""
    _assert_gates(_node('backbone %d @ %dx%d' % (c, h, w), c, c, (4, ((h, w),)),
                        layout='channels_last'))


@pytest.mark.parametrize('cin,cout,kw', [
    (256, 36, dict()),
    (64, 36, dict(bias=False)),
    (256, 36, dict(layout='channels_last', w_cl=True)),
    (64, 36, dict(w_cl=True, relu=True)),
    (256, 36, dict(relu=True, layout='channels_last')),
    (64, 36, dict(relu=True, bias=False)),
    (256, 36, dict(freeze=('w',))),
    (256, 36, dict(freeze=('w',), relu=True)),
    (64, 36, dict(freeze=('x',))),
    (64, 36, dict(freeze=('b',), relu=True)),
    (256, 36, dict(freeze=('x', 'b'), layout='channels_last')),
], ids=lambda v: '-'.join('%s=%s' % kv for kv in sorted(v.items())) if isinstance(v, dict) else str(v))
def test_node_variants_three_levels_vs_fp64(cin, cout, kw):
    """bias / layouts / weight strides / requires_grad patterns / ReLU on (37,53), (19,27), (5,3)"""
    _assert_gates(_node('three %d->%d %s' % (cin, cout, kw), cin, cout, 'three', **kw))


@pytest.mark.parametrize('relu', [False, True])
def test_node_odd_geometry_vs_fp64(relu):
    """levels smaller than a tile, batch 3, 12 -> 4 channels"""
    _assert_gates(_node('odd 12->4', 12, 4, (3, ((3, 2), (1, 7), (1, 1))), relu=relu))


def test_node_chain_with_another_level_list_in_between():
    """two nodes in a chain (no ReLU) on one level list; a second, larger list runs forward
    between the first list's forward and its backward: the shared scratch buffers and the plan
    cache must not leak into what the nodes saved"""
    from iouaware.winograd_train import wino_conv_levels
    c = 64
    w1, b1, xs, _ = _data(c, c, 2, THREE, 21)
    w2, b2, _, ups = _data(c, c, 2, THREE, 22)
    big = [(61, 45), (29, 31), (8, 8), (2, 5)]
    w3, b3, xs3, ups3 = _data(c, 128, 3, big, 23)

    def run(conv, double):
        cast = (lambda t: t.double()) if double else (lambda t: t.clone())
        p = [cast(t).requires_grad_(True) for t in (w1, b1, w2, b2, w3, b3)]
        xa = [cast(x).requires_grad_(True) for x in xs]
        xb = [cast(x).requires_grad_(True) for x in xs3]
        y1 = conv(xa, p[0], p[1])
        y2 = conv(y1, p[2], p[3])
        y3 = conv(xb, p[4], p[5])                        # another plan, larger scratch buffers
        ga = torch.autograd.grad([(y * cast(u)).sum() for y, u in zip(y2, ups)], p[:4] + xa)
        gb = torch.autograd.grad([(y * cast(u)).sum() for y, u in zip(y3, ups3)], p[4:] + xb)
        return dict(y2=[y.detach() for y in y2], y3=[y.detach() for y in y3], dW1=ga[0], db1=ga[1],
                    dW2=ga[2], db2=ga[3], dxa=list(ga[4:]), dW3=gb[0], db3=gb[1], dxb=list(gb[2:]))

    ref = run(lambda x, w, b: [F.conv2d(t, w, b, padding=1) for t in x], True)
    got = run(lambda x, w, b: wino_conv_levels(x, w, b), False)
    torch.cuda.synchronize()
    f32, cpu = torch.float32, (lambda ts: [t.cpu() for t in ts])
    h = {}
    y1h, v1 = R.conv_fwd(cpu(xs), w1.cpu(), b1.cpu(), f32, keep_v=True)
    h['y2'], v2 = R.conv_fwd(y1h, w2.cpu(), b2.cpu(), f32, keep_v=True)
    g1 = R.conv_dx(cpu(ups), w2.cpu(), f32)
    h['dW2'], h['db2'] = R.conv_dw(v2, cpu(ups), f32), R.conv_db(cpu(ups), f32)
    h['dW1'], h['db1'], h['dxa'] = R.conv_dw(v1, g1, f32), R.conv_db(g1, f32), R.conv_dx(g1, w1.cpu(), f32)
    h['y3'], v3 = R.conv_fwd(cpu(xs3), w3.cpu(), b3.cpu(), f32, keep_v=True)
    h['dW3'], h['db3'] = R.conv_dw(v3, cpu(ups3), f32), R.conv_db(cpu(ups3), f32)
    h['dxb'] = R.conv_dx(cpu(ups3), w3.cpu(), f32)
    rep = {}
    for name in ref:
        _report('chain', name, got[name], h[name], ref[name], rep)
    _assert_gates(rep)

"""GPU: the FCOS loss node on channels-last fp32 / bf16 rows (ia_point_head_loss_*_nhwc,
fcos_ops.point_head_loss_packed) -- rows [cls C | ctr | pad] and [reg 4 | iou? | pad] as the two HIP
tower routes leave them, exp(scale_l * x) formed inside the kernels.

Yardstick: the torch `_loss` body in fp64 on the CPU with bbox = exp(scale * raw) inside the graph, so
that autograd gives the raw-reg and scale gradients.  Bounds:
  * fp32 rows: every loss and gradient tensor, error relative to the tensor's max-abs in the yardstick,
    <= 1e-4 AND <= 4 x the error of the fp32 torch route on the same inputs on the device (floor
    2^-22) -- the bound of test_gpu_fcos_loss.py; with reg_scale NULL additionally within 1e-6 of the
    NCHW node on the same values (the forward sums are fp64 atomics in another order: no bit equality);
  * bf16 rows: losses and grad_scale under the fp32 bound against the yardstick on the ROUNDED operands;
    every bf16 gradient element within one bf16 ulp of the round-to-nearest-even bf16 value of the fp32
    instance's gradient on the same values (same fp32 arithmetic; the normalisers' last bits may differ);
  * grad_scale: |got - ref| <= 1e-4 x sum |g d x| (the sum of the yardstick's terms), exactly 0 for a
    level without positives."""
import functools

import numpy as np
import pytest
import torch

import gpu_util as G
import synth_fcos_loss as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOL = 1e-4
FLOOR = 2.0 ** -22
SIZES = S.synth_fcos.level_shapes(128, 160)          # 16x20, 8x10, 4x5, 2x3, 1x2
NL = len(SIZES)
SCALES = np.linspace(0.8, 1.2, NL).astype(np.float32)
KEYS = ('loss_cls', 'loss_reg', 'loss_centerness', 'loss_iou')
KINDS = ('cls', 'reg', 'ctr', 'iou')
NOPOS = (np.array([[0.5, 0.5, 3.0, 3.0]], np.float32), np.array([3], np.int64))   # between all points


def _bf16_round(x):
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def _case(name, rounded=False):
    """-> gt boxes, gt labels, (cls, raw reg, ctr, iou) NCHW fp32 arrays, (cls, distances, ctr, iou)"""
    _, gb, gl, outs = S.case_inputs(S.SMALL)
    if name == 'mixed':                               # one image of the batch without a positive
        gb, gl = [gb[0], NOPOS[0]], [gl[0], NOPOS[1]]
    elif name == 'nopos':
        gb, gl = [NOPOS[0]] * 2, [NOPOS[1]] * 2
    elif name == 'gt_1_512':
        one, many = S.gts(51, 1, 120, 150, 1, 1), S.gts(52, 1, 120, 150, 512, 512)
        gb, gl = [one[0][0], many[0][0]], [one[1][0], many[1][0]]
    else:
        assert name == 'small'
    cls, dist, ctr, iou = outs
    raw = [(np.log(d.astype(np.float64)) / float(s)).astype(np.float32) for d, s in zip(dist, SCALES)]
    if rounded:
        cls, raw, ctr, iou, dist = ([_bf16_round(x) for x in m] for m in (cls, raw, ctr, iou, dist))
    # the conditions the comparisons rest on, on the inputs actually used
    pos = S.check_conditions(SIZES, gb, gl)
    lab, tgt = S.np_targets(SIZES, gb, gl)
    used = [np.exp(float(s) * r.astype(np.float64)).astype(np.float32) for r, s in zip(raw, SCALES)]
    assert S.edge_ties(SIZES, lab, tgt, used) == 0 and (rounded or S.edge_ties(SIZES, lab, tgt, dist) == 0)
    assert {'small': sum(n > 0 for n in pos) >= 2, 'mixed': sum(pos) > 0, 'nopos': sum(pos) == 0,
            'gt_1_512': sum(pos) > 0 and gb[1].shape[0] == 512 and gb[0].shape[0] == 1}[name], pos
    return gb, gl, (cls, raw, ctr, iou), (cls, dist, ctr, iou), pos


def _which(iou_branch):
    return list(KEYS[:4 if iou_branch else 3]) + ['sum']


def _torch_route(iou_branch, vals, scaled, gb, gl, fp64):
    """the torch `_loss` body (fp64 on the CPU with the one-hot focal formula: the yardstick; fp32 on the
    device with the HIP focal op: the comparator) -> losses {key: float}, grads {which: {kind: [L]}}"""
    dev, dt = ('cpu', torch.float64) if fp64 else (DEV, torch.float32)
    n = 4 if iou_branch else 3
    leaves = [[torch.from_numpy(x).to(dev, dt).requires_grad_(True) for x in m] for m in vals[:n]]
    sc = [torch.tensor([float(s)], dtype=dt, device=dev, requires_grad=True) for s in SCALES]
    outs = list(leaves)
    if scaled:
        outs[1] = [(s * x).exp() for s, x in zip(sc, leaves[1])]
    head = S.make_head(iou_branch, False)
    with S.torch_route(cpu_focal=fp64):
        losses = S.head_loss(head, outs, [torch.from_numpy(b).to(dev, dt) for b in gb],
                             [torch.from_numpy(x).to(dev) for x in gl])
    assert list(losses) == list(KEYS[:n])
    flat = [t for m in leaves for t in m] + (sc if scaled else [])
    grads = {}
    for w in _which(iou_branch):
        tgt = sum(v.sum() for v in losses.values()) if w == 'sum' else losses[w].sum()
        gs = torch.autograd.grad(tgt, flat, allow_unused=True, retain_graph=True)
        gs = [np.zeros(tuple(t.shape)) if g is None else g.detach().double().cpu().numpy() for g, t in zip(gs, flat)]
        grads[w] = {k: gs[i * NL:(i + 1) * NL] for i, k in enumerate(KINDS[:n])}
        if scaled:
            grads[w]['scale'] = np.array([float(g.sum()) for g in gs[n * NL:]])
    return {k: float(v.detach().double().sum()) for k, v in losses.items()}, grads


@functools.lru_cache(maxsize=None)
def _yardstick(name, iou_branch, scaled, rounded=False):
    gb, gl, raw, dist, _ = _case(name, rounded)
    return _torch_route(iou_branch, raw if scaled else dist, scaled, gb, gl, True)


@functools.lru_cache(maxsize=None)
def _comparator(name, iou_branch, scaled, rounded=False):
    gb, gl, raw, dist, _ = _case(name, rounded)
    return _torch_route(iou_branch, raw if scaled else dist, scaled, gb, gl, False)


# ------------------------------------------------------------------ the node through its C entries
def _geom():
    from iouaware import fcos_ops
    return fcos_ops.PointGeometry(SIZES, S.STRIDES, S.C)


def _targets(gb, gl):
    from iouaware import fcos_ops
    dev = lambda xs: [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs]   # noqa: E731
    return fcos_ops.point_targets(_geom(), dev(gb), dev(gl), S.RANGES)


def _rows(vals, iou_branch, dtype, wc, wr, fill=7.0):
    """(B, H, W, width) rows [cls | ctr | fill] and [reg | iou? | fill] per level, on the device"""
    return G.point_rows(vals, iou_branch, dtype, wc, wr, S.C, fill)


def _ptrs(cc, ri, iou_branch, off_ctr=S.C, off_iou=4):
    return G.point_row_ptrs(cc, ri, iou_branch, off_ctr, off_iou)


class _Node(G.PointRowsNode):
    """forward once, backward per upstream vector, through ctypes (gpu_util.PointRowsNode)"""

    def __init__(self, name, iou_branch, vals, dtype, wc, wr, scaled, rounded=False):
        gb, gl = _case(name, rounded)[:2]
        super(_Node, self).__init__(SIZES, S.STRIDES, S.C, S.RANGES, gb, gl, iou_branch, vals, dtype, wc, wr,
                                    SCALES if scaled else None)

    def run(self):
        """-> losses {key: float}, raw gradient rows {which: (g_cc, g_ri, g_sc)}"""
        assert self.fwd() == 0
        out = {}
        for w in _which(self.iou):
            gin = torch.ones(4, device=DEV) if w == 'sum' else \
                torch.eye(4, device=DEV)[KEYS.index(w)].contiguous()
            grads = self.new_grads()
            assert self.bwd(gin, grads) == 0
            out[w] = grads
        torch.cuda.synchronize()
        res = self.res.cpu().numpy()
        return {k: float(res[i]) for i, k in enumerate(KEYS[:4 if self.iou else 3])}, out


def _maps(grads, iou_branch):
    """gradient rows -> {kind: [L] (B, ch, H, W) float64 arrays}, 'scale': (L,)"""
    return G.point_row_maps(grads, iou_branch, S.C)


def _judge(tag, got, ref32, ref64, scale):
    """the bound of test_gpu_fcos_loss.py on one quantity; prints the observed errors"""
    if scale == 0.0:
        assert not np.any(got), '%s: the yardstick is zero everywhere, the result is not' % tag
        return
    e = float(np.abs(np.asarray(got, np.float64) - ref64).max()) / scale
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) / scale
    print('%-52s node %.3e  torch fp32 %.3e' % (tag, e, e32))
    assert e <= TOL, '%s: error %.3e above %.0e' % (tag, e, TOL)
    assert e <= max(4.0 * e32, FLOOR), '%s: error %.3e above 4 x the torch route (%.3e)' % (tag, e, e32)


def _judge_scale(tag, got, y_grads, raw, pos):
    """|got - ref| <= 1e-4 x sum |g d x| per level (g d x = the raw-reg gradient x raw / scale in the
    yardstick); exactly 0 without positives"""
    for l in range(NL):
        terms = float(np.abs(y_grads['reg'][l] * raw[l].astype(np.float64)).sum()) / float(SCALES[l])
        ref = y_grads['scale'][l]
        print('%-52s got %.6e  ref %.6e  sum|terms| %.3e' % ('%s d scale[%d]' % (tag, l), got[l], ref, terms))
        assert abs(got[l] - ref) <= 1e-4 * terms, (tag, l, got[l], ref, terms)
        if pos[l] == 0:
            assert got[l] == 0.0 and ref == 0.0, (tag, l, got[l])


def _judge_all(tag, name, iou_branch, scaled, vals, grads, rounded=False, kinds=None):
    v64, g64 = _yardstick(name, iou_branch, scaled, rounded)
    v32, g32 = _comparator(name, iou_branch, scaled, rounded)
    raw, pos = _case(name, rounded)[2][1], _case(name, rounded)[4]
    for k in v64:
        _judge('%s %s' % (tag, k), vals[k], v32[k], v64[k], abs(v64[k]))
    for w in g64:
        m = _maps(grads[w], iou_branch)
        for kind in (kinds if kinds is not None else KINDS[:4 if iou_branch else 3]):
            for l in range(NL):
                ref = g64[w][kind][l]
                _judge('%s d %s / d %s[%d]' % (tag, w, kind, l), m[kind][l], g32[w][kind][l], ref,
                       float(np.abs(ref).max()))
        if scaled:
            _judge_scale('%s d %s' % (tag, w), m['scale'], g64[w], raw, pos)


# ------------------------------------------------------------------ 1. fp32 rows 84 / 8
@pytest.mark.parametrize('scaled', [False, True], ids=['distances', 'reg_scale'])
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
@pytest.mark.parametrize('name', ['small', 'mixed', 'gt_1_512'])
def test_fp32_rows_against_fp64(name, iou_branch, scaled):
    raw, dist = _case(name)[2:4]
    vals, grads = _Node(name, iou_branch, raw if scaled else dist, torch.float32, 84, 8, scaled).run()
    tag = 'f32/%s/%s/%s' % (name, 'iou' if iou_branch else 'plain', 'scale' if scaled else 'dist')
    _judge_all(tag, name, iou_branch, scaled, vals, grads)
    if name == 'mixed':                                # the image without positives: exact zeros
        m = _maps(grads['sum'], iou_branch)
        for kind in KINDS[1:4 if iou_branch else 3]:
            assert all(not np.any(x[1]) for x in m[kind]), kind
    if scaled:
        return
    # the NCHW node on the same values
    from iouaware import fcos_ops
    gb, gl = _case(name)[:2]
    n = 4 if iou_branch else 3
    outs = [[torch.from_numpy(x).to(DEV).requires_grad_(True) for x in m] for m in dist[:n]]
    lab, tgt, counts = _targets(gb, gl)
    losses = fcos_ops.point_head_loss(_geom(), outs[0], outs[1], outs[2], outs[3] if iou_branch else None,
                                      lab, tgt, counts, 2.0, 0.25)
    for k in losses:
        a, b = vals[k], float(losses[k].detach().sum())
        assert abs(a - b) <= 1e-6 * abs(b), (k, a, b)
    flat = [t for m in outs for t in m]
    gs = torch.autograd.grad(sum(v.sum() for v in losses.values()), flat)
    m = _maps(grads['sum'], iou_branch)
    for i, kind in enumerate(KINDS[:n]):
        for l in range(NL):
            r = gs[i * NL + l].double().cpu().numpy()
            assert np.abs(m[kind][l] - r).max() <= 1e-6 * np.abs(r).max(), (kind, l)


# ------------------------------------------------------------------ 2. bf16 rows 96 / 32
def _ordered(t):
    """bf16 tensor -> int32 keys whose difference counts representable values (+0 and -0 coincide)"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
@pytest.mark.parametrize('name', ['small', 'gt_1_512'])
def test_bf16_rows(name, iou_branch):
    raw = _case(name, True)[2]
    v16, g16 = _Node(name, iou_branch, raw, torch.bfloat16, 96, 32, True, rounded=True).run()
    v32, g32 = _Node(name, iou_branch, raw, torch.float32, 84, 8, True, rounded=True).run()
    tag = 'bf16/%s/%s' % (name, 'iou' if iou_branch else 'plain')
    # losses and grad_scale: the fp32 bound against the yardstick on the rounded operands
    _judge_all(tag, name, iou_branch, True, v16, g16, rounded=True, kinds=())
    nreg = 5 if iou_branch else 4
    for w in g16:
        for rows16, rows32, real in ((g16[w][0], g32[w][0], S.C + 1), (g16[w][1], g32[w][1], nreg)):
            for l in range(NL):
                assert rows16[l].dtype == torch.bfloat16
                a = _ordered(rows16[l][..., :real])
                b = _ordered(rows32[l][..., :real].to(torch.bfloat16))      # round to nearest even
                d = int((a - b).abs().max())
                assert d <= 1, '%s d %s level %d: %d bf16 ulps from the fp32 instance' % (tag, w, l, d)
                assert not bool((rows16[l][..., real:].view(torch.int16) != 0).any())


# ------------------------------------------------------------------ 3. no positives at all
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_no_positives(iou_branch, dtype):
    rounded = dtype == torch.bfloat16
    raw = _case('nopos', rounded)[2]
    wc, wr = (96, 32) if rounded else (84, 8)
    vals, grads = _Node('nopos', iou_branch, raw, dtype, wc, wr, True, rounded=rounded).run()
    v64, _ = _yardstick('nopos', iou_branch, True, rounded)
    v32, _ = _comparator('nopos', iou_branch, True, rounded)
    # loss_cls = the focal sum / (0 + B): what the yardstick computes
    _judge('nopos loss_cls', vals['loss_cls'], v32['loss_cls'], v64['loss_cls'], abs(v64['loss_cls']))
    for k in list(vals)[1:]:
        assert vals[k] == 0.0 and v64[k] == 0.0, (k, vals[k])
    for w in grads:
        g_cc, g_ri, g_sc = grads[w]
        assert not bool(g_sc.view(torch.int32).any()), 'grad_scale: exact +0'
        for l in range(NL):
            assert not bool(g_ri[l].view(torch.int16 if rounded else torch.int32).any()), (w, l)
            assert not bool(g_cc[l][..., S.C:].view(torch.int16 if rounded else torch.int32).any()), (w, l)
            assert bool(torch.isfinite(g_cc[l].float()).all())


# ------------------------------------------------------------------ 4. padding and the packed flag
@pytest.mark.parametrize('dtype,wc,wr', [(torch.float32, 84, 8), (torch.bfloat16, 96, 32),
                                         (torch.float32, 88, 4)], ids=['f32', 'bf16', 'f32-plain-4'])
def test_padding_channels(dtype, wc, wr):
    iou_branch = wr != 4
    rounded = dtype == torch.bfloat16
    node = _Node('small', iou_branch, _case('small', rounded)[2], dtype, wc, wr, True, rounded=rounded)
    assert node.fwd() == 0
    gin = torch.ones(4, device=DEV)
    bits = torch.int16 if rounded else torch.int32
    nreg = 5 if iou_branch else 4
    # packed rows: NaN-filled buffers come back with every channel written, the padding as exact +0
    grads = node.new_grads()
    assert node.bwd(gin, grads, packed=1) == 0
    torch.cuda.synchronize()
    for l in range(NL):
        assert bool(torch.isfinite(grads[0][l].float()).all()) and bool(torch.isfinite(grads[1][l].float()).all())
        assert not bool(grads[0][l][..., S.C + 1:].contiguous().view(bits).any())
        assert not bool(grads[1][l][..., nreg:].contiguous().view(bits).any())
    # without the flag: only the map slices are written
    loose = node.new_grads()
    before = [t[..., S.C + 1:].contiguous().view(bits).clone() for t in loose[0]] + \
             [t[..., nreg:].contiguous().view(bits).clone() for t in loose[1]]
    assert node.bwd(gin, loose, packed=0) == 0
    torch.cuda.synchronize()
    after = [t[..., S.C + 1:].contiguous().view(bits) for t in loose[0]] + \
            [t[..., nreg:].contiguous().view(bits) for t in loose[1]]
    assert all(torch.equal(a, b) for a, b in zip(before, after)), 'bytes outside the map slices were touched'
    for l in range(NL):
        assert torch.equal(loose[0][l][..., :S.C + 1], grads[0][l][..., :S.C + 1])
        assert torch.equal(loose[1][l][..., :nreg], grads[1][l][..., :nreg])
    # pointers that contradict the flag
    if wc > S.C + 2:
        bad = node.new_grads()
        gp, gst = _ptrs(bad[0], bad[1], iou_branch, off_ctr=S.C + 1)
        assert node.bwd(gin, bad, packed=1, gp=gp, gst=gst) == -1
        assert node.bwd(gin, bad, packed=0, gp=gp, gst=gst) == 0       # a legal slice without the flag
    if iou_branch:
        bad = node.new_grads()
        gp, gst = _ptrs(bad[0], bad[1], iou_branch, off_iou=5)
        assert node.bwd(gin, bad, packed=1, gp=gp, gst=gst) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. return codes, before any launch
def test_return_codes():
    from iouaware import _lib
    node = _Node('small', True, _case('small')[2], torch.float32, 84, 8, True)
    gin = torch.ones(4, device=DEV)
    grads = node.new_grads(-7.0)
    L = _lib.lib()
    bad_geom = _geom()
    bad_geom.struct.num_levels = 0
    assert L.ia_point_head_loss_nhwc_workspace_bytes(bad_geom.ref(), 2) == 0
    assert L.ia_point_head_loss_nhwc_workspace_bytes(node.geom.ref(), 0) == 0

    def shifted(what):
        p, st = _ptrs(node.cc, node.ri, True)
        for l in range(NL):
            if what == 'cls_ptr':
                p.cls[l] += 4
            elif what == 'reg_ptr':
                p.reg[l] += 8
            elif what == 'cls_stride':
                st.cls[l] += 1
            elif what == 'reg_stride':
                st.reg[l] += 2
            elif what == 'mixed_iou' and l % 2:
                p.iou[l] = None
        return p, st
    for what in ('cls_ptr', 'reg_ptr', 'cls_stride', 'reg_stride', 'mixed_iou'):
        p, st = shifted(what)
        assert node.fwd(p=p, st=st) == -1, what
        assert node.bwd(gin, grads, p=p, st=st) == -1, what
        assert node.bwd(gin, grads, gp=p, gst=st) == -1, what
    assert node.fwd(dt=2) == -1 and node.bwd(gin, grads, dt=2) == -1
    assert node.fwd(geom=bad_geom) == -1 and node.fwd(B=0) == -1 and node.fwd(ws=None) == -1
    assert node.fwd(n=node.nbytes - 1) == -2 and node.bwd(gin, grads, n=node.nbytes - 1) == -2
    assert node.bwd(gin, grads, g_sc=None) == -1                       # reg_scale without grad_scale
    assert node.bwd(gin, grads, sc=None) == -1                         # and the other way round
    torch.cuda.synchronize()
    assert bool((node.res == -7.0).all()), 'a refused call launched something'
    assert all(bool((t == -7.0).all()) for t in grads[0] + grads[1] + [grads[2]])
    assert node.fwd() == 0 and node.bwd(gin, grads) == 0
    torch.cuda.synchronize()
    assert all(bool((t != -7.0).all()) for t in grads[0] + grads[1] + [grads[2]])


# ------------------------------------------------------------------ 6. the autograd node
@pytest.mark.parametrize('dtype,wc,wr', [(torch.float32, 84, 8), (torch.bfloat16, 96, 32)], ids=['f32', 'bf16'])
@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_point_head_loss_packed(iou_branch, dtype, wc, wr):
    from iouaware import fcos_ops
    rounded = dtype == torch.bfloat16
    gb, gl, raw = _case('small', rounded)[:3]
    ref_vals, ref_grads = _Node('small', iou_branch, raw, dtype, wc, wr, True, rounded=rounded).run()
    cc, ri = _rows(raw, iou_branch, dtype, wc, wr)
    cc = [t.permute(0, 3, 1, 2).requires_grad_(True) for t in cc]
    ri = [t.permute(0, 3, 1, 2).requires_grad_(True) for t in ri]
    # (1,)-shaped and 0-dim scales: the gradient takes the parameter's shape
    sc = [torch.tensor([float(s)] if l % 2 else float(s), device=DEV, requires_grad=True)
          for l, s in enumerate(SCALES)]
    lab, tgt, counts = _targets(gb, gl)
    losses = fcos_ops.point_head_loss_packed(_geom(), cc, ri, sc, lab, tgt, counts, 2.0, 0.25,
                                             with_iou=iou_branch)
    assert list(losses) == list(KEYS[:4 if iou_branch else 3])
    for k, v in losses.items():
        assert tuple(v.shape) == (1,) and v.dtype == torch.float32
        assert abs(float(v.detach()) - ref_vals[k]) <= 1e-6 * abs(ref_vals[k]), (k, float(v.detach()), ref_vals[k])
    gs = torch.autograd.grad(sum(v.sum() for v in losses.values()), cc + ri + sc)
    for g, t in zip(gs, cc + ri + sc):
        assert g.dtype == t.dtype and g.shape == t.shape and g.stride() == t.stride()
    r_cc, r_ri, r_sc = ref_grads['sum']
    for l in range(NL):
        for got, ref in ((gs[l], r_cc[l]), (gs[NL + l], r_ri[l])):
            got = got.permute(0, 2, 3, 1).float()
            assert bool(torch.isfinite(got).all())
            tol = (2.0 ** -7 if rounded else 1e-6) * float(ref.float().abs().max())
            assert float((got - ref.float()).abs().max()) <= tol
        assert abs(float(gs[2 * NL + l]) - float(r_sc[l])) <= 1e-6 * max(abs(float(r_sc[l])), 1e-30)


# ------------------------------------------------------------------ 7. one backward body, two layouts
TWIN_GT_SEED = 133        # chosen on the CPU: positives on three levels (134, 82, 6), none on the last two


@functools.lru_cache(maxsize=None)
def _twin_inputs():
    """the head outputs of the small case on gts with positives on three levels; every third positive point
    predicts one edge exactly on the target's (the tie shares), every ninth the whole target box (the
    loss's minimum)"""
    gb, gl = S.gts(TWIN_GT_SEED, 2, 120, 150, 3, 8)
    cls, dist, ctr, iou = S.case_inputs(S.SMALL)[3]
    lab, tgt = S.np_targets(SIZES, gb, gl)
    dist = [np.ascontiguousarray(d).copy() for d in dist]
    i = 0
    for l in range(NL):
        d = dist[l].reshape(dist[l].shape[0], 4, -1)                  # a view: (B, 4, N_l)
        for b, n in zip(*np.nonzero(lab[l] > 0)):
            if i % 9 == 0:
                d[b, :, n] = tgt[l][b, n]
            elif i % 3 == 0:
                d[b, i % 4, n] = tgt[l][b, n, i % 4]
            i += 1
    pos = S.check_conditions(SIZES, gb, gl)
    assert sum(n > 0 for n in pos) >= 3 and min(pos) == 0, pos
    assert S.edge_ties(SIZES, lab, tgt, dist) >= 1
    return gb, gl, (cls, dist, ctr, iou), pos


@pytest.mark.parametrize('iou_branch', [True, False], ids=['iou', 'plain'])
def test_backward_is_one_body_in_both_layouts(iou_branch):
    """fp32, reg_scale NULL, no padding channels: ia_point_head_loss_bwd on NCHW maps and
    ia_point_head_loss_bwd_nhwc on the same values as pixel rows, with the same hand-filled result and
    upstream vectors, give d reg, d ctr and d iou BITWISE equal element for element -- blocks with a
    tail (320 points), levels of a single block, levels without a positive, ties and the minimum."""
    import ctypes as C
    from iouaware import _lib
    gb, gl, vals, pos = _twin_inputs()
    n = 4 if iou_branch else 3
    L, B, geom = _lib.lib(), len(gb), _geom()
    lab, tgt, counts = _targets(gb, gl)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    pt = _lib.PointTargets()
    for l in range(NL):
        pt.labels[l], pt.bbox_targets[l] = lab[l].data_ptr(), tgt[l].data_ptr()
    pt.counts = counts.data_ptr()
    cfg = _lib.PointLossCfg(2.0, 0.25, 1, 0)
    # not the forwards' own: their fp64 atomics may round the normalisers differently
    res = torch.tensor([0.71, 0.43, 0.62, 0.37, 222.0, 97.25], device=DEV)
    gin = torch.tensor([1.0, 0.75, 1.25, 0.5], device=DEV)
    scratch = torch.empty(6, device=DEV)

    def level_ptrs(maps):
        p = _lib.PointLevelPtrs()
        for l in range(NL):
            p.cls[l], p.reg[l], p.ctr[l] = (m[l].data_ptr() for m in maps[:3])
            p.iou[l] = maps[3][l].data_ptr() if iou_branch else None
        return p

    # NCHW maps; the forward leaves the packed labels and the focal kernel's vectors in the workspace
    planes = [[torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in m] for m in vals[:n]]
    g_planes = [[torch.full_like(t, float('nan')) for t in m] for m in planes]
    nb = L.ia_point_head_loss_workspace_bytes(geom.ref(), B)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    p, gp = level_ptrs(planes), level_ptrs(g_planes)
    assert L.ia_point_head_loss_fwd(geom.ref(), C.byref(p), B, C.byref(pt), C.byref(cfg), ptr(ws), nb,
                                    ptr(scratch), None) == 0
    assert L.ia_point_head_loss_bwd(geom.ref(), C.byref(p), B, C.byref(pt), C.byref(cfg), ptr(ws), ptr(res),
                                    ptr(gin), C.byref(gp), None) == 0
    # the same values as rows: every map its own rows, pixel stride = its channel count
    rows = [[t.permute(0, 2, 3, 1).contiguous() for t in m] for m in planes]
    g_rows = [[torch.full_like(t, float('nan')) for t in m] for m in rows]
    st = _lib.PointPixStrides()
    for l in range(NL):
        st.cls[l], st.reg[l], st.ctr[l], st.iou[l] = S.C, 4, 1, 1
    nbr = L.ia_point_head_loss_nhwc_workspace_bytes(geom.ref(), B)
    wsr = torch.empty(nbr, dtype=torch.uint8, device=DEV)
    pr, gpr = level_ptrs(rows), level_ptrs(g_rows)
    assert L.ia_point_head_loss_fwd_nhwc(geom.ref(), C.byref(pr), C.byref(st), _lib.IA_F32, B, C.byref(pt),
                                         C.byref(cfg), None, ptr(wsr), nbr, ptr(scratch), None) == 0
    assert L.ia_point_head_loss_bwd_nhwc(geom.ref(), C.byref(pr), C.byref(st), _lib.IA_F32, B, C.byref(pt),
                                         C.byref(cfg), None, ptr(wsr), nbr, ptr(res), ptr(gin), C.byref(gpr),
                                         C.byref(st), 0, None, None) == 0
    torch.cuda.synchronize()
    for k in range(1, n):
        for l in range(NL):
            a, b = g_planes[k][l], g_rows[k][l].permute(0, 3, 1, 2).contiguous()
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), (KINDS[k], l)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (KINDS[k], l)
            assert bool((a != 0).any()) == (pos[l] > 0), (KINDS[k], l)

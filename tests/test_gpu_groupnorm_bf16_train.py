"""GPU: the bf16 GroupNorm + ReLU training node (csrc/groupnorm.hip: k_gn_stats_bf16,
k_gn_apply_to_bf16, k_gn_bwd_reduce_bf16, k_gn_bwd_apply_bf16, k_gn_bwd_params;
fcos_ops.groupnorm_relu_bf16) against tests/gn_ref.py in fp64 on the CPU, evaluated on the
bf16-rounded x and dy.  The precision helper is the same functions in fp32 on the same values.

Gates, per level:
    y       the bits of the in-place inference pair (fcos_ops.groupnorm_relu_) on a copy of x, and
            |y - want| <= 2^-8 |want| + bar * max|want| with the forward bars of
            tests/test_gpu_fcos_bf16.py: 2e-5, and 2e-4 at |mean| / std = 200
    dx      |dx - want| <= 2^-8 |want| + bar * max|want|: 2^-8 is ONE rounding to bf16, bar =
            gn_ref.gate_b(the fp32 helper's rel_err on that level), which must not exceed GATE_A
            (helper here: 0.3e-7 .. 1.1e-6, so a second rounding, or fp32 statistics at
            |mean| >> std, fail)
    dgamma, dbeta (fp32)    rel_err <= GATE_A and <= gate_b(the helper's), as in
            tests/test_gpu_groupnorm_train.py
The upstream gradient goes through gn_ref.safe_upstream(margin=1e-4): no mask that rounding could
flip carries a gradient; the test fails if that zeroes more than 1 % of the elements.

Shapes: the smallest that take every path -- the head's 2F layout with levels below one chunk, two
full chunks and a partial one, odd sizes and a single pixel; 1024 and 8 channels, eight levels and
several columns per group.

Every figure is printed before it is asserted; what was observed is recorded in DESIGN 3.17 "bf16
training".
"""
import ctypes as C
import functools

import pytest
import torch

import gn_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BF, CL = torch.bfloat16, torch.channels_last
BF16_RNE = 2.0 ** -8
Y_BAR = {False: 2e-5, True: 2e-4}           # tests/test_gpu_fcos_bf16.py: GN_BAR

SHAPES = {
    # name: (level sizes, batch, channels, groups)
    'towers': ([(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)], 2, 512, 64),
    'chunks': ([(20, 30)], 3, 64, 8),       # 600 pixels: two full chunks of 256 and a partial one
    'odd': ([(17, 13), (1, 1)], 2, 256, 32),
    # the edges of the supported geometry: 128 columns per pixel and every per-channel LDS slot;
    # one column per pixel (256 pixels per pass, two full chunks and a partial one); eight levels
    # with four columns per group
    'max-channels': ([(5, 7), (2, 3)], 2, 1024, 128),
    'min-channels': ([(19, 29)], 2, 8, 1),
    'eight-levels': ([(9, 11), (5, 7), (4, 5), (3, 3), (2, 3), (2, 2), (1, 2), (1, 1)], 2, 64, 2),
}
SEED_ORDER = ['chunks', 'odd', 'towers', 'max-channels', 'min-channels', 'eight-levels']


def _bf(t):
    return t.to(BF).float()


@functools.lru_cache(maxsize=None)
def _case(shape, shifted, relu):
    """inputs (bf16 values held in fp32, on the CPU) and the fp64 / fp32 results, computed once"""
    sizes, batch, ch, groups = SHAPES[shape]
    g = torch.Generator().manual_seed(101 + 7 * SEED_ORDER.index(shape) + int(shifted))
    xs = []
    for (h, w) in sizes:
        x = torch.randn((batch, ch, h, w), generator=g) * 0.7
        if shifted:                               # every group: std 0.007, mean 1.4
            x = x * 0.01 + 0.007 * 200.0
        xs.append(_bf(x))
    ups = [_bf(torch.randn((batch, ch, h, w), generator=g)) for (h, w) in sizes]
    gamma = 1.0 + 0.5 * torch.randn(ch, generator=g)
    beta = 0.5 * torch.randn(ch, generator=g)
    dropped = 0.0
    if relu:
        ups, dropped = R.safe_upstream(xs, ups, gamma, beta, groups, margin=1e-4)
    want = dict(y=R.forward(xs, gamma, beta, groups, relu=relu))
    want['dx'], want['dgamma'], want['dbeta'] = R.backward(xs, ups, gamma, beta, groups, relu=relu)
    helper = {}
    helper['dx'], helper['dgamma'], helper['dbeta'] = R.backward(xs, ups, gamma, beta, groups, relu=relu,
                                                                 dtype=torch.float32)
    return xs, ups, gamma, beta, dropped, want, helper


def _cl(t):
    return t.to(DEV).to(BF).contiguous(memory_format=CL)


def _node(xs, ups, gamma, beta, groups, relu=True, param_grad=True, x_grad=True):
    """the autograd node -> (ys, dxs or None, dgamma or None, dbeta or None), on the host"""
    from iouaware import fcos_ops
    dx = [_cl(x).requires_grad_(x_grad) for x in xs]
    gm = gamma.to(DEV).requires_grad_(param_grad)
    bt = beta.to(DEV).requires_grad_(param_grad)
    ys = fcos_ops.groupnorm_relu_bf16(dx, gm, bt, groups, relu=relu)
    assert all(y.dtype == BF and y.is_contiguous(memory_format=CL) and y.data_ptr() != x.data_ptr()
               for x, y in zip(dx, ys))
    torch.autograd.backward(ys, [_cl(u) for u in ups])
    torch.cuda.synchronize()
    if x_grad:
        assert all(x.grad.dtype == BF and x.grad.is_contiguous(memory_format=CL) for x in dx)
    return ([y.detach().cpu() for y in ys], [x.grad.cpu() for x in dx] if x_grad else None,
            None if gm.grad is None else gm.grad.cpu(), None if bt.grad is None else bt.grad.cpu())


def _worst(got, want, bar):
    """the largest |got - want| as a fraction of 2^-8 |want| + bar * max|want|"""
    want = want.double()
    bound = BF16_RNE * want.abs() + bar * float(want.abs().max())
    return float(((got.double() - want).abs() / bound).max())


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'norelu'])
@pytest.mark.parametrize('shifted', [False, True], ids=['zero-mean', 'shifted'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_node_against_fp64(shape, shifted, relu):
    from iouaware import fcos_ops
    sizes, batch, ch, groups = SHAPES[shape]
    xs, ups, gamma, beta, dropped, want, helper = _case(shape, shifted, relu)
    tag = '%s/%s/%s' % (shape, 'shifted' if shifted else 'zero-mean', 'relu' if relu else 'norelu')
    print('%s: %.4f %% of the upstream gradient zeroed' % (tag, 100 * dropped))
    assert dropped <= 0.01
    ys, dxs, dg, db = _node(xs, ups, gamma, beta, groups, relu)
    # y: the bits of the in-place inference pair on a copy
    copy = [_cl(x) for x in xs]
    fcos_ops.groupnorm_relu_(copy, gamma.to(DEV), beta.to(DEV), groups, relu=relu)
    for l in range(len(sizes)):
        assert torch.equal(ys[l], copy[l].cpu()), (tag, l)
        wy = _worst(ys[l], want['y'][l], Y_BAR[shifted])
        e32 = R.rel_err(helper['dx'][l], want['dx'][l])
        bar = R.gate_b(e32)
        wx = _worst(dxs[l], want['dx'][l], bar)
        print('%s level %d: y worst / bound %.3f   dx worst / bound %.3f  (fp32 helper %.3e, bar %.3e)'
              % (tag, l, wy, wx, e32, bar))
        assert wy <= 1.0, (tag, l, wy)
        assert bar <= R.GATE_A, (tag, l, bar)
        assert wx <= 1.0, (tag, l, wx)
    for name, got in (('dgamma', dg), ('dbeta', db)):
        assert got.dtype == torch.float32
        e, e32 = R.rel_err(got, want[name]), R.rel_err(helper[name], want[name])
        print('%s %s: node %.3e  fp32 helper %.3e' % (tag, name, e, e32))
        assert e <= R.GATE_A, (tag, name, e)
        assert e <= R.gate_b(e32), (tag, name, e, e32)


def _same(a, b):
    flat_a = a[0] + a[1] + [a[2], a[3]]
    flat_b = b[0] + b[1] + [b[2], b[3]]
    return all(torch.equal(u, v) for u, v in zip(flat_a, flat_b))


def test_bits_repeat_with_a_nan_workspace_and_do_not_depend_on_the_batch():
    from iouaware import fcos_ops
    sizes, batch, ch, groups = SHAPES['chunks']
    xs, ups, gamma, beta, _, _, _ = _case('chunks', True, True)
    a = _node(xs, ups, gamma, beta, groups)
    assert fcos_ops._gn_ws
    for ws in fcos_ops._gn_ws.values():           # every partial sum the kernels read they wrote before
        ws.fill_(0xff)
    b = _node(xs, ups, gamma, beta, groups)
    assert _same(a, b)
    alone = _node([x[1:2] for x in xs], [u[1:2] for u in ups], gamma, beta, groups)
    for u, v in zip(a[0] + a[1], alone[0] + alone[1]):
        assert torch.equal(u[1:2], v)


def test_frozen_parameters_and_inputs():
    sizes, batch, ch, groups = SHAPES['odd']
    xs, ups, gamma, beta, _, _, _ = _case('odd', False, True)
    ref = _node(xs, ups, gamma, beta, groups)
    ys, dxs, dg, db = _node(xs, ups, gamma, beta, groups, param_grad=False)
    assert dg is None and db is None
    assert all(torch.equal(a, b) for a, b in zip(ys + dxs, ref[0] + ref[1]))
    ys, dxs, dg, db = _node(xs, ups, gamma, beta, groups, x_grad=False)
    assert dxs is None and torch.equal(dg, ref[2]) and torch.equal(db, ref[3])


def test_an_upstream_gradient_in_another_form_is_copied():
    """fp32 NCHW cotangents, and bf16 ones that start 2 bytes into their storage: the bits of the bf16
    channels-last ones"""
    from iouaware import fcos_ops
    sizes, batch, ch, groups = SHAPES['odd']
    xs, ups, gamma, beta, _, _, _ = _case('odd', False, True)
    ref = _node(xs, ups, gamma, beta, groups)
    for form in ('fp32', 'offset'):
        dx = [_cl(x).requires_grad_(True) for x in xs]
        gm, bt = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        ys = fcos_ops.groupnorm_relu_bf16(dx, gm, bt, groups)
        cot = []
        for u in ups:
            if form == 'fp32':
                cot.append(u.to(DEV).contiguous())
                continue
            B, c, h, w = u.shape
            flat = torch.zeros(u.numel() + 1, dtype=BF, device=DEV)
            v = flat[1:].view(B, h, w, c).permute(0, 3, 1, 2)
            v.copy_(u.to(DEV))
            assert v.data_ptr() % 16 == 2
            cot.append(v)
        torch.autograd.backward(ys, cot)
        torch.cuda.synchronize()
        got = [x.grad.cpu() for x in dx] + [gm.grad.cpu(), bt.grad.cpu()]
        assert all(torch.equal(a, b) for a, b in zip(got, ref[1] + [ref[2], ref[3]])), form


def test_two_towers_as_one_node():
    """the halves of one 2F-wide tensor: one node whose outputs and input gradients are halves of one
    tensor again, with the bits of the node on the wide tensor; separate tensors: a node per tower,
    the same bits (statistics are per group)"""
    from iouaware import fcos_ops
    sizes, batch, ch, groups = SHAPES['towers']
    xs, ups, gamma, beta, _, _, _ = _case('towers', False, True)
    ref = _node(xs, ups, gamma, beta, groups)
    F_ = ch // 2
    for joined in (True, False):
        wide = [_cl(x) for x in xs]
        if joined:
            leaves = [w.requires_grad_(True) for w in wide]
            xa, xb = [w[:, :F_] for w in leaves], [w[:, F_:] for w in leaves]
        else:
            xa = [w[:, :F_].contiguous(memory_format=CL).requires_grad_(True) for w in wide]
            xb = [w[:, F_:].contiguous(memory_format=CL).requires_grad_(True) for w in wide]
            leaves = xa + xb
        gm, bt = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        ya, yb = fcos_ops.groupnorm_relu_bf16_towers(xa, xb, gm, bt, groups)
        assert all(fcos_ops._halves_of_one(a, b) for a, b in zip(ya, yb)) == joined
        assert ('GroupNormReluBf16Fn' in type(ya[0].grad_fn).__name__)
        cot = [_cl(u) for u in ups]
        torch.autograd.backward(list(ya) + list(yb), [c[:, :F_] for c in cot] + [c[:, F_:] for c in cot])
        torch.cuda.synchronize()
        ys = [torch.cat((a, b), 1).detach().cpu() for a, b in zip(ya, yb)]
        if joined:
            dxs = [w.grad.cpu() for w in leaves]
        else:
            dxs = [torch.cat((a.grad, b.grad), 1).cpu() for a, b in zip(xa, xb)]
        got = (ys, dxs, gm.grad.cpu(), bt.grad.cpu())
        assert _same(got, ref), joined


# ------------------------------------------------------------------ the entries themselves
GUARD = 1024


def _guarded(shape):
    """a (B, C, H, W) bf16 channels-last view of a NaN-filled flat buffer, GUARD values of -7 behind"""
    B, ch, h, w = shape
    n = B * ch * h * w
    flat = torch.full((n + GUARD,), float('nan'), dtype=BF, device=DEV)
    flat[n:] = -7.0
    return flat[:n].view(B, h, w, ch).permute(0, 3, 1, 2), flat


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def test_entries_write_every_element_and_nothing_behind_and_refuse_bad_arguments():
    from iouaware import _lib, fcos_ops
    sizes, batch, ch, groups = SHAPES['odd']
    xs, ups, gamma, beta, _, _, _ = _case('odd', False, True)
    ref = _node(xs, ups, gamma, beta, groups)
    L, dt = _lib.lib(), _lib.IA_BF16
    g = fcos_ops.winograd._wino_geom(sizes, batch)
    x_, u_ = [_cl(x) for x in xs], [_cl(u) for u in ups]
    gm, bt = gamma.to(DEV), beta.to(DEV)
    nws = L.ia_groupnorm_workspace_bytes_dt(C.byref(g), ch, groups, dt)
    nsv = L.ia_groupnorm_saved_bytes_dt(C.byref(g), ch, groups, dt)
    nbw = L.ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), ch, groups, dt)
    assert nws and nsv and nbw
    # the fp32 queries answer as before, and what bf16 does not cover gives 0
    assert nsv == L.ia_groupnorm_saved_bytes(C.byref(g), ch, groups) == L.ia_groupnorm_saved_bytes_dt(C.byref(g), ch, groups, _lib.IA_F32)
    assert nbw == L.ia_groupnorm_bwd_workspace_bytes(C.byref(g), ch, groups)
    assert L.ia_groupnorm_saved_bytes_dt(C.byref(g), ch, 64, dt) == 0               # 4 channels per group
    assert L.ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), ch, 64, dt) == 0
    assert L.ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), ch, 64, _lib.IA_F32) != 0
    assert L.ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), 96, 12, dt) == 0       # not a power of two
    assert L.ia_groupnorm_saved_bytes_dt(C.byref(g), ch, groups, _lib.IA_F16) == 0
    assert not fcos_ops.groupnorm_bf16_supported(sizes, batch, ch, 64)
    assert fcos_ops.groupnorm_bf16_supported(sizes, batch, ch, groups)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    saved = torch.full((nsv // 8 + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    saved[nsv // 8:] = -7.0
    bws = torch.full((nbw // 8 + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    bws[nbw // 8:] = -7.0
    ys, dxs = [_guarded(x.shape) for x in xs], [_guarded(x.shape) for x in xs]
    dgamma = torch.full((ch + GUARD,), -7.0, device=DEV)
    dbeta = torch.full((ch + GUARD,), -7.0, device=DEV)
    px, pu = _ptrs(x_), _ptrs(u_)
    py, pdx = _ptrs([v for v, _ in ys]), _ptrs([v for v, _ in dxs])
    off = _ptrs([v.flatten()[1:] for v, _ in ys])                                   # 2-byte aligned

    def fwd(y=py, gr=groups, d=dt, ns=nsv):
        return L.ia_groupnorm_apply_to_dt(C.byref(g), px, y, d, ch, gr, _p(gm), _p(bt), 1e-5, 1, _p(ws), nws,
                                          _p(saved), ns, None)

    def red(u=pu, gr=groups, nw=nbw):
        return L.ia_groupnorm_bwd_reduce_dt(C.byref(g), px, u, dt, ch, gr, _p(gm), _p(bt), 1, _p(saved), nsv,
                                            _p(bws), nw, None)

    def app(d=pdx, gr=groups, nw=nbw):
        return L.ia_groupnorm_bwd_apply_dt(C.byref(g), px, pu, d, dt, ch, gr, _p(gm), _p(bt), 1, _p(saved), nsv,
                                           _p(bws), nw, _p(dgamma), _p(dbeta), None)
    assert L.ia_groupnorm_stats_dt(C.byref(g), px, dt, ch, groups, _p(ws), nws, None) == 0
    for call in (lambda: fwd(y=px), lambda: fwd(y=off), lambda: fwd(gr=64), lambda: fwd(d=_lib.IA_F16),
                 lambda: red(u=off), lambda: red(gr=64), lambda: app(d=pu), lambda: app(d=px),
                 lambda: app(d=off), lambda: app(gr=64)):
        assert call() == -1
    for call in (lambda: fwd(ns=nsv - 1), lambda: red(nw=nbw - 1), lambda: app(nw=nbw - 1)):
        assert call() == -2
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v, _ in ys + dxs) and bool((dgamma == -7.0).all())   # nothing ran
    assert fwd() == 0 and red() == 0 and app() == 0
    torch.cuda.synchronize()
    for view, flat in ys + dxs:
        n = view.numel()
        assert bool(torch.isfinite(flat[:n].float()).all()) and bool((flat[n:] == -7.0).all())
    n_saved = len(sizes) * batch * groups * 2
    assert bool(torch.isfinite(saved[:n_saved]).all()) and bool((saved[nsv // 8:] == -7.0).all())
    assert bool(torch.isfinite(bws[:nbw // 8]).all()) and bool((bws[nbw // 8:] == -7.0).all())
    assert bool((dgamma[ch:] == -7.0).all()) and bool((dbeta[ch:] == -7.0).all())
    assert all(torch.equal(d.cpu().float(), x) for d, x in zip(x_ + u_, xs + ups))   # inputs only read
    for (view, _), r in zip(ys + dxs, ref[0] + ref[1]):
        assert torch.equal(view.cpu(), r)
    assert torch.equal(dgamma[:ch].cpu(), ref[2]) and torch.equal(dbeta[:ch].cpu(), ref[3])


def test_front_end_refuses_before_the_device():
    from iouaware import _lib, fcos_ops
    x = torch.zeros((1, 64, 4, 4), dtype=BF, device=DEV).contiguous(memory_format=CL)
    g, b = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    for bad in ([x.float()], [x.contiguous()], [x, x.cpu()], [x.cpu()], [x] * 9,
                [x, torch.zeros((2, 64, 2, 2), dtype=BF, device=DEV).contiguous(memory_format=CL)]):
        with pytest.raises(ValueError):
            fcos_ops.groupnorm_relu_bf16(bad, g, b, 8)
    for gb in ((g.cpu(), b), (g.to(BF), b), (g[:32], b)):
        with pytest.raises(ValueError):
            fcos_ops.groupnorm_relu_bf16([x], gb[0], gb[1], 8)
    with pytest.raises(_lib.IouAwareLibraryError):
        fcos_ops.groupnorm_relu_bf16([x], g, b, 16)              # 4 channels per group
    # the fp32 node keeps its contract
    with pytest.raises(ValueError):
        fcos_ops.groupnorm_relu([x], g, b, 8)

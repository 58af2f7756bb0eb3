"""GPU: the GroupNorm + ReLU training node (csrc/groupnorm.hip: k_gn_apply_to, k_gn_bwd_reduce,
k_gn_bwd_apply, k_gn_bwd_params; fcos_ops.groupnorm_relu) against tests/gn_ref.py in fp64.

Error of a tensor (y_l, dx_l, dgamma, dbeta) = max|got - ref| / max|ref|.
    gate A  <= 1e-4, the project's contract
    gate B  <= max(4 x the same figure of gn_ref in fp32 on the CPU, 2^-22)
on data of zero mean.  A second data set with |mean| / std = 200 (the data of
test_gpu_fcos.py::test_groupnorm_against_fp64) is held to that test's bar for y (GN_TOL_SHIFTED,
absolute) and to gate A for the gradients; gate B is printed for it, not asserted: the fp32 helper
itself loses 5e-6 (y) and 1.4e-5 (dgamma) there, so 4 x is not a margin one can rely on.

Upstream gradients are zero where the fp64 pre-activation is within 1e-4 of its max-abs of zero
(at most 0.5 % of the elements, asserted), so no ReLU mask that rounding could flip moves a gradient.

Observed on an MI355X (first run; the six cases differ little, worst case given):
                       node               fp32 helper        ratio
    zero-mean  y       8.3e-8 .. 1.1e-7   1.5e-7 .. 1.7e-7   0.57 .. 0.76
               dx      6.4e-8 .. 1.0e-7   1.3e-7 .. 1.8e-7   0.43 .. 0.68
               dbeta   2.7e-8 .. 4.0e-8   1.0e-7 .. 1.5e-7   0.21 .. 0.34
               dgamma  2.6e-8 .. 4.8e-8   1.5e-7 .. 2.1e-7   0.17 .. 0.28
    shifted    y       4.4e-6 .. 5.8e-6   4.4e-6 .. 7.3e-6   0.65 .. 1.09
               dx      6.1e-8 .. 1.0e-7   1.5e-7 .. 3.7e-6   0.02 .. 0.58
               dbeta   3.0e-8 .. 3.6e-8   8.8e-8 .. 1.7e-7   0.18 .. 0.41
               dgamma  2.9e-8 .. 4.5e-8   1.3e-5 .. 2.4e-5   < 0.01
0.045 .. 0.061 % of the upstream gradient is zeroed.  The node stays below the fp32 helper because
its statistics, partial sums and per-channel constants are fp64 and only the element-wise
expressions round in fp32; gate B's factor of 4 is not used up anywhere.
"""
import ctypes as C

import pytest
import torch

import gn_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GN_TOL_SHIFTED = 2e-4         # tests/test_gpu_fcos.py: |mean| / std = 200, absolute, output scale ~ 1
MAIN = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]       # 800 x 1344, strides 8..128
ODD = [(23, 37), (11, 19), (3, 5)]                               # 11 x 19 = 209 < one chunk of 256
EIGHT = [(9, 11), (5, 7), (4, 5), (3, 3), (2, 3), (2, 2), (1, 2), (1, 1)]       # IA_MAX_LEVELS levels

CASES = {
    # name: (sizes, batch, channels, groups, relu, gamma trainable)
    'main': (MAIN, 4, 256, 32, True, True),
    'wide': (MAIN, 2, 512, 64, True, True),
    'odd': (ODD, 3, 64, 16, True, True),
    'batch1': (MAIN, 1, 256, 32, True, True),
    'norelu': (ODD, 2, 256, 32, False, True),
    'frozen': (ODD, 2, 256, 32, True, False),
    # the edges of the supported geometry: 256 columns per pixel and every per-channel LDS slot;
    # one column per pixel (256 pixels per pass, two full chunks and a partial one); eight levels
    'max-channels': ([(5, 7), (2, 3)], 2, 1024, 256, True, True),
    'min-channels': ([(19, 29)], 2, 4, 1, True, True),
    'eight-levels': (EIGHT, 2, 32, 4, True, True),
}
EDGES = ('max-channels', 'min-channels', 'eight-levels')


def _data(seed, sizes, batch, ch, shifted):
    g = torch.Generator().manual_seed(seed)
    xs = []
    for (h, w) in sizes:
        x = torch.randn((batch, ch, h, w), generator=g)
        if shifted:                                   # every group: std 0.007, mean 1.4
            x = x * 0.7 * 0.01 + 0.007 * 200.0
        xs.append(x)
    ups = [torch.randn((batch, ch, h, w), generator=g) for (h, w) in sizes]
    gamma = torch.rand(ch, generator=g) + 0.5
    beta = torch.randn(ch, generator=g) * 0.3
    return xs, ups, gamma, beta


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _node(xs, ups, gamma, beta, groups, relu=True, gamma_grad=True, x_grad=True):
    """the autograd node -> (ys, dxs or None, dgamma or None, dbeta), on the host"""
    from iouaware import fcos_ops
    dx = [_cl(x).requires_grad_(x_grad) for x in xs]
    gm = gamma.to(DEV).requires_grad_(gamma_grad)
    bt = beta.to(DEV).requires_grad_(True)
    ys = fcos_ops.groupnorm_relu(dx, gm, bt, groups, relu=relu)
    assert all(y.is_contiguous(memory_format=torch.channels_last) and y.data_ptr() != x.data_ptr()
               for x, y in zip(dx, ys))
    torch.autograd.backward(ys, [_cl(u) for u in ups])
    torch.cuda.synchronize()
    return ([y.detach().cpu() for y in ys], [x.grad.cpu() for x in dx] if x_grad else None,
            None if gm.grad is None else gm.grad.cpu(), bt.grad.cpu())


def _judge(tag, got, ref, helper, assert_b=True, abs_bar=None):
    e, e32 = R.rel_err(got, ref), R.rel_err(helper, ref)
    print('%-22s node %.3e  fp32 helper %.3e  ratio %.2f' % (tag, e, e32, e / max(e32, 1e-30)))
    if abs_bar is not None:
        a = float((got.double() - ref.double()).abs().max())
        assert a <= abs_bar, '%s: absolute error %.3e above %.0e' % (tag, a, abs_bar)
    else:
        assert e <= R.GATE_A, '%s: error %.3e above gate A' % (tag, e)
    if assert_b:
        assert e <= R.gate_b(e32), '%s: error %.3e above gate B (helper %.3e)' % (tag, e, e32)


@pytest.mark.parametrize('shifted', [False, True], ids=['zero-mean', 'shifted'])
@pytest.mark.parametrize('case', list(CASES))
def test_node_against_fp64(case, shifted):
    sizes, batch, ch, groups, relu, gamma_grad = CASES[case]
    xs, ups, gamma, beta = _data(11, sizes, batch, ch, shifted)
    if relu:
        ups, dropped = R.safe_upstream(xs, ups, gamma, beta, groups)
        print('%s: %.3f %% of the upstream gradient zeroed' % (case, 100 * dropped))
        assert dropped <= 0.005
    y64 = R.forward(xs, gamma, beta, groups, relu=relu)
    dx64, dg64, db64 = R.backward(xs, ups, gamma, beta, groups, relu=relu)
    y32 = R.forward(xs, gamma, beta, groups, relu=relu, dtype=torch.float32)
    dx32, dg32, db32 = R.backward(xs, ups, gamma, beta, groups, relu=relu, dtype=torch.float32)
    ys, dxs, dg, db = _node(xs, ups, gamma, beta, groups, relu, gamma_grad)
    tag = '%s/%s' % (case, 'shifted' if shifted else 'zero-mean')
    for l in range(len(sizes)):
        _judge('%s y[%d]' % (tag, l), ys[l], y64[l], y32[l], not shifted,
               GN_TOL_SHIFTED if shifted else None)
        _judge('%s dx[%d]' % (tag, l), dxs[l], dx64[l], dx32[l], not shifted)
    _judge('%s dbeta' % tag, db, db64, db32, not shifted)
    if gamma_grad:
        _judge('%s dgamma' % tag, dg, dg64, dg32, not shifted)
    else:
        assert dg is None
        # and without gradients for the inputs: the parameter gradient alone, the same bits
        _, none, dg2, db2 = _node(xs, ups, gamma, beta, groups, relu, False, x_grad=False)
        assert none is None and dg2 is None and torch.equal(db2, db)


def test_forward_bits_are_those_of_the_in_place_kernels():
    from iouaware import fcos_ops
    for sizes, batch, ch, groups in [(ODD, 2, 256, 32)] + [CASES[c][:4] for c in EDGES]:
        xs, _, gamma, beta = _data(12, sizes, batch, ch, False)
        dev = [_cl(x) for x in xs]
        with torch.no_grad():
            ys = fcos_ops.groupnorm_relu(dev, gamma.to(DEV), beta.to(DEV), groups)
        assert all(torch.equal(d.cpu(), x) for d, x in zip(dev, xs))       # x untouched
        fcos_ops.groupnorm_relu_(dev, gamma.to(DEV), beta.to(DEV), groups)
        assert all(torch.equal(y, d) for y, d in zip(ys, dev))


def test_bits_repeat_and_do_not_depend_on_the_batch():
    g = torch.Generator().manual_seed(13)
    xs = [torch.randn((8, 256, h, w), generator=g) * 0.7 * 0.01 + 0.07 for (h, w) in MAIN]
    ups = [torch.randn((8, 256, h, w), generator=g) for (h, w) in MAIN]
    gamma, beta = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    a = _node(xs, ups, gamma, beta, 32)
    b = _node(xs, ups, gamma, beta, 32)
    for u, v in zip(a[0] + a[1] + [a[2], a[3]], b[0] + b[1] + [b[2], b[3]]):
        assert torch.equal(u, v)
    alone = _node([x[5:6] for x in xs], [u[5:6] for u in ups], gamma, beta, 32)
    for u, v in zip(a[0] + a[1], alone[0] + alone[1]):
        assert torch.equal(u[5:6], v)


def test_an_upstream_gradient_off_16_bytes_is_taken():
    """a channels-last upstream gradient that starts 4 bytes into its storage: copied, same bits"""
    from iouaware import fcos_ops
    xs, ups, gamma, beta = _data(16, ODD, 2, 64, False)
    ref = _node(xs, ups, gamma, beta, 16)
    dx = [_cl(x).requires_grad_(True) for x in xs]
    gm, bt = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    ys = fcos_ops.groupnorm_relu(dx, gm, bt, 16)
    off = []
    for u in ups:
        B, ch, h, w = u.shape
        flat = torch.zeros(u.numel() + 1, device=DEV)
        v = flat[1:].view(B, h, w, ch).permute(0, 3, 1, 2)
        v.copy_(u.to(DEV))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous(memory_format=torch.channels_last)
        off.append(v)
    torch.autograd.backward(ys, off)
    torch.cuda.synchronize()
    for a, b in zip([x.grad.cpu() for x in dx] + [gm.grad.cpu(), bt.grad.cpu()], ref[1] + [ref[2], ref[3]]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the entries themselves
GUARD = 1024


def _guarded(shape, fill=float('nan')):
    """a (B, C, H, W) channels-last view of a flat buffer filled with `fill`, GUARD floats of -7
    behind it -> (view, flat)"""
    B, ch, h, w = shape
    n = B * ch * h * w
    flat = torch.full((n + GUARD,), fill, device=DEV)
    flat[n:] = -7.0
    return flat[:n].view(B, h, w, ch).permute(0, 3, 1, 2), flat


def _guard_ok(view, flat):
    n = view.numel()
    return bool(torch.isfinite(flat[:n]).all()) and bool((flat[n:] == -7.0).all())


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize('case', ['odd', 'main'])
def test_every_output_element_is_written_and_nothing_behind(case):
    """the C entries on NaN-filled outputs with a guard behind each: all written, the guard intact,
    and the same bits as the autograd node"""
    from iouaware import _lib, fcos_ops
    sizes, batch, ch, groups, relu, _ = CASES[case]
    xs, ups, gamma, beta = _data(14, sizes, batch, ch, False)
    ref = _node(xs, ups, gamma, beta, groups, relu)
    L = _lib.lib()
    g = fcos_ops.winograd._wino_geom(sizes, batch)
    dx_, du_ = [_cl(x) for x in xs], [_cl(u) for u in ups]
    gm, bt = gamma.to(DEV), beta.to(DEV)
    nws = L.ia_groupnorm_workspace_bytes(C.byref(g), ch, groups)
    nsv = L.ia_groupnorm_saved_bytes(C.byref(g), ch, groups)
    nbw = L.ia_groupnorm_bwd_workspace_bytes(C.byref(g), ch, groups)
    assert nws and nsv and nbw
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    saved = torch.full((nsv // 8 + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    saved[nsv // 8:] = -7.0
    bws = torch.full((nbw // 8 + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    bws[nbw // 8:] = -7.0
    ys = [_guarded(x.shape) for x in xs]
    dxs = [_guarded(x.shape) for x in xs]
    dgamma = torch.full((ch + GUARD,), float('nan'), device=DEV)
    dbeta = torch.full((ch + GUARD,), float('nan'), device=DEV)
    dgamma[ch:] = -7.0
    dbeta[ch:] = -7.0
    px, pu = _ptrs(dx_), _ptrs(du_)
    assert L.ia_groupnorm_stats(C.byref(g), px, ch, groups, _p(ws), nws, None) == 0
    assert L.ia_groupnorm_apply_to(C.byref(g), px, _ptrs([v for v, _ in ys]), ch, groups, _p(gm), _p(bt),
                                   1e-5, int(relu), _p(ws), nws, _p(saved), nsv, None) == 0
    assert L.ia_groupnorm_bwd_reduce(C.byref(g), px, pu, ch, groups, _p(gm), _p(bt), int(relu), _p(saved),
                                     nsv, _p(bws), nbw, None) == 0
    assert L.ia_groupnorm_bwd_apply(C.byref(g), px, pu, _ptrs([v for v, _ in dxs]), ch, groups, _p(gm),
                                    _p(bt), int(relu), _p(saved), nsv, _p(bws), nbw, _p(dgamma), _p(dbeta),
                                    None) == 0
    torch.cuda.synchronize()
    for view, flat in ys + dxs:
        assert _guard_ok(view, flat)
    n_saved = len(sizes) * batch * groups * 2
    assert bool(torch.isfinite(saved[:n_saved]).all()) and bool((saved[nsv // 8:] == -7.0).all())
    assert bool(torch.isfinite(bws[:nbw // 8]).all()) and bool((bws[nbw // 8:] == -7.0).all())
    for t in (dgamma, dbeta):
        assert bool(torch.isfinite(t[:ch]).all()) and bool((t[ch:] == -7.0).all())
    # the inputs are only read
    assert all(torch.equal(d.cpu(), x) for d, x in zip(dx_ + du_, xs + ups))
    for (view, _), r in zip(ys + dxs, ref[0] + ref[1]):
        assert torch.equal(view.cpu(), r)
    assert torch.equal(dgamma[:ch].cpu(), ref[2]) and torch.equal(dbeta[:ch].cpu(), ref[3])


def test_return_codes():
    from iouaware import _lib, fcos_ops
    sizes, batch, ch, groups = ODD, 2, 64, 16
    xs, ups, gamma, beta = _data(15, sizes, batch, ch, False)
    L = _lib.lib()
    g = fcos_ops.winograd._wino_geom(sizes, batch)
    bad_g = fcos_ops.winograd._wino_geom(sizes, batch)
    bad_g.num_levels = 0
    dx_, du_ = [_cl(x) for x in xs], [_cl(u) for u in ups]
    gm, bt = gamma.to(DEV), beta.to(DEV)
    nws = L.ia_groupnorm_workspace_bytes(C.byref(g), ch, groups)
    nsv = L.ia_groupnorm_saved_bytes(C.byref(g), ch, groups)
    nbw = L.ia_groupnorm_bwd_workspace_bytes(C.byref(g), ch, groups)
    assert L.ia_groupnorm_saved_bytes(C.byref(bad_g), ch, groups) == 0
    assert L.ia_groupnorm_bwd_workspace_bytes(C.byref(bad_g), ch, groups) == 0
    assert L.ia_groupnorm_bwd_workspace_bytes(C.byref(g), ch, 64) == 0          # one channel per group
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    saved = torch.empty(nsv, dtype=torch.uint8, device=DEV)
    bws = torch.empty(nbw, dtype=torch.uint8, device=DEV)
    ys = [torch.full_like(x, -7.0) for x in dx_]
    dxs = [torch.full_like(x, -7.0) for x in dx_]
    dg, db = torch.full((ch,), -7.0, device=DEV), torch.full((ch,), -7.0, device=DEV)
    assert L.ia_groupnorm_stats(C.byref(g), _ptrs(dx_), ch, groups, _p(ws), nws, None) == 0

    def fwd(g_=g, x=dx_, y=ys, c=ch, gr=groups, gamma_=gm, eps=1e-5, w=ws, nw=nws, s=saved, ns=nsv):
        return L.ia_groupnorm_apply_to(C.byref(g_), _ptrs(x) if x else None, _ptrs(y) if y else None, c, gr,
                                       _p(gamma_), _p(bt), eps, 1, _p(w), nw, _p(s), ns, None)

    def red(g_=g, x=dx_, u=du_, c=ch, gr=groups, s=saved, ns=nsv, w=bws, nw=nbw):
        return L.ia_groupnorm_bwd_reduce(C.byref(g_), _ptrs(x) if x else None, _ptrs(u) if u else None, c, gr,
                                         _p(gm), _p(bt), 1, _p(s), ns, _p(w), nw, None)

    def app(g_=g, x=dx_, u=du_, d=dxs, c=ch, gr=groups, s=saved, ns=nsv, w=bws, nw=nbw, dg_=dg, db_=db):
        return L.ia_groupnorm_bwd_apply(C.byref(g_), _ptrs(x) if x else None, _ptrs(u) if u else None,
                                        _ptrs(d) if d else None, c, gr, _p(gm), _p(bt), 1, _p(s), ns, _p(w),
                                        nw, _p(dg_), _p(db_), None)
    off = [x.flatten()[1:] for x in ys]                         # 4-byte aligned, not 16
    for call in (lambda: fwd(g_=bad_g), lambda: fwd(x=None), lambda: fwd(y=None), lambda: fwd(c=96),
                 lambda: fwd(gr=64), lambda: fwd(gamma_=None), lambda: fwd(eps=-1.0), lambda: fwd(w=None),
                 lambda: fwd(s=None), lambda: fwd(y=dx_), lambda: fwd(y=off),
                 lambda: red(g_=bad_g), lambda: red(x=None), lambda: red(u=None), lambda: red(c=96),
                 lambda: red(gr=64), lambda: red(s=None), lambda: red(w=None), lambda: red(u=off),
                 lambda: app(g_=bad_g), lambda: app(x=None), lambda: app(u=None), lambda: app(c=96),
                 lambda: app(gr=64), lambda: app(s=None), lambda: app(w=None), lambda: app(d=du_),
                 lambda: app(d=dx_), lambda: app(d=off)):
        assert call() == -1
    for call in (lambda: fwd(nw=nws - 1), lambda: fwd(ns=nsv - 1), lambda: red(ns=nsv - 1),
                 lambda: red(nw=nbw - 1), lambda: app(ns=nsv - 1), lambda: app(nw=nbw - 1)):
        assert call() == -2
    torch.cuda.synchronize()
    # nothing was launched: the outputs are as they were
    assert all(bool((t == -7.0).all()) for t in ys + dxs + [dg, db])
    assert fwd() == 0 and red() == 0 and app() == 0
    torch.cuda.synchronize()
    assert all(bool((t != -7.0).any()) for t in ys + dxs + [dg, db])
    ref = _node(xs, ups, gamma, beta, groups)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(ys + dxs + [dg, db], ref[0] + ref[1] + [ref[2], ref[3]]))
    # parameter gradients alone, and dx alone
    dg.fill_(-7.0)
    db.fill_(-7.0)
    assert app(d=None) == 0 and app(dg_=None, db_=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dg.cpu(), ref[2]) and torch.equal(db.cpu(), ref[3])


def test_front_end_refuses_before_the_device():
    from iouaware import fcos_ops
    x = _cl(torch.zeros((1, 64, 4, 4)))
    g, b = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    for bad in ([x.double()], [x.contiguous()], [x.cpu()], [x, _cl(torch.zeros((2, 64, 2, 2)))],
                [x, _cl(torch.zeros((1, 32, 2, 2)))], [x] * 9):
        with pytest.raises(ValueError):
            fcos_ops.groupnorm_relu(bad, g, b, 16)
    for gb in ((g.cpu(), b), (g.double(), b), (g[:32], b)):
        with pytest.raises(ValueError):
            fcos_ops.groupnorm_relu([x], gb[0], gb[1], 16)
    with pytest.raises(Exception):
        fcos_ops.groupnorm_relu([x], g, b, 64)                   # one channel per group

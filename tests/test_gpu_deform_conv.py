"""GPU: the deformable convolution kernels (csrc/deform.hip) and their autograd ops
(iouaware/deform_conv.py) against the definition (tests/dcn_ref.py).

Gates, the project's own (tests/test_gpu_wino_fp64.py): against the yardstick in fp64 on the same
fp32 tensors, for each of y, dx, d_offset, d_mask, dW, db as max|got - ref| / max|ref|,
    gate A  <= 1e-4, and
    gate B  <= 4 x the same figure of the yardstick evaluated in fp32 on the CPU.
The yardstick's fp32 figure is the largest over dcn_ref.ORDERS evaluations of the case that differ
only in the order of their sums (dcn_ref.evaluate's `order`; the reasoning stands next to
dcn_ref.GATE_B): at these sizes one order's figure is between a third of an ulp and three, by luck,
and dx -- whose order on the GPU is not fixed -- would be judged by that luck.  No floor under it.
tests/test_host_dcn_ref.py adds the kernel's own fp32 dx terms in thousands of random orders on the
CPU: none comes near the gate, so the outcome does not depend on the order the atomics arrive in.

Cases (dcn_ref.CHANNELS x MAPS x GEOMS x v1 / modulated, batch 3): the smallest that exercise every
index path -- 4 / 12 / 8 channels per deformable group (one float4, a run that is no power of two,
one group), odd maps smaller than a wavefront's runs and larger than a block's, stride and dilation
1 and 2, NCHW and channels-last inputs, and a column cap that holds 2 images so the batch goes in
two chunks, the second short.  Offsets are uniform in +-3 px with fractional sampling positions in
eighths: no sample on a kink, so no derivative depends on a tie.

Every buffer the new kernels write (col, y, dx, d_offset, d_mask) is handed over full of NaN with a
NaN guard behind it: every element is written and nothing behind the buffer is.  That covers dx,
which the entry zero-fills itself.

Reproducibility: y, d_offset, d_mask, dW and db are asserted bit-identical across two runs.  dx is
NOT: it is scattered with fp32 atomicAdd and the order in which the adds of different output pixels
arrive is not fixed; it is gated like the others and not compared across runs.

Measured on an MI355X (2026-10-19; worst over the 48 cases and the three chunkings, printed by
test_print_worst_ratios: error against fp64, in brackets the multiple of the fp32 figure):
    y 4.73e-07 (2.17 x)   d_offset 1.90e-07 (1.36 x)   d_mask 1.97e-07 (0.94 x)
    dW 3.41e-07 (1.24 x)   db 2.42e-07 (3.27 x)      -- the same bits, hence the same figures, in every run
    dx 2.74e-07 (1.37 x) in each of two runs, which says little about a quantity whose order is not fixed;
       what bounds it is not those samples but the CPU test: its fp32 terms in 2000 random orders of
       the worst case stay under 2.13 x, in 60 orders of each of the 48 cases under 1.70 x.
"""
import pytest
import torch
import torch.nn.functional as F

import dcn_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _cases():
    n = 0
    for (Cc, dg, Co) in R.CHANNELS:
        for (H, W) in R.MAPS:
            for (s, dl) in R.GEOMS:
                for mod in (False, True):
                    yield pytest.param(Cc, dg, Co, H, W, s, dl, mod, bool(n % 2),
                                       id='C%d-dg%d-o%d-%dx%d-s%d-d%d-%s-%s' % (
                                           Cc, dg, Co, H, W, s, dl, 'v2' if mod else 'v1', 'nhwc' if n % 2 else 'nchw'))
                    n += 1


def _layout(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()


def _cap_for(d, images=2):
    """a column cap (bytes) under which exactly `images` images fit"""
    B, Cc, H, W = d['x'].shape
    Ho, Wo = R.out_hw(H, W, 3, d['stride'], d['padding'], d['dilation'])
    return images * Ho * Wo * 9 * Cc * 4 + 4


def _run_op(d, channels_last, col_cap):
    from iouaware import deform_conv, modulated_deform_conv
    t = {}
    for k in ('x', 'offset', 'mask', 'weight', 'bias'):
        v = d[k]
        if v is None:
            t[k] = None
        else:
            v = v.detach().to(DEV)
            if v.dim() == 4 and k != 'weight':
                v = _layout(v, channels_last)
            t[k] = v.detach().requires_grad_(True)
            assert t[k].is_leaf
    geom = (d['stride'], d['padding'], d['dilation'], 1, d['dg'])
    if t['mask'] is None:
        y = deform_conv(t['x'], t['offset'], t['weight'], *geom, col_cap=col_cap)
    else:
        y = modulated_deform_conv(t['x'], t['offset'], t['mask'], t['weight'], t['bias'], *geom, col_cap=col_cap)
    cl = torch.channels_last
    assert y.is_contiguous(memory_format=cl) if channels_last else y.is_contiguous()     # the input's format
    y.backward(_layout(d['dy'].to(DEV), channels_last))
    torch.cuda.synchronize()
    g = lambda k: None if t[k] is None else t[k].grad                   # noqa: E731
    out = dict(y=y.detach(), dx=g('x'), d_offset=g('offset'), d_mask=g('mask'), dW=g('weight'), db=g('bias'))
    for k, src in (('dx', 'x'), ('d_offset', 'offset'), ('dW', 'weight')):
        assert out[k] is not None, k
        assert out[k].shape == d[src].shape, k
    return out


WORST = {}


def _gates(tag, got, d):
    ref = R.evaluate(d, torch.float64)
    fig = R.fp32_figure(d, ref)                         # per quantity: (largest, smallest) over the orders
    rep = {}
    for k in R.NAMES:
        if ref[k] is None:
            assert got[k] is None
            continue
        assert bool(torch.isfinite(got[k]).all()), k
        e, h = R.rel_err(got[k], ref[k]), fig[k][0]
        assert h > 0, k
        rep[k] = (e, h, e / h)
        w = WORST.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], e), max(w[1], rep[k][2])
    print('  %-34s ' % tag + '  '.join('%s %.2e (%.2f x)' % (k, v[0], v[2]) for k, v in rep.items()))
    for k, (e, h, ratio) in rep.items():
        assert e <= R.GATE_A, 'gate A: %s %s %.3e' % (tag, k, e)
        assert ratio <= R.GATE_B, 'gate B: %s %s HIP %.3e vs fp32 yardstick %.3e = %.2f x' % (tag, k, e, h, ratio)


# ------------------------------------------------------------------ forward + backward, gated
@pytest.mark.parametrize('Cc,dg,Co,H,W,s,dl,mod,cl', list(_cases()))
def test_forward_backward_against_fp64(Cc, dg, Co, H, W, s, dl, mod, cl):
    d = R.case(Cc, dg, Co, H, W, s, dl, mod)
    cap = _cap_for(d)                                   # batch 3 in chunks of 2 + 1
    a = _run_op(d, cl, cap)
    _gates('%s chunks of 2' % ('nhwc' if cl else 'nchw'), a, d)
    b = _run_op(d, cl, cap)
    for k in ('y', 'd_offset', 'd_mask', 'dW', 'db'):   # not dx: atomics, see the module docstring
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), 'not bit-identical across two runs: %s' % k


def test_every_chunking_passes_the_gates():
    """one chunk of 3, chunks of 2 + 1 and of 1 + 1 + 1 (the library GEMM may pick another kernel for
    another row count, so the chunkings are gated, not compared bit for bit)"""
    d = R.case(16, 4, 12, 7, 9, 1, 1, True, seed=1)
    _gates('one chunk', _run_op(d, True, None), d)
    for images in (2, 1):
        _gates('chunks of %d' % images, _run_op(d, True, _cap_for(d, images)), d)


def test_print_worst_ratios():
    """(collected last in this file) the worst figures over the cases above, for DESIGN 3.20"""
    print('\n  worst over all cases: ' + '  '.join('%s %.2e (%.2f x)' % (k, v[0], v[1]) for k, v in WORST.items()))


# ------------------------------------------------------------------ NaN-filled buffers with guards
GUARD = 64


def _guarded(shape):
    """a channels-last (B, C, H, W) view [or a (rows, k) matrix] of a NaN-filled buffer + NaN guard"""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + GUARD,), NAN, device=DEV)
    if len(shape) == 2:
        return buf, buf[:n].view(shape)
    B, Cn, H, W = shape
    return buf, buf[:n].view(B, H, W, Cn).permute(0, 3, 1, 2)


def _check_guard(name, buf, view):
    assert not bool(torch.isnan(view).any()), '%s: an element was not written' % name
    assert bool(torch.isnan(buf[view.numel():]).all()), '%s: written behind the buffer' % name


@pytest.mark.parametrize('Cc,dg,Co', R.CHANNELS)
@pytest.mark.parametrize('H,W,s,dl', [(7, 9, 1, 1), (5, 4, 2, 1), (7, 9, 2, 2), (5, 4, 1, 2)])
@pytest.mark.parametrize('mod', [False, True])
def test_every_element_is_written_and_nothing_behind(Cc, dg, Co, H, W, s, dl, mod):
    from iouaware import ops
    d = R.case(Cc, dg, Co, H, W, s, dl, mod, seed=3)
    cl = torch.channels_last
    x = d['x'].to(DEV).contiguous(memory_format=cl)
    off = d['offset'].to(DEV).contiguous(memory_format=cl)
    mask = None if not mod else d['mask'].to(DEV).contiguous(memory_format=cl)
    B = x.shape[0]
    Ho, Wo = off.shape[-2:]
    w_kn = ops.conv3x3_weight_kn(d['weight'].to(DEV))
    bias = None if d['bias'] is None else d['bias'].to(DEV)
    ref = R.evaluate(d, torch.float64)
    # col
    bc, col = _guarded((B * Ho * Wo, 9 * Cc))
    ops.deform_im2col3x3(x, off, mask, s, 1, dl, dg, out=col)
    # y, through the chunks
    by, y = _guarded((B, Co, Ho, Wo))
    ops.deform_conv3x3(x, off, mask, w_kn, bias, s, 1, dl, dg, col_cap=_cap_for(d), out=y)
    # dx (zero-filled by the entry), d_offset, d_mask
    outs = [_guarded((B, Cc, H, W)), _guarded((B, dg * 18, Ho, Wo)), _guarded((B, dg * 9, Ho, Wo)) if mod else (None, None)]
    g = d['dy'].to(DEV).contiguous(memory_format=cl)
    dx, do, dm, dw = ops.deform_conv3x3_backward(g, x, off, mask, w_kn, s, 1, dl, dg, col_cap=_cap_for(d),
                                                 out=tuple(v for _, v in outs))
    torch.cuda.synchronize()
    _check_guard('col', bc, col)
    _check_guard('y', by, y)
    for name, (buf, view) in zip(('dx', 'd_offset', 'd_mask'), outs):
        if buf is not None:
            _check_guard(name, buf, view)
    assert dx.data_ptr() == outs[0][1].data_ptr() and do.data_ptr() == outs[1][1].data_ptr()
    # and they are the right numbers
    assert R.rel_err(y, ref['y']) <= R.GATE_A and R.rel_err(dx, ref['dx']) <= R.GATE_A
    assert R.rel_err(do, ref['d_offset']) <= R.GATE_A
    if mod:
        assert R.rel_err(dm, ref['d_mask']) <= R.GATE_A
    assert R.rel_err(dw.view(Co, 3, 3, Cc).permute(0, 3, 1, 2), ref['dW']) <= R.GATE_A
    # col against the definition: the samples times the mask, row order (tap, channel)
    hh, ww = R.positions(d['offset'].double(), H, W, 3, 3, s, 1, dl, dg)
    smp = R.sample(d['x'].double(), hh, ww, dg)                                    # (B, C, K, Ho, Wo)
    if mod:
        smp = (smp.view(B, dg, Cc // dg, 9, Ho, Wo) * d['mask'].double().view(B, dg, 1, 9, Ho, Wo)).view(B, Cc, 9, Ho, Wo)
    want = smp.permute(0, 3, 4, 2, 1).reshape(B * Ho * Wo, 9 * Cc)
    assert R.rel_err(col, want) <= 1e-6


# ------------------------------------------------------------------ forward-only cases
def _fwd(x, off, mask, w, bias, s, p, dl, dg, cl=True):
    from iouaware import deform_conv, modulated_deform_conv
    x, off = _layout(x.to(DEV), cl), _layout(off.to(DEV), cl)
    with torch.no_grad():
        if mask is None:
            return deform_conv(x, off, w.to(DEV), s, p, dl, 1, dg)
        return modulated_deform_conv(x, off, _layout(mask.to(DEV), cl), w.to(DEV),
                                     None if bias is None else bias.to(DEV), s, p, dl, 1, dg)


@pytest.mark.parametrize('Cc,dg,Co', R.CHANNELS)
@pytest.mark.parametrize('s,p,dl', [(1, 1, 1), (2, 1, 1), (1, 2, 2), (2, 1, 2), (3, 0, 1)])
def test_zero_offsets_are_the_plain_convolution(Cc, dg, Co, s, p, dl):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, Cc, 7, 9, generator=g)
    w = torch.randn(Co, Cc, 3, 3, generator=g) / (3 * Cc ** 0.5)
    b = torch.randn(Co, generator=g)
    Ho, Wo = R.out_hw(7, 9, 3, s, p, dl)
    off = torch.zeros(3, dg * 18, Ho, Wo)
    ref = F.conv2d(x.double(), w.double(), b.double(), s, p, dl)
    y1 = _fwd(x, off, None, w, None, s, p, dl, dg, cl=False)
    y2 = _fwd(x, off, torch.ones(3, dg * 9, Ho, Wo), w, b, s, p, dl, dg)
    assert R.rel_err(y2, ref) <= 1e-5 and R.rel_err(y1, ref - b.double().view(1, -1, 1, 1)) <= 1e-5


@pytest.mark.parametrize('dy,dx', [(1, 0), (0, -2), (-3, 2)])
def test_integer_offsets_are_the_shifted_convolution(dy, dx):
    g = torch.Generator().manual_seed(6)
    H, W, p, m = 7, 9, 1, 5
    x = torch.randn(3, 8, H, W, generator=g)
    w = torch.randn(5, 8, 3, 3, generator=g) / 8
    for s, dl in ((1, 1), (2, 2)):
        Ho, Wo = R.out_hw(H, W, 3, s, p, dl)
        off = torch.zeros(3, 18, Ho, Wo)
        off[:, 0::2], off[:, 1::2] = dy, dx
        xb = F.pad(x.double(), (m, m, m, m))
        win = xb[:, :, m - p + dy: m - p + dy + H + 2 * p, m - p + dx: m - p + dx + W + 2 * p]
        ref = F.conv2d(win, w.double(), None, s, 0, dl)
        assert R.rel_err(_fwd(x, off, None, w, None, s, p, dl, 1), ref) <= 1e-5


def test_border_probes():
    """one output pixel per probe (a 1-wide map, stride 1, pad 0 would need H >= 3: instead a weight
    with a single 1 at the centre tap and the probe as that tap's offset): h = -1, -0.5, 0, H-1, H-0.5,
    H give 0, half of row 0, row 0, row H-1, half of row H-1, 0; the same in w"""
    H, W, Cn = 5, 6, 8
    x = torch.arange(1, 1 + Cn * H * W, dtype=torch.float32).view(1, Cn, H, W) / 16      # exact in fp32
    w = torch.zeros(Cn, Cn, 3, 3)
    w[:, :, 1, 1] = torch.eye(Cn)                                                       # y = the centre tap's sample
    for axis, size in ((0, H), (1, W)):
        probes = [-1.0, -0.5, 0.0, size - 1.0, size - 0.5, float(size)]
        for val in probes:
            off = torch.zeros(1, 18, H, W)
            # the centre tap of output pixel (ho, wo) sits at (ho, wo): move it to `val` along the axis
            base = torch.arange(size, dtype=torch.float32).view((size, 1) if axis == 0 else (1, size))
            off[0, 8 + axis] = val - base
            y = _fwd(x, off, None, w, None, 1, 1, 1, 1).cpu()
            if val <= -1 or val >= size:
                want = torch.zeros_like(x)
            else:
                lo = int(torch.tensor(val).floor())
                f = val - lo
                edge = lambda i: x.select(2 + axis, i) if 0 <= i <= size - 1 else 0 * x.select(2 + axis, 0)   # noqa: E731
                line = (1 - f) * edge(lo) + f * edge(lo + 1)
                want = line.unsqueeze(2 + axis).expand_as(x)
            assert torch.equal(y, want.contiguous()), (axis, val)


def test_offsets_that_empty_whole_rows_of_col():
    """every tap of some output pixels sampled far outside: their rows of col are zero, y there is the
    bias; NaN / inf offsets count as outside as well"""
    from iouaware import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 16, 7, 9, generator=g)
    w = torch.randn(12, 16, 3, 3, generator=g) / 12
    b = torch.randn(12, generator=g)
    off = torch.zeros(3, 72, 7, 9)
    off[:, :, 2] = 1e6
    off[:, :, 4] = -1e6
    off[:, :, 5, 3] = float('inf')
    off[:, :, 5, 4] = NAN
    off[:, :, 6] = 40.0
    mask = torch.ones(3, 36, 7, 9)
    y = _fwd(x, off, mask, w, b, 1, 1, 1, 4).cpu()
    for row in (2, 4, 6):
        assert torch.equal(y[:, :, row], b.view(1, -1, 1).expand(3, 12, 9))
    assert torch.equal(y[:, :, 5, 3:5], b.view(1, -1, 1).expand(3, 12, 2))
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    assert R.rel_err(y[:, :, :2], ref[:, :, :2]) <= 1e-5
    cl = torch.channels_last
    col = ops.deform_im2col3x3(x.to(DEV).contiguous(memory_format=cl), off.to(DEV).contiguous(memory_format=cl),
                               None, 1, 1, 1, 4).view(3, 7, 9, 144)
    assert float(col[:, 2].abs().max()) == 0 and float(col[:, 4].abs().max()) == 0 and float(col[:, 6].abs().max()) == 0
    assert float(col[:, 5, 3:5].abs().max()) == 0 and float(col[:, 0].abs().max()) > 0


def test_mask_logits_and_channel_slices_of_one_tensor():
    """the fused route's call: offsets and mask logits as channel slices of one channels-last tensor,
    the sigmoid taken in the kernel, BN-like bias and ReLU in the GEMM epilogue"""
    from iouaware import ops
    d = R.case(16, 4, 12, 7, 9, 2, 1, True, seed=4)
    cl = torch.channels_last
    logits = torch.randn(d['mask'].shape, generator=torch.Generator().manual_seed(9))
    om = torch.cat([d['offset'], logits], 1).to(DEV).contiguous(memory_format=cl)
    n = 18 * 4
    x = d['x'].to(DEV).contiguous(memory_format=cl)
    y = ops.deform_conv3x3(x, om[:, :n], om[:, n:], ops.conv3x3_weight_kn(d['weight'].to(DEV)), d['bias'].to(DEV),
                           2, 1, 1, 4, relu=True, mask_logits=True, col_cap=_cap_for(d))
    ref = F.relu(R.modulated_deform_conv(d['x'].double(), d['offset'].double(), torch.sigmoid(logits.double()),
                                         d['weight'].double(), d['bias'].double(), 2, 1, 1, 4))
    assert R.rel_err(y, ref) <= 1e-5

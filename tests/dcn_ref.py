"""Deformable convolution (DCN v1 / v2) written from its definition in plain torch, in any floating
dtype and on any device.  Test-only: nothing imported from the project, no code shared with the
kernels (csrc/deform.hip) or with the reference's extension; index arithmetic, validity masks and
`gather`, differentiable by autograd.  It is the yardstick of tests/test_gpu_deform_conv.py and
tests/test_gpu_dcn_backbone.py -- in fp64 as the definition, in fp32 as "what a correct fp32
evaluation loses" -- and is itself pinned by tests/test_host_dcn_ref.py.

    y[b, o, ho, wo] = bias[o] + sum_{c, i, j} W[o, c, i, j] * mask[b, g K + k, ho, wo] * S(x[b, c]; h, w)
    k = i * kw + j,  K = kh * kw,  g = c // (C / dg)
    h = ho * s - p + i * d + offset[b, g 2K + 2k,     ho, wo]
    w = wo * s - p + j * d + offset[b, g 2K + 2k + 1, ho, wo]
    S = 0 unless -1 < h < H and -1 < w < W; else bilinear over the corners (floor, floor + 1), a corner
        outside [0, H - 1] x [0, W - 1] contributing 0

`floor` has no derivative, so autograd differentiates exactly this piecewise formula with the corners
held: what the issue asks of the backward pass.

`variant` builds the nearest WRONG operators, for the tests that show the yardstick (and the data of
the GPU tests) tells them apart:
    'border_ge0'   the sample is dropped unless 0 <= h <= H - 1 (and w): loses the half-weighted rim
    'swap_xy'      offset channel 2k read as the x offset, 2k + 1 as the y offset
    'tap_major'    offset channel (2k) * dg + 2g instead of g * 2K + 2k (differs for dg > 1 only)
    'no_mask'      the mask is ignored
"""
import torch

VARIANTS = ('border_ge0', 'swap_xy', 'tap_major', 'no_mask')


def out_hw(H, W, k, stride, padding, dilation):
    e = dilation * (k - 1) + 1
    return (H + 2 * padding - e) // stride + 1, (W + 2 * padding - e) // stride + 1


def positions(offset, H, W, kh, kw, stride, padding, dilation, dg, variant=None):
    """offset (B, dg * 2K, Ho, Wo) -> sampling positions (h, w), each (B, dg, K, Ho, Wo)"""
    B, _, Ho, Wo = offset.shape
    K = kh * kw
    dt, dev = offset.dtype, offset.device
    if variant == 'tap_major':
        o = offset.reshape(B, K, dg, 2, Ho, Wo).permute(0, 2, 1, 3, 4, 5)
    else:
        o = offset.reshape(B, dg, K, 2, Ho, Wo)
    oy, ox = (o[:, :, :, 1], o[:, :, :, 0]) if variant == 'swap_xy' else (o[:, :, :, 0], o[:, :, :, 1])
    i = torch.arange(kh, device=dev).repeat_interleave(kw).to(dt).view(1, 1, K, 1, 1)
    j = torch.arange(kw, device=dev).repeat(kh).to(dt).view(1, 1, K, 1, 1)
    ho = torch.arange(Ho, device=dev).to(dt).view(1, 1, 1, Ho, 1)
    wo = torch.arange(Wo, device=dev).to(dt).view(1, 1, 1, 1, Wo)
    return ho * stride - padding + i * dilation + oy, wo * stride - padding + j * dilation + ox


def sample(x, h, w, dg, variant=None, perm=None):
    """x (B, C, H, W); h, w (B, dg, K, Ho, Wo) -> samples (B, C, K, Ho, Wo).  perm: a permutation of the
    K * Ho * Wo samples of an image -- the order in which they are gathered and hence in which autograd
    adds them into dx (the same numbers in exact arithmetic, another order of the fp sums)"""
    B, C, H, W = x.shape
    K, Ho, Wo = h.shape[2:]
    cg = C // dg
    if variant == 'border_ge0':
        inside = (h >= 0) & (w >= 0) & (h <= H - 1) & (w <= W - 1)
    else:
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    h0, w0 = torch.floor(h).detach(), torch.floor(w).detach()
    lh, lw = h - h0, w - w0
    xg = x.reshape(B, dg, cg, H * W)
    out = 0
    for dh in (0, 1):
        for dw in (0, 1):
            hc, wc = h0 + dh, w0 + dw
            valid = inside & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
            idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long().reshape(B, dg, 1, -1)
            idx = idx.expand(B, dg, cg, idx.shape[-1])
            if perm is None:
                v = xg.gather(3, idx)
            else:
                v = xg.gather(3, idx[..., perm])[..., torch.argsort(perm)]
            v = v.reshape(B, dg, cg, K, Ho, Wo)
            wt = (lh if dh else 1 - lh) * (lw if dw else 1 - lw)
            wt = torch.where(valid, wt, torch.zeros_like(wt))
            out = out + v * wt.unsqueeze(2)
    return out.reshape(B, C, K, Ho, Wo)


def modulated_deform_conv(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1,
                          deformable_groups=1, variant=None, perm=None):
    """mask None: DCN v1.  groups = 1.  perm: see sample()"""
    B, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    dg, K = deformable_groups, kh * kw
    h, w = positions(offset, H, W, kh, kw, stride, padding, dilation, dg, variant)
    s = sample(x, h, w, dg, variant, perm)                              # (B, C, K, Ho, Wo)
    if mask is not None and variant != 'no_mask':
        Ho, Wo = s.shape[-2:]
        m = mask.reshape(B, dg, 1, K, Ho, Wo)
        s = (s.reshape(B, dg, C // dg, K, Ho, Wo) * m).reshape(B, C, K, Ho, Wo)
    y = torch.einsum('bckhw,ock->bohw', s, weight.reshape(O, C, K))
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y


def deform_conv(x, offset, weight, stride=1, padding=0, dilation=1, deformable_groups=1, variant=None):
    return modulated_deform_conv(x, offset, None, weight, None, stride, padding, dilation,
                                 deformable_groups, variant)


# ------------------------------------------------------------------ the data of the GPU op tests
# (C, dg, Cout): the smallest run of 4 channels per group (16, 4), a group that is no power of two
# (24, 2 -> 12) and one group; output widths that are no multiple of 4
CHANNELS = [(8, 1, 5), (16, 4, 12), (24, 2, 7)]
MAPS = [(7, 9), (5, 4)]
GEOMS = [(1, 1), (2, 1), (1, 2), (2, 2)]          # (stride, dilation); padding 1
BATCH = 3


def case(C, dg, Cout, H, W, stride, dilation, modulated, seed=0, batch=BATCH, padding=1):
    """fp32 CPU tensors of one forward + backward case: offsets uniform in +-3 px whose sampling
    positions (an integer base + the offset) have a fractional part from {1/8 .. 7/8} in both
    directions -- no sample on a kink of the piecewise-linear formula, so no derivative depends on a
    tie -- normal mask logits (modulated: mask = sigmoid), normal x / weight / bias and an upstream
    gradient.  Eighths are exact in fp32 and fp64 alike."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * C + 5 * H + 3 * stride + dilation + int(modulated))
    Ho, Wo = out_hw(H, W, 3, stride, padding, dilation)
    assert Ho >= 1 and Wo >= 1
    d = dict(C=C, dg=dg, Cout=Cout, stride=stride, padding=padding, dilation=dilation)
    d['x'] = torch.randn(batch, C, H, W, generator=g)
    whole = torch.randint(-3, 3, (batch, dg * 18, Ho, Wo), generator=g).float()
    eighths = torch.randint(1, 8, (batch, dg * 18, Ho, Wo), generator=g).float() / 8
    d['offset'] = whole + eighths                                        # in (-3, 3)
    d['mask'] = torch.sigmoid(torch.randn(batch, dg * 9, Ho, Wo, generator=g)) if modulated else None
    d['weight'] = torch.randn(Cout, C, 3, 3, generator=g) / (3.0 * C ** 0.5)
    d['bias'] = torch.randn(Cout, generator=g) if modulated else None
    d['dy'] = torch.randn(batch, Cout, Ho, Wo, generator=g)
    return d


NAMES = ('y', 'dx', 'd_offset', 'd_mask', 'dW', 'db')


def evaluate(d, dtype, variant=None, device='cpu', order=None):
    """the yardstick on a case in `dtype`: {name: tensor} for NAMES (absent: None).

    order (an int seed; None: the data as it stands): the SAME case under a random relabelling -- the
    images, the output channels and the input channels inside each deformable group permuted, the
    samples of an image gathered in a permuted order -- with the results put back in place.  In exact
    arithmetic nothing changes; in fp32 every sum of the evaluation (over channels and taps in y, over
    output channels in dcol, over a group's channels in d_offset / d_mask, over images and pixels in
    dW / db, over the samples that touch a pixel in dx) runs in another order."""
    t = {k: (v.detach().clone().to(device=device, dtype=dtype) if torch.is_tensor(v) else v) for k, v in d.items()}
    B, C = t['x'].shape[:2]
    O, dg = t['weight'].shape[0], d['dg']
    pb, po, pc, ps = torch.arange(B), torch.arange(O), torch.arange(C), None
    if order is not None:
        g = torch.Generator().manual_seed(7919 * int(order) + 1)
        cg = C // dg
        pb, po = torch.randperm(B, generator=g), torch.randperm(O, generator=g)
        pc = torch.cat([i * cg + torch.randperm(cg, generator=g) for i in range(dg)])
        ps = torch.randperm(9 * t['offset'].shape[2] * t['offset'].shape[3], generator=g)
    pb, po, pc = pb.to(device), po.to(device), pc.to(device)
    ps = None if ps is None else ps.to(device)
    t['x'] = t['x'][pb][:, pc]
    t['offset'] = t['offset'][pb]
    t['mask'] = None if t['mask'] is None else t['mask'][pb]
    t['weight'] = t['weight'][po][:, pc]
    t['bias'] = None if t['bias'] is None else t['bias'][po]
    t['dy'] = t['dy'][pb][:, po]
    for k in ('x', 'offset', 'mask', 'weight', 'bias'):
        if t[k] is not None:
            t[k] = t[k].contiguous().requires_grad_(True)
    y = modulated_deform_conv(t['x'], t['offset'], t['mask'], t['weight'], t['bias'], d['stride'],
                              d['padding'], d['dilation'], dg, variant, ps)
    y.backward(t['dy'].contiguous())
    ib, io, ic = torch.argsort(pb), torch.argsort(po), torch.argsort(pc)
    def g(k, *back):                       # the gradient of t[k] put back in place (None: absent or unused)
        v = None if t[k] is None else t[k].grad
        if v is not None:
            v = v[back[0]] if len(back) == 1 else v[back[0]][:, back[1]]
        return v
    return dict(y=y.detach()[ib][:, io], dx=g('x', ib, ic), d_offset=g('offset', ib), d_mask=g('mask', ib),
                dW=g('weight', io, ic), db=g('bias', io))


def dx_terms(d, dtype):
    """dx from its definition as ONE sum per element: the terms dcol * mask * corner weight of every
    (sample, corner) that touches it, in `dtype`, with their flat destinations -> (index, value, numel).
    dcol = dy . W^T; each factor is rounded where csrc/deform.hip rounds it.  What is left open is the
    order in which the terms are added: dx_in_order."""
    x, off, w = (d[k].to(dtype) for k in ('x', 'offset', 'weight'))
    B, C, H, W = x.shape
    dg, O = d['dg'], w.shape[0]
    cg = C // dg
    h, ww = positions(off, H, W, 3, 3, d['stride'], d['padding'], d['dilation'], dg)
    Ho, Wo = h.shape[-2:]
    dcol = torch.einsum('bohw,ock->bckhw', d['dy'].to(dtype), w.reshape(O, C, 9))          # (B, C, 9, Ho, Wo)
    m = torch.ones_like(h) if d['mask'] is None else d['mask'].to(dtype).reshape(B, dg, 9, Ho, Wo)
    dm = dcol.reshape(B, dg, cg, 9, Ho, Wo) * m.unsqueeze(2)
    inside = (h > -1) & (ww > -1) & (h < H) & (ww < W)
    h0, w0 = torch.floor(h), torch.floor(ww)
    lh, lw = h - h0, ww - w0
    chan = torch.arange(dg).view(1, dg, 1, 1, 1, 1) * cg + torch.arange(cg).view(1, 1, cg, 1, 1, 1)
    base = (torch.arange(B).view(B, 1, 1, 1, 1, 1) * C + chan) * (H * W)
    idx, val = [], []
    for dh in (0, 1):
        for dw in (0, 1):
            hc, wc = h0 + dh, w0 + dw
            ok = inside & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
            wt = (lh if dh else 1 - lh) * (lw if dw else 1 - lw)
            pos = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long()
            sel = ok.unsqueeze(2).expand_as(dm)
            idx.append((base + pos.unsqueeze(2))[sel])
            val.append((dm * wt.unsqueeze(2))[sel])
    return torch.cat(idx), torch.cat(val), x.numel()


def dx_in_order(terms, shape, perm=None):
    """the terms added one after the other in the order `perm` (a serial index_add_ on the CPU)"""
    idx, val, n = terms
    if perm is not None:
        idx, val = idx[perm], val[perm]
    return torch.zeros(n, dtype=val.dtype).index_add_(0, idx, val).view(shape)


ORDERS = 16


def fp32_figure(d, ref, orders=ORDERS):
    """{name: (largest, smallest)} of rel_err(fp32 yardstick, ref) over the data as it stands and
    orders - 1 relabellings of it (evaluate's `order`): the fp32 yardstick's own error for gate B"""
    out = {}
    for o in [None] + list(range(1, orders)):
        f32 = evaluate(d, torch.float32, order=o)
        for k in NAMES:
            if ref[k] is not None:
                e = rel_err(f32[k], ref[k])
                hi, lo = out.get(k, (0.0, float('inf')))
                out[k] = (max(hi, e), min(lo, e))
    # dx is one sum per element whose order the GPU does not fix: its figure also covers the fp32 terms
    # added serially in `orders` random orders
    terms = dx_terms(d, torch.float32)
    g = torch.Generator().manual_seed(4242)
    for _ in range(orders):
        e = rel_err(dx_in_order(terms, d['x'].shape, torch.randperm(terms[0].numel(), generator=g)), ref['dx'])
        out['dx'] = (max(out['dx'][0], e), min(out['dx'][1], e))
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref|, in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


GATE_A = 1e-4         # the project's fp32 contract: every quantity within 1e-4 of its maximum
GATE_B = 4.0          # at most this multiple of the fp32 yardstick's own error (wino_ref.GATE_B's factor
                      # and reasoning: another summation order moves an fp32 error by up to ~2-3 x)
# What "the fp32 yardstick's own error" is at these sizes.  The cases are the smallest that reach every
# index path, so every sum has a few dozen terms and a correct fp32 evaluation loses about one ulp
# of the maximum -- or, by luck of its summation order, a third of one (3.4e-08 was seen) or three.
# One order's figure is therefore a statement about luck, and for dx, whose order on the GPU is not
# fixed (atomics), so is the figure it would be compared with.  The yardstick's fp32 error is taken
# as the LARGEST over ORDERS evaluations of the same case that differ in the order of every sum and
# in nothing else (evaluate's `order`): what a correct fp32 evaluation loses in an unlucky order.
# For dx the orders include the plain serial sum of its fp32 terms (dx_terms) in ORDERS random orders:
# that IS what the GPU computes, in an order nobody fixes, and autograd's own accumulation (four
# partial scatters, then added) is more accurate than any serial order.
# The gate is 4 x that figure, as the issue sets it, with no floor under it.
# tests/test_host_dcn_ref.py shows on the CPU that the figure is never 0 on the GPU test's data and
# that the kernel's own fp32 terms, added into dx in thousands of random orders, stay inside it.

"""A plain restatement of Winograd F(4x4,3x3) convolution over a list of pyramid levels, in any
floating dtype and on any device.  Test-only, pure torch, nothing imported from the project: it is
the yardstick the HIP transforms (csrc/wino.hip) and the training node (iouaware/winograd_train.py)
are measured against -- in fp64 as the definition, in fp32 as "what a correct fp32 evaluation of
the same algorithm loses".

Matrices: Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", interpolation points
0, +-1, +-2, inf.  Tile list: level-major, then image, then row-major 4x4 output tiles,
ceil(H/4) * ceil(W/4) per image; tile (ty, tx) reads the 6x6 input patch whose corner is
(4 ty - 1, 4 tx - 1) and owns the output pixels [4 ty, 4 ty + 4) x [4 tx, 4 tx + 4).

    V = B^T d B        (36, T, Cin)      input_transform
    U = G w G^T        (36, Cin, Cout)   weight_transform      (fp64, rounded once)
    M[k] = V[k] U[k]   (36, T, Cout)
    Y = A^T M A + b                      output_transform
    dM = A dY A^T      (36, T, Cout)     grad_output_transform (dY zero outside the map)
    dU[k] = V[k]^T dM[k], dW = G^T dU G  weight_grad           (fp64, rounded once)
    dX = the forward steps on dY with w transposed and rotated by 180 degrees
"""
import torch
import torch.nn.functional as F

BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                   [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
                  dtype=torch.float64)
G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
                  [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0],
                   [0, 1, -1, 8, -8, 1]], dtype=torch.float64)


def tiles_of(h, w):
    return ((h + 3) // 4) * ((w + 3) // 4)


def tile_count(sizes, batch):
    return batch * sum(tiles_of(h, w) for (h, w) in sizes)


def tile_index(sizes, batch, t):
    """flat tile index -> (level, image, tile row, tile column)"""
    for l, (h, w) in enumerate(sizes):
        n = batch * tiles_of(h, w)
        if t < n:
            b, i = divmod(t, tiles_of(h, w))
            ty, tx = divmod(i, (w + 3) // 4)
            return l, b, ty, tx
        t -= n
    raise IndexError(t)


def _mat(m, ref, absolute):
    m = m.to(device=ref.device, dtype=ref.dtype)
    return m.abs() if absolute else m


def _patches6(x):
    """(B, C, H, W) -> (B, C, ty, tx, 6, 6), zero padded"""
    H, W = x.shape[-2:]
    ty, tx = (H + 3) // 4, (W + 3) // 4
    return F.pad(x, (1, 4 * tx + 1 - W, 1, 4 * ty + 1 - H)).unfold(2, 6, 4).unfold(3, 6, 4)


def _patches4(y, edge='zero'):
    """(B, C, H, W) -> (B, C, ty, tx, 4, 4); outside the map zero (or, edge='replicate', the
    nearest pixel: what a transform that clamps its addresses and forgets the select computes)"""
    H, W = y.shape[-2:]
    ty, tx = (H + 3) // 4, (W + 3) // 4
    pad = (0, 4 * tx - W, 0, 4 * ty - H)
    yp = F.pad(y, pad, mode='replicate') if edge == 'replicate' and any(pad) else F.pad(y, pad)
    return yp.unfold(2, 4, 4).unfold(3, 4, 4)


def _group(v, groups):
    """(36, T, C) -> (groups * 36, T, C / groups): group g's matrices are [36 g, 36 g + 36)"""
    if groups == 1:
        return v
    k, T, C = v.shape
    return v.reshape(k, T, groups, C // groups).permute(2, 0, 1, 3).reshape(groups * k, T, C // groups)


def _ungroup(v, groups):
    if groups == 1:
        return v
    gk, T, cg = v.shape
    return v.reshape(groups, gk // groups, T, cg).permute(1, 2, 0, 3).reshape(gk // groups, T, groups * cg)


def pre_activation(x, pre):
    """pre = (scale or None, shift, relu): relu?(x * scale + shift) per channel, in x's dtype"""
    if pre is None:
        return x
    s, t, relu = pre
    v = x if s is None else x * s.to(x).view(1, -1, 1, 1)
    v = v + t.to(x).view(1, -1, 1, 1)
    return v.clamp(min=0) if relu else v


def input_transform(xs, dtype=torch.float64, pre=None, groups=1, absolute=False, bt=None):
    """per-level (B, C, H, W) -> V (groups * 36, T, C / groups).  The pre-activation is applied to
    the pixels of the map only: the padding stays zero.  absolute=True: |B^T| d |B| (error
    bounds; pass absolute values)."""
    out = []
    for x in xs:
        d = _patches6(pre_activation(x.to(dtype), pre))
        m = _mat(BT if bt is None else bt, d, absolute)
        v = torch.einsum('ik,bcyxkl,jl->ijbyxc', m, d, m)
        out.append(v.reshape(36, -1, x.shape[1]))
    return _group(torch.cat(out, dim=1), groups).contiguous()


def grad_output_transform(dys, dtype=torch.float64, absolute=False, edge='zero', at=None):
    """per-level (B, C, H, W) -> dM = A dY A^T (36, T, C)"""
    out = []
    for dy in dys:
        d = _patches4(dy.to(dtype), edge)
        m = _mat(AT if at is None else at, d, absolute)
        v = torch.einsum('ki,bcyxkl,lj->ijbyxc', m, d, m)
        out.append(v.reshape(36, -1, dy.shape[1]))
    return torch.cat(out, dim=1).contiguous()


def output_transform(m, sizes, batch, bias=None, relu=False, groups=1, absolute=False, at=None):
    """M (groups * 36, T, C / groups) -> per-level (batch, C, H, W) = A^T M A + bias (ReLU),
    cropped to the map"""
    m = _ungroup(m, groups)
    C = m.shape[2]
    a = _mat(AT if at is None else at, m, absolute)
    ys, t0 = [], 0
    for (h, w) in sizes:
        ty, tx = (h + 3) // 4, (w + 3) // 4
        n = batch * ty * tx
        ml = m[:, t0:t0 + n].reshape(6, 6, batch, ty, tx, C)
        t0 += n
        y = torch.einsum('ki,ijbyxo,lj->boykxl', a, ml, a).reshape(batch, C, 4 * ty, 4 * tx)[:, :, :h, :w]
        if bias is not None:
            b = bias.to(m).view(1, -1, 1, 1)
            y = y + (b.abs() if absolute else b)
        ys.append(y.clamp(min=0) if relu else y)
    assert t0 == m.shape[1]
    return ys


def weight_transform(w, dtype=torch.float64, adjoint=False):
    """(Cout, Cin, 3, 3) -> U (36, Cin, Cout) = G w G^T, evaluated in fp64 and rounded once.
    adjoint=True: the weight of the input-gradient convolution, w^T rotated by 180 degrees
    -> (36, Cout, Cin)"""
    w = w.double()
    if adjoint:
        w = w.flip(2, 3).transpose(0, 1)
    g = G.to(w.device)
    u = torch.einsum('ik,ockl,jl->ijco', g, w, g)
    return u.reshape(36, w.shape[1], w.shape[0]).to(dtype).contiguous()


def weight_grad(du, dtype=torch.float64):
    """dU (36, Cin, Cout) -> dW (Cout, Cin, 3, 3) = G^T dU G, evaluated in fp64, rounded once"""
    g = G.to(du.device)
    d = du.double().reshape(6, 6, du.shape[1], du.shape[2])
    return torch.einsum('ik,ijco,jl->ockl', g, d, g).to(dtype)


def cut_mantissa(t, bits):
    """round an fp32 tensor to `bits` significand bits (round to nearest, ties away): what a
    2-term bf16 split (bits = 16) or a single fp16 / bf16 operand keeps of it"""
    assert t.dtype == torch.float32
    drop = 24 - bits
    if drop <= 0:
        return t
    i = t.contiguous().view(torch.int32)
    i = (i + (1 << (drop - 1))) & ~((1 << drop) - 1)
    return i.view(torch.float32)


def _same(v):
    return v


def conv_fwd(xs, w, bias=None, dtype=torch.float64, relu=False, operand=_same, keep_v=False):
    """-> per-level y (and V when keep_v); `operand` is applied to both factors of the products"""
    xs = list(xs)
    v = input_transform(xs, dtype)
    u = weight_transform(w, dtype).to(v.device)
    m = torch.bmm(operand(v), operand(u))
    ys = output_transform(m, [tuple(x.shape[-2:]) for x in xs], xs[0].shape[0],
                          None if bias is None else bias.to(dtype), relu)
    return (ys, v) if keep_v else ys


def conv_dx(dys, w, dtype=torch.float64, operand=_same):
    """gradient w.r.t. the inputs of conv_fwd (without ReLU): the forward steps on dY with the
    adjoint weight"""
    dys = list(dys)
    v = input_transform(dys, dtype)
    u = weight_transform(w, dtype, adjoint=True).to(v.device)
    m = torch.bmm(operand(v), operand(u))
    return output_transform(m, [tuple(d.shape[-2:]) for d in dys], dys[0].shape[0])


def conv_dw(v, dys, dtype=torch.float64, operand=_same, edge='zero', at=None):
    """gradient w.r.t. the weight from V = input_transform(xs) and the upstream gradients"""
    dm = grad_output_transform(list(dys), dtype, edge=edge, at=at)
    du = torch.bmm(operand(v).transpose(1, 2), operand(dm))
    return weight_grad(du, dtype)


def conv_db(dys, dtype=torch.float64):
    return sum(d.to(dtype).sum((0, 2, 3)) for d in dys)


# ------------------------------------------------------------------ the gates of the node tests
GATE_A = 1e-4          # the project's contract: every quantity within 1e-4 of its maximum
# Precision: at most this multiple of the fp32 helper's own error on the same tensors.  The helper's
# error moves by up to 1.8 x with the order of its sums, the fault the gate exists for (GEMM
# operands of 16 significand bits) sits at 25-31 x (tests/test_host_wino_ref.py), so the gate was
# set at 2.  The first MI355X run put the HIP route at up to 2.7 x in y / dx and 6.9 x in dW, and
# the cause is the order of the sums, not the operands: the library's fp32 GEMMs (hipBLASLt here,
# torch.bmm alike) add the K terms of a dot product one after the other, a CPU GEMM in blocks.  In
# isolation, K = 5 720, against fp64: library 1.9-3.7e-6 of the maximum, the same product in chunks
# of 512 / 128 rows 5e-7 / 3.2e-7, the CPU 3e-7; K = 512 / 720 in the forward product 1.0e-6 /
# 1.3e-6 against 4e-7; sums of all-positive terms show no bias (mean relative error 1e-10: round
# to nearest, full fp32 operands).  The weight gradient now cuts its 5 720-term reduction into
# slices (winograd_train.weight_grad_product; dW back to <= 2.5 x); the forward and input-gradient
# products keep the library's order over K = C_in <= 720 (they are the hot path and lose 2.7 x at
# most).  That is benign and it is the whole difference, so the margin is 4, its ceiling: the
# 16-bit fault still fails it by 6 x.
GATE_B = 4.0
GATE_B_MAX = 4.0       # GATE_B never goes beyond this; the faults it exists for must still fail
                       # here (tests/test_host_wino_ref.py)


def rel_err(got, ref):
    """max|got - ref| / max|ref|, evaluated in fp64 where ref lives"""
    ref = ref.double()
    return float((got.to(ref.device).double() - ref).abs().max() / ref.abs().max())


def worst(gots, refs):
    """rel_err of a tensor, or the worst over a list of per-level tensors"""
    if isinstance(gots, torch.Tensor):
        return rel_err(gots, refs)
    assert len(gots) == len(refs)
    return max(rel_err(g, r) for g, r in zip(gots, refs))


U32 = 2.0 ** -24       # unit roundoff of fp32


def gates(got, helper, ref):
    """-> (error of got, error of the fp32 helper, their ratio), both against ref.  The helper's
    error counts as at least one unit roundoff: rounding the exact result to fp32 costs up to that
    much of the maximum, so a helper that lands closer (a bias gradient summed over a handful of
    pixels can be exact) got there by luck and says nothing about the candidate."""
    e, h = worst(got, ref), worst(helper, ref)
    return e, h, e / max(h, U32)

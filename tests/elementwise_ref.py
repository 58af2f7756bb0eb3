"""CPU yardstick, cases and data of tests/test_gpu_elementwise_edges.py and
tests/test_host_elementwise_ref.py: the inference epilogue kernels of csrc/elementwise.hip written from
their definitions in plain torch.  Test-only: nothing imported from the project.

    affine        y = x*s[c] + b[c];  y = y + (r*rs[c] + rb[c]);  ReLU that keeps a NaN
                  (absent s / rs = 1, absent b / rb = 0), NCHW (channel axis 1) or channels-last rows
    pool          max_pool2d(relu(affine(x)), 3, 2, 1) on (B, H, W, C) rows
    upsample_add  fine + coarse[y // 2, x // 2] on (B, H, W, C) rows
    transpose     (N, HW, C) -> (N, C, HW)

The kernels sum nothing and the library is built with -ffp-contract=off, so every product and sum
rounds once: the yardstick runs ONE torch op per rounding in fp32, in the kernel's order, and the
comparison (`same`) is exact -- equal NaN masks, torch.equal everywhere else (the sign of a zero is
not compared).  bf16: inputs widened exactly, fp32 arithmetic, one round-to-nearest-even at the end.
`affine64` / `pool64` evaluate the same operations in fp64 with one rounding to fp32 per operation and
say where every fp64 sum was exact (there the two routes must agree: test_host_elementwise_ref.py).
"""
import numpy as np
import torch

NAN = float('nan')
INF = float('inf')
GUARD = 16384               # elements per guard band: more than one workgroup of the epilogue (8192
#                             bf16 elements) and than 64 rows of the widest transposed map (64 x 130)
BAND = -8192.0              # the bands' marker (exact in bf16)
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def vec_width(dtype):
    return 4 if dtype == torch.float32 else 8


# ------------------------------------------------------------------ comparison
def same(got, want):
    """equal NaN masks, and torch.equal where neither is a NaN (+0 == -0)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        return False
    z = torch.zeros((), dtype=got.dtype)
    return torch.equal(torch.where(gn, z, got), torch.where(wn, z, want))


def first_difference(got, want):
    """for assertion messages: (number of differing elements, flat index of the first, got, want)"""
    g, w = got.detach().cpu().float().reshape(-1), want.detach().cpu().float().reshape(-1)
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    idx = torch.nonzero(bad).flatten()
    if idx.numel() == 0:
        return (0, None, None, None)
    i = int(idx[0])
    return (int(idx.numel()), i, float(g[i]), float(w[i]))


# ------------------------------------------------------------------ the definitions
def relu_keep_nan(y):
    return torch.where(y != y, y, y.clamp(min=0))


def _per_channel(v, x, caxis):
    shape = [1] * x.dim()
    shape[caxis] = x.shape[caxis]
    assert v.dtype == torch.float32 and v.numel() == x.shape[caxis]
    return v.view(shape)


def affine(x, scale=None, shift=None, res=None, res_scale=None, res_shift=None, relu=False, caxis=-1):
    """the epilogue in fp32, one torch op per rounding, in the kernel's order; result in x's dtype"""
    one, zero = torch.ones(()), torch.zeros(())
    f = lambda v, d: _per_channel(v, x, caxis) if v is not None else d          # noqa: E731
    y = x.float() * f(scale, one)
    y = y + f(shift, zero)
    if res is not None:
        t = res.float() * f(res_scale, one)
        t = t + f(res_shift, zero)
        y = y + t
    if relu:
        y = relu_keep_nan(y)
    assert y.dtype == torch.float32
    return y.to(x.dtype)


def _sum64(a, b):
    """fp64 a + b rounded to fp32 (as fp64), and where the fp64 sum itself was exact (TwoSum): only
    there is 'fp64, then one rounding to fp32' the correctly rounded fp32 sum"""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return s.float().double(), (err == 0) | ~torch.isfinite(s)


def affine64(x, scale=None, shift=None, res=None, res_scale=None, res_shift=None, relu=False, caxis=-1):
    """-> (the epilogue with every operation in fp64 and rounded once to fp32, in x's dtype;
    mask of the elements all of whose fp64 sums were exact).  The product of two fp32 values is exact
    in fp64 (48 bits)."""
    one, zero = torch.ones(()), torch.zeros(())
    f = lambda v, d: (_per_channel(v, x, caxis) if v is not None else d).double()   # noqa: E731
    y = (x.double() * f(scale, one)).float().double()
    y, exact = _sum64(y, f(shift, zero))
    if res is not None:
        t = (res.double() * f(res_scale, one)).float().double()
        t, e = _sum64(t, f(res_shift, zero))
        exact = exact & e
        y, e = _sum64(y, t)
        exact = exact & e
    if relu:
        y = relu_keep_nan(y)
    return y.float().to(x.dtype), exact.expand(y.shape)


def _pool_rows(a):
    """(B, H, W, C) fp32 -> MaxPool2d(3, 2, 1) -> (B, Ho, Wo, C)"""
    return torch.nn.functional.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def pool(x, scale, shift):
    """the definition in fp32 on (B, H, W, C) rows; a bf16 result is the fp32 one rounded once"""
    a = affine(x.float(), scale, shift, relu=True)
    return _pool_rows(a).to(x.dtype)


def pool64(x, scale, shift):
    a, exact = affine64(x.float(), scale, shift, relu=True)
    worst = _pool_rows((~exact).float()) == 0              # every tap of the window exact
    return _pool_rows(a).to(x.dtype), worst


def pool_eager_order(x, scale, shift):
    """the module route on bf16 values: affine (rounded) -> ReLU -> max-pool"""
    a = affine(x, scale, shift)                            # rounded to x's dtype
    return _pool_rows(relu_keep_nan(a.float())).to(x.dtype)


def pool_nan_mask(x):
    """which outputs have a NaN of x (B, H, W, C) in their window: the definition's NaN mask when
    scale and shift are finite"""
    return _pool_rows(torch.isnan(x).float()) > 0


def upsample_add(fine, coarse):
    """(B, 2 Hc, 2 Wc, C) + nearest-x2 of (B, Hc, Wc, C): fp32 sum, one rounding"""
    H, W = fine.shape[1], fine.shape[2]
    ys, xs = torch.arange(H) // 2, torch.arange(W) // 2
    up = coarse[:, ys][:, :, xs]
    return (fine.float() + up.float()).to(fine.dtype)


def transpose(src):
    """(N, HW, C) -> (N, C, HW)"""
    return src.permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------ data
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * m for v, m in zip(key, (1, 7, 131, 1009, 65537))) + 5)


def vecs(C):
    """per-channel scale / shift / res_scale / res_shift: every value distinct within its vector and
    exact in fp32, scales of both signs -- a wrong channel index shows in every element"""
    c = torch.arange(C, dtype=torch.float32)
    sign = torch.where(c % 3 == 1, -torch.ones(C), torch.ones(C))
    v = dict(s=(0.75 + c / 4096) * sign, b=-1.0 + c / 2048, rs=-(0.5 + c / 8192) * sign, rb=0.25 + c / 16384)
    assert all(t.unique().numel() == C for t in v.values())
    return v


def rand(shape, dtype, *key):
    return (torch.randn(shape, generator=_gen(*key)) * 2).to(dtype)


# operand combinations of the epilogue: (name, scale, shift, residual, res_scale, res_shift).  The first
# five are what fuse.py uses; the last two reach the remaining two instantiations of the fast kernel.
COMBOS = (('s b', 1, 1, 0, 0, 0), ('s b r', 1, 1, 1, 0, 0), ('s b r rs rb', 1, 1, 1, 1, 1), ('- b', 0, 1, 0, 0, 0),
          ('- -', 0, 0, 0, 0, 0), ('s -', 1, 0, 0, 0, 0), ('s b r rs', 1, 1, 1, 1, 0), ('s b r rb', 1, 1, 1, 0, 1),
          ('- b r', 0, 1, 1, 0, 0), ('- b r rs rb', 0, 1, 1, 1, 1))


def nhwc_kernel(combo):
    """which kernel ia_channel_affine_act_nhwc launches for a combination (restates its dispatch)"""
    _, s, b, r, rs, rb = combo
    if not b or (r and rs != rb):
        return 'generic'
    return 'fast<%d,%d,%d>' % (s, r, int(r and rs and rb))


def pick(combo, v, r):
    """-> (scale, shift, residual, res_scale, res_shift) of a combination, absent ones None"""
    _, us, ub, ur, urs, urb = combo
    return (v['s'] if us else None, v['b'] if ub else None, r if ur else None,
            v['rs'] if urs else None, v['rb'] if urb else None)


def nhwc_cases():
    """[(dtype name, pixels, C)]: the channels-last epilogue.  One workgroup = 4 packs x 256 threads
    = 1024 packs of 16 bytes (4096 fp32 / 8192 bf16 elements); one thread step = 256 packs."""
    out = []
    for name, dtype in DTYPES.items():
        n = vec_width(dtype)
        # totals (C = one pack, so pixels = packs): two packs, one short of a workgroup, one workgroup,
        # one beyond, two workgroups and a partial third
        out += [(name, packs, n) for packs in (2, 1023, 1024, 1025, 2 * 1024 + 300)]
        # the vector width: one pixel of one pack leaves 1023 of a workgroup's 1024 packs clamped
        out += [(name, pixels, C) for C in ((4, 8) if n == 4 else (8,)) for pixels in (1, 3, 37)]
        # not a power of two; the last of each is two (fp32) / one (bf16) workgroups and a partial one
        out += [(name, pixels, 24) for pixels in (1, 7, 345)]
        if n == 4:
            out += [(name, pixels, 36) for pixels in (1, 5, 229)]
        out += [(name, pixels, 720) for pixels in (1, 3, 12)]
        # above one thread step (1024 fp32 / 2048 bf16 elements): step_mod = the step itself at 2048
        # (fp32) and 4104 (bf16); 1032 wraps (step_mod 1024 fp32, 1016 bf16)
        out += [(name, pixels, C) for C in ((2048, 1032) if n == 4 else (4104, 1032)) for pixels in (1, 3)]
    return out


NCHW_HW = (1, 4, 7, 8, 4092, 4096, 4100)        # vector path, scalar path, the 4096-element chunk boundary
NCHW_NC = (3, 5)
NCHW_MISALIGNED_HW = (8, 4096)                   # HW % N == 0, but the tensor starts 4 bytes into its buffer
NONFINITE_NHWC = (40, 8)                         # (pixels, C)
NONFINITE_NCHW_HW = (7, 8)                       # scalar and vector path


def nhwc_data(pixels, C, dtype):
    return rand((pixels, C), dtype, pixels, C, 1), rand((pixels, C), dtype, pixels, C, 2)


def nchw_data(hw, dtype):
    shape = NCHW_NC + (hw,)
    return rand(shape, dtype, hw, 3), rand(shape, dtype, hw, 4)


def plant_nonfinite(x, r, v, caxis):
    """x, r with NaN, +Inf, -Inf and -0.0 planted (flat positions spread over the tensor), and a scale
    of 0 in the channel of one of x's infinities.  -> (x, r, vectors, channel of the zero scale)"""
    x, r, v = x.clone(), r.clone(), {k: t.clone() for k, t in v.items()}
    n = x.numel()
    xf, rf = x.view(-1), r.view(-1)
    spots = [(i * n) // 11 for i in range(11)]
    for t, vals in ((xf, (NAN, INF, -INF, -0.0, INF)), (rf, (-INF, NAN, 1.0, INF, -0.0))):
        # position 0: NaN in x, -Inf in r.  1: +Inf in x, NaN in r.  2: -Inf in x.  3: -0.0 in x, +Inf in r.
        # 4: +Inf in x (its scale is set to 0 below: 0 * Inf = NaN)
        for p, val in zip(spots[:5], vals):
            t[p] = val
    xf[spots[5]], rf[spots[5]] = INF, -INF                 # Inf - Inf = NaN only where the residual is added
    xf[spots[6]], rf[spots[6]] = -INF, -INF
    rf[spots[7]] = NAN
    ch = int(np.unravel_index(spots[4], tuple(x.shape))[caxis])
    v['s'][ch] = 0.0
    return x, r, v, ch


def nonfinite_case(layout, dtype, hw=None):
    """-> (x, r, vectors, channel of the zero scale) of the non-finite tests: 'nhwc' rows
    NONFINITE_NHWC, or 'nchw' NCHW_NC + (hw,)"""
    if layout == 'nhwc':
        pixels, C = NONFINITE_NHWC
        x, r = nhwc_data(pixels, C, dtype)
        return plant_nonfinite(x, r, vecs(C), -1)
    x, r = nchw_data(hw, dtype)
    return plant_nonfinite(x, r, vecs(NCHW_NC[1]), 1)


# ---- the stem pool
POOL_SMALL = tuple((2, h, w) for h in (1, 2, 3, 4, 5) for w in (1, 2, 3, 4, 5))       # (B, H, W), C = one pack
POOL_WIDE = (2, 9, 33, 24)                       # (B, H, W, C): 1020 (fp32) / 510 (bf16) threads


def pool_cases():
    """[(dtype name, B, H, W, C)]"""
    out = []
    for name, dtype in DTYPES.items():
        out += [(name,) + s + (vec_width(dtype),) for s in POOL_SMALL]
        out.append((name,) + POOL_WIDE)
    return out


def pool_data(B, H, W, C, dtype):
    """x (B, H, W, C), scale, shift.  Channel 0: a tie channel (x a power of two, scale 1 + 2^-8: every
    affine value lies halfway between two bf16 values, and equal taps abound).  Channel 1: every window
    negative (output exactly 0).  Channel 2: half-integers under a negative scale (ties between taps).
    The rest: random, scales of both signs."""
    g = _gen(B, H, W, C, 9)
    x = torch.randn((B, H, W, C), generator=g) * 2
    pw = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, (B, H, W), generator=g)]
    x[..., 0] = pw * (torch.randint(0, 2, (B, H, W), generator=g) * 2 - 1).float()
    x[..., 2] = torch.randint(-4, 5, (B, H, W), generator=g).float() * 0.5
    v = vecs(C)
    s, t = v['s'].clone(), v['b'].clone()
    s[0], t[0] = 1.0 + 2.0 ** -8, 0.0
    s[1], t[1] = 0.5, -50.0
    s[2], t[2] = -1.5, 0.25
    return x.to(dtype), s, t


def pool_nan_spots(B, H, W):
    """(b, y, x): a corner, the centre, and (1, 1), which four windows share when H, W >= 3"""
    spots = [(0, 0, 0), (B - 1, H // 2, W // 2)]
    if H >= 3 and W >= 3:
        spots.append((0, 1, 1))
    return spots


POOL_NAN_CASES = ((2, 1, 1), (2, 2, 5), (2, 4, 3), (2, 5, 5), POOL_WIDE[:3])


# ---- upsample-add
UPADD_COARSE = ((1, 4, 1, 1), (2, 8, 1, 3), (3, 24, 5, 2), (2, 64, 7, 5))        # (B, C, Hc, Wc)


def upadd_cases():
    return [(name, s) for name, dtype in DTYPES.items() for s in UPADD_COARSE if s[1] % vec_width(dtype) == 0]


def upadd_code(B, C, Hc, Wc):
    """coarse (B, Hc, Wc, C) = (128 + index of the pixel (b, y, x)) * 2^c: an integer of eight
    significant bits (exact in bf16) that names its pixel and its channel"""
    pix = torch.arange(B * Hc * Wc, dtype=torch.float32).view(B, Hc, Wc, 1)
    assert B * Hc * Wc <= 128 and C <= 64
    return (128.0 + pix) * torch.pow(2.0, torch.arange(C, dtype=torch.float32)).view(1, 1, 1, C)


def upadd_data(B, C, Hc, Wc, dtype):
    return (rand((B, 2 * Hc, 2 * Wc, C), dtype, B, C, Hc, Wc, 5), rand((B, Hc, Wc, C), dtype, B, C, Hc, Wc, 6))


# ---- transpose
TRANSPOSE_N = 3
TRANSPOSE_SIZES = (2, 63, 64, 65, 130)          # C and HW: the LDS tile is 64 x 64


def transpose_data(C, HW, dtype):
    """(N, HW, C): fp32 counts its elements (every value names its place), bf16 is random"""
    n = TRANSPOSE_N * HW * C
    if dtype == torch.float32:
        return torch.arange(n, dtype=torch.float32).view(TRANSPOSE_N, HW, C)
    return rand((TRANSPOSE_N, HW, C), dtype, C, HW, 7)

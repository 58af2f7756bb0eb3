"""CPU helpers of tests/test_gpu_stream_edges.py and tests/test_host_stream_ref.py: the streaming
MFMA kernels of csrc/conv1x1_stream.hip (k_conv1x1_stream / _wide / _chain, also behind
ia_batched_gemm_stream) and the stem kernels of csrc/stem.hip, written from their definitions in
plain torch, in any floating dtype and on any device.  Test-only: nothing imported from the project.

    1x1      y[p, :] = relu?(x[p, :] . W + bias + residual[p, :])                 (rows p, W (k, n))
    chain    y = relu(x . W + bias + residual),  h = relu(y . W2 + bias2)
    batched  D[b] = A[b] . W[b]
    stem     F.conv2d(x, w, stride=2, padding=3), 3 -> 64 channels, 7 x 7, on channels-last rows

Three instruments (the GPU file uses all three, the host file shows what each can see):

  * INTEGER data (`int_case`, `chain_int_case`, `stem_int_case`): x in -3..3, weights in -2..2, bias and
    residual in -3..3, stored in fp32.  Every partial sum of every product is an integer below 2^24
    in any order of summation (`int_bound`), so a correct kernel equals the fp64 product cast to fp32
    with torch.equal, and any wrong index, dropped or doubled term or wrong clamp breaks equality.
  * RANDOM data (`rand_case`, ...) under the project's two gates (dcn_ref.GATE_A, GATE_B): the fp32
    figure is the largest over ORDERS plain fp32 CPU evaluations with the reduction index permuted
    (`fp32_figure`, `stem_fp32_figure`), the scheme of tests/test_gpu_masked_conv._fp32_figure.
  * NaN-filled outputs between guard bands (`guarded`, `guard_ok`).

The case lists below are the smallest row counts that cross each edge of the launch geometry
(`geometry`, `stem_geometry` restate the host code of the entry points); `faulty_1x1`, `faulty_chain`
and `faulty_stem` build the nearest WRONG results for the host tests.
"""
import numpy as np
import torch

import dcn_ref as R

ORDERS = 4
GUARD = 4096                # floats per guard band
BAND = -8192.0              # the bands' marker (exact in bf16 too)

# ------------------------------------------------------------------ cases
STREAM_SHAPES = ((64, 256), (256, 64), (64, 64))
STREAM_ROWS = (1, 15, 16, 17, 127, 128, 129, 4113)
STREAM_GATE_ROWS = (17, 129, 4113)
STREAM_ALL_COMBO_ROWS = (17, 129)          # all eight combinations of bias, residual, ReLU
BIG_ROWS = 65793                           # 241 x 273: 4113 tiles on 4096 wavefronts, one row in the last tile
WIDE_SHAPE = (128, 512)
WIDE_ROWS = (1, 16, 17, 257)
WIDE_GATE_ROWS = (257,)
WIDE_BIG_ROWS = 32787                      # 2050 tiles on 2048 wavefronts, three rows in the last tile
CHAIN_SHAPE = (64, 256, 64)
CHAIN_ROWS = (1, 16, 17, 257, BIG_ROWS)
BMM_SHAPES = ((64, 64), (128, 128), (256, 48))
BMM_CASES = ((1, 1), (1, 17), (36, 17), (36, 1931), (513, 259))        # (batch, rows)
BMM_GATE_CASES = ((36, 17), (36, 1931))
BMM_BIG_CASE = (3, BIG_ROWS)               # (64, 64) only
STEM_CASES = ((1, 1, 1), (1, 2, 3), (1, 7, 8), (2, 8, 4), (1, 9, 127), (1, 9, 128), (1, 9, 129), (1, 9, 130),
              (2, 15, 132), (9, 456, 6), (9, 456, 8))                   # (B, H, W)
STEM_GATE_CASES = ((2, 15, 132), (1, 9, 129))
STEM_MISALIGNED_CASES = ((1, 9, 128), (9, 456, 8))
NAN_ROWS = (17, 129)                       # non-finite containment


def geometry(kernel, rows, batch=1):
    """-> (16-row tiles, wavefronts of the launch per matrix / column block)"""
    tiles = (rows + 15) // 16
    per_wg, cap = {'stream': (8, 512), 'batched': (8, (512 + batch - 1) // batch), 'wide': (16, 128),
                   'chain': (16, 256)}[kernel]
    wgs = max(1, min((tiles + per_wg - 1) // per_wg, cap))
    return tiles, wgs * per_wg


def stem_geometry(B, H, W):
    """-> (Ho, Wo, tiles of 4 x 64 outputs, workgroups)"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tiles = B * ((Wo + 63) // 64) * ((Ho + 3) // 4)
    return Ho, Wo, tiles, min(tiles, 512)


# ------------------------------------------------------------------ data
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * m for v, m in zip(key, (1, 7, 131, 1009, 65537))) + 11)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _lead(batch):
    return () if batch is None else (batch,)


def int_case(rows, k, n, batch=None):
    """-> x (rows, k) in -3..3, w (k, n) in -2..2, bias (n) and residual (rows, n) in -3..3, as fp32;
    with `batch`, x and w get a leading batch axis (every matrix its own weights)"""
    g = _gen(rows, k, n, batch or 0)
    b = _lead(batch)
    return (_ints(b + (rows, k), -3, 3, g), _ints(b + (k, n), -2, 2, g), _ints((n,), -3, 3, g),
            _ints((rows, n), -3, 3, g))


def rand_case(rows, k, n, batch=None):
    """the random data of the existing tests: x ~ N(0, 1), w ~ 0.1 N(0, 1), bias and residual ~ N(0, 1)"""
    g = _gen(rows, k, n, batch or 0, 1)
    b = _lead(batch)
    return (torch.randn(b + (rows, k), generator=g), torch.randn(b + (k, n), generator=g) * 0.1,
            torch.randn(n, generator=g), torch.randn(rows, n, generator=g))


def chain_int_case(rows):
    k, n, n2 = CHAIN_SHAPE
    g = _gen(rows, n, n2, 5)
    return int_case(rows, k, n) + (_ints((n, n2), -2, 2, g), _ints((n2,), -3, 3, g))


def chain_rand_case(rows):
    k, n, n2 = CHAIN_SHAPE
    g = _gen(rows, n, n2, 6)
    return rand_case(rows, k, n) + (torch.randn(n, n2, generator=g) * 0.05, torch.randn(n2, generator=g))


def int_bound(x, w, bias=None, res=None):
    """the largest value any partial sum of x . w + bias + residual can reach, in any order"""
    v = float((x.double().abs() @ w.double().abs()).max())
    return v + (float(bias.abs().max()) if bias is not None else 0.0) + (float(res.abs().max()) if res is not None else 0.0)


def stem_int_case(B, H, W, kind='fp32'):
    """-> x (B, H, W, 3), w (64, 3, 7, 7) as fp32.
    'fp32'        x in -3..3, w in -2..2: |y| <= 882
    'bf16_exact'  x, w in {-1, 0, 1}: |y| <= 147, exact in bf16
    'bf16_ties'   x in -3..3, w in {-1, 0, 1}: |y| <= 441.  Independent draws would never leave +-100,
                  so the left half of the image holds 2 and 3 only and output channels 0 / 1 weigh
                  everything with +1 / -1: sums of 300-441 of either parity and sign, of which every
                  odd one above 256 is a tie of the bf16 rounding"""
    g = _gen(B, H, W, ('fp32', 'bf16_exact', 'bf16_ties').index(kind), 3)
    if kind == 'fp32':
        return _ints((B, H, W, 3), -3, 3, g), _ints((64, 3, 7, 7), -2, 2, g)
    x, w = _ints((B, H, W, 3), -1 if kind == 'bf16_exact' else -3, 1 if kind == 'bf16_exact' else 3, g), \
        _ints((64, 3, 7, 7), -1, 1, g)
    if kind == 'bf16_ties':
        x[:, :, :(W + 1) // 2] = _ints((B, H, (W + 1) // 2, 3), 2, 3, g)
        w[0], w[1] = 1.0, -1.0
    return x, w


def stem_rand_case(B, H, W):
    g = _gen(B, H, W, 9)
    return torch.randn(B, H, W, 3, generator=g), torch.randn(64, 3, 7, 7, generator=g) * 0.1


def cut16(t):
    """fp32 with the low 16 bits of every value cleared: what a 16-bit operand path would feed"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


# ------------------------------------------------------------------ the operations
def conv1x1(x, w, bias=None, res=None, relu=False, dtype=torch.float64):
    """relu?(x . w + bias + res); x (..., rows, k), w (..., k, n)"""
    y = torch.matmul(x.to(dtype), w.to(dtype))
    if bias is not None:
        y = y + bias.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return y.clamp(min=0) if relu else y


def chain(x, w, bias, res, w2, bias2, dtype=torch.float64):
    y = conv1x1(x, w, bias, res, True, dtype)
    return y, conv1x1(y, w2, bias2, None, True, dtype)


def stem(x, w, dtype=torch.float64):
    """x (B, H, W, 3), w (64, 3, 7, 7) -> (B, Ho, Wo, 64)"""
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), stride=2, padding=3)
    return y.permute(0, 2, 3, 1).contiguous()


def _perm(n, o):
    return torch.arange(n) if o == 0 else torch.randperm(n, generator=torch.Generator().manual_seed(o))


def fp32_figure(x, w, bias, res, relu, ref):
    """the largest rel_err over ORDERS plain fp32 CPU evaluations with the reduction index permuted"""
    figs = []
    for o in range(ORDERS):
        p = _perm(x.shape[-1], o)
        figs.append(R.rel_err(conv1x1(x[..., p], w[..., p, :], bias, res, relu, torch.float32), ref))
    return max(figs)


def stem_fp32_figure(x, w, ref):
    """the same for the stem: the 147 products of an output as unfold + matmul, their order permuted"""
    B = x.shape[0]
    cols = torch.nn.functional.unfold(x.permute(0, 3, 1, 2).contiguous(), 7, padding=3, stride=2)     # (B, 147, Ho * Wo)
    wm = w.reshape(64, 147)
    figs = []
    for o in range(ORDERS):
        p = _perm(147, o)
        y = torch.matmul(wm[:, p], cols[:, p]).permute(0, 2, 1).reshape(ref.shape)
        figs.append(R.rel_err(y, ref))
    assert B == ref.shape[0]
    return max(figs)


# ------------------------------------------------------------------ guard bands
def guarded(n, device, dtype=torch.float32):
    """-> (flat buffer, its n-element middle): the middle full of NaN, GUARD floats' worth of BAND on
    either side; the middle starts at a multiple of 16 bytes"""
    guard = GUARD * 4 // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * guard,), float('nan'), dtype=dtype, device=device)
    buf[:guard] = BAND
    buf[guard + n:] = BAND
    out = buf[guard:guard + n]
    assert out.data_ptr() % 16 == 0
    return buf, out


def guard_ok(buf, n):
    guard = (buf.numel() - n) // 2
    return bool((buf[:guard] == BAND).all()) and bool((buf[guard + n:] == BAND).all())


# ------------------------------------------------------------------ the nearest wrong results
FAULTS_1X1 = ('last_tile_from_last_row', 'second_tile_skipped', 'bias_skipped_from_block_8', 'residual_twice',
              'k_groups_swapped', 'weights_of_matrix_0')


def faulty_1x1(fault, kernel, x, w, bias=None, res=None, relu=False):
    """the product as a kernel with one fault would leave it, in fp64 (NaN where nothing is stored):
    last_tile_from_last_row    every lane of the partial last tile computes the clamped row P - 1
    second_tile_skipped        a wavefront does not come back for its second tile
    bias_skipped_from_block_8  the second batch of 8 output blocks (WB) of a 256-wide step gets no bias
    residual_twice             the accumulators start at the residual and it is added again
    k_groups_swapped           k-groups 0 and 1 exchanged on the activation operand only
    weights_of_matrix_0        the batched weight stride is 0"""
    x, w = x.double().clone(), w.double()
    rows, n = x.shape[-2], w.shape[-1]
    tiles, waves = geometry(kernel, rows, x.shape[0] if x.dim() == 3 else 1)
    if fault == 'k_groups_swapped':
        x[..., 0:4], x[..., 4:8] = x[..., 4:8].clone(), x[..., 0:4].clone()
    if fault == 'weights_of_matrix_0':
        w = w[:1].expand_as(w)
    y = torch.matmul(x, w)
    if bias is not None:
        b = bias.double().clone()
        if fault == 'bias_skipped_from_block_8':
            b[(torch.arange(n) % 256) >= 128] = 0
        y = y + b
    if res is not None:
        y = y + res.double() * (2 if fault == 'residual_twice' else 1)
    if relu:
        y = y.clamp(min=0)
    if fault == 'last_tile_from_last_row':
        y[..., 16 * (tiles - 1):, :] = y[..., rows - 1:rows, :].clone()
    if fault == 'second_tile_skipped':
        y[..., 16 * waves:, :] = float('nan')
    return y


def faulty_chain(fault, x, w, bias, res, w2, bias2):
    y = faulty_1x1(fault, 'chain', x, w, bias, res, True)
    return y, conv1x1(y, w2, bias2, None, True)


FAULTS_STEM = ('edge_clamp', 'next_image')


def faulty_stem(fault, x, w):
    """edge_clamp  the clamped loads' values are kept where the padding's zeros belong
    next_image  the rows under the image come from the top of the next image (zeros under the last)"""
    B, H, W, _ = x.shape
    xt, F = x.permute(0, 3, 1, 2).double(), torch.nn.functional
    if fault == 'edge_clamp':
        p = F.pad(xt, (3, 3, 3, 3), mode='replicate')
    else:
        p = F.pad(xt, (3, 3, 3, 3))
        r = min(3, H)
        p[:-1, :, 3 + H:3 + H + r, 3:3 + W] = xt[1:, :, :r]
    return F.conv2d(p, w.double(), stride=2).permute(0, 2, 3, 1).contiguous()

"""GPU: the streaming MFMA kernels at the edges of their launch geometry -- k_conv1x1_stream (behind
ia_conv1x1_stream and ia_batched_gemm_stream), k_conv1x1_wide, k_conv1x1_chain
(csrc/conv1x1_stream.hip) and k_stem_conv7x7s2 / _bf16 (csrc/stem.hip), through their C entries
(the Python wrappers route large shapes only).  These kernels are the root of the bit-for-bit chain
ia_wino_conv3x3_c64 = ia_wino_in_gemm + output transform, ia_wino_in_gemm = input transform +
ia_batched_gemm_stream, ia_conv1x1_chain = two ia_conv1x1_stream: this file pins the root.

Three instruments (tests/stream_ref.py; tests/test_host_stream_ref.py shows what each can see):

  exact   integer data in fp32 (x in -3..3, weights in -2..2): every partial sum is an integer below
          2^24, so the result EQUALS the fp64 product cast to fp32 (torch.equal).  bf16 stem: x, w in
          {-1, 0, 1} (|y| <= 147, exact in bf16), and x in -3..3 with |y| up to 441, where every odd
          value above 256 is a tie: equal to the reference rounded to nearest even.
  gates   random data, fp64 reference of the same fp32 tensors: max|got - ref| / max|ref| <= 1e-4
          (dcn_ref.GATE_A) and <= 4 x (GATE_B) the same figure of a plain fp32 CPU evaluation, the
          largest over 4 orders of the reduction index.  At 4113 rows or fewer.
  guards  every output is a view into a flat NaN-filled buffer between two bands of 4096 floats: no
          NaN inside afterwards, both bands intact.  The stems' x sits between a row's worth of NaN.

Row counts: below one 16-row tile, one tile, one workgroup of tiles (128), the first tile of a second
workgroup, the grid cap with a wavefront's second tile (65 793 rows: 4113 tiles on 4096 wavefronts;
wide 32 787: 2050 on 2048; batched (36, 1931): 121 on 120 per matrix; (513, 259): one workgroup per
matrix, 17 tiles on 8 wavefronts).  Stems: maps smaller than a tile, the 64-column tile edge, 513
tiles on 512 workgroups on either staging path, and the scalar path forced by a misaligned x.

Non-finite containment (1x1 kernels): a NaN planted in one row of x makes that row NaN in every
output channel and leaves every other row's bits alone.  With ReLU the kernels compute v > 0 ? v : 0,
which turns the NaN row into zeros (torch.relu would keep it): documented in DESIGN.md section 3.22, not
changed.  Non-finite inputs to the stems are out of scope (zero-weight taps read neighbouring pixels).

Measured on an MI355X, 2026-10-20 (worst error, worst multiple of the fp32 figure, over the gated cases):
    ia_conv1x1_stream        8.98e-07 (256 x 64, 129 rows, residual + ReLU)   3.19 x (64 x 64, 129 rows, bias + residual + ReLU)
    ia_conv1x1_wide          6.23e-07 (257 rows, bias + ReLU)                 1.60 x (257 rows, bias + residual + ReLU)
    ia_batched_gemm_stream   7.08e-07 (256 x 48, 36 x 1931 rows)              1.61 x (the same case)
    ia_stem_conv7x7s2        4.36e-07 ((2, 15, 132))                          0.82 x (the same case)
Without bias and residual the K = 64 and 128 products and the stem are at 0.5-0.9 x and the K = 256
products at 1.1-2.2 x (a chain of 64 MFMA steps against the CPU's blocked sums); with bias or
residual the 1x1 kernels stand at 1.0-3.2 x: their accumulators START at residual + bias, so each of
the K / 4 chained MFMA steps rounds at the magnitude of the final value, while the CPU evaluation
rounds the bare product and adds bias and residual last.  All exact cases are equal; 82-368 ties per
bf16 case from 127 columns up.
"""
import ctypes as C
import itertools

import pytest
import torch

import dcn_ref as R
import stream_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
E_ARG = -1


def _lib():
    from iouaware import _lib as L
    return L.lib()


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else C.c_void_p(0)


def _s():
    from iouaware.ops import _stream
    return _stream()


def _dev(ts):
    return [t.to(DEV).contiguous() if t is not None else None for t in ts]


def _checked(buf, out, what):
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()), '%s: NaN left in (or written to) the output' % (what,)
    assert S.guard_ok(buf, out.numel()), '%s: a guard band was written' % (what,)


def _gates(tag, got, ref, fig):
    e = R.rel_err(got, ref)
    print('  %-52s %.2e (%.2f x the fp32 figure %.2e)' % (tag, e, e / fig, fig))
    assert fig > 0
    assert e <= R.GATE_A, 'gate A: %s %.3e' % (tag, e)
    assert e <= R.GATE_B * fig, 'gate B: %s HIP %.3e vs fp32 %.3e = %.2f x' % (tag, e, fig, e / fig)


# ------------------------------------------------------------------ the entries on guarded outputs
def _stream(x, w, b, r, relu, check=True):
    rows, k, n = x.shape[0], x.shape[1], w.shape[1]
    assert x.shape == (rows, k) and w.shape == (k, n) and (b is None or b.shape == (n,)) and (r is None or r.shape == (rows, n))
    buf, y = S.guarded(rows * n, DEV)
    assert _lib().ia_conv1x1_stream(_p(x), _p(w), _p(b), _p(r), _p(y), rows, k, n, int(relu), _s()) == 0
    if check:
        _checked(buf, y, ('stream', rows, k, n))
    return y.view(rows, n)


def _wide(x, w, b, r, relu, check=True):
    rows, k, n = x.shape[0], x.shape[1], w.shape[1]
    assert x.shape == (rows, k) and w.shape == (k, n) and (b is None or b.shape == (n,)) and (r is None or r.shape == (rows, n))
    buf, y = S.guarded(rows * n, DEV)
    assert _lib().ia_conv1x1_wide(_p(x), _p(w), _p(b), _p(r), _p(y), rows, k, n, int(relu), _s()) == 0
    if check:
        _checked(buf, y, ('wide', rows, k, n))
    return y.view(rows, n)


def _chain(x, w, b, r, w2, b2, check=True):
    rows, (k, n, n2) = x.shape[0], S.CHAIN_SHAPE
    assert x.shape == (rows, k) and w.shape == (k, n) and w2.shape == (n, n2) and (r is None or r.shape == (rows, n))
    assert (b is None or b.shape == (n,)) and (b2 is None or b2.shape == (n2,))
    bufy, y = S.guarded(rows * n, DEV)
    bufh, h = S.guarded(rows * n2, DEV)
    assert _lib().ia_conv1x1_chain(_p(x), _p(w), _p(b), _p(r), _p(w2), _p(b2), _p(y), _p(h), rows, k, n, n2, _s()) == 0
    if check:
        _checked(bufy, y, ('chain y', rows))
        _checked(bufh, h, ('chain h', rows))
    return y.view(rows, n), h.view(rows, n2)


def _bmm(a, w, check=True):
    batch, rows, k = a.shape
    n = w.shape[2]
    assert w.shape == (batch, k, n)
    buf, d = S.guarded(batch * rows * n, DEV)
    assert _lib().ia_batched_gemm_stream(_p(a), _p(w), _p(d), batch, rows, k, n, _s()) == 0
    if check:
        _checked(buf, d, ('batched', batch, rows, k, n))
    return d.view(batch, rows, n)


# ------------------------------------------------------------------ ia_conv1x1_stream
def _stream_combos(rows, n):
    if rows in S.STREAM_ALL_COMBO_ROWS:
        return list(itertools.product((False, True), repeat=3))        # (bias, residual, relu)
    return [(True, n == 256, True)]


@pytest.mark.parametrize('rows', S.STREAM_ROWS + (S.BIG_ROWS,))
@pytest.mark.parametrize('k,n', S.STREAM_SHAPES)
def test_stream_exact_on_integers(k, n, rows):
    x, w, b, r = _dev(S.int_case(rows, k, n))
    for (ub, ur, relu) in _stream_combos(rows, n):
        bb, rr = (b if ub else None), (r if ur else None)
        got = _stream(x, w, bb, rr, relu)
        assert torch.equal(got, S.conv1x1(x, w, bb, rr, relu).float()), (k, n, rows, ub, ur, relu)


@pytest.mark.parametrize('rows', S.STREAM_GATE_ROWS)
@pytest.mark.parametrize('k,n', S.STREAM_SHAPES)
def test_stream_within_the_gates_on_random_data(k, n, rows):
    cpu = S.rand_case(rows, k, n)
    x, w, b, r = _dev(cpu)
    for (ub, ur, relu) in _stream_combos(rows, n):
        got = _stream(x, w, b if ub else None, r if ur else None, relu).cpu()
        cb, cr = (cpu[2] if ub else None), (cpu[3] if ur else None)
        ref = S.conv1x1(cpu[0], cpu[1], cb, cr, relu)
        _gates('stream %dx%d rows %d bias %d res %d relu %d' % (k, n, rows, ub, ur, relu), got, ref,
               S.fp32_figure(cpu[0], cpu[1], cb, cr, relu, ref))


# ------------------------------------------------------------------ ia_conv1x1_wide
@pytest.mark.parametrize('rows', S.WIDE_ROWS + (S.WIDE_BIG_ROWS,))
def test_wide_exact_on_integers_and_within_the_gates(rows):
    k, n = S.WIDE_SHAPE
    x, w, b, r = _dev(S.int_case(rows, k, n))
    combos = list(itertools.product((False, True), repeat=3))
    for (ub, ur, relu) in combos:
        bb, rr = (b if ub else None), (r if ur else None)
        got = _wide(x, w, bb, rr, relu)
        ref = S.conv1x1(x, w, bb, rr, relu).float()
        for blk in (0, 1):                                              # both column blocks
            assert torch.equal(got[:, 256 * blk:256 * blk + 256], ref[:, 256 * blk:256 * blk + 256]), (rows, ub, ur, relu, blk)
    if rows in S.WIDE_GATE_ROWS:
        cpu = S.rand_case(rows, k, n)
        x, w, b, r = _dev(cpu)
        for (ub, ur, relu) in combos:
            got = _wide(x, w, b if ub else None, r if ur else None, relu).cpu()
            cb, cr = (cpu[2] if ub else None), (cpu[3] if ur else None)
            ref = S.conv1x1(cpu[0], cpu[1], cb, cr, relu)
            _gates('wide rows %d bias %d res %d relu %d' % (rows, ub, ur, relu), got, ref,
                   S.fp32_figure(cpu[0], cpu[1], cb, cr, relu, ref))


# ------------------------------------------------------------------ ia_conv1x1_chain
@pytest.mark.parametrize('rows', S.CHAIN_ROWS)
def test_chain_exact_on_integers_and_equal_to_two_stream_calls(rows):
    for integers, data in ((True, S.chain_int_case(rows)), (False, S.chain_rand_case(rows))):
        x, w, b, r, w2, b2 = _dev(data)
        for (ur, ub) in itertools.product((True, False), repeat=2):
            rr, bb, bb2 = (r if ur else None), (b if ub else None), (b2 if ub else None)
            y, h = _chain(x, w, bb, rr, w2, bb2)
            if integers:
                ry, rh = S.chain(x, w, bb, rr, w2, bb2)
                assert torch.equal(y, ry.float()) and torch.equal(h, rh.float()), (rows, ur, ub)
            y0 = _stream(x, w, bb, rr, True)
            h0 = _stream(y0, w2, bb2, None, True)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), (rows, ur, ub)
            assert torch.equal(h.view(torch.int32), h0.view(torch.int32)), (rows, ur, ub)


# ------------------------------------------------------------------ ia_batched_gemm_stream
@pytest.mark.parametrize('k,n,batch,rows', [s + c for s in S.BMM_SHAPES for c in S.BMM_CASES] + [(64, 64) + S.BMM_BIG_CASE])
def test_batched_exact_on_integers_and_within_the_gates(k, n, batch, rows):
    x, w, _, _ = S.int_case(rows, k, n, batch)
    x, w = _dev((x, w))
    got = _bmm(x, w)
    assert torch.equal(got, S.conv1x1(x, w).float()), (k, n, batch, rows)
    if (batch, rows) in S.BMM_GATE_CASES:
        cx, cw, _, _ = S.rand_case(rows, k, n, batch)
        got = _bmm(*_dev((cx, cw))).cpu()
        ref = S.conv1x1(cx, cw)
        _gates('batched %dx%d batch %d rows %d' % (k, n, batch, rows), got, ref, S.fp32_figure(cx, cw, None, None, False, ref))


# ------------------------------------------------------------------ non-finite containment
def _planted(rows, k):
    """(row, channel): first, middle and last row, a different k-group of the 16-channel step each"""
    return ((0, 1), (rows // 2, k // 2 + 6), (rows - 1, k - 5))


def _rows_differ(a, b):
    """indices of the rows whose bits differ"""
    return torch.nonzero((a.view(torch.int32) != b.view(torch.int32)).any(dim=-1)).flatten().tolist()


@pytest.mark.parametrize('rows', S.NAN_ROWS)
@pytest.mark.parametrize('kernel,k,n', [('stream',) + s for s in S.STREAM_SHAPES] + [('wide',) + S.WIDE_SHAPE])
def test_a_nan_row_stays_in_its_row_stream_and_wide(kernel, k, n, rows):
    run = _stream if kernel == 'stream' else _wide
    x, w, b, r = _dev(S.rand_case(rows, k, n))
    assert len({(c // 4) % 4 for (_, c) in _planted(rows, k)}) == 3
    for relu in (False, True):
        clean = run(x, w, b, r, relu)
        for (p, c) in _planted(rows, k):
            xn = x.clone()
            xn[p, c] = NAN
            got = run(xn, w, b, r, relu, check=False)
            torch.cuda.synchronize()
            assert _rows_differ(got, clean) == [p], (kernel, rows, p, c, relu)
            if relu:
                print('  %s %dx%d rows %d ReLU: the row of the NaN holds %s' % (kernel, k, n, rows, sorted(set(got[p].tolist()))[:4]))
            else:
                assert bool(torch.isnan(got[p]).all()), (kernel, rows, p, c)


@pytest.mark.parametrize('rows', S.NAN_ROWS)
def test_a_nan_row_stays_in_its_row_chain(rows):
    x, w, b, r, w2, b2 = _dev(S.chain_rand_case(rows))
    cy, ch = _chain(x, w, b, r, w2, b2)
    for (p, c) in _planted(rows, 64):
        xn = x.clone()
        xn[p, c] = NAN
        y, h = _chain(xn, w, b, r, w2, b2, check=False)
        torch.cuda.synchronize()
        assert _rows_differ(y, cy) in ([p], []) and _rows_differ(h, ch) in ([p], []), (rows, p, c)
        print('  chain rows %d: the row of the NaN holds y %s, h == relu(bias2): %s'
              % (rows, sorted(set(y[p].tolist()))[:4], bool(torch.equal(h[p], b2.clamp(min=0)))))


@pytest.mark.parametrize('rows', S.NAN_ROWS)
@pytest.mark.parametrize('k,n', S.BMM_SHAPES)
def test_a_nan_row_stays_in_its_row_batched(k, n, rows):
    x, w, _, _ = S.rand_case(rows, k, n, batch=3)
    x, w = _dev((x, w))
    clean = _bmm(x, w)
    for m, (p, c) in enumerate(_planted(rows, k)):
        xn = x.clone()
        xn[m, p, c] = NAN
        got = _bmm(xn, w, check=False)
        torch.cuda.synchronize()
        assert _rows_differ(got.view(3 * rows, n), clean.view(3 * rows, n)) == [m * rows + p], (k, n, rows, m, p, c)
        assert bool(torch.isnan(got[m, p]).all())


# ------------------------------------------------------------------ the stems
def _stem_x(x, dtype, misalign=False):
    """x (B, H, W, 3) on the CPU -> (allocation, view): x inside a NaN-filled allocation, a row's worth
    (or more) of NaN before and after; aligned to 16 bytes, or one element past that"""
    row, n = x.shape[2] * 3, x.numel()
    pre = (row + 7) // 8 * 8 + (1 if misalign else 0)
    buf = torch.full((pre + n + row + 8,), NAN, dtype=dtype, device=DEV)
    v = buf[pre:pre + n]
    v.copy_(x.reshape(-1).to(dtype))
    es = buf.element_size()
    assert v.data_ptr() % 16 == (es if misalign else 0) and bool(torch.isnan(buf[:pre]).all()) and bool(torch.isnan(buf[pre + n:]).all())
    return buf, v


def _stem(x, w, dtype, misalign=False):
    """x (B, H, W, 3), w (64, 3, 7, 7) on the CPU -> (B, Ho, Wo, 64) from the kernel, on the CPU"""
    from iouaware import ops
    B, H, W, _ = x.shape
    Ho, Wo = S.stem_geometry(B, H, W)[:2]
    hold, xv = _stem_x(x, dtype, misalign)
    if dtype == torch.float32:
        wp, fn = ops.stem_weight(w.to(DEV)), _lib().ia_stem_conv7x7s2
        assert wp.shape == (148, 64) and wp.dtype == torch.float32 and wp.is_contiguous()
    else:
        wp, fn = ops.stem_weight_bf16(w.to(DEV)), _lib().ia_stem_conv7x7s2_bf16
        assert wp.shape == (11, 4, 64, 4) and wp.dtype == torch.bfloat16 and wp.is_contiguous()
    buf, y = S.guarded(B * Ho * Wo * 64, DEV, dtype)
    assert fn(_p(xv), _p(wp), _p(y), B, H, W, _s()) == 0
    _checked(buf, y, ('stem', dtype, B, H, W, misalign))
    del hold
    return y.view(B, Ho, Wo, 64).cpu()


@pytest.mark.parametrize('B,H,W', S.STEM_CASES)
def test_stem_fp32_exact_on_integers(B, H, W):
    x, w = S.stem_int_case(B, H, W)
    got = _stem(x, w, torch.float32)
    assert torch.equal(got, S.stem(x, w).float())
    if (B, H, W) in S.STEM_MISALIGNED_CASES:                            # the scalar path at a vector width
        assert torch.equal(_stem(x, w, torch.float32, misalign=True).view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize('B,H,W', S.STEM_CASES)
def test_stem_bf16_exact_on_integers_and_ties_to_even(B, H, W):
    for kind in ('bf16_exact', 'bf16_ties'):
        x, w = S.stem_int_case(B, H, W, kind)
        ref = S.stem(x, w)
        got = _stem(x, w, torch.bfloat16)
        if kind == 'bf16_exact':
            assert torch.equal(got.double(), ref)
        else:
            print('  bf16 stem %s: %d ties' % ((B, H, W), int(((ref.abs() > 256) & (ref % 2 != 0)).sum())))
        assert torch.equal(got, ref.float().to(torch.bfloat16)), (B, H, W, kind)
        if (B, H, W) in S.STEM_MISALIGNED_CASES:
            assert torch.equal(_stem(x, w, torch.bfloat16, misalign=True).view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize('B,H,W', S.STEM_GATE_CASES)
def test_stem_fp32_within_the_gates_on_random_data(B, H, W):
    x, w = S.stem_rand_case(B, H, W)
    ref = S.stem(x, w)
    _gates('stem %s' % ((B, H, W),), _stem(x, w, torch.float32), ref, S.stem_fp32_figure(x, w, ref))


# ------------------------------------------------------------------ rejections
def test_every_entry_rejects_bad_arguments_and_leaves_the_output_alone():
    from iouaware import ops
    L, s = _lib(), _s()
    calls = []                                                          # (what, return code), outputs

    def t(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=DEV)

    def out(*shape, dtype=torch.float32):
        return torch.full(shape, NAN, dtype=dtype, device=DEV)

    outs = []

    def fresh(*shape, dtype=torch.float32):
        outs.append(out(*shape, dtype=dtype))
        return outs[-1]

    rows = 17
    # ia_conv1x1_stream and ia_conv1x1_wide: the same signature
    for name, fn, (k, n), bad_kn in (('stream', L.ia_conv1x1_stream, (64, 256), (128, 128)),
                                     ('wide', L.ia_conv1x1_wide, S.WIDE_SHAPE, (64, 256))):
        x, w, b, r = t(rows + 1, k), t(k + 1, n), t(n), t(rows + 1, n)
        x2, w2 = t(rows + 1, bad_kn[0]), t(bad_kn[0] + 1, bad_kn[1])
        for what, a in (('x null', (None, _p(w), _p(b), _p(r), None, rows, k, n)),
                        ('w null', (_p(x), None, _p(b), _p(r), None, rows, k, n)),
                        ('0 rows', (_p(x), _p(w), _p(b), _p(r), None, 0, k, n)),
                        ('(k, n)', (_p(x2), _p(w2), _p(b), _p(r), None, rows) + bad_kn),
                        ('x + 4 bytes', (_p(x, 4), _p(w), _p(b), _p(r), None, rows, k, n)),
                        ('w + 4 bytes', (_p(x), _p(w, 4), _p(b), _p(r), None, rows, k, n)),
                        ('residual + 4 bytes', (_p(x), _p(w), _p(b), _p(r, 4), None, rows, k, n)),
                        ('y + 4 bytes', (_p(x), _p(w), _p(b), _p(r), 4, rows, k, n))):
            y = fresh(rows + 1, max(n, bad_kn[1]))
            a = list(a)
            a[4] = _p(y, a[4] or 0)
            calls.append(((name, what), fn(*(a + [1, s]))))
        calls.append(((name, 'y null'), fn(_p(x), _p(w), _p(b), _p(r), None, rows, k, n, 1, s)))
    # ia_conv1x1_chain
    k, n, n2 = S.CHAIN_SHAPE
    x, w, b, r, w2, b2 = t(rows + 1, k), t(k + 1, n), t(n), t(rows + 1, n), t(n + 1, n2), t(n2)
    for what, a in (('x null', dict(x=None)), ('w null', dict(w=None)), ('w2 null', dict(w2=None)), ('0 rows', dict(rows=0)),
                    ('(k, n, n2)', dict(kn=(64, 64, 64))), ('(k, n, n2) wide', dict(kn=(128, 256, 64))),
                    ('x + 4 bytes', dict(x=_p(x, 4))), ('w + 4 bytes', dict(w=_p(w, 4))), ('w2 + 4 bytes', dict(w2=_p(w2, 4))),
                    ('residual + 4 bytes', dict(r=_p(r, 4))), ('y + 4 bytes', dict(yo=4)), ('h + 4 bytes', dict(ho=4)),
                    ('y null', dict(yn=True)), ('h null', dict(hn=True))):
        y, h = fresh(rows + 1, n), fresh(rows + 1, n2)
        d = dict(x=_p(x), w=_p(w), r=_p(r), w2=_p(w2), rows=rows, kn=S.CHAIN_SHAPE, yo=0, ho=0, yn=False, hn=False)
        d.update(a)
        calls.append((('chain', what), L.ia_conv1x1_chain(
            d['x'], d['w'], _p(b), d['r'], d['w2'], _p(b2), None if d['yn'] else _p(y, d['yo']), None if d['hn'] else _p(h, d['ho']),
            d['rows'], d['kn'][0], d['kn'][1], d['kn'][2], s)))
    # ia_batched_gemm_stream
    k, n, batch = 64, 64, 3
    a_, w_ = t(batch, rows + 1, k), t(batch, k + 1, n)
    a2, w2_ = t(batch, rows + 1, 64), t(batch, 64 + 1, 256)
    for what, a in (('A null', dict(a=None)), ('W null', dict(w=None)), ('D null', dict(dn=True)), ('0 rows', dict(rows=0)),
                    ('(k, n)', dict(a=_p(a2), w=_p(w2_), kn=(64, 256))), ('A + 4 bytes', dict(a=_p(a_, 4))),
                    ('W + 4 bytes', dict(w=_p(w_, 4))), ('D + 4 bytes', dict(do=4)), ('batch 0', dict(batch=0)),
                    ('batch -1', dict(batch=-1)), ('batch 65 536', dict(batch=65536))):
        dd = fresh(batch, rows + 1, 256)
        d = dict(a=_p(a_), w=_p(w_), rows=rows, kn=(k, n), do=0, dn=False, batch=batch)
        d.update(a)
        calls.append((('batched', what), L.ia_batched_gemm_stream(
            d['a'], d['w'], None if d['dn'] else _p(dd, d['do']), d['batch'], d['rows'], d['kn'][0], d['kn'][1], s)))
    # the stems
    B, H, W = 2, 9, 8
    Ho, Wo = S.stem_geometry(B, H, W)[:2]
    wz = torch.zeros(64, 3, 7, 7, device=DEV)
    for name, fn, dtype, wp in (('stem', L.ia_stem_conv7x7s2, torch.float32, ops.stem_weight(wz)),
                                ('stem bf16', L.ia_stem_conv7x7s2_bf16, torch.bfloat16, ops.stem_weight_bf16(wz))):
        x = t(B * H * W * 3 + 8, dtype=dtype)
        wp = torch.cat([wp.reshape(-1), wp.reshape(-1)[:8]])            # room behind the offset pointer
        for what, a in (('x null', dict(x=None)), ('w null', dict(w=None)), ('y null', dict(yn=True)), ('batch 0', dict(B=0)),
                        ('0 rows', dict(H=0)), ('0 columns', dict(W=0)), ('w + 4 bytes', dict(w=_p(wp, 4))), ('y + 4 bytes', dict(yo=4)),
                        ('x + half an element', dict(x=_p(x, x.element_size() // 2)))):
            y = fresh(B * Ho * Wo * 64 + 8, dtype=dtype)
            d = dict(x=_p(x), w=_p(wp), yo=0, yn=False, B=B, H=H, W=W)
            d.update(a)
            calls.append(((name, what), fn(d['x'], d['w'], None if d['yn'] else _p(y, d['yo']), d['B'], d['H'], d['W'], s)))
    torch.cuda.synchronize()
    bad = [c for c in calls if c[1] != E_ARG]
    assert not bad, bad
    assert len(calls) == 2 * 9 + 14 + 11 + 2 * 9
    for o in outs:
        assert bool(torch.isnan(o).all())

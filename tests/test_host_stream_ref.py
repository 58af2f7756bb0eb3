"""CPU: the instruments of tests/test_gpu_stream_edges.py can see what they are meant to see.

The GPU file pins the streaming MFMA kernels (csrc/conv1x1_stream.hip, csrc/stem.hip) with integer
data that a correct kernel reproduces exactly, with the project's two gates on random data, and with
NaN-filled outputs between guard bands (tests/stream_ref.py).  Here, without a GPU:

  * the case lists cross the edges of the launch geometry they are named for;
  * the integer generators keep every partial sum below 2^24 (147 for the exact bf16 set), and the
    second bf16 set does contain ties of the bf16 rounding;
  * each fault a kernel of this kind can have -- emulated on the same integer data -- breaks equality
    at the shapes that are meant to catch it;
  * operands cut to 16 bits fail gate B on the random data;
  * a write past either end of a guarded output is seen.
"""
import pytest
import torch

import dcn_ref as R
import stream_ref as S


def _exact(x, w, bias=None, res=None, relu=False):
    return S.conv1x1(x, w, bias, res, relu).float()


def _differs(bad, ref):
    """what torch.equal(kernel result, ref) would say of the faulty result (NaN = never stored)"""
    return not torch.equal(bad.float(), ref)


def test_the_cases_cross_the_geometry_edges():
    assert S.geometry('stream', 15) == (1, 8) and S.geometry('stream', 17)[0] == 2
    assert S.geometry('stream', 128) == (8, 8) and S.geometry('stream', 129) == (9, 16)       # one workgroup of tiles, then two
    assert S.geometry('stream', S.BIG_ROWS) == (4113, 4096) and S.BIG_ROWS == 241 * 273 and S.BIG_ROWS % 16 == 1
    assert S.geometry('chain', S.BIG_ROWS) == (4113, 4096)
    assert S.geometry('wide', 257) == (17, 32)
    assert S.geometry('wide', S.WIDE_BIG_ROWS) == (2050, 2048) and S.WIDE_BIG_ROWS % 16 == 3
    assert S.geometry('batched', 1931, 36) == (121, 120) and 1931 % 16 == 11                  # 15 workgroups per matrix
    assert S.geometry('batched', 259, 513) == (17, 8)                                         # one workgroup per matrix
    assert S.geometry('batched', 259, 512) == (17, 8) and S.geometry('batched', 259, 511) == (17, 16)
    assert S.geometry('batched', S.BIG_ROWS, 3) == (4113, 171 * 8)
    assert S.stem_geometry(9, 456, 6)[2:] == (513, 512) and S.stem_geometry(9, 456, 8)[2:] == (513, 512)
    assert S.stem_geometry(1, 9, 128)[1] == 64 and S.stem_geometry(1, 9, 129)[1] == 65        # the 64-column tile edge
    assert S.stem_geometry(2, 15, 132)[:3] == (8, 66, 2 * 2 * 2)
    # the staging paths: fp32 takes vectors at W % 4 == 0, bf16 at even W; both sides occur
    ws = [W for (_, _, W) in S.STEM_CASES]
    assert {W % 4 == 0 for W in ws} == {True, False} and {W % 2 == 0 for W in ws} == {True, False}
    assert (9, 456, 6)[2] % 4 != 0 and (9, 456, 6)[2] % 2 == 0 and (9, 456, 8)[2] % 4 == 0
    for c in S.STEM_GATE_CASES + S.STEM_MISALIGNED_CASES:
        assert c in S.STEM_CASES
    for (_, _, W) in S.STEM_MISALIGNED_CASES:
        assert W % 4 == 0


def test_integer_sums_stay_exact():
    """every partial sum an integer below 2^24; the chain's second product below 2.1e5; the bf16 sets
    within 147 and 441"""
    for (k, n) in S.STREAM_SHAPES + (S.WIDE_SHAPE,):
        x, w, b, r = S.int_case(129, k, n)
        for t, lo, hi in ((x, -3, 3), (w, -2, 2), (b, -3, 3), (r, -3, 3)):
            assert t.dtype == torch.float32 and bool((t == t.round()).all()) and lo <= float(t.min()) and float(t.max()) <= hi
        assert S.int_bound(x, w, b, r) <= 6 * k + 6 <= 1542 < 2 ** 24
    for (k, n) in S.BMM_SHAPES:
        x, w, _, _ = S.int_case(17, k, n, batch=36)
        assert x.shape == (36, 17, k) and w.shape == (36, k, n) and not torch.equal(w[0], w[1])
        assert S.int_bound(x, w) <= 6 * k
    x, w, b, r, w2, b2 = S.chain_int_case(257)
    y, h = S.chain(x, w, b, r, w2, b2)
    assert float(y.max()) <= 6 * 64 + 6 and S.int_bound(y, w2, b2) <= 390 * 2 * 256 + 3 < 2.1e5 < 2 ** 24
    assert bool((h == h.round()).all()) and float(h.max()) > 0
    for case in S.STEM_CASES:
        x, w = S.stem_int_case(*case)
        assert float(x.abs().max()) <= 3 and float(w.abs().max()) <= 2
        assert float(S.stem(x.abs(), w.abs()).max()) <= 147 * 6
        x, w = S.stem_int_case(*case, kind='bf16_exact')
        assert float(x.abs().max()) <= 1 and float(w.abs().max()) <= 1
        y = S.stem(x, w)
        assert float(S.stem(x.abs(), w.abs()).max()) <= 147
        assert torch.equal(y.float().to(torch.bfloat16).double(), y)                          # exact in bf16
        x, w = S.stem_int_case(*case, kind='bf16_ties')
        assert float(x.abs().max()) <= 3 and float(w.abs().max()) <= 1
        assert float(S.stem(x.abs(), w.abs()).max()) <= 441


@pytest.mark.parametrize('case', [(1, 9, 127), (1, 9, 128), (1, 9, 129), (1, 9, 130), (2, 15, 132)])
def test_the_second_bf16_set_holds_ties_of_both_signs_and_parities(case):
    """(the cases narrower than 7 pixels of 2..3 cannot reach 256: no ties there)"""
    x, w = S.stem_int_case(*case, kind='bf16_ties')
    y = S.stem(x, w)
    odd = (y.abs() > 256) & (y % 2 != 0)                    # bf16 spacing is 2 above 256: every odd value is a tie
    assert int((odd & (y > 0)).sum()) > 0 and int((odd & (y < 0)).sum()) > 0
    # ties whose even neighbours differ in which one has the even mantissa: both roundings are asked for
    up = odd & (((y.abs() + 1) / 2) % 2 == 0)
    assert int(up.sum()) > 0 and int((odd & ~up).sum()) > 0
    # round-to-nearest-even against the two wrong tie rules
    rne = y.float().to(torch.bfloat16).double()
    away = torch.where(odd, y + y.sign(), rne)
    trunc = torch.where(odd, y - y.sign(), rne)
    assert not torch.equal(rne, away) and not torch.equal(rne, trunc)


# ------------------------------------------------------------------ faults of the 1x1 kernels
def _catchers_1x1(fault):
    """-> [(kernel, k, n, rows, batch, bias, residual)]: the GPU cases meant to catch the fault"""
    stream = [('stream', k, n, rows, None) for (k, n) in S.STREAM_SHAPES for rows in S.STREAM_ROWS + (S.BIG_ROWS,)]
    wide = [('wide',) + S.WIDE_SHAPE + (rows, None) for rows in S.WIDE_ROWS + (S.WIDE_BIG_ROWS,)]
    bmm = [('batched', k, n, rows, batch) for (k, n) in S.BMM_SHAPES for (batch, rows) in S.BMM_CASES]
    bmm.append(('batched', 64, 64, S.BMM_BIG_CASE[1], S.BMM_BIG_CASE[0]))
    cases = stream + wide + bmm
    if fault == 'last_tile_from_last_row':                  # a partial last tile of at least two rows
        keep = [c for c in cases if c[3] % 16 >= 2]
        assert {c[3] for c in keep} == {15, 127, S.WIDE_BIG_ROWS, 1931, 259}
    elif fault == 'second_tile_skipped':                    # more tiles than wavefronts
        keep = [c for c in cases if S.geometry(c[0], c[3], c[4] or 1)[0] > S.geometry(c[0], c[3], c[4] or 1)[1]]
        assert {c[3] for c in keep} == {S.BIG_ROWS, S.WIDE_BIG_ROWS, 1931, 259}
    elif fault == 'bias_skipped_from_block_8':              # 256 output columns per workgroup
        keep = [c for c in stream + wide if c[2] >= 256]
    elif fault == 'residual_twice':
        keep = [c for c in stream if c[3] in S.STREAM_ALL_COMBO_ROWS or c[2] == 256] + wide
    elif fault == 'k_groups_swapped':
        keep = cases
    else:
        keep = [c for c in bmm if c[4] > 1]
    return keep


@pytest.mark.parametrize('fault', S.FAULTS_1X1)
def test_every_1x1_fault_breaks_equality_where_it_should(fault):
    keep = _catchers_1x1(fault)
    assert keep
    for (kernel, k, n, rows, batch) in keep:
        x, w, b, r = S.int_case(rows, k, n, batch)
        if kernel == 'batched':
            b = r = None
        elif fault != 'residual_twice' and not (kernel == 'wide' or n == 256 or rows in S.STREAM_ALL_COMBO_ROWS):
            r = None                                        # the combination the GPU case runs: bias + ReLU
        ref = _exact(x, w, b, r, kernel != 'batched')
        assert torch.equal(S.faulty_1x1(None, kernel, x, w, b, r, kernel != 'batched').float(), ref)
        assert _differs(S.faulty_1x1(fault, kernel, x, w, b, r, kernel != 'batched'), ref), (fault, kernel, k, n, rows, batch)


@pytest.mark.parametrize('fault', S.FAULTS_1X1[:5])
def test_every_chain_fault_breaks_equality_of_both_outputs(fault):
    rows_of = {'last_tile_from_last_row': (), 'second_tile_skipped': (S.BIG_ROWS,)}.get(fault, S.CHAIN_ROWS)
    # (no chain case has a partial last tile of two rows or more: that clamp is the wide kernel's own
    # 64-bit one, which the 32 787-row wide case holds; the 32-bit one of k_conv1x1_stream has 15 / 127)
    assert all(r % 16 < 2 for r in S.CHAIN_ROWS)
    for rows in rows_of:
        x, w, b, r, w2, b2 = S.chain_int_case(rows)
        y, h = (t.float() for t in S.chain(x, w, b, r, w2, b2))
        by, bh = S.faulty_chain(fault, x, w, b, r, w2, b2)
        assert _differs(by, y) and _differs(bh, h), (fault, rows)
        gy, gh = S.faulty_chain(None, x, w, b, r, w2, b2)
        assert torch.equal(gy.float(), y) and torch.equal(gh.float(), h)


# ------------------------------------------------------------------ faults of the stems
@pytest.mark.parametrize('kind', ['fp32', 'bf16_exact', 'bf16_ties'])
@pytest.mark.parametrize('fault', S.FAULTS_STEM)
def test_every_stem_fault_breaks_equality_where_it_should(fault, kind):
    cases = S.STEM_CASES if fault == 'edge_clamp' else [c for c in S.STEM_CASES if c[0] > 1]
    assert len(cases) >= 4
    for case in cases:
        x, w = S.stem_int_case(*case, kind=kind)
        ref = S.stem(x, w)
        assert torch.equal(S.stem(x.double(), w.double(), torch.float32).double(), ref)       # exact in fp32 as well
        bad = S.faulty_stem(fault, x, w)
        if kind != 'fp32':
            ref, bad = ref.float().to(torch.bfloat16), bad.float().to(torch.bfloat16)
        assert bad.shape == ref.shape and not torch.equal(bad, ref), (fault, kind, case)


# ------------------------------------------------------------------ the gates
def test_operands_cut_to_16_bits_fail_gate_b():
    for (k, n), rows in ((S.STREAM_SHAPES[0], 17), (S.STREAM_SHAPES[1], 4113), (S.WIDE_SHAPE, 257), (S.BMM_SHAPES[2], 17)):
        x, w, b, r = S.rand_case(rows, k, n)
        ref = S.conv1x1(x, w, b, r, True)
        fig = S.fp32_figure(x, w, b, r, True, ref)
        assert 0 < fig <= R.GATE_A / 10
        for cx, cw in ((S.cut16(x), w), (x, S.cut16(w))):
            e = R.rel_err(S.conv1x1(cx, cw, b, r, True), ref)
            assert e > R.GATE_B * fig, (k, n, rows, e, fig)
    for case in S.STEM_GATE_CASES:
        x, w = S.stem_rand_case(*case)
        ref = S.stem(x, w)
        fig = S.stem_fp32_figure(x, w, ref)
        assert 0 < fig <= R.GATE_A / 10
        assert R.rel_err(S.stem(x, w, torch.float32), ref) <= fig * R.GATE_B                  # the library's own order passes
        for cx, cw in ((S.cut16(x), w), (x, S.cut16(w))):
            assert R.rel_err(S.stem(cx, cw), ref) > R.GATE_B * fig, case


def test_the_fp32_figure_moves_with_the_order_but_not_past_gate_b():
    """why the figure is a maximum over orders: single orders differ, by less than the gate's factor"""
    x, w, b, r = S.rand_case(129, 256, 64)
    ref = S.conv1x1(x, w, b, r, False)
    figs = [R.rel_err(S.conv1x1(x[:, S._perm(256, o)], w[S._perm(256, o)], b, r, False, torch.float32), ref)
            for o in range(S.ORDERS)]
    assert len(set(figs)) > 1 and max(figs) <= R.GATE_B * min(figs) and max(figs) == S.fp32_figure(x, w, b, r, False, ref)


# ------------------------------------------------------------------ the guard bands
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_guard_bands_see_a_write_past_either_end(dtype):
    n = 17 * 64
    buf, out = S.guarded(n, 'cpu', dtype)
    guard = S.GUARD * 4 // out.element_size()
    assert buf.numel() == n + 2 * guard and out.numel() == n and bool(torch.isnan(out).all()) and S.guard_ok(buf, n)
    out.fill_(1.0)
    assert S.guard_ok(buf, n)
    for i in (guard - 1, guard + n, 0, buf.numel() - 1):
        keep = buf[i].clone()
        buf[i] = 1.0
        assert not S.guard_ok(buf, n)
        buf[i] = keep
    assert S.guard_ok(buf, n)

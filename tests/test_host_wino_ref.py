"""Host: the F(4x4,3x3) restatement of tests/wino_ref.py is right (fp64: it IS the convolution and
its autograd, to 1e-12), and the two gates the GPU tests of the training node apply
(tests/test_gpu_wino_fp64.py) separate a correct fp32 evaluation from the faults they exist for.

    gate A  max|got - ref| / max|ref| <= 1e-4            the project's contract
    gate B  the same figure <= 4 x that of the fp32 helper on the same tensors (wino_ref.GATE_B:
            set at 2, raised once to its ceiling, with the reason, after the first MI355X run)

Shown on the helper alone, with the fp32 helper as the "candidate": GEMM operands cut to 16
significand bits (a 2-term bf16 split) fail gate B for y and dW; one tile lost, the edge select of
dM = A dY A^T lost, one coefficient of A changed each fail gate A.  If a bar is loosened until a
fault passes, this file fails."""
import pytest
import torch
import torch.nn.functional as F

import wino_ref as R


def _data(seed, batch, cin, cout, sizes):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xs = [torch.randn(batch, cin, h, ww, generator=g) for (h, ww) in sizes]
    ups = [torch.randn(batch, cout, h, ww, generator=g) for (h, ww) in sizes]
    return w, b, xs, ups


def _autograd64(w, b, xs, ups):
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    x64 = [x.double().requires_grad_(True) for x in xs]
    y64 = [F.conv2d(x, w64, b64, padding=1) for x in x64]
    sum((y * u.double()).sum() for y, u in zip(y64, ups)).backward()
    return [y.detach() for y in y64], [x.grad for x in x64], w64.grad, b64.grad


def test_fp64_helper_is_the_convolution_and_its_autograd():
    """partial tiles in both directions, a level with H < 4 and W < 4, a 1x1 level, batch 3"""
    sizes = [(9, 14), (6, 5), (3, 2), (1, 1)]
    w, b, xs, ups = _data(0, 3, 8, 12, sizes)
    y64, dx64, dw64, db64 = _autograd64(w, b, xs, ups)
    ys, v = R.conv_fwd(xs, w, b, torch.float64, keep_v=True)
    assert v.shape == (36, R.tile_count(sizes, 3), 8)
    dxs = R.conv_dx(ups, w, torch.float64)
    for got, ref in zip(ys + dxs, y64 + dx64):
        assert got.shape == ref.shape and R.rel_err(got, ref) <= 1e-12
    assert R.rel_err(R.conv_dw(v, ups, torch.float64), dw64) <= 1e-12
    assert R.rel_err(R.conv_db(ups, torch.float64), db64) <= 1e-12
    # ReLU and groups are layout / element-wise: V of two channel groups = the two halves
    yr = R.conv_fwd(xs, w, b, torch.float64, relu=True)
    assert all(torch.equal(a, c.clamp(min=0)) for a, c in zip(yr, ys))
    v2 = R.input_transform(xs, torch.float64, groups=2)
    assert torch.equal(v2[:36], v[:, :, :4]) and torch.equal(v2[36:], v[:, :, 4:])
    m = torch.randn(72, v.shape[1], 4, dtype=torch.float64)
    a = R.output_transform(m, sizes, 3, groups=2)
    c = R.output_transform(torch.cat([m[:36], m[36:]], dim=2), sizes, 3)
    assert all(torch.equal(p, q) for p, q in zip(a, c))


def test_tile_order_and_padding():
    """V[:, t] is the transform of tile t's zero-padded 6x6 patch, tiles level-major, then image,
    then row-major; the pre-activation leaves the padding zero"""
    sizes = [(5, 9), (2, 3)]
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(2, 4, h, w, generator=g, dtype=torch.float64) for (h, w) in sizes]
    s, t = torch.randn(4, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    v = R.input_transform(xs, pre=(s, t, True))
    T = R.tile_count(sizes, 2)
    assert v.shape == (36, T, 4) and T == 2 * 6 + 2 * 1
    for tt in range(T):
        l, b, ty, tx = R.tile_index(sizes, 2, tt)
        h, w = sizes[l]
        d = torch.zeros(4, 6, 6, dtype=torch.float64)
        for i in range(6):
            for j in range(6):
                y, x = 4 * ty - 1 + i, 4 * tx - 1 + j
                if 0 <= y < h and 0 <= x < w:
                    d[:, i, j] = (xs[l][b, :, y, x] * s + t).clamp(min=0)
        ref = torch.einsum('ik,ckl,jl->ijc', R.BT, d, R.BT).reshape(36, 4)
        assert float((v[:, tt] - ref).abs().max()) <= 1e-12 * float(ref.abs().max() + 1)


def test_cut_mantissa_keeps_the_requested_bits():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -16, 1.0 + 2.0 ** -15, -3.1415927, 1e-20, 65504.0])
    c = R.cut_mantissa(x, 16)
    assert float(c[0]) == 1.0 and float(c[1]) == 1.0 + 2.0 ** -15 and float(c[2]) == 1.0 + 2.0 ** -15
    assert float(((c - x).abs() / x.abs()).max()) <= 2.0 ** -16
    assert torch.equal(R.cut_mantissa(c, 16), c) and torch.equal(R.cut_mantissa(x, 24), x)


# the five pyramid levels of a 400 x 672 pad: partial tiles at every level but the first
_SIZES = [(50, 84), (25, 42), (13, 21), (7, 11), (4, 6)]


@pytest.fixture(scope='module')
def case():
    w, b, xs, ups = _data(5, 2, 128, 48, _SIZES)
    ref = _autograd64(w, b, xs, ups)
    ys, v = R.conv_fwd(xs, w, b, torch.float32, keep_v=True)
    dw = R.conv_dw(v, ups, torch.float32)
    return dict(w=w, b=b, xs=xs, ups=ups, ref=ref, ys=ys, v=v, dw=dw)


def test_gates_pass_the_fp32_helper_itself(case):
    """other summation orders of the same fp32 products stay inside a margin of 2: gate B is not
    consumed by reassociation on the CPU"""
    y64, dx64, dw64, db64 = case['ref']
    e_y = R.worst(case['ys'], y64)
    e_dw = R.rel_err(case['dw'], dw64)
    assert e_y <= R.GATE_A and e_dw <= R.GATE_A
    T = case['v'].shape[1]
    for k, perm in enumerate([torch.arange(T - 1, -1, -1), torch.randperm(T, generator=torch.Generator().manual_seed(9))]):
        dm = R.grad_output_transform(case['ups'], torch.float32)
        parts = [torch.bmm(case['v'][:, p].transpose(1, 2), dm[:, p]) for p in perm.chunk(7 + k)]
        dw = R.weight_grad(sum(parts[1:], parts[0]), torch.float32)
        e, h, ratio = R.gates(dw, case['dw'], dw64)
        print('dW order %d: %.2e vs helper %.2e, ratio %.2f' % (k, e, h, ratio))
        assert ratio <= 2.0


def test_gate_b_fails_16_bit_operands(case):
    y64, dx64, dw64, db64 = case['ref']
    cut = lambda t: R.cut_mantissa(t, 16)                                          # noqa: E731
    ys, v = R.conv_fwd(case['xs'], case['w'], case['b'], torch.float32, operand=cut, keep_v=True)
    e, h, ratio = R.gates(ys, case['ys'], y64)
    print('y  16-bit operands: %.2e vs helper %.2e, ratio %.1f' % (e, h, ratio))
    assert ratio > R.GATE_B_MAX
    dw = R.conv_dw(v, case['ups'], torch.float32, operand=cut)
    e, h, ratio = R.gates(dw, case['dw'], dw64)
    print('dW 16-bit operands: %.2e vs helper %.2e, ratio %.1f' % (e, h, ratio))
    assert ratio > R.GATE_B_MAX


def test_gate_a_fails_structural_faults(case):
    y64, dx64, dw64, db64 = case['ref']
    v, ups = case['v'], case['ups']
    lost = v.clone()
    lost[:, -1] = 0                                     # the last tile never reaches the product
    e = R.rel_err(R.conv_dw(lost, ups, torch.float32), dw64)
    print('dW, one tile of %d lost: %.2e' % (v.shape[1], e))
    assert e > 10 * R.GATE_A
    e = R.rel_err(R.conv_dw(v, ups, torch.float32, edge='replicate'), dw64)
    print('dW, dY outside the map not zeroed: %.2e' % e)
    assert e > 10 * R.GATE_A
    at = R.AT.clone()
    at[2, 3] = 2.0                                      # t02 = y0 + 2 y2 instead of y0 + 4 y2
    e = R.rel_err(R.conv_dw(v, ups, torch.float32, at=at), dw64)
    print('dW, one coefficient of A changed: %.2e' % e)
    assert e > 10 * R.GATE_A
    # the same faults in the forward direction
    ys = R.output_transform(torch.bmm(lost, R.weight_transform(case['w'], torch.float32)),
                            _SIZES, 2, case['b'])
    assert R.worst(ys, y64) > 10 * R.GATE_A


def test_weight_gradient_slices_divide_the_tile_list():
    """winograd_train._du_slices: equal slices (views of V and dM) of at most DU_ROWS tiles; one
    slice when the tile count has no divisor in reach"""
    from iouaware.winograd_train import DU_ROWS, _du_slices
    for tiles in (1, 380, 1092, 4200, 5720, 16800, 1031, 2 * 1031, 4 * 5720, 9973):
        n = _du_slices(tiles)
        assert n >= 1 and tiles % n == 0 and (n == 1 or tiles // n <= DU_ROWS), (tiles, n)
    assert _du_slices(380) == 1 and _du_slices(5720) == 8 and _du_slices(2 * 1031) == 1

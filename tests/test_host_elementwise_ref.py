"""CPU: the yardstick of tests/test_gpu_elementwise_edges.py (tests/elementwise_ref.py) held to account
on the very inputs of the GPU tests, and the argument checks of ia_channel_affine_act_nhwc that return
before any launch.

  * the fp32 op-by-op epilogue equals the same operations in fp64 rounded once each, wherever every
    fp64 sum was exact; the remaining elements are counted and capped at 1 in 10 000 (the test prints
    the share: 0 of 10 350 440 elements on the committed inputs);
  * an evaluation that contracts the product and the sum into one rounding (what -ffp-contract=off
    forbids) is NOT equal: the yardstick can see a fused multiply-add;
  * bf16 pool: "round, then ReLU, then pool" (the module route) equals "pool in fp32, then round" (the
    kernel), with ties to even planted in channel 0;
  * the NaN masks: of the planted epilogue inputs, and of the pool (an output is NaN exactly when a
    tap of its window is).
"""
import ctypes

import numpy as np
import pytest
import torch

import elementwise_ref as E

CAP = 1e-4
IA_E_ARG = -1


def _affine_inputs():
    """every (x, r, vectors, channel axis) the GPU epilogue tests use"""
    for name, pixels, C in E.nhwc_cases():
        x, r = E.nhwc_data(pixels, C, E.DTYPES[name])
        yield x, r, E.vecs(C), -1
    for name, dtype in E.DTYPES.items():
        for hw in E.NCHW_HW:
            x, r = E.nchw_data(hw, dtype)
            yield x, r, E.vecs(E.NCHW_NC[1]), 1
        for layout, hw, caxis in _NONFINITE:
            yield E.nonfinite_case(layout, dtype, hw)[:3] + (caxis,)


_NONFINITE = [('nhwc', None, -1)] + [('nchw', hw, 1) for hw in E.NONFINITE_NCHW_HW]


def test_same_sees_one_ulp_and_a_nan_but_not_the_sign_of_a_zero():
    a = torch.tensor([1.0, 0.0, E.NAN, -2.5])
    assert E.same(a, a.clone())
    assert E.same(a, torch.tensor([1.0, -0.0, E.NAN, -2.5]))
    assert not E.same(a, torch.tensor([1.0 + 2.0 ** -23, 0.0, E.NAN, -2.5]))
    assert not E.same(a, torch.tensor([1.0, 0.0, 0.0, -2.5]))
    assert not E.same(a, torch.tensor([E.NAN, 0.0, E.NAN, -2.5]))
    assert not E.same(a, a.to(torch.bfloat16))
    b = a.to(torch.bfloat16)
    assert E.same(b, b.clone()) and not E.same(b, torch.tensor([1.0, 0.0, E.NAN, -2.515625]).to(torch.bfloat16))


def test_fp32_route_equals_fp64_rounded_once_per_operation():
    total = excluded = fused_differs = 0
    for x, r, v, caxis in _affine_inputs():
        for combo in E.COMBOS:
            s, b, rr, rs, rb = E.pick(combo, v, r)
            for relu in (False, True):
                want = E.affine(x, s, b, rr, rs, rb, relu, caxis)
                ref, exact = E.affine64(x, s, b, rr, rs, rb, relu, caxis)
                assert torch.equal(torch.isnan(want), torch.isnan(ref)), combo
                ok = (want == ref) | torch.isnan(want)
                assert bool(ok[exact].all()), (combo, relu, tuple(x.shape), x.dtype)
                total += want.numel()
                excluded += int((~exact).sum())
            if s is not None and b is not None and rr is None and x.dtype == torch.float32:
                f = lambda t: E._per_channel(t, x, caxis).double()           # noqa: E731
                fused = (x.double() * f(s) + f(b)).float()
                fused_differs += int((fused != E.affine(x, s, b, caxis=caxis)).sum())
    print('  fp64 cross-check: %d of %d elements excluded (share %.2e)' % (excluded, total, excluded / total))
    assert excluded <= CAP * total
    assert fused_differs > 1000                     # a contracted multiply-add would not pass for the yardstick


def test_nan_masks_of_the_planted_epilogue_inputs():
    for layout, hw, caxis in _NONFINITE:
        for dtype in E.DTYPES.values():
            x, r, v, ch = E.nonfinite_case(layout, dtype, hw)
            n = x.numel()
            spots = [(i * n) // 11 for i in range(11)]
            assert len(set(spots)) == 11 and float(v['s'][ch]) == 0.0
            assert bool(torch.isinf(x.view(-1)[spots[4]]))
            for combo in E.COMBOS:
                s, b, rr, rs, rb = E.pick(combo, v, r)
                off = E.affine(x, s, b, rr, rs, rb, False, caxis).view(-1)
                on = E.affine(x, s, b, rr, rs, rb, True, caxis).view(-1)
                assert on.dtype == dtype
                m = torch.isnan(off)
                assert torch.equal(m, torch.isnan(on)), combo                  # the ReLU keeps every NaN
                assert bool((on[~m] >= 0).all()) and bool(torch.equal(on[~m], off[~m].clamp(min=0)))
                want = {spots[0]}                                               # NaN in x
                if s is not None:
                    want.add(spots[4])                                          # 0 * Inf
                if rr is not None:
                    want |= {spots[1], spots[7]}                                # NaN in the residual
                    if rs is None and s is None:
                        want.add(spots[5])                                      # +Inf + -Inf
                got = set(torch.nonzero(m).flatten().tolist())
                assert want <= got, (combo, sorted(want - got))
                # everything else that is NaN is an Inf - Inf of the two branches at a planted position
                assert got <= set(spots), (combo, sorted(got - set(spots)))
                if rr is None:
                    assert got == want, combo


@pytest.mark.parametrize('name,B,H,W,C', E.pool_cases())
def test_pool_yardstick(name, B, H, W, C):
    dtype = E.DTYPES[name]
    x, s, t = E.pool_data(B, H, W, C, dtype)
    want = E.pool(x, s, t)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert want.shape == (B, Ho, Wo, C) and want.dtype == dtype and not bool(torch.isnan(want).any())
    ref, exact = E.pool64(x, s, t)
    assert bool((want == ref)[exact].all()) and int((~exact).sum()) <= CAP * exact.numel()
    assert bool((want[..., 1] == 0).all())                                     # every window negative
    assert bool((want >= 0).all())
    # a brute-force statement of the definition: the maximum over the in-range taps, at least 0
    a = E.affine(x.float(), s, t)
    for yo in range(Ho):
        for xo in range(Wo):
            win = a[:, max(2 * yo - 1, 0):2 * yo + 2, max(2 * xo - 1, 0):2 * xo + 2]
            assert torch.equal(win.amax(dim=(1, 2)).clamp(min=0).to(dtype), want[:, yo, xo])
    if dtype == torch.bfloat16:
        # channel 0: every affine value is a tie between two bf16 values
        bits = a[..., 0].contiguous().view(torch.int32) & 0xffff
        assert bool((bits == 0x8000).all())
        assert torch.equal(E.pool_eager_order(x, s, t), want)
    if B * H * W > 9:
        # ties between taps: the half-integer channel has nine values, so taps repeat
        a2 = a[..., 2]
        assert a2.unique().numel() < a2.numel()


@pytest.mark.parametrize('name', list(E.DTYPES))
@pytest.mark.parametrize('B,H,W', E.POOL_NAN_CASES)
def test_pool_nan_mask_is_the_windows_that_hold_one(name, B, H, W):
    dtype = E.DTYPES[name]
    C = E.POOL_WIDE[3] if (B, H, W) == E.POOL_WIDE[:3] else E.vec_width(dtype)
    x, s, t = E.pool_data(B, H, W, C, dtype)
    clean = E.pool(x, s, t)
    for k, (b, y, xx) in enumerate(E.pool_nan_spots(B, H, W)):
        xn = x.clone()
        xn[b, y, xx, k % C] = E.NAN
        got = E.pool(xn, s, t)
        m = torch.isnan(got)
        assert torch.equal(m, E.pool_nan_mask(xn))
        # windows of rows 2 yo - 1 .. 2 yo + 1: an odd coordinate is shared by two windows
        rows = [yo for yo in range((H - 1) // 2 + 1) if abs(2 * yo - y) <= 1]
        cols = [xo for xo in range((W - 1) // 2 + 1) if abs(2 * xo - xx) <= 1]
        assert int(m.sum()) == len(rows) * len(cols) and bool(m[b, rows][:, cols, k % C].all())
        if (y, xx) == (1, 1):
            assert int(m.sum()) == 4
        assert torch.equal(got[~m], clean[~m])
        if dtype == torch.bfloat16:
            assert E.same(E.pool_eager_order(xn, s, t), got)


@pytest.mark.parametrize('name,shape', E.upadd_cases())
def test_upsample_add_yardstick(name, shape):
    dtype = E.DTYPES[name]
    B, C, Hc, Wc = shape
    fine, coarse = E.upadd_data(B, C, Hc, Wc, dtype)
    want = E.upsample_add(fine, coarse)
    up = torch.nn.functional.interpolate(coarse.float().permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
    assert torch.equal(want, (fine.float() + up.permute(0, 2, 3, 1)).to(dtype))
    code = E.upadd_code(B, C, Hc, Wc)
    assert torch.equal(code.to(torch.bfloat16).float(), code) and code.unique().numel() == code.numel()
    out = E.upsample_add(torch.zeros_like(fine), code.to(dtype)).float()
    for b in range(B):
        for y in range(2 * Hc):
            for xx in range(2 * Wc):
                assert torch.equal(out[b, y, xx], code[b, y // 2, xx // 2])


def test_transpose_yardstick():
    for dtype in E.DTYPES.values():
        for C in E.TRANSPOSE_SIZES[:3]:
            src = E.transpose_data(C, 65, dtype)
            want = E.transpose(src)
            assert want.shape == (E.TRANSPOSE_N, C, 65) and want.is_contiguous()
            assert np.array_equal(want.float().numpy(), np.transpose(src.float().numpy(), (0, 2, 1)))
    assert E.transpose_data(130, 130, torch.float32).unique().numel() == 3 * 130 * 130


def test_the_cases_cover_the_geometry_they_claim():
    for name, dtype in E.DTYPES.items():
        n = E.vec_width(dtype)
        cases = [(p, C) for (d, p, C) in E.nhwc_cases() if d == name]
        packs = {p * C // n for (p, C) in cases}
        assert {1, 2, 1023, 1024, 1025}.issubset(packs) and any(2048 < k < 3072 for k in packs)
        step = 256 * n
        mods = {C: step % C for (_, C) in cases}
        assert any(C > step and m == step for C, m in mods.items())             # C above one thread step
        assert any(m == 0 for m in mods.values())                               # C divides the step
        assert any(0 < m < C < step for C, m in mods.items())                   # the wrap, C below the step
        assert mods[1032] == (1024 if n == 4 else 1016)                         # the wrap, C above half a step
        assert all(C % n == 0 for (_, C) in cases)
    kernels = {E.nhwc_kernel(c) for c in E.COMBOS}
    assert kernels == {'generic'} | {'fast<%d,%d,%d>' % k for k in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 0), (0, 1, 0), (0, 1, 1))}
    assert [E.nhwc_kernel(c) for c in E.COMBOS[:5]] == ['fast<1,0,0>', 'fast<1,1,0>', 'fast<1,1,1>', 'fast<0,0,0>', 'generic']


def test_nhwc_entry_rejects_misaligned_vectors_before_any_launch():
    """x, residual and the four per-channel vectors are read 16 bytes at a time; the checks return
    before anything touches a device, so host memory stands in for the pointers"""
    from iouaware import _lib
    L = _lib.lib()
    buf = np.zeros(4096, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    x, r = base, base + 4096
    vec = [base + 8192 + 256 * i for i in range(4)]
    p = ctypes.c_void_p

    def call(x=x, r=r, v=vec, dtype=_lib.IA_F32, C=8, nhw=4):
        return L.ia_channel_affine_act_nhwc(p(x), dtype, p(v[0]), p(v[1]), p(r), p(v[2]), p(v[3]), 1, nhw, C, None)

    for i in range(4):
        for off in (4, 8, 12):
            v = list(vec)
            v[i] += off
            assert call(v=v) == IA_E_ARG, (i, off)
            assert call(v=v, dtype=_lib.IA_BF16) == IA_E_ARG, (i, off)
    assert call(x=x + 4) == IA_E_ARG and call(r=r + 8) == IA_E_ARG
    assert call(C=6) == IA_E_ARG and call(C=4, dtype=_lib.IA_BF16) == IA_E_ARG
    assert call(nhw=0) == IA_E_ARG and call(dtype=7) == IA_E_ARG and call(x=None) == IA_E_ARG

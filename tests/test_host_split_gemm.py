"""CPU: the numerics of the split GEMM (csrc/wino_split_gemm.hip, ia_batched_gemm_split3) before any GPU run.

  * the three-way split x = h + m + l (round-to-nearest bf16 casts: h = bf16(x), m = bf16(x - h),
    l = bf16(x - h - m)) is exact, for normals across 2^-60 .. 2^60, +-0 and values next to a bf16
    rounding tie -- through iouaware.winograd.split3_pack_u, the host side that splits U;
  * a numpy fp32 emulation of the kernel's scheme (six terms hh, hm, mh, hl, lh, mm; hh in one
    accumulator, the other five in a second, the two added once) at K = 256 passes gate A and gate B of
    tests/wino_ref.py against fp64, with numpy's fp32 matmul as the helper;
  * a two-piece split with three terms (hh, hm, mh) fails gate B: the gate sees that fault."""
import numpy as np
import pytest
import torch

import wino_ref as R


def _bf16(x):
    """round-to-nearest-even to bf16, kept as fp32 (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
    return r.view(np.float32)


def _split(x, pieces=3):
    out, r = [], x.astype(np.float32)
    for _ in range(pieces):
        p = _bf16(r)
        out.append(p)
        r = (r - p).astype(np.float32)
    return out


def _unpack(p, k, n):
    """split3_pack_u's layout back to (batch, 3, K, N)"""
    b = p.shape[0]
    npad = p.shape[2] * 32
    x = p.view(b, k // 16, npad // 32, 3, 2, 32, 8).permute(0, 3, 1, 4, 6, 2, 5).reshape(b, 3, k, npad)
    return x[..., :n]


def _values():
    rng = np.random.default_rng(0)
    e = rng.integers(-60, 61, size=4000)
    sig = rng.uniform(1.0, 2.0, size=4000)
    sign = rng.choice([-1.0, 1.0], size=4000)
    normals = (sign * sig * np.exp2(e.astype(np.float64))).astype(np.float32)
    # next to a bf16 tie: h + half an ulp of h (a tie, rounds to even), and one fp32 ulp on either side
    base = _bf16(normals[:1000])
    half = np.ldexp(np.ones(1000), np.frexp(base.astype(np.float64))[1] - 9)
    tie = (base.astype(np.float64) + np.sign(base) * half).astype(np.float32)
    near = np.concatenate([tie, np.nextafter(tie, np.float32(np.inf)), np.nextafter(tie, np.float32(-np.inf))])
    zeros = np.array([0.0, -0.0], dtype=np.float32)
    return np.concatenate([normals, near, zeros]).astype(np.float32)


def test_three_way_split_is_exact():
    from iouaware import winograd as wg
    x = _values()
    k, n = 32, x.size // 32
    x = x[:k * n]
    u = torch.from_numpy(x.reshape(1, k, n).copy())
    packed = wg.split3_pack_u(u)
    assert packed.dtype == torch.bfloat16 and packed.shape == (1, k // 16, (n + 127) // 128 * 4, 3, 64, 8)
    pieces = _unpack(packed, k, n).double()
    assert pieces.shape == (1, 3, k, n)
    total = pieces[:, 0] + pieces[:, 1] + pieces[:, 2]        # exact in fp64: 3 x 8 bits within 2^-25 of h
    assert torch.equal(total, u.double())
    # bit for bit, signed zeros included: h carries the sign of x
    h = pieces[:, 0].float()
    assert torch.equal(torch.signbit(h[u == 0]), torch.signbit(u[u == 0]))
    # the pieces are the round-to-nearest casts (numpy's own RNE here)
    h_np, m_np, l_np = _split(x.reshape(1, k, n))
    for got, want in zip(pieces.unbind(1), (h_np, m_np, l_np)):
        assert np.array_equal(got.float().numpy(), want)
    # and the packed planes beyond N are zero
    npad = (n + 127) // 128 * 128
    full = wg.split3_pack_u(u).view(1, k // 16, npad // 32, 3, 2, 32, 8).permute(0, 3, 1, 4, 6, 2, 5) \
        .reshape(1, 3, k, npad)
    assert bool((full[..., n:] == 0).all())


def _scheme(v, u, pieces, terms):
    """the kernel's sums in numpy fp32: the hh chain and the correction chain, added once"""
    vs, us = _split(v, pieces), _split(u, pieces)
    hi = np.matmul(vs[0], us[0])
    lo = np.zeros_like(hi)
    for (i, j) in terms:
        lo = (lo + np.matmul(vs[i], us[j])).astype(np.float32)
    return (hi + lo).astype(np.float32)


SIX = [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0)]         # mm, hl, lh, hm, mh (the kernel's order)
THREE = [(0, 1), (1, 0)]                               # two pieces: hm, mh


@pytest.fixture(scope='module')
def operands():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((4, 300, 256)).astype(np.float32)
    u = (rng.standard_normal((4, 256, 320)) * 0.05).astype(np.float32)
    ref = torch.from_numpy(np.matmul(v.astype(np.float64), u.astype(np.float64)))
    helper = torch.from_numpy(np.matmul(v, u))
    return v, u, ref, helper


def test_six_term_scheme_passes_both_gates(operands):
    v, u, ref, helper = operands
    got = torch.from_numpy(_scheme(v, u, 3, SIX))
    e, h, ratio = R.gates(got, helper, ref)
    print('six terms: error %.3e, fp32 helper %.3e, ratio %.2f' % (e, h, ratio))
    assert e <= R.GATE_A
    assert ratio <= R.GATE_B


def test_two_piece_three_term_variant_fails_gate_b(operands):
    v, u, ref, helper = operands
    got = torch.from_numpy(_scheme(v, u, 2, THREE))
    e, h, ratio = R.gates(got, helper, ref)
    print('two pieces, three terms: error %.3e, fp32 helper %.3e, ratio %.2f' % (e, h, ratio))
    assert ratio > R.GATE_B_MAX

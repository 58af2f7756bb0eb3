"""CPU: the host side of the bf16 grouped 3x3 convolution (csrc/gconv_bf16.hip): the weight
arrangement ia_grouped_conv3x3_pack_bf16 against a numpy restatement of the index formula that
include/iouaware.h documents, and every argument check of the three entries -- they return
IA_E_ARG before anything touches the device, so no GPU is needed."""
import ctypes

import numpy as np
import pytest
import torch

IA_E_ARG = -1
INT32_MAX = 2 ** 31 - 1


def _lib():
    from iouaware import _lib
    return _lib.lib()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else ctypes.c_void_p(0)


def _bf16_bits(a):
    """RNE bf16 bits of an fp32 numpy array, by torch's own conversion"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16) \
        .numpy().view(np.uint16)


def _pack(w, scale, C, groups):
    n = _lib().ia_grouped_conv3x3_packed_bytes_bf16(C, groups)
    assert n == C // 32 * 9 * 2 * 64 * 8 * 2
    out = np.full(n // 2, 0xdead, np.uint16)
    assert _lib().ia_grouped_conv3x3_pack_bf16(_p(w), _p(scale), C, groups, _p(out)) == 0
    return out


@pytest.mark.parametrize('with_scale', [False, True])
@pytest.mark.parametrize('C', [32, 64])
@pytest.mark.parametrize('cg', [4, 8, 16, 32])
def test_pack_bf16_follows_the_documented_index_formula(cg, C, with_scale):
    groups = C // cg
    rng = np.random.RandomState(100 * cg + C + int(with_scale))
    w = rng.standard_normal((C, cg, 3, 3)).astype(np.float32)
    scale = (rng.standard_normal(C).astype(np.float32) + 2.0) if with_scale else None
    got = _pack(w, scale, C, groups).reshape(C // 32, 9, 2, 64, 8)
    # element [sg][t][co][lane][j]: o = 32 sg + 16 co + (lane & 15), in = 32 sg + 8 (lane >> 4) + j
    sg, t, co, lane, j = np.meshgrid(np.arange(C // 32), np.arange(9), np.arange(2), np.arange(64),
                                     np.arange(8), indexing='ij')
    o = 32 * sg + 16 * co + (lane & 15)
    i = 32 * sg + 8 * (lane >> 4) + j
    same = (o // cg) == (i // cg)
    # the product in fp32 (numpy float32 * float32), then ONE rounding to bf16
    folded = w.reshape(C, cg, 9) * (scale[:, None, None] if with_scale else np.float32(1.0))
    assert folded.dtype == np.float32
    want = np.where(same, _bf16_bits(folded)[o, i % cg, t], np.uint16(0))
    assert same.sum() == C * cg * 9                      # every weight appears exactly once
    assert np.all(got[~same] == 0)                       # nothing couples two groups
    assert np.array_equal(got, want)
    # and the non-zero part holds every weight: no value lost to the arrangement
    assert np.array_equal(np.sort(got[same]), np.sort(_bf16_bits(folded).ravel()))


def test_pack_bf16_rounds_ties_to_even_after_the_fp32_product():
    C, cg = 32, 32
    w = np.zeros((C, cg, 3, 3), np.float32)
    # 1 + 2^-8 lies halfway between the bf16 neighbours 1 and 1 + 2^-7: ties go to the even one (1);
    # 1 + 3 * 2^-8 halfway between 1 + 2^-7 and 1 + 2^-6: even is 1 + 2^-6
    w[0, 0, 0, 0] = 1.0 + 2.0 ** -8
    w[1, 0, 0, 0] = 1.0 + 3.0 * 2.0 ** -8
    w[2, 0, 0, 0] = 0.5 + 2.0 ** -9                      # x 2 (scale) = the first tie again
    scale = np.ones(C, np.float32)
    scale[2] = 2.0
    got = _pack(w, scale, C, 1).reshape(1, 9, 2, 64, 8)
    # tap 0, block 0, input channel 0 = lane >> 4 == 0, j == 0; output channel = lane & 15
    assert got[0, 0, 0, 0, 0] == 0x3f80 and got[0, 0, 0, 1, 0] == 0x3f82 and got[0, 0, 0, 2, 0] == 0x3f80


def test_packed_bytes_bf16_is_zero_for_what_the_kernel_does_not_cover():
    lib = _lib()
    for C, g in [(48, 12), (16, 4), (64, 32), (64, 1), (96, 7), (0, 1), (64, 0), (-32, 1)]:
        assert lib.ia_grouped_conv3x3_packed_bytes_bf16(C, g) == 0, (C, g)
    assert lib.ia_grouped_conv3x3_packed_bytes_bf16(2048, 64) == 2048 * 9 * 32 * 2


def test_pack_bf16_argument_checks():
    lib = _lib()
    w = np.zeros((64, 32, 3, 3), np.float32)
    out = np.zeros(64 * 9 * 32, np.uint16)
    ok = lambda *a: lib.ia_grouped_conv3x3_pack_bf16(*a)
    assert ok(_p(w), None, 64, 2, _p(out)) == 0
    assert ok(None, None, 64, 2, _p(out)) == IA_E_ARG               # NULL weight
    assert ok(_p(w), None, 64, 2, None) == IA_E_ARG                 # NULL wpack
    assert ok(_p(w), None, 64, 32, _p(out)) == IA_E_ARG             # Cg = 2
    assert ok(_p(w), None, 64, 1, _p(out)) == IA_E_ARG              # Cg = 64
    assert ok(_p(w), None, 48, 4, _p(out)) == IA_E_ARG              # Cg = 12
    assert ok(_p(w), None, 48, 12, _p(out)) == IA_E_ARG             # Cg = 4, channels % 32
    assert ok(_p(w), None, 16, 4, _p(out)) == IA_E_ARG              # Cg = 4, channels % 32
    assert ok(_p(w), None, 64, 3, _p(out)) == IA_E_ARG              # channels % groups
    assert ok(_p(w), None, 64, 0, _p(out)) == IA_E_ARG
    assert ok(_p(w), None, 0, 1, _p(out)) == IA_E_ARG


def test_conv_bf16_argument_checks_return_before_the_device():
    lib = _lib()
    # host memory stands in for the tensors: every call below must return before it is looked at
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    x, y, wp = ctypes.c_void_p(base), ctypes.c_void_p(base + 1024), ctypes.c_void_p(base + 2048)
    bias = ctypes.c_void_p(base + 3072)

    def call(x=x, wp=wp, bias=bias, y=y, batch=1, H=4, W=4, C=64, groups=8, stride=1, relu=1):
        return lib.ia_grouped_conv3x3_bf16_nhwc(x, wp, bias, y, batch, H, W, C, groups, stride, relu, None)
    assert call(x=None) == IA_E_ARG
    assert call(wp=None) == IA_E_ARG
    assert call(y=None) == IA_E_ARG
    for C, g in [(64, 32), (64, 1), (48, 4), (48, 12), (16, 4), (64, 3), (64, 0), (0, 1)]:
        assert call(C=C, groups=g) == IA_E_ARG, (C, g)               # Cg, channels % 32, channels % groups
    for s in (0, 3, 4, -1):
        assert call(stride=s) == IA_E_ARG, s
    for off in (2, 4, 8):
        assert call(x=ctypes.c_void_p(base + off)) == IA_E_ARG, off  # x / y not 16-byte aligned
        assert call(y=ctypes.c_void_p(base + 1024 + off)) == IA_E_ARG, off
    for batch, H in [(0, 4), (-1, 4), (1, 0)]:
        assert call(batch=batch, H=H) == IA_E_ARG
    assert call(W=0) == IA_E_ARG
    # batch * Ho above INT32_MAX: stride 1 (Ho = H) and stride 2 (Ho = ceil(H / 2))
    assert call(batch=2, H=2 ** 30) == IA_E_ARG
    assert call(batch=INT32_MAX, H=2) == IA_E_ARG
    assert call(batch=4, H=2 ** 30, stride=2) == IA_E_ARG
    assert call(batch=INT32_MAX, H=3, stride=2) == IA_E_ARG


def test_ops_grouped_conv3x3_bf16_refuses_other_dtypes_and_layouts():
    from iouaware import ops, _lib
    wp = ops.pack_grouped_weight_bf16(torch.zeros(64, 8, 3, 3))
    assert wp.dtype == torch.bfloat16 and wp.numel() == 64 * 9 * 32
    with pytest.raises(ValueError):
        ops.grouped_conv3x3_bf16(torch.zeros(1, 64, 4, 4).contiguous(memory_format=torch.channels_last),
                                 wp, None, 8)                                       # fp32
    with pytest.raises(ValueError):
        ops.grouped_conv3x3_bf16(torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16), wp, None, 8)   # NCHW
    with pytest.raises(ValueError):
        ops.pack_grouped_weight_bf16(torch.zeros(48, 4, 3, 3))                       # channels % 32
    with pytest.raises(ValueError):
        ops.pack_grouped_weight_bf16(torch.zeros(64, 2, 3, 3))                       # Cg = 2
    # a CPU tensor of the right dtype and layout is refused as everywhere else: no CPU fallback
    with pytest.raises(_lib.IouAwareLibraryError):
        ops.grouped_conv3x3_bf16(torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16)
                                 .contiguous(memory_format=torch.channels_last), wp, None, 8)

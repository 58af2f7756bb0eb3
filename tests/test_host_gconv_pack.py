"""CPU: ia_grouped_conv3x3_pack (csrc/gconv.hip) walks the element function the device pack calls
(gconv_pack_elem, csrc/ia_gconv.hpp).  Its bytes equal a numpy transcription of the documented
operand layout (tests/gconv_ref.py: pack_fp32) -- 4, 8 and 32 channels per group, one and two
16-channel blocks per supergroup, with and without the folded scale; a single fp32 product per
element, so the comparison is bitwise."""
import ctypes

import numpy as np
import pytest

import gconv_ref as G

SHAPES = [(16, 4), (32, 4), (64, 2), (128, 32)]       # (C, groups): Cg = 4, 8, 32 (NB = 2), 4


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
@pytest.mark.parametrize('C,groups', SHAPES)
def test_host_pack_bytes(C, groups, scaled):
    from iouaware import _lib
    L = _lib.lib()
    cg = C // groups
    rs = np.random.RandomState(1000 * C + groups)
    w = rs.standard_normal((C, cg, 3, 3)).astype(np.float32)
    scale = rs.uniform(0.5, 2.0, C).astype(np.float32) if scaled else None
    ref = G.pack_fp32(w, scale)
    nb = 2 if cg == 32 else 1
    assert ref.shape == (C // (16 * nb), 9, nb, 4, nb, 64)
    out = np.full(ref.size, np.float32(-7.0), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None   # noqa: E731
    assert L.ia_grouped_conv3x3_pack(p(w), p(scale), C, groups, p(out)) == 0
    assert out.tobytes() == ref.tobytes()
    # every weight of a group lands somewhere: the pack is not all zeros outside a corner
    assert np.count_nonzero(out) == C * cg * 9

"""CPU: the C ABI of the bf16 FCOS path (declared, bound, exported), its size query and the
argument contracts that hold without a device."""
import ctypes
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ('ia_groupnorm_workspace_bytes_dt', 'ia_groupnorm_stats_dt', 'ia_groupnorm_apply_dt',
               'ia_scale_exp_levels_dt', 'ia_point_decode_stage_dt', 'ia_point_get_bboxes_dt',
               'ia_point_ctr_decode_stage_dt', 'ia_point_ctr_get_bboxes_dt')


def test_header_declares_and_library_exports_the_dt_entries():
    from iouaware import _lib
    text = open(os.path.join(HERE, '..', 'include', 'iouaware.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(ia_[a-z0-9_]+)\s*\(', text))
    h = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(h, name), 'missing export %s' % name


def test_bf16_groupnorm_size_query_on_the_host():
    """what the bf16 kernels take: channels / groups % 8 == 0, channels a power of two <= 1024;
    the fp32 answer is the existing entry's"""
    from iouaware import _lib, fcos_ops
    xs = [torch.empty((2, 512, h, w)) for (h, w) in ((16, 24), (8, 12), (1, 2))]
    g = fcos_ops._wino_geom(xs)
    L = _lib.lib()
    q = lambda ch, groups, dt: L.ia_groupnorm_workspace_bytes_dt(ctypes.byref(g), ch, groups, dt)  # noqa: E731
    chunks = 2 + 1 + 1
    assert q(512, 64, _lib.IA_BF16) == q(512, 64, _lib.IA_F32) == 2 * chunks * 64 * 16
    assert q(512, 64, _lib.IA_F32) == L.ia_groupnorm_workspace_bytes(ctypes.byref(g), 512, 64)
    assert q(256, 64, _lib.IA_BF16) == 0 and q(256, 64, _lib.IA_F32) > 0      # 4 channels per group
    assert q(384, 32, _lib.IA_BF16) == 0                                       # not a power of two
    assert q(2048, 64, _lib.IA_BF16) == 0                                      # above 1024
    assert q(4, 1, _lib.IA_BF16) == 0 and q(4, 1, _lib.IA_F32) > 0             # below one 16-byte column
    assert q(512, 64, _lib.IA_F16) == 0                                        # no such instance


def test_training_node_keeps_its_fp32_contract():
    from iouaware import fcos_ops
    x = torch.zeros((1, 512, 4, 4), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError):
        fcos_ops.groupnorm_relu([x], torch.ones(512), torch.zeros(512), 64)


def test_point_ptrs_refuse_cpu_tensors():
    from iouaware import _lib, fcos_ops
    geom = fcos_ops.PointGeometry([(2, 3)], (8,), 80, nms_pre=10)
    for dt in (torch.float32, torch.bfloat16):
        maps = [[torch.zeros((1, ch, 2, 3), dtype=dt)] for ch in (80, 4, 1)]
        with pytest.raises(_lib.IouAwareLibraryError):
            fcos_ops._point_ptrs(geom, *maps)

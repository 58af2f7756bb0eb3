"""Seeded synthetic inputs of the plain FCOS fixtures (tests/golden/fcos_plain_*.npz,
tests/golden/make_golden_fcos_plain.py), on top of synth_fcos: the head outputs without the IoU
map, and the get_bboxes cases."""
import synth_fcos

# (tag, pad_h, pad_w, nms_pre, rescale, class-logit shift) of fcos_plain_get_bboxes.npz: the
# per-level top-k active on the two large levels, and not at all (pre1000_r, on a smaller map);
# the shifted case is sparse (few raw scores above score_thr): every survivor is kept, those whose
# centerness product falls below score_thr included
GET_BBOXES_CASES = (('pre60_r', 160, 224, 60, True, 0.0), ('pre60', 160, 224, 60, False, 0.0),
                    ('pre1000_r', 96, 128, 1000, True, 0.0), ('sparse_r', 160, 224, 100, True, -6.0))


def head_outputs(seed, batch, sizes, cls_shift=0.0):
    """(cls, bbox, centerness) per level, NCHW fp32: synth_fcos.head_outputs without the IoU map,
    the class logits shifted by cls_shift"""
    cls, reg, ctr, _ = synth_fcos.head_outputs(seed, batch, sizes)
    if cls_shift:
        cls = [(c + cls_shift).astype(c.dtype) for c in cls]
    return cls, reg, ctr


def get_bboxes_metas(pad_h, pad_w):
    """the two images' metas of the get_bboxes cases"""
    return [dict(img_shape=(pad_h - 10, pad_w - 11, 3), scale_factor=0.75, pad_shape=(pad_h, pad_w, 3)),
            dict(img_shape=(pad_h, pad_w - 24, 3), scale_factor=1.25, pad_shape=(pad_h, pad_w, 3))]

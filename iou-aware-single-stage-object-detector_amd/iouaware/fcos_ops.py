"""torch front-end of the FCOS kernels (csrc/groupnorm.hip, csrc/pointdecode.hip): the point
heads' post-conv paths (ia_point_get_bboxes: IoU-aware; ia_point_ctr_get_bboxes: plain FCOS, the
centerness map in the third slot) and the towers' GroupNorm + ReLU.
Device tensors only, launched on the current torch stream, like ops.py."""
import ctypes as C

import torch

from . import _lib
from ._lib import LevelPtrs, PointHeadGeom
from . import winograd
from .ops import (_LayoutTwin, _det_outputs, _meta_tensors, _ptr, _require_gpu, _state_workspace,
                  _stream, _ws_views, stream_id, to_nchw)


class PointGeometry(_LayoutTwin):
    """Static geometry of a point head for one set of feature-map sizes (ia_point_head_geom)."""

    def __init__(self, featmap_sizes, strides, num_classes, nms_pre=-1, score_alpha=0.3):
        L = len(featmap_sizes)
        if L != len(strides) or L > _lib.IA_MAX_LEVELS:
            raise ValueError('unsupported point-head geometry (%d levels)' % L)
        g = PointHeadGeom()
        g.num_levels, g.num_classes, g.nms_pre = L, int(num_classes), int(nms_pre)
        for l, ((h, w), s) in enumerate(zip(featmap_sizes, strides)):
            g.H[l], g.W[l], g.stride[l] = int(h), int(w), int(s)
        g.layout = _lib.IA_LAYOUT_NCHW
        g.score_alpha = float(score_alpha)
        self.struct = g
        self.L, self.C = L, int(num_classes)
        self.featmap_sizes = [tuple(int(v) for v in s) for s in featmap_sizes]
        self.strides = [int(s) for s in strides]
        self.level_points = [h * w for (h, w) in self.featmap_sizes]
        self.level_cands = [min(nms_pre, n) if nms_pre > 0 else n for n in self.level_points]
        self.N, self.R = sum(self.level_points), sum(self.level_cands)
        self.Rs = (self.R + 63) // 64 * 64
        self.layout = _lib.IA_LAYOUT_NCHW
        self.key = ('point', tuple(self.featmap_sizes), self.C, int(nms_pre), float(score_alpha))

    def ref(self):
        return C.byref(self.struct)


def _point_ptrs(geom, cls, reg, iou, third='iou_pred'):
    if not (len(cls) == len(reg) == len(iou) == geom.L):
        raise AssertionError('expected %d levels' % geom.L)
    B = cls[0].shape[0]
    tensors = list(cls) + list(reg) + list(iou)
    for l in range(geom.L):
        h, w = geom.featmap_sizes[l]
        for name, t, ch in (('cls_score', cls[l], geom.C), ('bbox_pred', reg[l], 4),
                            (third, iou[l], 1)):
            _require_gpu(t, name)
            if tuple(t.shape) != (B, ch, h, w):
                raise AssertionError('%s level %d has shape %s, expected %s'
                                     % (name, l, tuple(t.shape), (B, ch, h, w)))
            if t.dtype != torch.float32:
                raise TypeError('the point-head decode takes fp32 head outputs')
    nhwc = (geom.C * 4) % 16 == 0 and not all(t.is_contiguous() for t in tensors) and all(
        t.is_contiguous(memory_format=torch.channels_last) for t in tensors)
    geom = geom.with_layout(_lib.IA_LAYOUT_NHWC if nhwc else _lib.IA_LAYOUT_NCHW)
    p = LevelPtrs()
    for l in range(geom.L):
        if not nhwc:
            cls[l], reg[l], iou[l] = to_nchw(cls[l]), to_nchw(reg[l]), to_nchw(iou[l])
        p.cls[l], p.reg[l], p.iou[l] = cls[l].data_ptr(), reg[l].data_ptr(), iou[l].data_ptr()
    return p, B, geom


def _workspace(geom, B, dev):
    nbytes = _lib.lib().ia_point_workspace_bytes(geom.ref(), B)
    if nbytes == 0:
        raise _lib.IouAwareLibraryError('unsupported geometry / batch for ia_point_get_bboxes '
                                        '(more than %d candidates per image?)' % _lib.IA_MAX_CANDIDATES)
    return nbytes, _state_workspace(dev, nbytes, (geom.key, geom.layout, B))


def _views(geom, B, ws):
    return _ws_views('ia_point_workspace_layout', geom, B, ws)


def point_decode_stage(geom, cls, reg, iou, img_shapes, scale_factors, rescale):
    """decode stage only (row max, top-k, gather / distance2bbox) -> dict of workspace views
    rowmax (B,N), cand_idx (B,R), boxes (B,R,4), scores_t (B,C,Rs), best_score (B,R)"""
    cls, reg, iou = list(cls), list(reg), list(iou)
    p, B, geom = _point_ptrs(geom, cls, reg, iou)
    dev = cls[0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    _lib.check(_lib.lib().ia_point_decode_stage(geom.ref(), C.byref(p), B, _ptr(hw), _ptr(sf),
                                                int(bool(rescale)), _ptr(ws), nbytes, _stream()),
               'ia_point_decode_stage')
    return _views(geom, B, ws)


def point_ctr_decode_stage(geom, cls, reg, ctr, img_shapes, scale_factors, rescale, score_thr):
    """plain FCOS decode stage -> the views of point_decode_stage; scores_t holds
    sigmoid(cls) * sigmoid(ctr) where sigmoid(cls) > score_thr and a negative sentinel elsewhere"""
    cls, reg, ctr = list(cls), list(reg), list(ctr)
    p, B, geom = _point_ptrs(geom, cls, reg, ctr, 'centerness')
    dev = cls[0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    _lib.check(_lib.lib().ia_point_ctr_decode_stage(geom.ref(), C.byref(p), B, _ptr(hw), _ptr(sf),
                                                    int(bool(rescale)), float(score_thr), _ptr(ws),
                                                    nbytes, _stream()),
               'ia_point_ctr_decode_stage')
    return _views(geom, B, ws)


def _get_bboxes(entry, third, geom, cls, reg, iou, img_shapes, scale_factors, rescale, score_thr,
                iou_thr, max_per_img, lazy, debug):
    if max_per_img > _lib.IA_MAX_PER_IMG:
        raise _lib.IouAwareLibraryError('max_per_img above %d' % _lib.IA_MAX_PER_IMG)
    cls, reg, iou = list(cls), list(reg), list(iou)
    p, B, geom = _point_ptrs(geom, cls, reg, iou, third)
    dev = cls[0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    dets, labels, rows, num = _det_outputs(B, max_per_img, dev)
    _lib.check(getattr(_lib.lib(), entry)(
        geom.ref(), C.byref(p), B, _ptr(hw), _ptr(sf), int(bool(rescale)), float(score_thr),
        float(iou_thr), int(max_per_img), 0 if lazy else -1, _ptr(ws), nbytes, _ptr(dets),
        _ptr(labels), _ptr(rows), _ptr(num), _stream()), entry)
    if not debug:
        return dets, labels, rows, num
    return dets, labels, rows, num, _views(geom, B, ws)


def point_get_bboxes(geom, cls, reg, iou, img_shapes, scale_factors, rescale, score_thr, iou_thr,
                     max_per_img, lazy=True, debug=False):
    """Whole post-conv path of the point head for a batch -> device tensors dets (B,max,5),
    labels (B,max) int32, rows (B,max) int32 (candidate rows), num (B) int32 (+ the decode-stage
    views with debug=True)."""
    return _get_bboxes('ia_point_get_bboxes', 'iou_pred', geom, cls, reg, iou, img_shapes,
                       scale_factors, rescale, score_thr, iou_thr, max_per_img, lazy, debug)


def point_ctr_get_bboxes(geom, cls, reg, ctr, img_shapes, scale_factors, rescale, score_thr,
                         iou_thr, max_per_img, lazy=True, debug=False):
    """point_get_bboxes for plain FCOS (ia_point_ctr_get_bboxes): the raw score sigmoid(cls) is
    thresholded, NMS and the final sort run on sigmoid(cls) * sigmoid(ctr); geom.score_alpha is
    not used."""
    return _get_bboxes('ia_point_ctr_get_bboxes', 'centerness', geom, cls, reg, ctr, img_shapes,
                       scale_factors, rescale, score_thr, iou_thr, max_per_img, lazy, debug)


def _wino_geom(xs):
    return winograd._wino_geom([x.shape[2:] for x in xs], xs[0].shape[0])


_gn_ws = {}


def groupnorm_relu_(xs, gamma, beta, groups, eps=1e-5, relu=True):
    """In place over the levels xs[l] (B, ch, H_l, W_l) fp32 channels-last: GroupNorm (statistics
    per level and image) + ReLU, two launches for all of them.  gamma / beta (ch,) fp32."""
    if not xs or len(xs) > _lib.IA_MAX_LEVELS:
        raise ValueError('1..%d levels' % _lib.IA_MAX_LEVELS)
    ch = int(xs[0].shape[1])
    for x in xs:
        _require_gpu(x, 'x')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != ch or x.shape[0] != xs[0].shape[0] \
                or not x.is_contiguous(memory_format=torch.channels_last):
            raise ValueError('groupnorm_relu_ takes fp32 channels-last (B, %d, H, W) levels' % ch)
    for t in (gamma, beta):
        if t.dtype != torch.float32 or t.numel() != ch or not t.is_contiguous() or t.device != xs[0].device:
            raise ValueError('gamma / beta: (%d,) fp32 on the device' % ch)
    g = _wino_geom(xs)
    L = _lib.lib()
    nbytes = L.ia_groupnorm_workspace_bytes(C.byref(g), ch, int(groups))
    if nbytes == 0:
        raise _lib.IouAwareLibraryError('unsupported GroupNorm geometry (channels %d, groups %d)'
                                        % (ch, groups))
    key = (xs[0].device.index, stream_id())
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _gn_ws[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=xs[0].device)
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    _lib.check(L.ia_groupnorm_stats(C.byref(g), ptrs, ch, int(groups), _ptr(ws), nbytes, _stream()),
               'ia_groupnorm_stats')
    _lib.check(L.ia_groupnorm_apply(C.byref(g), ptrs, ch, int(groups), _ptr(gamma), _ptr(beta),
                                    float(eps), int(bool(relu)), _ptr(ws), nbytes, _stream()),
               'ia_groupnorm_apply')
    return xs

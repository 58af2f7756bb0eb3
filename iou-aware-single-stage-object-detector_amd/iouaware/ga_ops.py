"""torch front-end of the guided-anchor decode (csrc/guideddecode.hip): the post-conv path of
IoUawareGARetinaHead -- row max with the location filter, the shared top-k, the guided-anchor gather
/ decode and the shared batched NMS (ia_guided_get_bboxes), and its stage entries.
Device tensors only (fp32, NCHW; other layouts are converted), launched on the current torch stream,
like ops.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import GuidedGeom, GuidedLevelPtrs
from .ops import (HeadGeometry, _det_outputs, _meta_tensors, _ptr, _require_gpu, _state_workspace,
                  _stream, _ws_views, to_nchw)


class GuidedGeometry(object):
    """Static geometry of the guided-anchor head for one set of feature-map sizes (ia_guided_geom):
    an A = 1 HeadGeometry of the square anchors plus the anchoring means / stds and the location
    filter."""

    def __init__(self, featmap_sizes, strides, base_squares, num_classes, nms_pre=-1,
                 target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.),
                 anchoring_means=(0., 0., 0., 0.), anchoring_stds=(1., 1., 1., 1.),
                 loc_filter_thr=0.01, use_loc_filter=True):
        base = np.asarray(base_squares, dtype=np.float32).reshape(len(featmap_sizes), 1, 4)
        self.head = HeadGeometry(featmap_sizes, strides, base, num_classes, nms_pre, target_means, target_stds)
        g = GuidedGeom()
        g.head = self.head.struct
        for k in range(4):
            g.anchoring_means[k], g.anchoring_stds[k] = float(anchoring_means[k]), float(anchoring_stds[k])
        g.loc_filter_thr = float(loc_filter_thr)
        g.use_loc_filter = int(bool(use_loc_filter))
        self.struct = g
        h = self.head
        self.L, self.C, self.N, self.R, self.Rs = h.L, h.C, h.N, h.R, h.Rs
        self.featmap_sizes, self.strides = h.featmap_sizes, h.strides
        self.level_points, self.level_cands = h.level_anchors, h.level_cands
        self.key = ('guided', h.key, tuple(float(v) for v in anchoring_means),
                    tuple(float(v) for v in anchoring_stds), float(loc_filter_thr), bool(use_loc_filter))

    def ref(self):
        return C.byref(self.struct)


_MAPS = (('cls_score', 'cls', None), ('bbox_pred', 'reg', 4), ('iou_pred', 'iou', 1),
         ('shape_pred', 'shape', 2), ('loc_pred', 'loc', 1))


def _guided_ptrs(geom, cls, reg, iou, shape, loc):
    """-> (level pointers, batch, the NCHW-contiguous tensors kept alive)"""
    maps = [list(cls), list(reg), list(iou), list(shape), list(loc)]
    if any(len(m) != geom.L for m in maps):
        raise AssertionError('expected %d levels' % geom.L)
    B = maps[0][0].shape[0]
    p = GuidedLevelPtrs()
    for l in range(geom.L):
        h, w = geom.featmap_sizes[l]
        for (name, field, ch), m in zip(_MAPS, maps):
            t = m[l]
            ch = geom.C if ch is None else ch
            _require_gpu(t, name)
            if tuple(t.shape) != (B, ch, h, w):
                raise AssertionError('%s level %d has shape %s, expected %s'
                                     % (name, l, tuple(t.shape), (B, ch, h, w)))
            if t.dtype != torch.float32:
                raise TypeError('%s has dtype %s: the guided-anchor decode takes fp32 head outputs'
                                % (name, t.dtype))
            m[l] = to_nchw(t.detach())
            getattr(p, field)[l] = m[l].data_ptr()
    return p, B, maps


def _workspace(geom, B, dev):
    nbytes = _lib.lib().ia_guided_get_bboxes_workspace_bytes(geom.ref(), B)
    if nbytes == 0:
        raise _lib.IouAwareLibraryError('unsupported geometry / batch for ia_guided_get_bboxes '
                                        '(more than %d candidates per image?)' % _lib.IA_MAX_CANDIDATES)
    return nbytes, _state_workspace(dev, nbytes, (geom.key, B))


def guided_rowmax(geom, cls, reg, iou, shape, loc):
    """(B, N) fp32: per kept location max_c(sigmoid(cls_c) * sigmoid(iou)), +0.0 where filtered out"""
    p, B, keep = _guided_ptrs(geom, cls, reg, iou, shape, loc)
    out = torch.empty((B, geom.N), dtype=torch.float32, device=keep[0][0].device)
    _lib.check(_lib.lib().ia_guided_rowmax(geom.ref(), C.byref(p), B, _ptr(out), _stream()), 'ia_guided_rowmax')
    return out


def guided_gather_decode(geom, cls, reg, iou, shape, loc, cand_idx, img_shapes, scale_factors, rescale):
    """cand_idx (B, R) int32 -> boxes (B, R, 4), scores_t (B, C, Rs), best_score (B, R)"""
    p, B, keep = _guided_ptrs(geom, cls, reg, iou, shape, loc)
    dev = keep[0][0].device
    _require_gpu(cand_idx, 'cand_idx')
    if tuple(cand_idx.shape) != (B, geom.R) or cand_idx.dtype != torch.int32 or not cand_idx.is_contiguous():
        raise ValueError('cand_idx must be a contiguous (B, R) int32 tensor')
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    boxes = torch.empty((B, geom.R, 4), dtype=torch.float32, device=dev)
    scores_t = torch.zeros((B, geom.C, geom.Rs), dtype=torch.float32, device=dev)
    best = torch.empty((B, geom.R), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ia_guided_gather_decode(geom.ref(), C.byref(p), B, _ptr(cand_idx), _ptr(hw), _ptr(sf),
                                                  int(bool(rescale)), _ptr(boxes), _ptr(scores_t), _ptr(best),
                                                  _stream()), 'ia_guided_gather_decode')
    return boxes, scores_t, best


def guided_get_bboxes(geom, cls, reg, iou, shape, loc, img_shapes, scale_factors, rescale, score_thr,
                      iou_thr, max_per_img, debug=False):
    """Whole post-conv path of the guided-anchor head for a batch -> device tensors dets (B,max,5),
    labels (B,max) int32, rows (B,max) int32 (candidate rows), num (B) int32 (+ the decode-stage
    workspace views with debug=True).  No host synchronisation."""
    if max_per_img > _lib.IA_MAX_PER_IMG:
        raise _lib.IouAwareLibraryError('max_per_img above %d' % _lib.IA_MAX_PER_IMG)
    if not float(score_thr) >= 0.0:
        raise ValueError('score_thr=%r: the guided-anchor decode needs a threshold >= 0' % (score_thr,))
    p, B, keep = _guided_ptrs(geom, cls, reg, iou, shape, loc)
    dev = keep[0][0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    dets, labels, rows, num = _det_outputs(B, max_per_img, dev)
    _lib.check(_lib.lib().ia_guided_get_bboxes(
        geom.ref(), C.byref(p), B, _ptr(hw), _ptr(sf), int(bool(rescale)), float(score_thr), float(iou_thr),
        int(max_per_img), _ptr(ws), nbytes, _ptr(dets), _ptr(labels), _ptr(rows), _ptr(num), _stream()),
        'ia_guided_get_bboxes')
    if not debug:
        return dets, labels, rows, num
    return dets, labels, rows, num, _ws_views('ia_guided_workspace_layout', geom, B, ws)

"""torch front-end of the SSD kernels: the L2Norm layer (csrc/l2norm.hip) and the post-conv path of
SSDHead (csrc/ssddecode.hip): row scores, the compaction of the rows above score_thr, gather / decode,
the shared batched NMS (ia_ssd_get_bboxes), and its stage entries.
Device tensors only (fp32, NCHW; other layouts are converted), launched on the current torch stream,
like ops.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import IA_F32, SsdGeom, SsdLevelPtrs
from .ops import (_det_outputs, _meta_tensors, _ptr, _require_gpu, _state_workspace, _stream, nms_indices,
                  to_nchw)


def l2norm(x, weight, eps=1e-10):
    """(B, C, H, W) fp32 -> weight[c] * x / (sqrt(sum_c x^2) + eps) on the HIP kernel (a new tensor)"""
    _require_gpu(x, 'x')
    _require_gpu(weight, 'weight')
    if x.dim() != 4:
        raise ValueError('l2norm takes a (B, C, H, W) tensor, got %s' % (tuple(x.shape),))
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError('l2norm is float32 only (x %s, weight %s)' % (x.dtype, weight.dtype))
    B, Cn, H, W = x.shape
    if weight.numel() != Cn:
        raise ValueError('weight has %d entries for %d channels' % (weight.numel(), Cn))
    x = to_nchw(x.detach())
    y = torch.empty_like(x)
    l2norm_into(x, weight.detach().contiguous(), eps, y)
    return y


def l2norm_into(x, weight, eps, y):
    """the kernel on caller-owned contiguous fp32 NCHW buffers; raises on the library's error code
    (y overlapping x: argument error)"""
    B, Cn, H, W = x.shape
    _lib.check(_lib.lib().ia_l2norm_nchw(_ptr(x), _ptr(weight), float(eps), B, Cn, H, W, _ptr(y), _stream()),
               'ia_l2norm_nchw')
    return y


class SsdGeometry(object):
    """Static geometry of an SSD head for one set of feature-map sizes (fills ia_ssd_geom).
    base_anchors: one (A_l, 4) array per level; num_classes: the C foreground classes."""

    def __init__(self, featmap_sizes, strides, base_anchors, num_classes, means=(0., 0., 0., 0.),
                 stds=(1., 1., 1., 1.)):
        L = len(featmap_sizes)
        if L != len(strides) or L != len(base_anchors):
            raise ValueError('level count mismatch')
        base = [np.asarray(b, dtype=np.float32).reshape(-1, 4) for b in base_anchors]
        if L > _lib.IA_MAX_LEVELS or max(b.shape[0] for b in base) > _lib.IA_MAX_ANCHORS:
            raise ValueError('unsupported SSD geometry (levels %d, anchors %s)' % (L, [b.shape[0] for b in base]))
        g = SsdGeom()
        g.num_levels, g.num_classes = L, int(num_classes)
        for l, ((h, w), s) in enumerate(zip(featmap_sizes, strides)):
            g.H[l], g.W[l], g.stride[l], g.num_anchors[l] = int(h), int(w), int(s), base[l].shape[0]
            for a in range(base[l].shape[0]):
                for k in range(4):
                    g.base_anchors[l][a][k] = float(base[l][a, k])
        for k in range(4):
            g.means[k], g.stds[k] = float(means[k]), float(stds[k])
        self.struct = g
        self.L, self.C, self.Cin = L, int(num_classes), int(num_classes) + 1
        self.A = [b.shape[0] for b in base]
        self.featmap_sizes = [tuple(int(v) for v in s) for s in featmap_sizes]
        self.strides = [int(s) for s in strides]
        r, off = C.c_int32(), (C.c_int32 * (_lib.IA_MAX_LEVELS + 1))()
        _lib.check(_lib.lib().ia_ssd_geom_rows(C.byref(g), C.byref(r), C.byref(off)), 'ia_ssd_geom_rows')
        self.R = r.value                                        # anchor rows per image
        self.level_off = [off[l] for l in range(L + 1)]
        self.Rk = min(self.R, _lib.IA_MAX_CANDIDATES)           # compacted rows of the batched entry
        self.Rs = (self.Rk + 63) // 64 * 64
        self.key = ('ssd', tuple(self.featmap_sizes), tuple(self.A), self.C)

    def ref(self):
        return C.byref(self.struct)


def _ssd_ptrs(geom, cls, reg):
    """-> (level pointers, batch, the NCHW-contiguous tensors kept alive)"""
    cls, reg = list(cls), list(reg)
    if not (len(cls) == len(reg) == geom.L):
        raise AssertionError('expected %d levels' % geom.L)
    B = cls[0].shape[0]
    p = SsdLevelPtrs()
    for l in range(geom.L):
        h, w = geom.featmap_sizes[l]
        for name, m, ch in (('cls_score', cls, geom.A[l] * geom.Cin), ('bbox_pred', reg, geom.A[l] * 4)):
            t = m[l]
            _require_gpu(t, name)
            if tuple(t.shape) != (B, ch, h, w):
                raise AssertionError('%s level %d has shape %s, expected %s' % (name, l, tuple(t.shape), (B, ch, h, w)))
            if t.dtype != torch.float32:
                raise TypeError('%s has dtype %s: the SSD decode takes fp32 head outputs' % (name, t.dtype))
            m[l] = to_nchw(t.detach())
        p.cls[l], p.reg[l] = cls[l].data_ptr(), reg[l].data_ptr()
    return p, B, (cls, reg)


def ssd_rowscore(geom, cls, reg):
    """(B, R) fp32: the largest foreground softmax score of every anchor row, rows in the reference's
    order (level, then (y, x), then anchor)"""
    p, B, keep = _ssd_ptrs(geom, cls, reg)
    out = torch.empty((B, geom.R), dtype=torch.float32, device=keep[0][0].device)
    _lib.check(_lib.lib().ia_ssd_rowscore(geom.ref(), C.byref(p), B, IA_F32, _ptr(out), _stream()), 'ia_ssd_rowscore')
    return out


def ssd_compact(best, score_thr, out=None):
    """best (B, R) -> kept_rows (B, IA_MAX_CANDIDATES) int32 (ascending rows with best > score_thr, -1
    behind the count), kept_count (B) int32 (the true count), overflow (B) int32.
    out: caller-owned (kept_rows, kept_count, overflow) to write into."""
    _require_gpu(best, 'best')
    if best.dim() != 2 or best.dtype != torch.float32 or not best.is_contiguous():
        raise ValueError('best must be a contiguous (B, R) float32 tensor')
    B, R = best.shape
    dev = best.device
    if out is None:
        out = (torch.empty((B, _lib.IA_MAX_CANDIDATES), dtype=torch.int32, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    kept_rows, kept_count, overflow = out
    nbytes = _lib.lib().ia_ssd_compact_workspace_bytes(B, R)
    ws = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().ia_ssd_compact(_ptr(best), B, R, float(score_thr), _ptr(kept_rows), _ptr(kept_count),
                                         _ptr(overflow), _ptr(ws), nbytes, _stream()), 'ia_ssd_compact')
    return kept_rows, kept_count, overflow


def ssd_gather_decode(geom, cls, reg, kept_rows, kept_count, Rk, img_shapes, scale_factors, rescale):
    """kept_rows (B, stride >= Rk) int32, kept_count (B) int32 -> boxes (B, Rk, 4), scores_t (B, C, Rs),
    best_score (B, Rk) of the first kept_count[b] rows; zeros behind them.  Any Rk >= 1."""
    p, B, keep = _ssd_ptrs(geom, cls, reg)
    dev = keep[0][0].device
    for name, t in (('kept_rows', kept_rows), ('kept_count', kept_count)):
        _require_gpu(t, name)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.shape[0] != B:
            raise ValueError('%s must be a contiguous int32 tensor with %d rows' % (name, B))
    Rk = int(Rk)
    if kept_rows.dim() != 2 or kept_rows.shape[1] < Rk or Rk < 1:
        raise ValueError('kept_rows must be (B, >= Rk)')
    Rs = (Rk + 63) // 64 * 64
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    boxes = torch.empty((B, Rk, 4), dtype=torch.float32, device=dev)
    scores_t = torch.zeros((B, geom.C, Rs), dtype=torch.float32, device=dev)
    best = torch.empty((B, Rk), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ia_ssd_gather_decode(
        geom.ref(), C.byref(p), B, IA_F32, _ptr(kept_rows), int(kept_rows.shape[1]), _ptr(kept_count), Rk, _ptr(hw),
        _ptr(sf), int(bool(rescale)), _ptr(boxes), _ptr(scores_t), _ptr(best), _stream()), 'ia_ssd_gather_decode')
    return boxes, scores_t, best


_SSD_VIEWS = ('rowscore', 'kept_rows', 'kept_count', 'boxes', 'scores_t', 'best_score', 'keep_count', 'keep_rows')


def ssd_workspace_views(geom, B, ws):
    """dict of views into the workspace of ia_ssd_get_bboxes (ia_ssd_workspace_layout)"""
    off = (C.c_size_t * 8)()
    _lib.check(_lib.lib().ia_ssd_workspace_layout(geom.ref(), B, C.byref(off)), 'ia_ssd_workspace_layout')
    f32, i32 = torch.float32, torch.int32
    shapes = ((f32, (B, geom.R)), (i32, (B, _lib.IA_MAX_CANDIDATES)), (i32, (B,)), (f32, (B, geom.Rk, 4)),
              (f32, (B, geom.C, geom.Rs)), (f32, (B, geom.Rk)), (i32, (B, geom.C)), (i32, (B, geom.C, geom.Rs)))
    out = {}
    for i, (name, (dtype, shape)) in enumerate(zip(_SSD_VIEWS, shapes)):
        out[name] = ws[off[i]:off[i] + int(np.prod(shape)) * 4].view(dtype).view(*shape)
    return out


def ssd_get_bboxes(geom, cls, reg, img_shapes, scale_factors, rescale, score_thr, iou_thr, max_per_img,
                   debug=False, workspace=None, outputs=None):
    """Whole post-conv path of SSDHead for a batch -> device tensors dets (B,max,5), labels (B,max) int32,
    rows (B,max) int32 (anchor row ids), num (B) int32, overflow (B) int32 (+ the workspace views with
    debug=True).  An image with overflow[b] = 1 (more than IA_MAX_CANDIDATES rows above score_thr) has
    num[b] = 0: resolve it with ssd_get_bboxes_per_class.  No host synchronisation.
    workspace / outputs: caller-owned buffers (tests: guard checks)."""
    if max_per_img > _lib.IA_MAX_PER_IMG:
        raise _lib.IouAwareLibraryError('max_per_img above %d' % _lib.IA_MAX_PER_IMG)
    if not float(score_thr) >= 0.0:
        raise ValueError('score_thr=%r: the SSD decode needs a threshold >= 0' % (score_thr,))
    p, B, keep = _ssd_ptrs(geom, cls, reg)
    dev = keep[0][0].device
    nbytes = _lib.lib().ia_ssd_get_bboxes_workspace_bytes(geom.ref(), B)
    if nbytes == 0:
        raise _lib.IouAwareLibraryError('unsupported geometry / batch for ia_ssd_get_bboxes')
    ws = _state_workspace(dev, nbytes, (geom.key, B)) if workspace is None else workspace
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    if outputs is None:
        outputs = _det_outputs(B, max_per_img, dev) + (torch.empty((B,), dtype=torch.int32, device=dev),)
    dets, labels, rows, num, overflow = outputs
    _lib.check(_lib.lib().ia_ssd_get_bboxes(
        geom.ref(), C.byref(p), B, IA_F32, _ptr(hw), _ptr(sf), int(bool(rescale)), float(score_thr), float(iou_thr),
        int(max_per_img), _ptr(ws), nbytes, _ptr(dets), _ptr(labels), _ptr(rows), _ptr(num), _ptr(overflow),
        _stream()), 'ia_ssd_get_bboxes')
    if not debug:
        return dets, labels, rows, num, overflow
    return dets, labels, rows, num, overflow, ssd_workspace_views(geom, B, ws)


def ssd_get_bboxes_per_class(geom, cls, reg, img_shapes, scale_factors, rescale, score_thr, iou_thr, max_per_img):
    """The unbounded route for any number of rows above score_thr: the SSD stage entries (row scores,
    the kept rows, gather / decode at Rk = the largest kept count), then multiclass_nms as the
    reference writes it -- the per-class loop of ops._get_bboxes_per_class: one ia_nms per class,
    class-major concatenation, a stable score sort when more than max_per_img survive.  Same return
    values as ssd_get_bboxes without the flags; a host synchronisation per class problem."""
    cls, reg = list(cls), list(reg)
    best = ssd_rowscore(geom, cls, reg)
    B, dev = best.shape[0], best.device
    over = best > score_thr
    counts = over.sum(dim=1).to(torch.int32)
    Rk = max(int(counts.max()), 1)
    kept = torch.full((B, Rk), -1, dtype=torch.int32, device=dev)
    for b in range(B):
        idx = over[b].nonzero().flatten()
        kept[b, :idx.numel()] = idx.to(torch.int32)
    boxes, scores_t, _ = ssd_gather_decode(geom, cls, reg, kept, counts.contiguous(), Rk, img_shapes, scale_factors,
                                           rescale)
    dets, labels, rows, num = _det_outputs(B, max_per_img, dev, fill=True)
    for b in range(B):
        n_b = int(counts[b])
        sc = scores_t[b, :, :n_b] > score_thr                          # (C, n_b)
        live = sc.any(dim=1).nonzero().flatten().tolist()
        d_all, l_all, r_all = [], [], []
        for c in live:
            inds = sc[c].nonzero().flatten()                            # ascending compacted rows
            d = torch.cat([boxes[b, inds], scores_t[b, c, inds, None]], dim=1)
            keep = nms_indices(d, iou_thr)
            d_all.append(d[keep]); r_all.append(kept[b, inds[keep]])
            l_all.append(torch.full((keep.numel(),), c, dtype=torch.int32, device=dev))
        if not d_all:
            continue
        d_all, l_all, r_all = torch.cat(d_all), torch.cat(l_all), torch.cat(r_all)
        if d_all.shape[0] > max_per_img:
            order = torch.sort(d_all[:, 4], descending=True, stable=True)[1][:max_per_img]
            d_all, l_all, r_all = d_all[order], l_all[order], r_all[order]
        n = d_all.shape[0]
        dets[b, :n], labels[b, :n], rows[b, :n], num[b] = d_all, l_all, r_all.to(torch.int32), n
    return dets, labels, rows, num

"""torch front-end of the SSD kernels: the L2Norm layer (csrc/l2norm.hip), the post-conv path of
SSDHead (csrc/ssddecode.hip): row scores, the compaction of the rows above score_thr, gather / decode,
the shared batched NMS (ia_ssd_get_bboxes), and its stage entries; and the training loss
(csrc/ssdloss.hip): cross-entropy rows, hard-negative mining, smooth-L1, as one autograd node
(ssd_head_loss) and its stage entries.
Device tensors only (fp32, NCHW; other layouts are converted), launched on the current torch stream,
like ops.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import IA_F32, SsdGeom, SsdLevelPtrs
from .ops import (_det_outputs, _meta_tensors, _own_workspace, _ptr, _require_gpu, _state_workspace, _stream,
                  nms_indices, to_nchw)


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


# ------------------------------------------------------------------ training loss (csrc/ssdloss.hip)
_SSD_LOSS_VIEWS = ('ce', 'lse', 'sel', 'counts', 'partials')


def ssd_mine_lds_rows():
    """rows up to which ia_ssd_mine keeps its keys in LDS (above: re-read from global memory)"""
    return int(_lib.lib().ia_ssd_mine_lds_rows())


def ssd_loss_partials(geom):
    """number of fp64 box partial sums per image that ia_ssd_loss_rows writes"""
    n = C.c_int32()
    _lib.check(_lib.lib().ia_ssd_loss_partials(geom.ref(), C.byref(n)), 'ia_ssd_loss_partials')
    return n.value


def _ssd_targets(B, R, labels, label_weights, bbox_targets, bbox_weights):
    """the four image-major target tensors, checked and made contiguous"""
    out = []
    for name, t, dtype, shape in (('labels', labels, torch.int64, (B, R)),
                                  ('label_weights', label_weights, torch.float32, (B, R)),
                                  ('bbox_targets', bbox_targets, torch.float32, (B, R, 4)),
                                  ('bbox_weights', bbox_weights, torch.float32, (B, R, 4))):
        _require_gpu(t, name)
        if tuple(t.shape) != shape:
            raise ValueError('%s has shape %s, expected %s' % (name, tuple(t.shape), shape))
        out.append(t.detach().to(dtype).contiguous())
    return out


def _ssd_avg(avg_factor):
    """-> (device pointer or NULL, host value, tensor kept alive): the convention of ia_head_targets"""
    if isinstance(avg_factor, torch.Tensor):
        _require_gpu(avg_factor, 'avg_factor')
        t = avg_factor.detach().to(torch.float32).reshape(-1)[:1].contiguous()
        return _ptr(t), 0.0, t
    if not float(avg_factor) > 0:
        raise ValueError('avg_factor=%r: must be positive' % (avg_factor,))
    return C.c_void_p(0), float(avg_factor), None


def _check_loss_cfg(neg_pos_ratio, beta):
    if int(neg_pos_ratio) != neg_pos_ratio or neg_pos_ratio < 0:
        raise ValueError('neg_pos_ratio=%r: must be an integer >= 0' % (neg_pos_ratio,))
    if not float(beta) > 0:
        raise ValueError('beta=%r: the smooth-L1 beta must be positive' % (beta,))


def ssd_loss_rows(geom, cls, reg, labels, label_weights, bbox_targets, bbox_weights, beta=1.0):
    """stage 1 -> ce (B, R), lse (B, R) fp32 and the box partial sums (B, nparts) fp64"""
    _check_loss_cfg(0, beta)
    p, B, keep = _ssd_ptrs(geom, cls, reg)
    tg = _ssd_targets(B, geom.R, labels, label_weights, bbox_targets, bbox_weights)
    dev = keep[0][0].device
    ce = torch.empty((B, geom.R), dtype=torch.float32, device=dev)
    lse = torch.empty_like(ce)
    parts = torch.empty((B, ssd_loss_partials(geom)), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ia_ssd_loss_rows(geom.ref(), C.byref(p), B, IA_F32, _ptr(tg[0]), _ptr(tg[1]), _ptr(tg[2]),
                                           _ptr(tg[3]), float(beta), _ptr(ce), _ptr(lse), _ptr(parts), _stream()),
               'ia_ssd_loss_rows')
    return ce, lse, parts


def ssd_mine(ce, labels, neg_pos_ratio, avg_factor=1.0, box_partials=None):
    """stage 2 on ce (B, R) fp32 and labels (B, R) int64 -> sel (B, R) uint8, counts (B, 2) int32 =
    (num_pos, k), losses (B, 2) fp32 (classification, box; box 0 without partials)"""
    _check_loss_cfg(neg_pos_ratio, 1.0)
    _require_gpu(ce, 'ce')
    _require_gpu(labels, 'labels')
    if ce.dim() != 2 or ce.dtype != torch.float32 or labels.dtype != torch.int64 or labels.shape != ce.shape:
        raise ValueError('ce must be (B, R) float32 and labels (B, R) int64')
    ce, labels = ce.contiguous(), labels.contiguous()
    B, R = ce.shape
    dev = ce.device
    nparts = 0
    if box_partials is not None:
        _require_gpu(box_partials, 'box_partials')
        if box_partials.dtype != torch.float64 or box_partials.dim() != 2 or box_partials.shape[0] != B:
            raise ValueError('box_partials must be (B, nparts) float64')
        box_partials = box_partials.contiguous()
        nparts = box_partials.shape[1]
    avg_p, avg_h, avg_keep = _ssd_avg(avg_factor)
    sel = torch.empty((B, R), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    losses = torch.empty((B, 2), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ia_ssd_mine(_ptr(ce), _ptr(labels), B, R, int(neg_pos_ratio), _ptr(box_partials), nparts,
                                      avg_p, avg_h, _ptr(sel), _ptr(counts), _ptr(losses), _stream()), 'ia_ssd_mine')
    return sel, counts, losses


def ssd_loss_workspace_views(geom, B, ws):
    """dict of views into the workspace of ia_ssd_head_loss_fwd (ia_ssd_head_loss_workspace_layout)"""
    off = (C.c_size_t * 5)()
    _lib.check(_lib.lib().ia_ssd_head_loss_workspace_layout(geom.ref(), B, C.byref(off)),
               'ia_ssd_head_loss_workspace_layout')
    shapes = ((torch.float32, (B, geom.R)), (torch.float32, (B, geom.R)), (torch.uint8, (B, geom.R)),
              (torch.int32, (B, 2)), (torch.float64, (B, ssd_loss_partials(geom))))
    out = {}
    for i, (name, (dtype, shape)) in enumerate(zip(_SSD_LOSS_VIEWS, shapes)):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        out[name] = ws[off[i]:off[i] + n].view(dtype).view(*shape)
    return out


class _SsdHeadLossFn(torch.autograd.Function):
    """SSD's loss of a batch (csrc/ssdloss.hip): 2 launches forward, 1 backward, no host
    synchronisation.  Outputs: loss_cls (B,), loss_bbox (B,)."""

    @staticmethod
    def forward(ctx, geom, targets, avg_factor, neg_pos_ratio, beta, workspace, grads, *outs):
        L = geom.L
        p, B, keep = _ssd_ptrs(geom, outs[:L], outs[L:])
        dev = keep[0][0].device
        tg = _ssd_targets(B, geom.R, *targets)
        avg_p, avg_h, avg_keep = _ssd_avg(avg_factor)
        nbytes = _lib.lib().ia_ssd_head_loss_workspace_bytes(geom.ref(), B)
        if nbytes == 0:
            raise _lib.IouAwareLibraryError('unsupported geometry / batch for ia_ssd_head_loss')
        # own buffer: it carries lse and the selection from forward to backward
        ws = _own_workspace(dev, nbytes) if workspace is None else workspace
        if ws.numel() < nbytes:
            raise ValueError('workspace has %d bytes, ia_ssd_head_loss needs %d' % (ws.numel(), nbytes))
        losses = torch.empty((B, 2), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ia_ssd_head_loss_fwd(
            geom.ref(), C.byref(p), B, IA_F32, _ptr(tg[0]), _ptr(tg[1]), _ptr(tg[2]), _ptr(tg[3]), avg_p, avg_h,
            int(neg_pos_ratio), float(beta), _ptr(ws), ws.numel(), _ptr(losses), _stream()), 'ia_ssd_head_loss_fwd')
        ctx.geom, ctx.B, ctx.beta, ctx.ws, ctx.grads = geom, B, float(beta), ws, grads
        ctx.keep = (p, keep, tg, (avg_p, avg_h, avg_keep))
        ctx.set_materialize_grads(False)
        return losses[:, 0], losses[:, 1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        p, (cls, reg), tg, (avg_p, avg_h, _) = ctx.keep
        geom, B, dev = ctx.geom, ctx.B, cls[0].device
        z = torch.zeros(B, dtype=torch.float32, device=dev)
        gin = torch.stack([z if g is None else g.detach().to(torch.float32).reshape(B) for g in (g_cls, g_box)],
                          dim=1).contiguous()
        grads = ctx.grads
        if grads is None:
            grads = [torch.empty_like(t) for t in cls + reg]
        gp = SsdLevelPtrs()
        for l in range(geom.L):
            gp.cls[l], gp.reg[l] = grads[l].data_ptr(), grads[geom.L + l].data_ptr()
        _lib.check(_lib.lib().ia_ssd_head_loss_bwd(
            geom.ref(), C.byref(p), B, IA_F32, _ptr(tg[0]), _ptr(tg[1]), _ptr(tg[2]), _ptr(tg[3]), avg_p, avg_h,
            ctx.beta, _ptr(ctx.ws), ctx.ws.numel(), _ptr(gin), C.byref(gp), _stream()), 'ia_ssd_head_loss_bwd')
        return (None,) * 7 + tuple(grads)


def ssd_head_loss(geom, cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor,
                  neg_pos_ratio=3, beta=1.0, workspace=None, grads=None):
    """SSDHead's loss for a batch on the HIP node -> (loss_cls (B,), loss_bbox (B,)), differentiable in
    the head outputs.  cls_scores / bbox_preds: per-level fp32 device tensors (other layouts are
    converted by to_nchw); labels (B, R) int64 in 0..C, label_weights (B, R), bbox_targets / bbox_weights
    (B, R, 4); avg_factor: a python number or a device scalar; neg_pos_ratio an integer >= 0; beta > 0.
    Launched on the current stream, no device-to-host copy.
    workspace / grads: caller-owned buffers (tests: guard checks); grads = the 2 L contiguous gradient
    maps (class maps first) the backward writes and returns."""
    _check_loss_cfg(neg_pos_ratio, beta)
    outs = list(cls_scores) + list(bbox_preds)
    if len(outs) != 2 * geom.L:
        raise AssertionError('expected %d levels' % geom.L)
    for t in outs:
        _require_gpu(t, 'head output')
    return _SsdHeadLossFn.apply(geom, (labels, label_weights, bbox_targets, bbox_weights), avg_factor,
                                int(neg_pos_ratio), float(beta), workspace, grads, *outs)

"""torch front-end of the FCOS kernels (csrc/groupnorm.hip, csrc/pointdecode.hip,
csrc/pointloss.hip): the point heads' post-conv paths (ia_point_get_bboxes: IoU-aware;
ia_point_ctr_get_bboxes: plain FCOS, the centerness map in the third slot), the towers'
GroupNorm + ReLU (in place for inference; groupnorm_relu / groupnorm_relu_bf16: the fp32 and bf16
autograd nodes), and the training
side: point targets and the all-levels loss node.
Device tensors only, launched on the current torch stream, like ops.py."""
import ctypes as C

import torch

from . import _lib
from ._lib import LevelPtrs, PointHeadGeom, PointLevelPtrs, PointPixStrides
from . import winograd
from .ops import (_LayoutTwin, _det_outputs, _meta_tensors, _own_workspace, _ptr, _require_gpu,
                  _state_workspace, _stream, _ws_views, _zero1, stream_id, to_nchw)


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


_DTYPES = {torch.float32: _lib.IA_F32, torch.bfloat16: _lib.IA_BF16}


def _point_ptrs(geom, cls, reg, iou, third='iou_pred'):
    """-> (level pointers, batch, geometry in the maps' layout, dtype code); the maps are fp32 or
    bf16, all of one dtype"""
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
            if t.dtype not in _DTYPES or t.dtype != cls[0].dtype:
                raise TypeError('the point-head decode takes fp32 or bf16 head outputs, all of '
                                'one dtype')
    nhwc = (geom.C * cls[0].element_size()) % 16 == 0 and not all(t.is_contiguous() for t in tensors) and all(
        t.is_contiguous(memory_format=torch.channels_last) for t in tensors)
    geom = geom.with_layout(_lib.IA_LAYOUT_NHWC if nhwc else _lib.IA_LAYOUT_NCHW)
    p = LevelPtrs()
    for l in range(geom.L):
        if not nhwc:
            cls[l], reg[l], iou[l] = to_nchw(cls[l]), to_nchw(reg[l]), to_nchw(iou[l])
        p.cls[l], p.reg[l], p.iou[l] = cls[l].data_ptr(), reg[l].data_ptr(), iou[l].data_ptr()
    return p, B, geom, _DTYPES[cls[0].dtype]


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
    p, B, geom, dt = _point_ptrs(geom, cls, reg, iou)
    dev = cls[0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    _lib.check(_lib.lib().ia_point_decode_stage_dt(geom.ref(), C.byref(p), B, dt, _ptr(hw), _ptr(sf),
                                                   int(bool(rescale)), _ptr(ws), nbytes, _stream()),
               'ia_point_decode_stage_dt')
    return _views(geom, B, ws)


def point_ctr_decode_stage(geom, cls, reg, ctr, img_shapes, scale_factors, rescale, score_thr):
    """plain FCOS decode stage -> the views of point_decode_stage; scores_t holds
    sigmoid(cls) * sigmoid(ctr) where sigmoid(cls) > score_thr and a negative sentinel elsewhere"""
    cls, reg, ctr = list(cls), list(reg), list(ctr)
    p, B, geom, dt = _point_ptrs(geom, cls, reg, ctr, 'centerness')
    dev = cls[0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    _lib.check(_lib.lib().ia_point_ctr_decode_stage_dt(geom.ref(), C.byref(p), B, dt, _ptr(hw),
                                                       _ptr(sf), int(bool(rescale)),
                                                       float(score_thr), _ptr(ws), nbytes, _stream()),
               'ia_point_ctr_decode_stage_dt')
    return _views(geom, B, ws)


def _get_bboxes(entry, third, geom, cls, reg, iou, img_shapes, scale_factors, rescale, score_thr,
                iou_thr, max_per_img, lazy, debug):
    if max_per_img > _lib.IA_MAX_PER_IMG:
        raise _lib.IouAwareLibraryError('max_per_img above %d' % _lib.IA_MAX_PER_IMG)
    cls, reg, iou = list(cls), list(reg), list(iou)
    p, B, geom, dt = _point_ptrs(geom, cls, reg, iou, third)
    dev = cls[0].device
    nbytes, ws = _workspace(geom, B, dev)
    hw, sf = _meta_tensors(img_shapes, scale_factors, dev)
    dets, labels, rows, num = _det_outputs(B, max_per_img, dev)
    _lib.check(getattr(_lib.lib(), entry)(
        geom.ref(), C.byref(p), B, dt, _ptr(hw), _ptr(sf), int(bool(rescale)), float(score_thr),
        float(iou_thr), int(max_per_img), 0 if lazy else -1, _ptr(ws), nbytes, _ptr(dets),
        _ptr(labels), _ptr(rows), _ptr(num), _stream()), entry)
    if not debug:
        return dets, labels, rows, num
    return dets, labels, rows, num, _views(geom, B, ws)


def point_get_bboxes(geom, cls, reg, iou, img_shapes, scale_factors, rescale, score_thr, iou_thr,
                     max_per_img, lazy=True, debug=False):
    """Whole post-conv path of the point head for a batch (fp32 or bf16 maps) -> device tensors dets (B,max,5),
    labels (B,max) int32, rows (B,max) int32 (candidate rows), num (B) int32 (+ the decode-stage
    views with debug=True)."""
    return _get_bboxes('ia_point_get_bboxes_dt', 'iou_pred', geom, cls, reg, iou, img_shapes,
                       scale_factors, rescale, score_thr, iou_thr, max_per_img, lazy, debug)


def point_ctr_get_bboxes(geom, cls, reg, ctr, img_shapes, scale_factors, rescale, score_thr,
                         iou_thr, max_per_img, lazy=True, debug=False):
    """point_get_bboxes for plain FCOS (ia_point_ctr_get_bboxes): the raw score sigmoid(cls) is
    thresholded, NMS and the final sort run on sigmoid(cls) * sigmoid(ctr); geom.score_alpha is
    not used."""
    return _get_bboxes('ia_point_ctr_get_bboxes_dt', 'centerness', geom, cls, reg, ctr, img_shapes,
                       scale_factors, rescale, score_thr, iou_thr, max_per_img, lazy, debug)


def _wino_geom(xs):
    return winograd._wino_geom([x.shape[2:] for x in xs], xs[0].shape[0])


_gn_ws = {}


def _gn_workspace(dev, nbytes):
    """the partials' buffer of (device, stream): written and read by consecutive launches only"""
    key = (dev.index, stream_id())
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _gn_ws[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return ws


def groupnorm_relu_(xs, gamma, beta, groups, eps=1e-5, relu=True):
    """In place over the levels xs[l] (B, ch, H_l, W_l) channels-last, all fp32 or all bf16:
    GroupNorm (statistics per level and image) + ReLU, two launches for all of them.  gamma / beta
    (ch,) fp32.  bf16: fp64 statistics of the stored values, fp32 x * s + t, one rounding."""
    for x in xs:
        _require_gpu(x, 'x')
    dtype = xs[0].dtype if xs and xs[0].dtype in _DTYPES else torch.float32
    ch = _gn_check('groupnorm_relu_', xs, gamma, beta, dtype)
    dt = _DTYPES[dtype]
    g = _wino_geom(xs)
    L = _lib.lib()
    nbytes = L.ia_groupnorm_workspace_bytes_dt(C.byref(g), ch, int(groups), dt)
    if nbytes == 0:
        raise _lib.IouAwareLibraryError('unsupported GroupNorm geometry (channels %d, groups %d, %s)'
                                        % (ch, groups, dtype))
    ws = _gn_workspace(xs[0].device, nbytes)
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    _lib.check(L.ia_groupnorm_stats_dt(C.byref(g), ptrs, dt, ch, int(groups), _ptr(ws), nbytes,
                                       _stream()), 'ia_groupnorm_stats_dt')
    _lib.check(L.ia_groupnorm_apply_dt(C.byref(g), ptrs, dt, ch, int(groups), _ptr(gamma), _ptr(beta),
                                       float(eps), int(bool(relu)), _ptr(ws), nbytes, _stream()),
               'ia_groupnorm_apply_dt')
    return xs


def scale_exp_(xs, scales):
    """In place over the levels xs[l] (B, ch, H_l, W_l) channels-last, all fp32 or all bf16 (ch % 4
    == 0): exp(scales[l] * x), the FCOS regression epilogue; scales (L,) fp32 on the device.  bf16:
    the fp32 evaluation, rounded once."""
    for x in xs:
        _require_gpu(x, 'x')
        if x.dtype not in _DTYPES or x.dtype != xs[0].dtype or x.dim() != 4 \
                or not x.is_contiguous(memory_format=torch.channels_last):
            raise ValueError('scale_exp_ takes fp32 or bf16 channels-last levels of one dtype')
    if scales.dtype != torch.float32 or scales.numel() < len(xs) or not scales.is_contiguous():
        raise ValueError('scales: one fp32 value per level')
    g = _wino_geom(xs)
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    _lib.check(_lib.lib().ia_scale_exp_levels_dt(C.byref(g), ptrs, _DTYPES[xs[0].dtype],
                                                 int(xs[0].shape[1]), _ptr(scales), _stream()),
               'ia_scale_exp_levels_dt')
    return xs


def _gn_check(name, xs, gamma, beta, dtype=torch.float32, takes=None):
    """the argument contract of groupnorm_relu_ / groupnorm_relu / groupnorm_relu_bf16: ValueError
    before the device is touched -> channels.  dtype: what the levels hold (the fp32 training node:
    fp32 only; the bf16 one: bf16 only)"""
    if not xs or len(xs) > _lib.IA_MAX_LEVELS:
        raise ValueError('1..%d levels' % _lib.IA_MAX_LEVELS)
    ch = int(xs[0].shape[1]) if xs[0].dim() == 4 else -1
    for x in xs:
        if not x.is_cuda or x.dtype != dtype or x.dim() != 4 or x.shape[1] != ch \
                or x.shape[0] != xs[0].shape[0] or x.device != xs[0].device \
                or not x.is_contiguous(memory_format=torch.channels_last):
            raise ValueError('%s takes %s channels-last (B, %d, H, W) levels on one device'
                             % (name, takes or ('fp32' if dtype == torch.float32 else 'fp32 or bf16'), ch))
    for t in (gamma, beta):
        if t.dtype != torch.float32 or t.numel() != ch or not t.is_contiguous() or t.device != xs[0].device:
            raise ValueError('gamma / beta: (%d,) fp32 on the device' % ch)
    return ch


def _gn_upstream(d):
    """an upstream gradient as the kernels read it: fp32, channels-last, 16-byte aligned (a copy
    where autograd hands over anything else, e.g. a slice with a storage offset)"""
    d = d.to(torch.float32).contiguous(memory_format=torch.channels_last)
    return d.clone(memory_format=torch.channels_last) if d.data_ptr() % 16 else d


def _level_ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class _GroupNormReluFn(torch.autograd.Function):
    """y_l = relu?(GroupNorm(x_l)) over a level list, out of place (csrc/groupnorm.hip): 2 launches
    forward, 2 (+ 1 for the parameter gradients) backward.  Keeps x and (mean, rstd) in fp64 per
    (level, image, group); y is not kept."""

    @staticmethod
    def forward(ctx, gamma, beta, groups, eps, relu, *xs):
        ch = int(xs[0].shape[1])
        g = _wino_geom(xs)
        L = _lib.lib()
        nbytes = L.ia_groupnorm_workspace_bytes(C.byref(g), ch, groups)
        nsaved = L.ia_groupnorm_saved_bytes(C.byref(g), ch, groups)
        nbwd = L.ia_groupnorm_bwd_workspace_bytes(C.byref(g), ch, groups)
        if nbytes == 0 or nsaved == 0 or nbwd == 0:
            raise _lib.IouAwareLibraryError('unsupported GroupNorm geometry (channels %d, groups %d)'
                                            % (ch, groups))
        dev = xs[0].device
        gamma_, beta_ = gamma.detach(), beta.detach()
        ws = _gn_workspace(dev, max(nbytes, nbwd))
        saved = torch.empty(int(nsaved), dtype=torch.uint8, device=dev)
        ys = [torch.empty_like(x) for x in xs]
        px = _level_ptrs(xs)
        _lib.check(L.ia_groupnorm_stats(C.byref(g), px, ch, groups, _ptr(ws), nbytes, _stream()),
                   'ia_groupnorm_stats')
        _lib.check(L.ia_groupnorm_apply_to(C.byref(g), px, _level_ptrs(ys), ch, groups, _ptr(gamma_),
                                           _ptr(beta_), eps, int(relu), _ptr(ws), nbytes, _ptr(saved),
                                           nsaved, _stream()), 'ia_groupnorm_apply_to')
        ctx.geom, ctx.cfg, ctx.sizes = g, (ch, groups, int(relu)), (nsaved, nbwd)
        ctx.save_for_backward(gamma, beta, saved, *xs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        gamma, beta, saved = ctx.saved_tensors[:3]
        xs = ctx.saved_tensors[3:]
        ch, groups, relu = ctx.cfg
        nsaved, nbwd = ctx.sizes
        g, L, dev = ctx.geom, _lib.lib(), xs[0].device
        gamma_, beta_ = gamma.detach(), beta.detach()
        dys = [_gn_upstream(d) for d in dys]
        ws = _gn_workspace(dev, nbwd)
        px, pdy = _level_ptrs(xs), _level_ptrs(dys)
        _lib.check(L.ia_groupnorm_bwd_reduce(C.byref(g), px, pdy, ch, groups, _ptr(gamma_), _ptr(beta_),
                                             relu, _ptr(saved), nsaved, _ptr(ws), nbwd, _stream()),
                   'ia_groupnorm_bwd_reduce')
        need_x = any(ctx.needs_input_grad[5:])
        dxs = [torch.empty_like(x) for x in xs] if need_x else None
        dgamma = torch.empty(ch, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dbeta = torch.empty(ch, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if need_x or dgamma is not None or dbeta is not None:
            _lib.check(L.ia_groupnorm_bwd_apply(C.byref(g), px, pdy, _level_ptrs(dxs) if need_x else None,
                                                ch, groups, _ptr(gamma_), _ptr(beta_), relu, _ptr(saved),
                                                nsaved, _ptr(ws), nbwd, _ptr(dgamma), _ptr(dbeta),
                                                _stream()), 'ia_groupnorm_bwd_apply')
        return (dgamma, dbeta, None, None, None) + (tuple(dxs) if need_x else (None,) * len(xs))


def groupnorm_supported(sizes, batch, channels, groups):
    """whether the GroupNorm training kernels cover per-level (H, W) sizes at this batch, channel
    and group count (the library's own answer: its workspace query)"""
    g = winograd._wino_geom([tuple(int(v) for v in s) for s in sizes], int(batch))
    return _lib.lib().ia_groupnorm_bwd_workspace_bytes(C.byref(g), int(channels), int(groups)) != 0


def groupnorm_relu(xs, gamma, beta, groups, eps=1e-5, relu=True):
    """Out of place over the levels xs[l] (B, ch, H_l, W_l) fp32 channels-last: GroupNorm (statistics
    per level and image) + ReLU as one autograd node with gradients for every x_l, gamma and beta
    (those that require them).  -> list of new channels-last tensors."""
    xs = list(xs)
    _gn_check('groupnorm_relu', xs, gamma, beta)
    return list(_GroupNormReluFn.apply(gamma, beta, int(groups), float(eps), bool(relu), *xs))


# ------------------------------------------------------------------ the bf16 training node
_CL = torch.channels_last


def _gn_upstream_bf16(d):
    """an upstream gradient as the bf16 kernels read it: bf16, channels-last, 16-byte aligned -- taken
    as it is when autograd hands it over that way (what the bf16 convolution node's backward
    returns), a copy otherwise"""
    if d.dtype == torch.bfloat16 and d.is_contiguous(memory_format=_CL) and d.data_ptr() % 16 == 0:
        return d
    d = d.to(torch.bfloat16).contiguous(memory_format=_CL)
    return d.clone(memory_format=_CL) if d.data_ptr() % 16 else d


def _halves_of_one(a, b):
    """whether a and b are the channel halves [0, F) and [F, 2F) of ONE dense channels-last
    (B, 2F, H, W) bf16 tensor: views of one storage, b right behind a in every pixel.  Never true for
    separate allocations that merely lie side by side."""
    F_ = a.shape[1]
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.dim() != 4 or a.shape != b.shape \
            or a.stride() != b.stride() or a.device != b.device \
            or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr() \
            or b.data_ptr() != a.data_ptr() + 2 * F_ or a.data_ptr() % 16:
        return False
    return _wide(a).is_contiguous(memory_format=_CL)


def _wide(a):
    """the (B, 2F, H, W) tensor that starts where the channel half `a` starts"""
    return a.as_strided((a.shape[0], 2 * a.shape[1], a.shape[2], a.shape[3]), a.stride())


def _empty_cl(like):
    B, ch, h, w = like.shape
    return torch.empty((B, h, w, ch), dtype=like.dtype, device=like.device).permute(0, 3, 1, 2)


class _GroupNormReluBf16Fn(torch.autograd.Function):
    """_GroupNormReluFn on bf16 channels-last levels (k_gn_stats_bf16, k_gn_apply_to_bf16,
    k_gn_bwd_reduce_bf16, k_gn_bwd_apply_bf16, k_gn_bwd_params): 2 launches forward, 2 (+ 1 for the
    parameter gradients) backward; keeps x and the fp64 (mean, rstd), not y.

    halves == 2: the inputs are 2 x L channel halves (tower-major) of L dense (B, 2F, H, W) tensors
    (_halves_of_one holds for every level: the caller checks) and the node runs on the wide tensors;
    its outputs, and the input gradients it returns, are again the two halves of one tensor per
    level, so that the bf16 convolution nodes on either side keep addressing both towers in one
    pass."""

    @staticmethod
    def forward(ctx, gamma, beta, groups, eps, relu, halves, *xs):
        L_ = len(xs) // halves
        wide = [_wide(x) for x in xs[:L_]] if halves == 2 else list(xs)
        ch = int(wide[0].shape[1])
        g = _wino_geom(wide)
        L = _lib.lib()
        dt = _lib.IA_BF16
        nbytes = L.ia_groupnorm_workspace_bytes_dt(C.byref(g), ch, groups, dt)
        nsaved = L.ia_groupnorm_saved_bytes_dt(C.byref(g), ch, groups, dt)
        nbwd = L.ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), ch, groups, dt)
        if nbytes == 0 or nsaved == 0 or nbwd == 0:
            raise _lib.IouAwareLibraryError('unsupported bf16 GroupNorm geometry (channels %d, groups %d)'
                                            % (ch, groups))
        dev = wide[0].device
        gamma_, beta_ = gamma.detach(), beta.detach()
        ws = _gn_workspace(dev, max(nbytes, nbwd))
        saved = torch.empty(int(nsaved), dtype=torch.uint8, device=dev)
        ys = [_empty_cl(x) for x in wide]
        px = _level_ptrs(wide)
        _lib.check(L.ia_groupnorm_stats_dt(C.byref(g), px, dt, ch, groups, _ptr(ws), nbytes, _stream()),
                   'ia_groupnorm_stats_dt')
        _lib.check(L.ia_groupnorm_apply_to_dt(C.byref(g), px, _level_ptrs(ys), dt, ch, groups, _ptr(gamma_),
                                              _ptr(beta_), eps, int(relu), _ptr(ws), nbytes, _ptr(saved),
                                              nsaved, _stream()), 'ia_groupnorm_apply_to_dt')
        ctx.geom, ctx.cfg, ctx.sizes, ctx.halves = g, (ch, groups, int(relu)), (nsaved, nbwd), halves
        ctx.save_for_backward(gamma, beta, saved, *wide)
        if halves == 2:
            F_ = ch // 2
            return tuple([y[:, :F_] for y in ys] + [y[:, F_:] for y in ys])
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        gamma, beta, saved = ctx.saved_tensors[:3]
        xs = ctx.saved_tensors[3:]
        ch, groups, relu = ctx.cfg
        nsaved, nbwd = ctx.sizes
        g, L, dev, dt = ctx.geom, _lib.lib(), xs[0].device, _lib.IA_BF16
        gamma_, beta_ = gamma.detach(), beta.detach()
        if ctx.halves == 2:
            # the two towers' gradients as one tensor per level: in place where they are the halves of
            # one (the next convolution node's input gradients are), one copy otherwise
            n = len(xs)
            dys = [_wide(a) if _halves_of_one(a, b) else torch.cat((a.to(torch.bfloat16), b.to(torch.bfloat16)), 1)
                   for a, b in zip(dys[:n], dys[n:])]
        dys = [_gn_upstream_bf16(d) for d in dys]
        ws = _gn_workspace(dev, nbwd)
        px, pdy = _level_ptrs(xs), _level_ptrs(dys)
        _lib.check(L.ia_groupnorm_bwd_reduce_dt(C.byref(g), px, pdy, dt, ch, groups, _ptr(gamma_), _ptr(beta_),
                                                relu, _ptr(saved), nsaved, _ptr(ws), nbwd, _stream()),
                   'ia_groupnorm_bwd_reduce_dt')
        need_x = any(ctx.needs_input_grad[6:])
        dxs = [_empty_cl(x) for x in xs] if need_x else None
        dgamma = torch.empty(ch, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dbeta = torch.empty(ch, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if need_x or dgamma is not None or dbeta is not None:
            _lib.check(L.ia_groupnorm_bwd_apply_dt(C.byref(g), px, pdy, _level_ptrs(dxs) if need_x else None,
                                                   dt, ch, groups, _ptr(gamma_), _ptr(beta_), relu,
                                                   _ptr(saved), nsaved, _ptr(ws), nbwd, _ptr(dgamma),
                                                   _ptr(dbeta), _stream()), 'ia_groupnorm_bwd_apply_dt')
        if not need_x:
            gx = (None,) * (ctx.halves * len(xs))
        elif ctx.halves == 2:
            F_ = ch // 2
            gx = tuple([d[:, :F_] for d in dxs] + [d[:, F_:] for d in dxs])
        else:
            gx = tuple(dxs)
        return (dgamma, dbeta, None, None, None, None) + gx


def groupnorm_bf16_supported(sizes, batch, channels, groups):
    """whether the bf16 GroupNorm training kernels cover per-level (H, W) sizes at this batch, channel
    and group count (the library's own answer: its workspace query; whole 16-byte columns inside a
    group, i.e. channels / groups % 8 == 0)"""
    g = winograd._wino_geom([tuple(int(v) for v in s) for s in sizes], int(batch))
    return _lib.lib().ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), int(channels), int(groups),
                                                          _lib.IA_BF16) != 0


def groupnorm_relu_bf16(xs, gamma, beta, groups, eps=1e-5, relu=True):
    """groupnorm_relu for bf16 training: xs[l] (B, ch, H_l, W_l) bf16 channels-last, gamma / beta (ch,)
    fp32 -> list of new bf16 channels-last tensors, y = bf16(relu?(float(x) * s + t)) with fp64
    statistics of the stored values (the bits of groupnorm_relu_ on a copy).  One autograd node with
    gradients for every x_l (bf16, rounded once), gamma and beta (fp32), for those that require them.
    The upstream gradient is read as it is when it is bf16 channels-last."""
    xs = list(xs)
    _gn_check('groupnorm_relu_bf16', xs, gamma, beta, torch.bfloat16, 'bf16')
    return list(_GroupNormReluBf16Fn.apply(gamma, beta, int(groups), float(eps), bool(relu), 1, *xs))


def groupnorm_relu_bf16_towers(xa, xb, gamma, beta, groups, eps=1e-5, relu=True):
    """two towers at once: xa[l] / xb[l] (B, F, H_l, W_l) bf16, gamma / beta (2F,) fp32 (the towers'
    parameters concatenated), groups = the sum of both towers' groups -> (ya, yb).  Where every level's
    xa[l] and xb[l] are the channel halves of one dense channels-last tensor (the bf16 convolution
    node's outputs) this is ONE node on the 2F-channel tensors whose outputs and input gradients are
    halves of one tensor again; otherwise one node per tower on contiguous copies."""
    xa, xb = list(xa), list(xb)
    if len(xa) != len(xb) or not xa or len(xa) > _lib.IA_MAX_LEVELS:
        raise ValueError('1..%d levels per tower' % _lib.IA_MAX_LEVELS)
    if all(_halves_of_one(a, b) for a, b in zip(xa, xb)):
        _gn_check('groupnorm_relu_bf16_towers', [_wide(a) for a in xa], gamma, beta, torch.bfloat16, 'bf16')
        out = _GroupNormReluBf16Fn.apply(gamma, beta, int(groups), float(eps), bool(relu), 2, *(xa + xb))
        return list(out[:len(xa)]), list(out[len(xa):])
    F_ = int(xa[0].shape[1])
    return tuple(groupnorm_relu_bf16([x.contiguous(memory_format=_CL) for x in xs], gamma[k * F_:(k + 1) * F_],
                                     beta[k * F_:(k + 1) * F_], int(groups) // 2, eps, relu)
                 for k, xs in enumerate((xa, xb)))


# ------------------------------------------------------------------ training
class PackedLabels(list):
    """per-level int64 label views (B, N_l) of point_targets, plus `.packed`: the int32 copy the
    loss node's focal kernel reads, written by the same launch"""
    packed = None


def point_loss_supported(geom, batch):
    """whether the training kernels cover this geometry and batch (level sizes whose packed labels
    the focal kernel can read in 16-byte pieces)"""
    g = geom.with_layout(_lib.IA_LAYOUT_NCHW)
    return _lib.lib().ia_point_head_loss_workspace_bytes(g.ref(), int(batch)) != 0


def point_targets(geom, gt_bboxes, gt_labels, regress_ranges):
    """fcos_target for a batch in one launch (ia_point_targets_ptrs).  gt_bboxes: list of (G_i, 4)
    device tensors, gt_labels: list of (G_i,) int64 tensors, 1 <= G_i <= 512, at most
    IA_MAX_TARGET_BATCH images; regress_ranges: L pairs (lo, hi).  -> (labels[L] (B, N_l) int64,
    bbox_targets[L] (B, N_l, 4) fp32, counts (B,) int32 positives per image): views of one
    allocation each, on the device, no host sync."""
    B = len(gt_bboxes)
    if B < 1 or len(gt_labels) != B:
        raise ValueError('one gt_labels tensor per image')
    for t in list(gt_bboxes) + list(gt_labels):
        _require_gpu(t, 'gt_bboxes / gt_labels')
    if len(regress_ranges) != geom.L:
        raise ValueError('one regress range per level')
    dev = gt_bboxes[0].device
    sizes = [int(g_.shape[0]) for g_ in gt_bboxes]
    L_ = _lib.lib()
    g = geom.with_layout(_lib.IA_LAYOUT_NCHW)
    n_packed = L_.ia_point_packed_labels_elems(g.ref(), B)
    if n_packed == 0 or B > _lib.IA_MAX_TARGET_BATCH or min(sizes) < 1 or max(sizes) > 512:
        raise _lib.IouAwareLibraryError(
            'ia_point_targets_ptrs: unsupported geometry, batch %d (1..%d) or gts per image %d..%d '
            '(1..512)' % (B, _lib.IA_MAX_TARGET_BATCH, min(sizes), max(sizes)))
    keep = [g_.to(dev, torch.float32).contiguous() for g_ in gt_bboxes]
    keep_l = [l_.to(dev, torch.int64).contiguous() for l_ in gt_labels]
    gp = (C.c_void_p * B)(*[g_.data_ptr() for g_ in keep])
    lp = (C.c_void_p * B)(*[l_.data_ptr() for l_ in keep_l])
    ng = (C.c_int32 * B)(*sizes)
    rr = (C.c_float * (2 * geom.L))(*[float(v) for r in regress_ranges for v in r])
    N = geom.N
    labels = torch.empty(B * N, dtype=torch.int64, device=dev)
    bt = torch.empty(B * N * 4, dtype=torch.float32, device=dev)
    packed = torch.empty(int(n_packed), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(L_.ia_point_targets_ptrs(g.ref(), gp, lp, ng, B, rr, _ptr(labels), _ptr(bt),
                                        _ptr(packed), _ptr(counts), _stream()),
               'ia_point_targets_ptrs')
    out_l, out_t = PackedLabels(), []
    off = 0
    for n_l in geom.level_points:
        out_l.append(labels[B * off:B * (off + n_l)].view(B, n_l))
        out_t.append(bt[4 * B * off:4 * B * (off + n_l)].view(B, n_l, 4))
        off += n_l
    out_l.packed = packed
    return out_l, out_t, counts


class _PointHeadLossFn(torch.autograd.Function):
    """the three / four FCOS losses of every level (csrc/pointloss.hip): 3 launches forward (4
    without packed labels), 2 backward.  Outputs: four (1,) views of one result vector
    (loss_cls, loss_reg, loss_centerness, loss_iou)."""

    @staticmethod
    def forward(ctx, geom, targets, cfg, with_iou, *outs):
        L = geom.L
        if len(outs) != (4 if with_iou else 3) * L:
            raise AssertionError('expected %d head outputs' % ((4 if with_iou else 3) * L))
        for t in outs:
            _require_gpu(t, 'head output')
            if t.dtype != torch.float32:
                raise TypeError('the point-head loss takes fp32 head outputs')
        maps = [[t.contiguous() for t in outs[k * L:(k + 1) * L]] for k in range(len(outs) // L)]
        B, dev = maps[0][0].shape[0], maps[0][0].device
        for l in range(L):
            h, w = geom.featmap_sizes[l]
            for m, ch in zip(maps, (geom.C, 4, 1, 1)):
                if tuple(m[l].shape) != (B, ch, h, w):
                    raise AssertionError('level %d: head output of shape %s, expected %s'
                                         % (l, tuple(m[l].shape), (B, ch, h, w)))
        labels, bbox_targets, counts = targets
        packed = getattr(labels, 'packed', None)
        labels = [t.contiguous().to(torch.int64) for t in labels]
        bbox_targets = [t.contiguous().to(torch.float32) for t in bbox_targets]
        for t in labels + bbox_targets:
            _require_gpu(t, 'targets')
        p, pt = PointLevelPtrs(), _lib.PointTargets()
        for l in range(L):
            p.cls[l], p.reg[l], p.ctr[l] = (m[l].data_ptr() for m in maps[:3])
            p.iou[l] = maps[3][l].data_ptr() if with_iou else None
            pt.labels[l], pt.bbox_targets[l] = labels[l].data_ptr(), bbox_targets[l].data_ptr()
        pt.packed = packed.data_ptr() if packed is not None else None
        pt.counts = counts.data_ptr() if counts is not None else None
        pc = _lib.PointLossCfg(*cfg)
        g = geom.with_layout(_lib.IA_LAYOUT_NCHW)
        nbytes = _lib.lib().ia_point_head_loss_workspace_bytes(g.ref(), B)
        if nbytes == 0:
            raise _lib.IouAwareLibraryError('unsupported geometry / batch for ia_point_head_loss')
        # own buffer: it carries the normalisers (and packed labels) from forward to backward
        ws = _own_workspace(dev, nbytes)
        res = torch.empty(6, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ia_point_head_loss_fwd(g.ref(), C.byref(p), B, C.byref(pt),
                                                     C.byref(pc), _ptr(ws), nbytes, _ptr(res),
                                                     _stream()), 'ia_point_head_loss_fwd')
        ctx.ws, ctx.res, ctx.geom, ctx.cfg, ctx.B = ws, res, g, pc, B
        ctx.keep = (maps, p, pt, (labels, bbox_targets, counts, packed))
        ctx.set_materialize_grads(False)
        return tuple(res[:4].view(4, 1).unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        maps, p, pt, _ = ctx.keep
        L, dev = ctx.geom.L, maps[0][0].device
        z = _zero1(dev)
        gin = torch.cat([z if g is None else g.detach().reshape(1).to(torch.float32) for g in gs])
        grads = [[torch.empty(t.shape, dtype=torch.float32, device=dev) for t in m] for m in maps]
        gp = PointLevelPtrs()
        for l in range(L):
            gp.cls[l], gp.reg[l], gp.ctr[l] = (m[l].data_ptr() for m in grads[:3])
            gp.iou[l] = grads[3][l].data_ptr() if len(grads) == 4 else None
        _lib.check(_lib.lib().ia_point_head_loss_bwd(ctx.geom.ref(), C.byref(p), ctx.B,
                                                     C.byref(pt), C.byref(ctx.cfg), _ptr(ctx.ws),
                                                     _ptr(ctx.res), _ptr(gin), C.byref(gp),
                                                     _stream()), 'ia_point_head_loss_bwd')
        return (None, None, None, None) + tuple(g for m in grads for g in m)


def point_head_loss(geom, cls, reg, ctr, iou, labels, bbox_targets, counts, gamma=2.0, alpha=0.25,
                    attach_iou_target=True, exact_large_logits=False):
    """Loss of the FCOS heads for all levels (ia_point_head_loss_*).  cls / reg / ctr / iou: per-level
    fp32 NCHW device tensors (reg = the exponentiated distances; iou = None: plain FCOS); labels /
    bbox_targets / counts as point_targets returns them (counts may be None).  -> dict of (1,)
    tensors with the reference's keys loss_cls, loss_reg, loss_centerness [, loss_iou]."""
    with_iou = iou is not None
    outs = list(cls) + list(reg) + list(ctr) + (list(iou) if with_iou else [])
    for t in outs:
        _require_gpu(t, 'head output')
    cfg = (float(gamma), float(alpha), int(bool(attach_iou_target)), int(bool(exact_large_logits)))
    res = _PointHeadLossFn.apply(geom, (labels, bbox_targets, counts), cfg, with_iou, *outs)
    losses = dict(loss_cls=res[0], loss_reg=res[1], loss_centerness=res[2])
    if with_iou:
        losses['loss_iou'] = res[3]
    return losses


# ------------------------------------------------------------------ the loss on packed channels-last rows
def point_loss_packed_supported(geom, batch):
    """whether the channels-last loss kernels cover this geometry and batch (C % 4 == 0)"""
    return _lib.lib().ia_point_head_loss_nhwc_workspace_bytes(geom.ref(), int(batch)) != 0


def _packed_rows(geom, cls_ctr, reg_iou, with_iou):
    """the argument contract of point_head_loss_packed, checked before the device is touched
    -> (batch, dtype)"""
    L = geom.L
    if len(cls_ctr) != L or len(reg_iou) != L:
        raise ValueError('point_head_loss_packed: expected %d levels, got %d / %d'
                         % (L, len(cls_ctr), len(reg_iou)))
    dtype = cls_ctr[0].dtype
    if dtype not in _DTYPES or any(t.dtype != dtype for t in list(cls_ctr) + list(reg_iou)):
        raise TypeError('point_head_loss_packed takes fp32 or bf16 rows, all of one dtype')
    B = cls_ctr[0].shape[0] if cls_ctr[0].dim() == 4 else -1
    for l in range(L):
        h, w = geom.featmap_sizes[l]
        for name, t, need in (('cls_ctr', cls_ctr[l], geom.C + 1), ('reg_iou', reg_iou[l], 5 if with_iou else 4)):
            if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (h, w):
                raise ValueError('%s level %d has shape %s, expected (%d, width, %d, %d)'
                                 % (name, l, tuple(t.shape), B, h, w))
            if t.shape[1] < need:
                raise ValueError('%s level %d: a row of %d channels is too narrow for its maps (%d)'
                                 % (name, l, t.shape[1], need))
            if t.shape[1] % 4 or not t.is_contiguous(memory_format=_CL) \
                    or t.data_ptr() % (4 * t.element_size()):
                raise ValueError('%s level %d: rows must be dense channels-last, a multiple of 4 channels '
                                 'wide and aligned to 4 elements' % (name, l))
    for t in list(cls_ctr) + list(reg_iou):
        _require_gpu(t, 'packed head output')
    return B, dtype


def _packed_ptrs(geom, cls_ctr, reg_iou, with_iou):
    p, st = PointLevelPtrs(), PointPixStrides()
    es = cls_ctr[0].element_size()
    for l in range(geom.L):
        c, r = cls_ctr[l], reg_iou[l]
        p.cls[l], p.ctr[l] = c.data_ptr(), c.data_ptr() + geom.C * es
        p.reg[l], p.iou[l] = r.data_ptr(), (r.data_ptr() + 4 * es) if with_iou else None
        st.cls[l] = st.ctr[l] = int(c.shape[1])
        st.reg[l] = st.iou[l] = int(r.shape[1])
    return p, st


class _PointHeadLossPackedFn(torch.autograd.Function):
    """the FCOS losses of every level on the towers' own output rows (ia_point_head_loss_*_nhwc): 3
    launches forward, 3 backward.  Inputs: L rows [cls C | ctr | pad], L rows [reg 4 | iou? | pad] (the
    raw fcos_reg output: exp(scale_l * x) is formed in the kernels), L scales."""

    @staticmethod
    def forward(ctx, geom, targets, cfg, with_iou, *ins):
        L = geom.L
        cls_ctr, reg_iou, scales = list(ins[:L]), list(ins[L:2 * L]), list(ins[2 * L:])
        B, dtype = _packed_rows(geom, cls_ctr, reg_iou, with_iou)
        dev = cls_ctr[0].device
        labels, bbox_targets, counts = targets
        labels = [t.contiguous().to(torch.int64) for t in labels]
        bbox_targets = [t.contiguous().to(torch.float32) for t in bbox_targets]
        for t in labels + bbox_targets:
            _require_gpu(t, 'targets')
        pt = _lib.PointTargets()
        for l in range(L):
            pt.labels[l], pt.bbox_targets[l] = labels[l].data_ptr(), bbox_targets[l].data_ptr()
        pt.packed = None
        pt.counts = counts.data_ptr() if counts is not None else None
        p, st = _packed_ptrs(geom, cls_ctr, reg_iou, with_iou)
        pc = _lib.PointLossCfg(*cfg)
        sc = torch.cat([s.detach().reshape(1).to(torch.float32) for s in scales])
        nbytes = _lib.lib().ia_point_head_loss_nhwc_workspace_bytes(geom.ref(), B)
        if nbytes == 0:
            raise _lib.IouAwareLibraryError('unsupported geometry / batch for ia_point_head_loss_fwd_nhwc')
        ws = _own_workspace(dev, nbytes)   # carries the normalisers from forward to backward
        res = torch.empty(6, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ia_point_head_loss_fwd_nhwc(
            geom.ref(), C.byref(p), C.byref(st), _DTYPES[dtype], B, C.byref(pt), C.byref(pc), _ptr(sc),
            _ptr(ws), nbytes, _ptr(res), _stream()), 'ia_point_head_loss_fwd_nhwc')
        ctx.ws, ctx.res, ctx.geom, ctx.cfg, ctx.B, ctx.with_iou = ws, res, geom, pc, B, with_iou
        ctx.keep = (cls_ctr, reg_iou, sc, p, st, pt, (labels, bbox_targets, counts))
        ctx.scale_shapes = [tuple(s.shape) for s in scales]
        ctx.set_materialize_grads(False)
        return tuple(res[:4].view(4, 1).unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        cls_ctr, reg_iou, sc, p, st, pt, _ = ctx.keep
        geom, L, dev = ctx.geom, ctx.geom.L, cls_ctr[0].device
        z = _zero1(dev)
        gin = torch.cat([z if g is None else g.detach().reshape(1).to(torch.float32) for g in gs])
        # of the inputs' dtype, shape and memory format; the kernels write every channel (rows stated packed)
        g_cc = [torch.empty_like(t) for t in cls_ctr]
        g_ri = [torch.empty_like(t) for t in reg_iou]
        gp, gst = _packed_ptrs(geom, g_cc, g_ri, ctx.with_iou)
        g_sc = torch.empty(L, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ia_point_head_loss_bwd_nhwc(
            geom.ref(), C.byref(p), C.byref(st), _DTYPES[cls_ctr[0].dtype], ctx.B, C.byref(pt),
            C.byref(ctx.cfg), _ptr(sc), _ptr(ctx.ws), ctx.ws.numel(), _ptr(ctx.res), _ptr(gin),
            C.byref(gp), C.byref(gst), 1, _ptr(g_sc), _stream()), 'ia_point_head_loss_bwd_nhwc')
        g_scales = [g_sc[l:l + 1].reshape(shape) for l, shape in enumerate(ctx.scale_shapes)]
        return (None, None, None, None) + tuple(g_cc) + tuple(g_ri) + tuple(g_scales)


def point_head_loss_packed(geom, cls_ctr, reg_iou, scales, labels, bbox_targets, counts, gamma=2.0,
                           alpha=0.25, attach_iou_target=True, exact_large_logits=False, with_iou=True):
    """point_head_loss on the packed channels-last outputs of the HIP tower routes, consumed in place:
    cls_ctr[l] (B, wc, H_l, W_l) rows [cls C | centerness | padding], reg_iou[l] (B, wr, H_l, W_l) rows
    [raw fcos_reg 4 | iou (with_iou) | padding], fp32 or bf16 (one dtype), dense channels-last, any
    width that is a multiple of 4; scales: the L Scale parameters -- bbox_pred = exp(scale_l * reg) is
    formed inside the kernels.  One autograd node: its gradients are one tensor per packed input, of
    that input's dtype, shape and memory format with every channel written (zeros in the padding), and
    one fp32 gradient per scale.  -> the reference's loss dict (loss_iou with with_iou only).
    CPU tensors: IouAwareLibraryError; a mixed dtype: TypeError; a wrong level count, shape, layout or
    a row too narrow for its maps: ValueError -- all before the device is touched."""
    cls_ctr, reg_iou, scales = list(cls_ctr), list(reg_iou), list(scales)
    if len(scales) != geom.L:
        raise ValueError('point_head_loss_packed: expected %d scales, got %d' % (geom.L, len(scales)))
    _packed_rows(geom, cls_ctr, reg_iou, bool(with_iou))
    for s in scales:
        _require_gpu(s, 'scale')
        if s.numel() != 1:
            raise ValueError('point_head_loss_packed: one scalar scale per level')
    cfg = (float(gamma), float(alpha), int(bool(attach_iou_target)), int(bool(exact_large_logits)))
    res = _PointHeadLossPackedFn.apply(geom, (labels, bbox_targets, counts), cfg, bool(with_iou),
                                       *(cls_ctr + reg_iou + scales))
    losses = dict(loss_cls=res[0], loss_reg=res[1], loss_centerness=res[2])
    if with_iou:
        losses['loss_iou'] = res[3]
    return losses

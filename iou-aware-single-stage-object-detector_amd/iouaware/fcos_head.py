"""FCOS heads: plain FCOS (reference mmdet/models/anchor_heads/fcos_head.py) and IoU-aware FCOS
(reference mmdet/models/anchor_heads/iou_aware_fcos_head.py), with the reference's registry names,
constructor kwargs, parameter names and method signatures.

  * forward / forward_single: the 4 + 4 GN towers and the output convolutions as PyTorch
    modules.  In training with `train_winograd = True` (opt-in; where
    winograd_train.fcos_usable holds) forward instead runs every tower convolution as one
    Winograd autograd node over all levels and every GroupNorm + ReLU as one HIP node with a HIP
    backward (fcos_ops.groupnorm_relu); with `train_bf16 = True` (opt-in, tried first; where
    conv3x3_bf16_train.fcos_usable holds) the towers run in bf16 on the MFMA convolution node
    and the bf16 GroupNorm node (fcos_ops.groupnorm_relu_bf16); at inference `fuse.fuse_inference(winograd=True)` swaps
    in the Winograd runner with the in-place HIP GroupNorm + ReLU (winograd.WinogradFCOSHead)
    and, for bf16 channels-last features, the MFMA convolution towers with the bf16 GroupNorm +
    ReLU (conv3x3_bf16.Bf16ConvFCOSHead);
  * get_bboxes: one call into the HIP library for the whole batch (row max, per-level top-k,
    distance2bbox, batched NMS): ia_point_get_bboxes with the fused alpha score (IoU-aware),
    ia_point_ctr_get_bboxes with the raw-threshold / centerness-product scores (plain); fp32 or
    bf16 maps (the _dt entries);
  * loss: point targets and all terms of every level on HIP kernels (fcos_ops.point_targets,
    fcos_ops.point_head_loss: csrc/pointloss.hip), no host synchronisation; `fuse_loss = False`, or
    inputs the node does not cover (see _fused_loss_ok), take the torch transcription of the
    reference with the class term through the HIP sigmoid focal-loss op.
  * forward_loss (opt-in, `fuse_head_loss = True`): forward + loss as one call; on the two HIP tower
    routes the packed channels-last outputs of the output convolutions go straight into the loss
    node (fcos_ops.point_head_loss_packed), exp(scale * x) inside it.
There is no CPU fallback for get_bboxes / loss: they need tensors on a gfx950 device.

Both heads are `_FCOSHeadBase` with the class attribute `iou_branch` (fcos_iou present or absent):
layers, forward, targets, the loss body (`_loss`) and the decode call (`_get_bboxes_batched`) are
written once; the two classes keep the reference's differing public signatures.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fcos_ops
from .bbox import bbox_overlaps, distance2bbox, multi_apply, per_image
from .focal_op import sigmoid_focal_loss
from .layers import ConvModule, Scale, bias_init_with_prob, normal_init
from .losses import iou_loss
from .registry import HEADS

INF = 1e8


class _FCOSHeadBase(nn.Module):
    """what the two FCOS heads share: constructor, points, targets, the flattened loss inputs and
    the point geometry of the HIP decode"""
    # the geometry's score_alpha (ia_point_head_geom); the plain head's entries ignore it
    score_alpha = 0.3

    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4,
                 strides=(4, 8, 16, 32, 64),
                 regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)),
                 conv_cfg=None, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)):
        super(_FCOSHeadBase, self).__init__()
        self.num_classes = num_classes
        self.cls_out_channels = num_classes - 1
        self.in_channels = in_channels
        self.feat_channels = feat_channels
        self.stacked_convs = stacked_convs
        self.strides = strides
        self.regress_ranges = regress_ranges
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        self._init_layers()

    iou_branch = False                    # IoUawareFCOSHead: fcos_iou on the reg tower

    def _init_layers(self):
        """the GN towers, fcos_cls / fcos_centerness / fcos_reg [/ fcos_iou] and the scales, in
        the reference's order"""
        self.cls_convs = nn.ModuleList()
        self.reg_convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            for convs in (self.cls_convs, self.reg_convs):
                convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                                        conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                                        bias=self.norm_cfg is None))
        self.fcos_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)
        self.fcos_centerness = nn.Conv2d(self.feat_channels, 1, 3, padding=1)
        self.fcos_reg = nn.Conv2d(self.feat_channels, 4, 3, padding=1)
        if self.iou_branch:
            self.fcos_iou = nn.Conv2d(self.feat_channels, 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])

    def init_weights(self):
        for m in self.cls_convs:
            normal_init(m.conv, std=0.01)
        for m in self.reg_convs:
            normal_init(m.conv, std=0.01)
        normal_init(self.fcos_cls, std=0.01, bias=bias_init_with_prob(0.01))
        normal_init(self.fcos_reg, std=0.01)
        normal_init(self.fcos_centerness, std=0.01)
        if self.iou_branch:
            normal_init(self.fcos_iou, std=0.01)

    # training: all-levels Winograd towers + HIP GroupNorm when set and usable.  Off by default (the
    # whole-iteration comparison against the module route: DESIGN 3.17, "Whole FCOS training iterations")
    train_winograd = False
    # training: bf16 activations on the MFMA convolution kernels and the bf16 GroupNorm node, fp32
    # master weights (conv3x3_bf16_train.fcos_head_forward).  Off by default: it changes the
    # training numerics
    train_bf16 = False

    def forward(self, feats):
        """-> (cls_scores[L], bbox_preds[L] (exponentiated distances), centernesses[L][, ious[L]]).
        With `train_winograd = True`, in training on a ROCm device every tower convolution runs once for all levels on the
        Winograd path and every GroupNorm + ReLU as one HIP node, each with its own backward
        (winograd_train.fcos_head_forward) -- same parameters, same outputs to fp32 rounding.
        `train_bf16 = True` is tried first: the same towers in bf16 (conv3x3_bf16_train.
        fcos_head_forward), fp32 maps out; what it does not cover takes the next route."""
        if self.training and self.train_bf16:
            from . import conv3x3_bf16_train
            if conv3x3_bf16_train.fcos_usable(feats, self):
                return conv3x3_bf16_train.fcos_head_forward(self, feats)
        if self.training and self.train_winograd:
            from . import winograd_train
            if winograd_train.fcos_usable(feats, self):
                return winograd_train.fcos_head_forward(self, feats)
        return multi_apply(self.forward_single, feats, self.scales)

    def forward_single(self, x, scale):
        cls_feat = x
        reg_feat = x
        for cls_layer in self.cls_convs:
            cls_feat = cls_layer(cls_feat)
        cls_score = self.fcos_cls(cls_feat)
        centerness = self.fcos_centerness(cls_feat)
        for reg_layer in self.reg_convs:
            reg_feat = reg_layer(reg_feat)
        bbox_pred = scale(self.fcos_reg(reg_feat)).exp()
        if not self.iou_branch:
            return cls_score, bbox_pred, centerness
        return cls_score, bbox_pred, centerness, self.fcos_iou(reg_feat)

    # ------------------------------------------------------------------ points / targets
    def get_points(self, featmap_sizes, dtype, device):
        return [self.get_points_single(featmap_sizes[i], self.strides[i], dtype, device)
                for i in range(len(featmap_sizes))]

    def get_points_single(self, featmap_size, stride, dtype, device):
        h, w = featmap_size
        x_range = torch.arange(0, w * stride, stride, dtype=dtype, device=device)
        y_range = torch.arange(0, h * stride, stride, dtype=dtype, device=device)
        y, x = torch.meshgrid(y_range, x_range, indexing='ij')
        return torch.stack((x.reshape(-1), y.reshape(-1)), dim=-1) + stride // 2

    def fcos_target(self, points, gt_bboxes_list, gt_labels_list):
        """-> (labels[L], bbox_targets[L]), each level's rows image-major (num_imgs * N_l)"""
        if len(points) != len(self.regress_ranges):
            raise AssertionError('one regress range per level')
        num_levels = len(points)
        expanded = [points[i].new_tensor(self.regress_ranges[i])[None].expand_as(points[i])
                    for i in range(num_levels)]
        concat_ranges = torch.cat(expanded, dim=0)
        concat_points = torch.cat(points, dim=0)
        labels_list, bbox_targets_list = multi_apply(
            self.fcos_target_single, gt_bboxes_list, gt_labels_list, points=concat_points,
            regress_ranges=concat_ranges)
        num_points = [center.size(0) for center in points]
        labels_list = [labels.split(num_points, 0) for labels in labels_list]
        bbox_targets_list = [t.split(num_points, 0) for t in bbox_targets_list]
        lvl_labels = [torch.cat([labels[i] for labels in labels_list]) for i in range(num_levels)]
        lvl_targets = [torch.cat([t[i] for t in bbox_targets_list]) for i in range(num_levels)]
        return lvl_labels, lvl_targets

    def fcos_target_single(self, gt_bboxes, gt_labels, points, regress_ranges):
        """each point -> the gt of minimal area that contains it (strictly) with its largest
        distance inside the level's range (both ends inclusive); label 0 = background"""
        num_points = points.size(0)
        num_gts = gt_labels.size(0)
        areas = (gt_bboxes[:, 2] - gt_bboxes[:, 0] + 1) * (gt_bboxes[:, 3] - gt_bboxes[:, 1] + 1)
        areas = areas[None].repeat(num_points, 1)
        regress_ranges = regress_ranges[:, None, :].expand(num_points, num_gts, 2)
        gt_bboxes = gt_bboxes[None].expand(num_points, num_gts, 4)
        xs = points[:, 0][:, None].expand(num_points, num_gts)
        ys = points[:, 1][:, None].expand(num_points, num_gts)
        left = xs - gt_bboxes[..., 0]
        right = gt_bboxes[..., 2] - xs
        top = ys - gt_bboxes[..., 1]
        bottom = gt_bboxes[..., 3] - ys
        bbox_targets = torch.stack((left, top, right, bottom), -1)
        inside_gt_bbox_mask = bbox_targets.min(-1)[0] > 0
        max_regress_distance = bbox_targets.max(-1)[0]
        inside_regress_range = (max_regress_distance >= regress_ranges[..., 0]) & \
                               (max_regress_distance <= regress_ranges[..., 1])
        areas[inside_gt_bbox_mask == 0] = INF
        areas[inside_regress_range == 0] = INF
        min_area, min_area_inds = areas.min(dim=1)
        labels = gt_labels[min_area_inds]
        labels[min_area == INF] = 0
        bbox_targets = bbox_targets[range(num_points), min_area_inds]
        return labels, bbox_targets

    def centerness_target(self, pos_bbox_targets):
        left_right = pos_bbox_targets[:, [0, 2]]
        top_bottom = pos_bbox_targets[:, [1, 3]]
        c = (left_right.min(dim=-1)[0] / left_right.max(dim=-1)[0]) * \
            (top_bottom.min(dim=-1)[0] / top_bottom.max(dim=-1)[0])
        return torch.sqrt(c)

    # ------------------------------------------------------------------ training
    # targets and loss on the HIP kernels of csrc/pointloss.hip where they apply (_fused_loss_ok)
    fuse_loss = True

    def _fused_targets_ok(self, L, B, gt_bboxes, gt_labels, cfg):
        """what the HIP target and loss kernels cover whatever the maps' layout: gamma 2, at most 8
        levels, 1..512 gts per image on the device, at most 16 images"""
        if not 1 <= L <= fcos_ops._lib.IA_MAX_LEVELS or L != len(self.strides):
            return False
        if float(cfg.gamma) != 2.0:
            return False
        if not 1 <= B <= fcos_ops._lib.IA_MAX_TARGET_BATCH or len(gt_bboxes) != B or len(gt_labels) != B:
            return False
        for b, l in zip(gt_bboxes, gt_labels):
            if not (b.is_cuda and l.is_cuda) or not 1 <= b.size(0) <= 512 or l.size(0) != b.size(0):
                return False
        return True

    def _fused_loss_ok(self, maps, gt_bboxes, gt_labels, cfg):
        """what the HIP node covers: fp32 NCHW-contiguous device maps, gamma 2, at most 8 levels,
        1..512 gts per image, at most 16 images"""
        if not maps[0] or not self._fused_targets_ok(len(maps[0]), maps[0][0].size(0), gt_bboxes, gt_labels, cfg):
            return False
        for t in [t for m in maps for t in m]:
            if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
                return False
        return True

    # training: towers, output convolutions, point targets and the loss node on the packed channels-last
    # rows with nothing in between (forward_loss).  Off by default: see DESIGN 3.17 for what it buys
    fuse_head_loss = False

    def _packed_route(self, feats):
        """the HIP tower route that produces packed rows for these features (its
        fcos_head_forward_packed), or None"""
        if not self.training:
            return None
        if self.train_bf16:
            from . import conv3x3_bf16_train
            if conv3x3_bf16_train.fcos_usable(feats, self):
                return conv3x3_bf16_train.fcos_head_forward_packed
        if self.train_winograd:
            from . import winograd_train
            if winograd_train.fcos_usable(feats, self):
                return winograd_train.fcos_head_forward_packed
        return None

    def forward_loss(self, feats, gt_bboxes, gt_labels, img_metas, cfg, gt_bboxes_ignore=None):
        """loss(*forward(feats), ...) -- the same dict.  With `fuse_head_loss = True`, in training on one
        of the two HIP tower routes and where the conditions of _fused_loss_ok hold (the dtype and
        layout being the route's own: fp32 or bf16 channels-last rows), the towers' packed outputs go
        straight into fcos_ops.point_head_loss_packed: no slice, no conversion, no Scale / exp node --
        exp(scale_l * reg) is formed in the loss kernels, which return the scales' gradients."""
        feats = list(feats)
        route = self._packed_route(feats) if (self.fuse_head_loss and self.fuse_loss and feats) else None
        if route is not None and self._fused_targets_ok(len(feats), feats[0].size(0), gt_bboxes,
                                                        gt_labels, cfg):
            B = feats[0].size(0)
            geom = self.geometry([tuple(x.shape[-2:]) for x in feats])
            if fcos_ops.point_loss_supported(geom, B) and fcos_ops.point_loss_packed_supported(geom, B):
                cls_ctr, reg_iou = route(self, feats)
                labels, bbox_targets, counts = fcos_ops.point_targets(geom, gt_bboxes, gt_labels,
                                                                      self.regress_ranges)
                return fcos_ops.point_head_loss_packed(
                    geom, cls_ctr, reg_iou, [s.scale for s in list(self.scales)[:geom.L]], labels,
                    bbox_targets, counts, cfg.gamma, cfg.alpha, with_iou=self.iou_branch)
        return self.loss(*self(feats), gt_bboxes, gt_labels, img_metas, cfg)

    def _loss(self, cls_scores, bbox_preds, centernesses, ious, gt_bboxes, gt_labels, cfg):
        """focal classification over (num_pos + num_imgs), the centerness-weighted IoU loss, the
        centerness BCE and, with the IoU branch, the IoU BCE whose target is
        NOT detached (as in the reference: its gradient reaches bbox_preds too)"""
        maps = (cls_scores, bbox_preds, centernesses) + ((ious,) if self.iou_branch else ())
        if len(set(len(m) for m in maps)) != 1:
            raise AssertionError('level count mismatch')
        geom = None
        if self.fuse_loss and self._fused_loss_ok(maps, gt_bboxes, gt_labels, cfg):
            geom = self.geometry([tuple(c.shape[-2:]) for c in cls_scores])
        if geom is not None and fcos_ops.point_loss_supported(geom, cls_scores[0].size(0)):
            labels, bbox_targets, counts = fcos_ops.point_targets(geom, gt_bboxes, gt_labels,
                                                                  self.regress_ranges)
            return fcos_ops.point_head_loss(geom, cls_scores, bbox_preds, centernesses,
                                            ious if self.iou_branch else None, labels,
                                            bbox_targets, counts, cfg.gamma, cfg.alpha)
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        all_level_points = self.get_points(featmap_sizes, bbox_preds[0].dtype, bbox_preds[0].device)
        labels, bbox_targets = self.fcos_target(all_level_points, gt_bboxes, gt_labels)
        num_imgs = cls_scores[0].size(0)
        # per-point flattened outputs of the batch (image-major inside a level)
        flat_cls = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
                              for c in cls_scores])
        flat_bbox = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds])
        flat_ctr = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in centernesses])
        flat_labels = torch.cat(labels)
        flat_bbox_targets = torch.cat(bbox_targets)
        flat_points = torch.cat([points.repeat(num_imgs, 1) for points in all_level_points])
        if self.iou_branch:
            flat_iou = torch.cat([i.permute(0, 2, 3, 1).reshape(-1) for i in ious])

        pos_inds = flat_labels.nonzero().reshape(-1)
        num_pos = len(pos_inds)
        loss_cls = sigmoid_focal_loss(flat_cls.contiguous(), flat_labels, cfg.gamma, cfg.alpha,
                                      'none').sum()[None] / (num_pos + num_imgs)
        pos_bbox_preds = flat_bbox[pos_inds]
        pos_bbox_targets = flat_bbox_targets[pos_inds]
        pos_centerness = flat_ctr[pos_inds]
        if self.iou_branch:
            pos_iou = flat_iou[pos_inds]
        pos_centerness_targets = self.centerness_target(pos_bbox_targets)
        if num_pos > 0:
            pos_points = flat_points[pos_inds]
            pos_decoded_bbox_preds = distance2bbox(pos_points, pos_bbox_preds)
            pos_decoded_target_preds = distance2bbox(pos_points, pos_bbox_targets)
            loss_reg = ((iou_loss(pos_decoded_bbox_preds, pos_decoded_target_preds,
                                  reduction='none') * pos_centerness_targets).sum() /
                        pos_centerness_targets.sum())[None]
            loss_centerness = F.binary_cross_entropy_with_logits(
                pos_centerness, pos_centerness_targets, reduction='mean')[None]
            if self.iou_branch:
                pos_iou_target = bbox_overlaps(pos_decoded_target_preds, pos_decoded_bbox_preds,
                                               is_aligned=True)
                loss_iou = F.binary_cross_entropy_with_logits(pos_iou, pos_iou_target,
                                                              reduction='mean')[None]
        else:
            loss_reg = pos_bbox_preds.sum()[None]
            loss_centerness = pos_centerness.sum()[None]
            if self.iou_branch:
                loss_iou = pos_iou.sum()[None]
        losses = dict(loss_cls=loss_cls, loss_reg=loss_reg, loss_centerness=loss_centerness)
        if self.iou_branch:
            losses['loss_iou'] = loss_iou
        return losses

    # ------------------------------------------------------------------ inference
    def geometry(self, featmap_sizes, nms_pre=-1):
        key = (tuple(tuple(int(v) for v in s) for s in featmap_sizes), int(nms_pre))
        cache = self.__dict__.setdefault('_geom_cache', {})
        g = cache.get(key)
        if g is None:
            g = cache[key] = fcos_ops.PointGeometry(key[0], self.strides[:len(featmap_sizes)],
                                                    self.cls_out_channels, nms_pre,
                                                    self.score_alpha)
        return g

    def _get_bboxes_batched(self, cls_scores, bbox_preds, third, img_metas, cfg, rescale):
        """third: the maps of the decode's third slot -- ious with the IoU branch (fused alpha
        score), centernesses without (score = sigmoid(cls) * sigmoid(centerness))"""
        if not len(cls_scores) == len(bbox_preds) == len(third) == len(self.strides):
            raise AssertionError('level count mismatch')
        nms_cfg = dict(cfg.nms)
        nms_type = nms_cfg.pop('type', 'nms')
        if nms_type != 'nms':
            raise NotImplementedError('%s: test_cfg.nms.type %r (hard NMS only)'
                                      % (type(self).__name__, nms_type))
        featmap_sizes = [tuple(c.shape[-2:]) for c in cls_scores]
        geom = self.geometry(featmap_sizes, cfg.get('nms_pre', -1))
        shapes = [m['img_shape'] for m in img_metas]
        factors = [m['scale_factor'] for m in img_metas]
        entry = fcos_ops.point_get_bboxes if self.iou_branch else fcos_ops.point_ctr_get_bboxes
        return entry(geom, [c.detach() for c in cls_scores], [b.detach() for b in bbox_preds],
                     [t.detach() for t in third], shapes, factors, rescale, cfg.score_thr,
                     nms_cfg['iou_thr'], cfg.max_per_img)


@HEADS.register_module
class IoUawareFCOSHead(_FCOSHeadBase):
    # score = sigmoid(cls) ** alpha * sigmoid(iou) ** (1 - alpha), hard-coded in the reference
    # (iou_aware_fcos_head.py:326)
    score_alpha = 0.3
    iou_branch = True

    def loss(self, cls_scores, bbox_preds, centernesses, ious, gt_bboxes, gt_labels, img_metas,
             cfg, gt_bboxes_ignore=None):
        """the reference's four terms (iou_aware_fcos_head.py:121-244)"""
        return self._loss(cls_scores, bbox_preds, centernesses, ious, gt_bboxes, gt_labels, cfg)

    def get_bboxes_batched(self, cls_scores, bbox_preds, centernesses, ious, img_metas, cfg,
                           rescale=False):
        """Device-side result of the whole batch: dets (B,max,5), labels (B,max) int32,
        rows (B,max) int32, num (B) int32 -- no host synchronisation.  Centerness is not used
        (the reference has its use commented out, iou_aware_fcos_head.py:350-370)."""
        return self._get_bboxes_batched(cls_scores, bbox_preds, ious, img_metas, cfg, rescale)

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, ious, gt_bboxes, gt_labels,
                   img_metas, cfg, rescale=None):
        """-> list over images of (det_bboxes (k,5) fp32, det_labels (k,) int64)"""
        return per_image(*self.get_bboxes_batched(cls_scores, bbox_preds, centernesses, ious,
                                                  img_metas, cfg, rescale))


@HEADS.register_module
class FCOSHead(_FCOSHeadBase):
    """plain FCOS (reference fcos_head.py): centerness on the cls tower, no IoU branch; at
    inference the raw class score is thresholded and NMS ranks sigmoid(cls) * sigmoid(centerness)
    (multiclass_nms with score_factors, bbox_nms.py:37-48)"""

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, cfg,
             gt_bboxes_ignore=None):
        """the reference's three terms (fcos_head.py:105-191)"""
        return self._loss(cls_scores, bbox_preds, centernesses, None, gt_bboxes, gt_labels, cfg)

    def get_bboxes_batched(self, cls_scores, bbox_preds, centernesses, img_metas, cfg,
                           rescale=False):
        """Device-side result of the whole batch: dets (B,max,5) (score = sigmoid(cls) *
        sigmoid(centerness)), labels (B,max) int32, rows (B,max) int32, num (B) int32 -- no host
        synchronisation."""
        return self._get_bboxes_batched(cls_scores, bbox_preds, centernesses, img_metas, cfg,
                                        rescale)

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg, rescale=None):
        """-> list over images of (det_bboxes (k,5) fp32, det_labels (k,) int64)"""
        return per_image(*self.get_bboxes_batched(cls_scores, bbox_preds, centernesses, img_metas,
                                                  cfg, rescale))

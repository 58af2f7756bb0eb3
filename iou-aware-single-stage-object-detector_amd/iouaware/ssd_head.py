"""SSD head (reference mmdet/models/anchor_heads/ssd_head.py on anchor_head.py): inference and training,
with the reference's registry name, constructor arguments, parameter names (`reg_convs.N`,
`cls_convs.N`) and method signatures, so that a reference checkpoint loads.

  * anchors: the reference's min_sizes / max_sizes table (its four basesize_ratio_range special
    cases), per level scales [1, sqrt(max / min)], ratios [1, 1/r, r, ...], scale_major=False, centre
    ((stride - 1) / 2, (stride - 1) / 2), and the reorder that moves the large square next to the
    small one -- on this build's anchors.AnchorGenerator.  4 or 6 anchors per location.
  * forward: one 3x3 convolution per level and branch, on torch modules.
  * get_bboxes: one call into the HIP library for the whole batch (ia_ssd_get_bboxes: softmax row
    scores, compaction of the rows above score_thr, decode, batched NMS).  SSD has no nms_pre: all
    8 732 (SSD300) / 24 564 (SSD512) rows are candidates; the batched NMS holds IA_MAX_CANDIDATES rows
    ABOVE score_thr per image.  A batch with an image beyond that goes through the per-class route
    (ssd_ops.ssd_get_bboxes_per_class) when check_overflow is on; otherwise the flags stay in
    `self.overflow` and such an image has zero detections.
  * loss: targets from targets.anchor_target (MaxIoUAssigner as the configs set it, torch ops), then per
    image the softmax cross-entropy with hard-negative mining (train_cfg.neg_pos_ratio) and smooth-L1
    (train_cfg.smoothl1_beta).  `fuse_loss = True` (the default; measured faster in every alternating
    pair): the HIP node ssd_ops.ssd_head_loss (csrc/ssdloss.hip) on the NCHW maps in place:
    2 launches forward, 1 backward, no host synchronisation, the same bits in every run; among equal
    losses at the mining threshold it takes the lowest row ids (torch's topk leaves that choice open;
    the loss value does not depend on it).  `fuse_loss = False`: the torch transcription of the
    reference's loss_single, on any device -- the fallback and the yardstick's twin.
    The reference's dormant IoU_balanced_* branches (hard-coded off there) are not built.
Softmax classification (use_sigmoid_cls = False, channel 0 = background), hard NMS, fp32.  There is no
CPU fallback for get_bboxes or the fused loss: they need tensors on a gfx950 device.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ssd_ops
from .anchors import AnchorGenerator
from .bbox import per_image
from .layers import xavier_init
from .registry import HEADS
from .targets import anchor_target


def ssd_anchor_sizes(input_size, basesize_ratio_range, num_levels):
    """-> (min_sizes, max_sizes), one entry per level: the sizes step evenly (in whole percent of the
    input size) from the lower to the upper ratio over the levels 1 .. L-1, and level 0 gets the
    published special value of the four (input size, lower ratio) settings"""
    lo, hi = int(basesize_ratio_range[0] * 100), int(basesize_ratio_range[1] * 100)
    step = int(np.floor(hi - lo) / (num_levels - 2))
    min_sizes = [int(input_size * r / 100) for r in range(lo, hi + 1, step)]
    max_sizes = [int(input_size * (r + step) / 100) for r in range(lo, hi + 1, step)]
    first = {(300, 0.15): (7, 15), (300, 0.2): (10, 20), (512, 0.1): (4, 10), (512, 0.15): (7, 15)}
    pct = first.get((input_size, basesize_ratio_range[0]))
    if pct is not None:
        min_sizes.insert(0, int(input_size * pct[0] / 100))
        max_sizes.insert(0, int(input_size * pct[1] / 100))
    return min_sizes, max_sizes


@HEADS.register_module
class SSDHead(nn.Module):
    """SSD head."""

    fuse_loss = True                         # the HIP loss node (device tensors only); False: torch ops, any device

    def __init__(self, input_size=300, num_classes=81, in_channels=(512, 1024, 512, 256, 256, 256),
                 anchor_strides=(8, 16, 32, 64, 100, 300), basesize_ratio_range=(0.1, 0.9),
                 anchor_ratios=([2], [2, 3], [2, 3], [2, 3], [2], [2]), target_means=(.0, .0, .0, .0),
                 target_stds=(1.0, 1.0, 1.0, 1.0)):
        super(SSDHead, self).__init__()
        self.input_size = input_size
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.cls_out_channels = num_classes
        self.num_anchors = [len(ratios) * 2 + 2 for ratios in anchor_ratios]
        self.reg_convs = nn.ModuleList(nn.Conv2d(c, a * 4, kernel_size=3, padding=1)
                                       for c, a in zip(in_channels, self.num_anchors))
        self.cls_convs = nn.ModuleList(nn.Conv2d(c, a * num_classes, kernel_size=3, padding=1)
                                       for c, a in zip(in_channels, self.num_anchors))
        min_sizes, max_sizes = ssd_anchor_sizes(input_size, basesize_ratio_range, len(in_channels))
        self.anchor_strides = anchor_strides
        self.anchor_generators = []
        for k, stride in enumerate(anchor_strides):
            ratios = [1.]
            for r in anchor_ratios[k]:
                ratios += [1 / r, r]
            gen = AnchorGenerator(min_sizes[k], [1., np.sqrt(max_sizes[k] / min_sizes[k])], ratios,
                                  scale_major=False, ctr=((stride - 1) / 2., (stride - 1) / 2.))
            # scale-minor order is [small x ratios..., large x ratios...]: keep the small scale's anchors,
            # with the large square (the first of the second block) moved behind the small square
            order = list(range(len(ratios)))
            order.insert(1, len(order))
            gen.base_anchors = torch.index_select(gen.base_anchors, 0, torch.LongTensor(order))
            self.anchor_generators.append(gen)
        self.target_means = target_means
        self.target_stds = target_stds
        self.use_sigmoid_cls = False
        self.cls_focal_loss = False
        self.overflow = None                     # the (B,) int32 flags of the last batched get_bboxes
        self._geom_cache = {}

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                xavier_init(m, distribution='uniform', bias=0)

    def forward(self, feats):
        """-> (cls_scores[L], bbox_preds[L])"""
        cls_scores = [conv(x) for x, conv in zip(feats, self.cls_convs)]
        bbox_preds = [conv(x) for x, conv in zip(feats, self.reg_convs)]
        return cls_scores, bbox_preds

    # ------------------------------------------------------------------ training
    def get_anchors(self, featmap_sizes, img_metas, device='cpu'):
        """anchors once per batch, valid flags per image from pad_shape and the stride
        (reference anchor_head.py get_anchors)"""
        levels = [self.anchor_generators[i].grid_anchors(featmap_sizes[i], self.anchor_strides[i], device=device)
                  for i in range(len(featmap_sizes))]
        anchor_list = [list(levels) for _ in img_metas]
        valid_flag_list = []
        for meta in img_metas:
            h, w = meta['pad_shape'][:2]
            flags = []
            for i, (fh, fw) in enumerate(featmap_sizes):
                s = self.anchor_strides[i]
                vh, vw = min(int(np.ceil(h / s)), int(fh)), min(int(np.ceil(w / s)), int(fw))
                flags.append(self.anchor_generators[i].valid_flags((fh, fw), (vh, vw), device=device))
            valid_flag_list.append(flags)
        return anchor_list, valid_flag_list

    def loss_single(self, cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights,
                    num_total_samples, cfg):
        """one image, torch ops (the reference's loss_single with its IoU_balanced_* switches off):
        cls_score (R, C + 1), bbox_pred (R, 4) -> loss_cls (1,), loss_bbox (1,)"""
        loss_cls_all = F.cross_entropy(cls_score, labels, reduction='none') * label_weights
        pos_inds = (labels > 0).nonzero().view(-1)
        neg_inds = (labels == 0).nonzero().view(-1)
        num_neg = min(cfg.neg_pos_ratio * pos_inds.size(0), neg_inds.size(0))
        topk_loss_cls_neg, _ = loss_cls_all[neg_inds].topk(num_neg)
        loss_cls = (loss_cls_all[pos_inds].sum() + topk_loss_cls_neg.sum()) / num_total_samples
        beta = cfg.smoothl1_beta
        diff = torch.abs(bbox_pred - bbox_targets)
        loss = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
        loss_bbox = torch.sum(loss * bbox_weights)[None] / num_total_samples
        return loss_cls[None], loss_bbox

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, cfg, gt_bboxes_ignore=None):
        """-> dict(loss_cls=[B tensors (1,)], loss_bbox=[B tensors (1,)]), or None when an image has no
        valid anchor (the reference's structure)"""
        featmap_sizes = [tuple(int(v) for v in f.shape[-2:]) for f in cls_scores]
        if len(featmap_sizes) != len(self.anchor_generators):
            raise AssertionError('expected %d levels' % len(self.anchor_generators))
        device = cls_scores[0].device
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=device)
        cls_reg_targets = anchor_target(anchor_list, valid_flag_list, gt_bboxes, img_metas, self.target_means,
                                        self.target_stds, cfg, gt_bboxes_ignore_list=gt_bboxes_ignore,
                                        gt_labels_list=gt_labels, label_channels=1, sampling=False,
                                        unmap_outputs=False)
        if cls_reg_targets is None:
            return None
        labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, num_total_pos = cls_reg_targets[:5]
        B = len(img_metas)
        all_labels = torch.cat(labels_list, -1).view(B, -1)
        all_label_weights = torch.cat(label_weights_list, -1).view(B, -1)
        all_bbox_targets = torch.cat(bbox_targets_list, -2).view(B, -1, 4)
        all_bbox_weights = torch.cat(bbox_weights_list, -2).view(B, -1, 4)
        if self.fuse_loss:
            geom = self.geometry(featmap_sizes)
            loss_cls, loss_bbox = ssd_ops.ssd_head_loss(
                geom, cls_scores, bbox_preds, all_labels, all_label_weights, all_bbox_targets, all_bbox_weights,
                float(num_total_pos), cfg.neg_pos_ratio, cfg.smoothl1_beta)
            return dict(loss_cls=[loss_cls[b:b + 1] for b in range(B)],
                        loss_bbox=[loss_bbox[b:b + 1] for b in range(B)])
        all_cls_scores = torch.cat([s.permute(0, 2, 3, 1).reshape(B, -1, self.cls_out_channels)
                                    for s in cls_scores], 1)
        all_bbox_preds = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1, 4) for p in bbox_preds], -2)
        losses_cls, losses_bbox = [], []
        for b in range(B):
            lc, lb = self.loss_single(all_cls_scores[b], all_bbox_preds[b], all_labels[b], all_label_weights[b],
                                      all_bbox_targets[b], all_bbox_weights[b], num_total_pos, cfg)
            losses_cls.append(lc)
            losses_bbox.append(lb)
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox)

    # ------------------------------------------------------------------ inference
    def geometry(self, featmap_sizes):
        """ia_ssd_geom for these feature-map sizes (cached)"""
        key = tuple(tuple(int(v) for v in s) for s in featmap_sizes)
        g = self._geom_cache.get(key)
        if g is None:
            L = len(key)
            g = self._geom_cache[key] = ssd_ops.SsdGeometry(
                key, self.anchor_strides[:L], [gen.base_anchors.numpy() for gen in self.anchor_generators[:L]],
                self.num_classes - 1, self.target_means, self.target_stds)
        return g

    def get_bboxes_batched(self, cls_scores, bbox_preds, img_metas, cfg, rescale=False, check_overflow=True):
        """Device-side result of the whole batch: dets (B,max,5), labels (B,max) int32, rows (B,max)
        int32 (anchor row ids), num (B) int32.  check_overflow=True reads the B overflow flags (one
        small device-to-host copy) and resolves a batch with a flag set on the per-class route;
        check_overflow=False (serving loops) leaves the flags in `self.overflow` for the caller and
        does not synchronise."""
        if len(cls_scores) != len(bbox_preds):
            raise AssertionError('level count mismatch')
        if len(cls_scores) > len(self.anchor_generators):
            raise AssertionError('more levels than anchor strides')
        nms_cfg = dict(cfg.nms)
        nms_type = nms_cfg.pop('type', 'nms')
        if nms_type != 'nms':
            raise NotImplementedError('%s: test_cfg.nms.type %r (hard NMS only)' % (type(self).__name__, nms_type))
        if cfg.get('nms_pre', -1) > 0:
            raise NotImplementedError('%s: test_cfg.nms_pre is not built (the SSD configs have none)'
                                      % type(self).__name__)
        geom = self.geometry([tuple(c.shape[-2:]) for c in cls_scores])
        shapes = [m['img_shape'] for m in img_metas]
        factors = [m['scale_factor'] for m in img_metas]
        args = (geom, cls_scores, bbox_preds, shapes, factors, rescale, cfg.score_thr, nms_cfg['iou_thr'],
                cfg.max_per_img)
        dets, labels, rows, num, overflow = ssd_ops.ssd_get_bboxes(*args)
        self.overflow = overflow
        if check_overflow and bool(overflow.any()):
            return ssd_ops.ssd_get_bboxes_per_class(*args)
        return dets, labels, rows, num

    def get_bboxes(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, cfg, rescale=False):
        """-> list over images of (det_bboxes (k,5) fp32, det_labels (k,) int64)"""
        return per_image(*self.get_bboxes_batched(cls_scores, bbox_preds, img_metas, cfg, rescale))

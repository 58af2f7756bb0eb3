"""SSD head (reference mmdet/models/anchor_heads/ssd_head.py on anchor_head.py): inference, with the
reference's registry name, constructor arguments, parameter names (`reg_convs.N`, `cls_convs.N`) and
method signatures, so that a reference checkpoint loads.

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
  * loss: not built -- NotImplementedError naming what is missing.
Softmax classification (use_sigmoid_cls = False, channel 0 = background), hard NMS, fp32.  There is no
CPU fallback for get_bboxes: it needs tensors on a gfx950 device.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ssd_ops
from .anchors import AnchorGenerator
from .bbox import per_image
from .layers import xavier_init
from .registry import HEADS


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
    """SSD head (inference)."""

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
    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, cfg, gt_bboxes_ignore=None):
        raise NotImplementedError(
            'SSDHead.loss is not built: training needs the softmax cross-entropy with hard-negative mining '
            '(neg_pos_ratio) and the smooth-L1 box loss (smoothl1_beta) over all levels; the head runs '
            'inference only')

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

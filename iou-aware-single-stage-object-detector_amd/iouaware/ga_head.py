"""IoU-aware guided-anchor RetinaNet head (reference
mmdet/models/anchor_heads/iou_aware_ga_retina_head.py on guided_anchor_head.py): inference, with the
reference's registry name, constructor arguments, parameter names and method signatures, so that a
reference checkpoint loads.

  * forward: the two 4-conv towers, `conv_loc` / `conv_shape`, the two FeatureAdaption blocks (a 1x1
    `conv_offset` on the detached shape prediction feeding the HIP DeformConv, deformable_groups 4)
    and the three MaskedConv2d output layers.  In eval the mask is sigmoid(loc_pred) >=
    loc_filter_thr PER IMAGE (the reference takes image 0's mask and asserts a batch of 1): every
    level's mask is compacted once and shared by its three masked layers, `retina_reg` and
    `retina_iou` run as one 5-column product on their common input, and the kept counts of all
    levels come back in ONE device-to-host copy per forward (the library GEMM takes its row count
    from the host; the reference synchronises per layer).  The threshold is taken inside the
    compaction kernels with the library's own sigmoid (the decode recomputes the keep decision from
    loc_pred with the same function, so a location the masked layers skipped can never be decoded
    from its zero outputs).  In training mode the
    mask is None and the layers are plain convolutions, as in the reference.
  * get_bboxes: one call into the HIP library for the whole batch at any batch size
    (ia_guided_get_bboxes: row max under the location filter, per-level top-k, guided-anchor decode,
    batched NMS).  An image without any kept location gives zero detections (the reference raises).
  * loss: not built -- NotImplementedError naming what is missing.
The towers stay on the module route (`fuse.fuse_inference` leaves this head as it is).
There is no CPU fallback for the eval forward / get_bboxes: they need tensors on a gfx950 device.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ga_ops, masked_conv, ops
from .anchors import AnchorGenerator
from .bbox import per_image
from .deform_conv import DeformConv
from .layers import ConvModule, bias_init_with_prob, normal_init
from .masked_conv import MaskedConv2d
from .registry import HEADS, build_loss


class FeatureAdaption(nn.Module):
    """reference guided_anchor_head.py:18-56: the offsets of a 3x3 DCN v1 layer predicted from the
    anchor shape (2 channels) by a 1x1 convolution without bias, then ReLU"""

    def __init__(self, in_channels, out_channels, kernel_size=3, deformable_groups=4):
        super(FeatureAdaption, self).__init__()
        offset_channels = kernel_size * kernel_size * 2
        self.conv_offset = nn.Conv2d(2, deformable_groups * offset_channels, 1, bias=False)
        self.conv_adaption = DeformConv(in_channels, out_channels, kernel_size=kernel_size,
                                        padding=(kernel_size - 1) // 2, deformable_groups=deformable_groups)
        self.relu = nn.ReLU(inplace=True)

    def init_weights(self):
        normal_init(self.conv_offset, std=0.1)
        normal_init(self.conv_adaption, std=0.01)

    def forward(self, x, shape):
        offset = self.conv_offset(shape.detach())
        return self.relu(self.conv_adaption(x, offset))


@HEADS.register_module
class IoUawareGARetinaHead(nn.Module):
    """IoU-aware Guided-Anchor-based RetinaNet head (inference)."""

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None, norm_cfg=None,
                 feat_channels=256, octave_base_scale=8, scales_per_octave=3, octave_ratios=[0.5, 1.0, 2.0],
                 anchor_strides=[4, 8, 16, 32, 64], anchor_base_sizes=None,
                 anchoring_means=(.0, .0, .0, .0), anchoring_stds=(1.0, 1.0, 1.0, 1.0),
                 target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0), deformable_groups=4,
                 loc_filter_thr=0.01,
                 loss_loc=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_shape=dict(type='IoULoss', style='bounded', beta=0.2, loss_weight=1.0),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)):
        super(IoUawareGARetinaHead, self).__init__()
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        self.in_channels, self.num_classes, self.feat_channels = in_channels, num_classes, feat_channels
        self.octave_base_scale, self.scales_per_octave = octave_base_scale, scales_per_octave
        self.octave_scales = octave_base_scale * np.array(
            [2 ** (i / scales_per_octave) for i in range(scales_per_octave)])
        self.approxs_per_octave = len(self.octave_scales) * len(octave_ratios)
        self.octave_ratios = octave_ratios
        self.anchor_strides = anchor_strides
        self.anchor_base_sizes = list(anchor_strides) if anchor_base_sizes is None else anchor_base_sizes
        self.anchoring_means, self.anchoring_stds = anchoring_means, anchoring_stds
        self.target_means, self.target_stds = target_means, target_stds
        self.deformable_groups = deformable_groups
        self.loc_filter_thr = loc_filter_thr
        self.approx_generators = [AnchorGenerator(b, self.octave_scales, self.octave_ratios)
                                  for b in self.anchor_base_sizes]
        self.square_generators = [AnchorGenerator(b, [self.octave_base_scale], [1.0])
                                  for b in self.anchor_base_sizes]
        self.num_anchors = 1                      # one guided anchor per location
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        if not self.use_sigmoid_cls:
            raise NotImplementedError('IoUawareGARetinaHead: use_sigmoid_cls=False (a softmax loss_cls) is not '
                                      'built; the guided-anchor decode scores with sigmoid(cls) * sigmoid(iou)')
        self.cls_focal_loss = loss_cls['type'] in ['FocalLoss']
        self.loc_focal_loss = loss_loc['type'] in ['FocalLoss']
        self.cls_out_channels = self.num_classes - 1
        # the loss modules carry no parameters; loss() itself is not built, and neither is the bounded
        # IoU loss of loss_shape, whose settings are kept as given
        self.loss_loc = build_loss(loss_loc)
        self.loss_shape_cfg = dict(loss_shape)
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.IoU_balanced_Cls = loss_cls['type'] in ['IOUbalancedCrossEntropyLoss', 'IOUbalancedSigmoidFocalLoss']
        self.IoU_balanced_Loc = loss_bbox['type'] in ['IoUbalancedSmoothL1Loss']
        self._geom_cache = {}
        self._packed = {}
        self._init_layers()

    def _init_layers(self):
        self.relu = nn.ReLU(inplace=True)
        self.cls_convs = nn.ModuleList()
        self.reg_convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            for tower in (self.cls_convs, self.reg_convs):
                tower.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                                        conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg))
        self.conv_loc = nn.Conv2d(self.feat_channels, 1, 1)
        self.conv_shape = nn.Conv2d(self.feat_channels, self.num_anchors * 2, 1)
        self.feature_adaption_cls = FeatureAdaption(self.feat_channels, self.feat_channels, kernel_size=3,
                                                    deformable_groups=self.deformable_groups)
        self.feature_adaption_reg = FeatureAdaption(self.feat_channels, self.feat_channels, kernel_size=3,
                                                    deformable_groups=self.deformable_groups)
        self.retina_cls = MaskedConv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.retina_reg = MaskedConv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)
        self.retina_iou = MaskedConv2d(self.feat_channels, self.num_anchors, 3, padding=1)

    def init_weights(self):
        for m in list(self.cls_convs) + list(self.reg_convs):
            normal_init(m.conv, std=0.01)
        self.feature_adaption_cls.init_weights()
        self.feature_adaption_reg.init_weights()
        bias_cls = bias_init_with_prob(0.01)
        normal_init(self.conv_loc, std=0.01, bias=bias_cls)
        normal_init(self.conv_shape, std=0.01)
        normal_init(self.retina_cls, std=0.01, bias=bias_cls)
        normal_init(self.retina_reg, std=0.01)
        normal_init(self.retina_iou, std=0.01)

    # ------------------------------------------------------------------ forward
    def _adapted(self, x):
        """towers, loc / shape predictions, feature adaption -> (cls_feat, reg_feat, shape_pred, loc_pred)"""
        cls_feat = reg_feat = x
        for conv in self.cls_convs:
            cls_feat = conv(cls_feat)
        for conv in self.reg_convs:
            reg_feat = conv(reg_feat)
        loc_pred = self.conv_loc(cls_feat)
        shape_pred = self.conv_shape(reg_feat)
        cls_feat = self.feature_adaption_cls(cls_feat, shape_pred)
        reg_feat = self.feature_adaption_reg(reg_feat, shape_pred)
        return cls_feat, reg_feat, shape_pred, loc_pred

    def forward_single(self, x):
        """one level -> (cls_score, bbox_pred, iou_pred, shape_pred, loc_pred)"""
        return tuple(t[0] for t in self.forward([x]))

    def loc_mask(self, loc_pred):
        """(B, 1, H, W) location logits -> the (B, H, W) bool mask of the masked layers and of the
        decode as a tensor, for inspection and tools: the library's sigmoid (its self-test export) >=
        loc_filter_thr.  forward does not call this: it thresholds inside the compaction kernels
        (masked_conv.compact_logits), with the same device function"""
        return ops.test_math(2, loc_pred.detach()[:, 0].float().contiguous()) >= self.loc_filter_thr

    def _packed_weights(self):
        """GEMM operands of the three masked layers -- retina_reg and retina_iou as one 5-column
        product -- repacked when a parameter changes"""
        params = (self.retina_cls.weight, self.retina_cls.bias, self.retina_reg.weight, self.retina_reg.bias,
                  self.retina_iou.weight, self.retina_iou.bias)
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in params)
        if self._packed.get('key') != key:
            self._packed = dict(
                key=key, cls=masked_conv.pack_weight(self.retina_cls.weight, self.retina_cls.bias),
                reg_iou=masked_conv.pack_weight(torch.cat((self.retina_reg.weight, self.retina_iou.weight)),
                                                torch.cat((self.retina_reg.bias, self.retina_iou.bias))))
        return self._packed

    def forward(self, feats):
        """-> (cls_scores[L], bbox_preds[L], iou_preds[L], shape_preds[L], loc_preds[L])"""
        if self.training:
            outs = []
            for x in feats:
                cls_feat, reg_feat, shape_pred, loc_pred = self._adapted(x)
                outs.append((self.retina_cls(cls_feat), self.retina_reg(reg_feat), self.retina_iou(reg_feat),
                             shape_pred, loc_pred))
            return tuple(map(list, zip(*outs)))
        feats = list(feats)
        pre = [self._adapted(x) for x in feats]
        for name, t in (('feature', feats[0]), ('retina_cls.weight', self.retina_cls.weight)):
            ops._require_gpu(t, name)
        dev = feats[0].device
        # every level's mask compacted first, then ONE copy of all counts to the host
        counts = torch.empty(len(pre), dtype=torch.int32, device=dev)
        comps = [masked_conv.compact_logits(p[3].detach()[:, 0].float(), self.loc_filter_thr, counts[l:l + 1])
                 for l, p in enumerate(pre)]
        for comp, n in zip(comps, counts.tolist()):
            comp.set_n(n)
        packed = self._packed_weights()
        cl = torch.channels_last
        outs = []
        for (cls_feat, reg_feat, shape_pred, loc_pred), comp in zip(pre, comps):
            for t in (cls_feat, reg_feat):
                if t.dtype != torch.float32:
                    raise TypeError('feature has dtype %s: the masked convolution kernels are float32 only' % t.dtype)
            cls_score = masked_conv.masked_conv_packed(cls_feat.detach().contiguous(memory_format=cl), comp,
                                                       packed['cls'], 3)
            reg_iou = masked_conv.masked_conv_packed(reg_feat.detach().contiguous(memory_format=cl), comp,
                                                     packed['reg_iou'], 3)
            outs.append((cls_score, reg_iou[:, :4], reg_iou[:, 4:5], shape_pred, loc_pred))
        return tuple(map(list, zip(*outs)))

    # ------------------------------------------------------------------ training
    def loss(self, cls_scores, bbox_preds, iou_preds, shape_preds, loc_preds, gt_bboxes, gt_labels, img_metas,
             cfg, gt_bboxes_ignore=None):
        raise NotImplementedError(
            'IoUawareGARetinaHead.loss is not built: training needs ga_loc_target, ga_shape_target, '
            'ApproxMaxIoUAssigner and the bounded IoU loss (loss_shape), none of which this build has; '
            'the head runs inference only')

    # ------------------------------------------------------------------ inference
    def geometry(self, featmap_sizes, nms_pre=-1, use_loc_filter=True):
        """ia_guided_geom for these feature-map sizes (cached)"""
        key = (tuple(tuple(int(v) for v in s) for s in featmap_sizes), int(nms_pre), bool(use_loc_filter))
        g = self._geom_cache.get(key)
        if g is None:
            L = len(key[0])
            base = np.stack([gen.base_anchors.numpy()[0] for gen in self.square_generators[:L]])
            g = self._geom_cache[key] = ga_ops.GuidedGeometry(
                key[0], self.anchor_strides[:L], base, self.cls_out_channels, nms_pre, self.target_means,
                self.target_stds, self.anchoring_means, self.anchoring_stds, self.loc_filter_thr, use_loc_filter)
        return g

    def get_bboxes_batched(self, cls_scores, bbox_preds, iou_preds, shape_preds, loc_preds, img_metas, cfg,
                           rescale=False):
        """Device-side result of the whole batch: dets (B,max,5), labels (B,max) int32, rows (B,max)
        int32, num (B) int32 -- no host synchronisation.  The location filter is on outside training
        (the reference's use_loc_filter = not self.training)."""
        if not (len(cls_scores) == len(bbox_preds) == len(iou_preds) == len(shape_preds) == len(loc_preds)):
            raise AssertionError('level count mismatch')
        if len(cls_scores) > len(self.square_generators):
            raise AssertionError('more levels than anchor strides')
        nms_cfg = dict(cfg.nms)
        nms_type = nms_cfg.pop('type', 'nms')
        if nms_type != 'nms':
            raise NotImplementedError('%s: test_cfg.nms.type %r (hard NMS only)' % (type(self).__name__, nms_type))
        featmap_sizes = [tuple(c.shape[-2:]) for c in cls_scores]
        geom = self.geometry(featmap_sizes, cfg.get('nms_pre', -1), use_loc_filter=not self.training)
        shapes = [m['img_shape'] for m in img_metas]
        factors = [m['scale_factor'] for m in img_metas]
        return ga_ops.guided_get_bboxes(geom, cls_scores, bbox_preds, iou_preds, shape_preds, loc_preds, shapes,
                                        factors, rescale, cfg.score_thr, nms_cfg['iou_thr'], cfg.max_per_img)

    def get_bboxes(self, cls_scores, bbox_preds, iou_preds, shape_preds, loc_preds, gt_bboxes, gt_labels,
                   img_metas, cfg, rescale=False):
        """-> list over images of (det_bboxes (k,5) fp32, det_labels (k,) int64)"""
        return per_image(*self.get_bboxes_batched(cls_scores, bbox_preds, iou_preds, shape_preds, loc_preds,
                                                  img_metas, cfg, rescale))

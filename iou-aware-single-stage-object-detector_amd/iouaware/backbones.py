"""ResNet / ResNeXt feature extractors (C2..C5) on PyTorch-ROCm.

Host-side modules only: the 3x3 / 1x1 / grouped convolutions are dense
contractions that MIOpen / rocBLAS execute on MFMA; nothing here is a
hand-written kernel.  Constructor kwargs, parameter names (`conv1`, `bn1`,
`layerN.M.conv{1,2,3}`, `layerN.M.bn{1,2,3}`, `layerN.M.downsample.{0,1}`) and
train()/init semantics follow the reference so its configs and checkpoints
drop in (reference mmdet/models/backbones/resnet.py:88-267,333-527;
resnext.py:12-91,157-226).  `dcn=` puts a deformable convolution (DCN v1 / v2,
iouaware/deform_conv.py: HIP kernels, fp32) in place of conv2 of the bottlenecks of the stages
`stage_with_dcn` names; GCNet and attention plugins are outside the IoU-aware RetinaNet path and
are rejected explicitly, as is `dcn` on a BasicBlock (the reference refuses it too) and on a
grouped (ResNeXt) conv2.
"""
import math

import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from .layers import build_conv_layer, build_norm_layer, constant_init, kaiming_init
from .registry import BACKBONES


def _reject_plugins(dcn, gcb, gen_attention):
    if dcn is not None or gcb is not None or gen_attention is not None:
        raise NotImplementedError('dcn / gcb / gen_attention are outside the IoU-aware '
                                  'RetinaNet hot path of this build')


def _dcn_cfg(dcn):
    """-> (modulated, deformable_groups, fallback_on_stride) of a `dcn=dict(...)`"""
    if not isinstance(dcn, dict):
        raise AssertionError('dcn must be a dict or None')
    return (bool(dcn.get('modulated', False)), int(dcn.get('deformable_groups', 1)),
            bool(dcn.get('fallback_on_stride', False)))


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch',
                 with_cp=False, conv_cfg=None, norm_cfg=dict(type='BN'), dcn=None, gcb=None,
                 gen_attention=None, groups=1, base_width=4):
        super(BasicBlock, self).__init__()
        _reject_plugins(dcn, gcb, gen_attention)
        if with_cp:
            raise AssertionError('with_cp is not supported by BasicBlock')
        self.norm1_name, n1 = build_norm_layer(norm_cfg, planes, postfix=1)
        self.norm2_name, n2 = build_norm_layer(norm_cfg, planes, postfix=2)
        self.conv1 = build_conv_layer(conv_cfg, inplanes, planes, 3, stride=stride,
                                      padding=dilation, dilation=dilation, bias=False)
        self.add_module(self.norm1_name, n1)
        self.conv2 = build_conv_layer(conv_cfg, planes, planes, 3, padding=1, bias=False)
        self.add_module(self.norm2_name, n2)
        self.relu = nn.ReLU(inplace=True)
        self.downsample, self.stride, self.dilation = downsample, stride, dilation

    norm1 = property(lambda self: getattr(self, self.norm1_name))
    norm2 = property(lambda self: getattr(self, self.norm2_name))

    def forward(self, x):
        out = self.relu(self.norm1(self.conv1(x)))
        out = self.norm2(self.conv2(out))
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.relu(out)


class Bottleneck(nn.Module):
    """1x1 -> 3x3 (stride here for style='pytorch', grouped for ResNeXt) -> 1x1."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch',
                 with_cp=False, conv_cfg=None, norm_cfg=dict(type='BN'), dcn=None, gcb=None,
                 gen_attention=None, groups=1, base_width=4):
        super(Bottleneck, self).__init__()
        if style not in ('pytorch', 'caffe'):
            raise AssertionError(style)
        _reject_plugins(None, gcb, gen_attention)
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        self.style, self.with_cp, self.conv_cfg, self.norm_cfg = style, with_cp, conv_cfg, norm_cfg
        s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
        self.conv1_stride, self.conv2_stride = s1, s2
        width = planes if groups == 1 else int(math.floor(planes * (base_width / 64))) * groups
        self.norm1_name, n1 = build_norm_layer(norm_cfg, width, postfix=1)
        self.norm2_name, n2 = build_norm_layer(norm_cfg, width, postfix=2)
        self.norm3_name, n3 = build_norm_layer(norm_cfg, planes * self.expansion, postfix=3)
        self.conv1 = build_conv_layer(conv_cfg, inplanes, width, kernel_size=1, stride=s1,
                                      bias=False)
        self.add_module(self.norm1_name, n1)
        self.dcn, self.with_dcn, self.with_modulated_dcn = dcn, False, False
        modulated, dg, fallback = _dcn_cfg(dcn) if dcn is not None else (False, 1, False)
        if dcn is None or (fallback and s2 > 1):
            self.conv2 = build_conv_layer(conv_cfg, width, width, kernel_size=3, stride=s2,
                                          padding=dilation, dilation=dilation, groups=groups,
                                          bias=False)
        else:
            # conv2 as a deformable convolution; its offsets (modulated: and mask logits) come from
            # conv2_offset, an ordinary convolution of the same geometry on the same input.
            # dg * 18 offset channels, modulated dg * 27: offsets first, then dg * 9 mask logits
            # (the reference slices a literal 18 / 9: the same for dg = 1)
            from .deform_conv import DeformConv, ModulatedDeformConv
            if conv_cfg is not None:
                raise AssertionError('conv_cfg must be None for DCN')
            if groups != 1:
                raise NotImplementedError('dcn with groups=%d (ResNeXt): the HIP deformable '
                                          'convolution supports groups=1 only' % groups)
            self.with_dcn, self.with_modulated_dcn, self.deformable_groups = True, modulated, dg
            self.conv2_offset = nn.Conv2d(width, dg * (27 if modulated else 18), 3, stride=s2,
                                          padding=dilation, dilation=dilation)
            self.conv2 = (ModulatedDeformConv if modulated else DeformConv)(
                width, width, 3, stride=s2, padding=dilation, dilation=dilation,
                deformable_groups=dg, bias=False)
        self.add_module(self.norm2_name, n2)
        self.conv3 = build_conv_layer(conv_cfg, width, planes * self.expansion, kernel_size=1,
                                      bias=False)
        self.add_module(self.norm3_name, n3)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    norm1 = property(lambda self: getattr(self, self.norm1_name))
    norm2 = property(lambda self: getattr(self, self.norm2_name))
    norm3 = property(lambda self: getattr(self, self.norm3_name))

    def _conv2(self, out):
        if not self.with_dcn:
            return self.conv2(out)
        if out.dtype in (torch.bfloat16, torch.float16):
            raise TypeError('dcn: the deformable conv2 of this block is fp32 only, got a %s '
                            'activation (a bf16 network with DCN blocks is not supported)' % out.dtype)
        om = self.conv2_offset(out)
        if not self.with_modulated_dcn:
            return self.conv2(out, om)
        n = 18 * self.deformable_groups
        return self.conv2(out, om[:, :n], om[:, n:].sigmoid())

    def _residual(self, x):
        out = self.relu(self.norm1(self.conv1(x)))
        out = self.relu(self.norm2(self._conv2(out)))
        out = self.norm3(self.conv3(out))
        return out + (x if self.downsample is None else self.downsample(x))

    def forward(self, x):
        if self.with_cp and x.requires_grad:
            import torch.utils.checkpoint as cp
            return self.relu(cp.checkpoint(self._residual, x))
        return self.relu(self._residual(x))


def make_res_layer(block, inplanes, planes, blocks, stride=1, dilation=1, style='pytorch',
                   with_cp=False, conv_cfg=None, norm_cfg=dict(type='BN'), dcn=None, gcb=None,
                   gen_attention=None, gen_attention_blocks=(), groups=1, base_width=4):
    out_ch = planes * block.expansion
    downsample = None
    if stride != 1 or inplanes != out_ch:
        downsample = nn.Sequential(
            build_conv_layer(conv_cfg, inplanes, out_ch, kernel_size=1, stride=stride, bias=False),
            build_norm_layer(norm_cfg, out_ch)[1])
    common = dict(style=style, with_cp=with_cp, conv_cfg=conv_cfg, norm_cfg=norm_cfg, dcn=dcn,
                  gcb=gcb, groups=groups, base_width=base_width)
    layers = [block(inplanes, planes, stride, dilation, downsample,
                    gen_attention=gen_attention if 0 in gen_attention_blocks else None, **common)]
    for i in range(1, blocks):
        layers.append(block(out_ch, planes, 1, dilation,
                            gen_attention=gen_attention if i in gen_attention_blocks else None,
                            **common))
    return nn.Sequential(*layers)


@BACKBONES.register_module
class ResNet(nn.Module):
    """depth in {18,34,50,101,152}; returns the stage outputs listed in out_indices."""

    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)),
                     50: (Bottleneck, (3, 4, 6, 3)), 101: (Bottleneck, (3, 4, 23, 3)),
                     152: (Bottleneck, (3, 8, 36, 3))}
    _groups, _base_width = 1, 4
    # ResNeXt in bf16 inference: conv2 on the bf16 MFMA kernel of csrc/gconv_bf16.hip (False: the
    # library's grouped convolution + an affine pass).  Read by fuse_inference.
    gconv_bf16 = True
    # training, opt-in: the stride-2 conv2 of a fused training block (train_fuse.bottleneck_forward)
    # on the im2col / col2im node instead of the framework's convolution -- the same bits in every
    # run.  Read by fuse_inference, like gconv_bf16.
    train_strided = False
    # training, opt-in: the grouped 3x3 conv2 of a fused ResNeXt training block on the MFMA kernels
    # of csrc/gconv.hip / csrc/gconv_bwd.hip (train_fuse.grouped_conv3x3_train) instead of the module
    # route (framework convolutions + BatchNorm modules).  Read by fuse_inference, like train_strided.
    train_gconv = False

    def __init__(self, depth, num_stages=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=(0, 1, 2, 3), style='pytorch', frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), gcb=None,
                 stage_with_gcb=(False, False, False, False), gen_attention=None,
                 stage_with_gen_attention=((), (), (), ()), with_cp=False,
                 zero_init_residual=True):
        super(ResNet, self).__init__()
        if depth not in self.arch_settings:
            raise KeyError('invalid depth {} for resnet'.format(depth))
        if not 1 <= num_stages <= 4:
            raise AssertionError('num_stages must be in 1..4')
        if not len(strides) == len(dilations) == num_stages:
            raise AssertionError('strides / dilations must have num_stages entries')
        if max(out_indices) >= num_stages:
            raise AssertionError('out_indices exceed num_stages')
        _reject_plugins(None, gcb, gen_attention)
        if dcn is not None:
            _dcn_cfg(dcn)
            if len(stage_with_dcn) != num_stages:
                raise AssertionError('stage_with_dcn must have num_stages entries')
        self.depth, self.num_stages, self.strides, self.dilations = depth, num_stages, strides, dilations
        self.out_indices, self.style, self.frozen_stages = out_indices, style, frozen_stages
        self.conv_cfg, self.norm_cfg, self.with_cp, self.norm_eval = conv_cfg, norm_cfg, with_cp, norm_eval
        self.dcn, self.gcb, self.gen_attention = dcn, gcb, gen_attention
        self.stage_with_dcn, self.stage_with_gcb = stage_with_dcn, stage_with_gcb
        self.zero_init_residual = zero_init_residual
        self.block, stage_blocks = self.arch_settings[depth]
        self.stage_blocks = stage_blocks[:num_stages]

        # stem
        self.conv1 = build_conv_layer(conv_cfg, 3, 64, kernel_size=7, stride=2, padding=3,
                                      bias=False)
        self.norm1_name, n1 = build_norm_layer(norm_cfg, 64, postfix=1)
        self.add_module(self.norm1_name, n1)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)

        self.inplanes = 64
        self.res_layers = []
        for i, nblocks in enumerate(self.stage_blocks):
            planes = 64 * 2 ** i
            layer = make_res_layer(self.block, self.inplanes, planes, nblocks, stride=strides[i],
                                   dilation=dilations[i], style=style, with_cp=with_cp,
                                   conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                                   dcn=dcn if dcn is not None and stage_with_dcn[i] else None,
                                   groups=self._groups, base_width=self._base_width)
            self.inplanes = planes * self.block.expansion
            name = 'layer{}'.format(i + 1)
            self.add_module(name, layer)
            self.res_layers.append(name)
        self._freeze_stages()
        self.feat_dim = self.block.expansion * 64 * 2 ** (len(self.stage_blocks) - 1)

    norm1 = property(lambda self: getattr(self, self.norm1_name))

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.norm1.eval()
            for m in (self.conv1, self.norm1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            stage = getattr(self, 'layer{}'.format(i))
            stage.eval()
            for p in stage.parameters():
                p.requires_grad = False

    def init_weights(self, pretrained=None):
        if isinstance(pretrained, str):
            from .checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)
            return
        if pretrained is not None:
            raise TypeError('pretrained must be a str or None')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                kaiming_init(m)
            elif isinstance(m, (_BatchNorm, nn.GroupNorm)):
                constant_init(m, 1)
        if self.dcn is not None:
            for m in self.modules():
                if isinstance(m, Bottleneck) and hasattr(m, 'conv2_offset'):
                    constant_init(m.conv2_offset, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    constant_init(m.norm3, 0)
                elif isinstance(m, BasicBlock):
                    constant_init(m.norm2, 0)

    def forward(self, x):
        x = self.maxpool(self.relu(self.norm1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super(ResNet, self).train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self


@BACKBONES.register_module
class ResNeXt(ResNet):
    """ResNet with grouped 3x3 convolutions (groups x base_width), e.g. 32x4d / 64x4d."""

    arch_settings = {50: (Bottleneck, (3, 4, 6, 3)), 101: (Bottleneck, (3, 4, 23, 3)),
                     152: (Bottleneck, (3, 8, 36, 3))}

    def __init__(self, groups=1, base_width=4, **kwargs):
        self._groups, self._base_width = groups, base_width
        super(ResNeXt, self).__init__(**kwargs)
        self.groups, self.base_width = groups, base_width

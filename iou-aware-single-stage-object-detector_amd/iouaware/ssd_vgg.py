"""SSD backbone (reference mmdet/models/backbones/ssd_vgg.py): VGG-16 with the SSD tail, the extra
feature layers and the L2Norm of conv4_3, with the reference's registry name, constructor arguments
and state-dict names (`features.N.*`, `extra.N.*`, `l2_norm.weight`), so that a reference checkpoint
loads.

The reference derives from mmcv's VGG, which this build does not depend on; the VGG-16 body is
written out here.  `features` is an nn.Sequential of conv3x3 / ReLU / MaxPool2d(2, 2, ceil_mode) in the
2-2-3-3-3 layout (30 entries without the last pool), the layout the indices the reference uses imply:
features[21] is conv4_3 (512 output channels), its ReLU at 22 is the first tap, the five modules the
reference appends land at 30-34 and the second tap is 34.  (DESIGN: unverified against mmcv itself.)

In eval mode on a gfx950 fp32 tensor L2Norm runs on the HIP kernel (csrc/l2norm.hip); in training mode
it evaluates the reference's expression in torch.  The convolutions are torch modules.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ssd_ops
from .layers import constant_init, kaiming_init, xavier_init
from .registry import BACKBONES

_VGG16_STAGES = (2, 2, 3, 3, 3)


def _vgg16_features(with_last_pool, ceil_mode):
    layers, inplanes = [], 3
    for i, num_blocks in enumerate(_VGG16_STAGES):
        planes = 64 * 2 ** i if i < 4 else 512
        for _ in range(num_blocks):
            layers += [nn.Conv2d(inplanes, planes, 3, padding=1), nn.ReLU(inplace=True)]
            inplanes = planes
        layers.append(nn.MaxPool2d(kernel_size=2, stride=2, ceil_mode=ceil_mode))
    if not with_last_pool:
        layers.pop(-1)
    return layers


class L2Norm(nn.Module):
    """reference ssd_vgg.py L2Norm: weight[c] * x / (sqrt(sum_c x^2) + eps)"""

    def __init__(self, n_dims, scale=20., eps=1e-10):
        super(L2Norm, self).__init__()
        self.n_dims = n_dims
        self.weight = nn.Parameter(torch.Tensor(self.n_dims))
        self.eps = eps
        self.scale = scale

    def forward(self, x):
        if self.training:
            norm = x.pow(2).sum(1, keepdim=True).sqrt() + self.eps
            return self.weight[None, :, None, None].expand_as(x) * x / norm
        return ssd_ops.l2norm(x, self.weight, self.eps)


@BACKBONES.register_module
class SSDVGG(nn.Module):
    extra_setting = {
        300: (256, 'S', 512, 128, 'S', 256, 128, 256, 128, 256),
        512: (256, 'S', 512, 128, 'S', 256, 128, 'S', 256, 128, 'S', 256, 128),
    }

    def __init__(self, input_size, depth, with_last_pool=False, ceil_mode=True, out_indices=(3, 4),
                 out_feature_indices=(22, 34), l2_norm_scale=20.):
        super(SSDVGG, self).__init__()
        if depth != 16:
            raise NotImplementedError('SSDVGG: depth %r is not built (VGG-16 only)' % (depth,))
        if input_size not in (300, 512):
            raise AssertionError('input_size must be 300 or 512')
        self.input_size = input_size
        self.out_indices = out_indices
        layers = _vgg16_features(with_last_pool, ceil_mode)
        layers += [nn.MaxPool2d(kernel_size=3, stride=1, padding=1),
                   nn.Conv2d(512, 1024, kernel_size=3, padding=6, dilation=6), nn.ReLU(inplace=True),
                   nn.Conv2d(1024, 1024, kernel_size=1), nn.ReLU(inplace=True)]
        self.features = nn.Sequential(*layers)
        self.out_feature_indices = out_feature_indices
        self.inplanes = 1024
        self.extra = self._make_extra_layers(self.extra_setting[input_size])
        self.l2_norm = L2Norm(self.features[out_feature_indices[0] - 1].out_channels, l2_norm_scale)

    def init_weights(self, pretrained=None):
        """a checkpoint path, or None: kaiming for the convolutions of `features`; `extra` (xavier,
        uniform) and the L2Norm weight (its scale) are initialised in both cases, as in the reference"""
        if isinstance(pretrained, str):
            from .checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)
        elif pretrained is not None:
            raise TypeError('pretrained must be a str or None')
        else:
            for m in self.features:
                if isinstance(m, nn.Conv2d):
                    kaiming_init(m)
        for conv in self.extra:
            xavier_init(conv, distribution='uniform')
        constant_init(self.l2_norm, self.l2_norm.scale)

    def forward(self, x):
        """-> (L2Norm(conv4_3), fc7, every second extra layer): 6 maps for SSD300, 7 for SSD512"""
        taps = []
        for i, layer in enumerate(self.features):
            x = layer(x)
            if i in self.out_feature_indices:
                taps.append(x)
        for i, conv in enumerate(self.extra):
            x = F.relu(conv(x), inplace=True)
            if i & 1:
                taps.append(x)
        taps[0] = self.l2_norm(taps[0])
        return tuple(taps) if len(taps) > 1 else taps[0]

    def _make_extra_layers(self, setting):
        """the extra feature layers as the reference lays them out: 1x1 and 3x3 convolutions in turn; an
        'S' in front of a width makes that (3x3) convolution stride 2 with padding 1, all others have
        stride 1 and no padding; SSD512 closes with a 4x4 convolution (padding 1)"""
        convs, tokens = [], iter(setting)
        for tok in tokens:
            strided = tok == 'S'
            planes = next(tokens) if strided else tok
            ksize = 3 if len(convs) % 2 else 1
            convs.append(nn.Conv2d(self.inplanes, planes, ksize, stride=2 if strided else 1,
                                   padding=1 if strided else 0))
            self.inplanes = planes
        if self.input_size == 512:
            convs.append(nn.Conv2d(self.inplanes, 256, 4, padding=1))
        return nn.Sequential(*convs)

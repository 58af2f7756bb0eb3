"""The conv towers and the class-output convolution of an IoUawareRetinaHead in bf16 on this
library's MFMA implicit-GEMM kernel (csrc/conv3x3_bf16.hip) -- BASELINE config 3 (R-101 bf16).

Reference: mmdet/models/anchor_heads/iou_aware_retina_head.py:171-219 (4 + 4 tower ConvModules
256 -> 256 with ReLU, retina_cls 256 -> A*C, retina_reg / retina_iou), weights shared by the five
pyramid levels.  Per tower layer ONE launch covers all levels and both towers (the towers are two
groups reading / writing the channel halves of one 2F-channel activation); bias and ReLU are the
kernel's epilogue; retina_reg | retina_iou (36 + 9 output channels) are one more launch on the reg
tower (padded to 46 channels, split afterwards).

Bf16ConvFCOSHead: the same for the GroupNorm towers of IoUawareFCOSHead / FCOSHead (reference
iou_aware_fcos_head.py:41-110, fcos_head.py): the tower convolutions without bias / ReLU, the HIP
bf16 GroupNorm + ReLU (csrc/groupnorm.hip) on the 2F-channel activation behind each, the output
convolutions reading the channel halves in place.
"""
import collections

import torch

from . import ops


def _plain3(c):
    return (tuple(c.kernel_size) == (3, 3) and tuple(c.stride) == (1, 1) and tuple(c.padding) == (1, 1)
            and tuple(c.dilation) == (1, 1) and c.groups == 1 and getattr(c, 'padding_mode', 'zeros') == 'zeros')


def _joined(convs, F):
    """output convolutions on one tower as ONE convolution: weights (n_pad, F, 3, 3) and fp32 bias
    (n_pad,), n_pad = the channel sum rounded up to even (the kernel stores channel pairs); the
    padding column has zero weights and bias"""
    ws = [c.weight.detach() for c in convs]
    bs = [(c.bias.detach().float() if c.bias is not None
           else torch.zeros(c.out_channels, device=c.weight.device)) for c in convs]
    n = sum(w.shape[0] for w in ws)
    pad = (n + 1) // 2 * 2 - n
    if pad:
        ws.append(torch.zeros((pad,) + tuple(ws[0].shape[1:]), dtype=ws[0].dtype, device=ws[0].device))
        bs.append(torch.zeros(pad, device=ws[0].device))
    return torch.cat(ws, 0), torch.cat(bs).contiguous(), n + pad


class _Bf16Towers(object):
    """what the bf16 head runners share: the input test, the activation buffers and the channel
    halves of a 2F-channel activation"""

    def usable(self, feats):
        return (not torch.is_grad_enabled()) and all(
            x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] == self.cin
            and x.is_contiguous(memory_format=torch.channels_last) for x in feats)

    def _acts(self, name, feats, channels):
        key = (name, channels, tuple(tuple(x.shape) for x in feats), feats[0].device,
               ops.stream_id())
        a = self._bufs.get(key)
        if a is None:
            # ping-pong activations of ONE pad shape (4 names); real evaluation sees many pad shapes
            # (keep-ratio 1333 x 800 padded to /32): keep the two most recent shapes' buffers, the
            # caching allocator recycles the rest (the cache grew without bound, ~1.1 GB
            # per shape at batch 16)
            while len(self._bufs) >= 8:
                self._bufs.popitem(last=False)
            a = self._bufs[key] = [torch.empty((x.shape[0], channels, x.shape[2], x.shape[3]),
                                               dtype=torch.bfloat16, device=x.device,
                                               memory_format=torch.channels_last) for x in feats]
        else:
            self._bufs.move_to_end(key)
        return a

    def _halves(self, ts):
        F = self.F
        return [[t[:, :F] for t in ts], [t[:, F:] for t in ts]]

    @staticmethod
    def _new(feats, channels):
        return [torch.empty((x.shape[0], channels, x.shape[2], x.shape[3]), dtype=torch.bfloat16,
                            device=x.device, memory_format=torch.channels_last) for x in feats]


class Bf16ConvHead(_Bf16Towers):
    def __init__(self, head):
        convs_c, convs_r = list(head.cls_convs), list(head.reg_convs)
        if any(m.with_norm or not m.with_activatation for m in convs_c + convs_r):
            raise NotImplementedError('towers with norm layers / without ReLU')
        if len(convs_c) != len(convs_r) or not convs_c:
            raise NotImplementedError('towers of different depth')
        from .fuse import _wino_ok               # plain 3x3 / stride 1 / pad 1 / dilation 1 / groups 1
        plain = [m.conv for m in convs_c + convs_r] + [head.retina_cls]
        if not all(_wino_ok(c) and getattr(c, 'padding_mode', 'zeros') == 'zeros' for c in plain):
            raise NotImplementedError('the kernel covers plain 3x3 / stride-1 / pad-1 convolutions')
        F = head.feat_channels
        if head.in_channels % 32 or F % 32 or head.retina_cls.out_channels % 2:
            raise NotImplementedError('channel counts')
        self.F, self.cin, self.n_layers = F, head.in_channels, len(convs_c)
        self.head = head

        def wb(m):
            conv = m.conv if hasattr(m, 'conv') else m
            b = conv.bias if conv.bias is not None else torch.zeros(conv.out_channels, device=conv.weight.device)
            return conv.weight.detach(), b.detach().float()
        # layer 0: both towers read the FPN feature -> one group with 2F output channels
        (wc, bc), (wr, br) = wb(convs_c[0]), wb(convs_r[0])
        self.w0 = ops.conv3x3_bf16_pack(torch.cat([wc, wr], 0))
        self.b0 = torch.cat([bc, br]).contiguous()
        # layers 1..: two groups (cls tower = channels [0, F), reg tower = [F, 2F))
        self.w, self.b = [], []
        for i in range(1, self.n_layers):
            (wc, bc), (wr, br) = wb(convs_c[i]), wb(convs_r[i])
            self.w.append(ops.conv3x3_bf16_pack(torch.cat([wc, wr], 0), groups=2))
            self.b.append(torch.cat([bc, br]).contiguous())
        wcls, self.b_cls = wb(head.retina_cls)
        self.w_cls = ops.conv3x3_bf16_pack(wcls)
        self.c_cls = head.retina_cls.out_channels
        # retina_reg | retina_iou (36 + 9 output channels) as ONE convolution on the reg tower, padded
        # to an even channel count (the kernel stores channel pairs); the outputs are split afterwards
        if not (_plain3(head.retina_reg) and _plain3(head.retina_iou)):
            raise NotImplementedError('the kernel covers plain 3x3 / stride-1 / pad-1 convolutions')
        (wr, brg), (wi, bi) = wb(head.retina_reg), wb(head.retina_iou)
        self.c_reg, self.c_iou = head.retina_reg.out_channels, head.retina_iou.out_channels
        self.c_ri = (self.c_reg + self.c_iou + 1) // 2 * 2
        pad = self.c_ri - self.c_reg - self.c_iou
        w_ri = torch.cat([wr, wi] + ([torch.zeros((pad,) + tuple(wr.shape[1:]), dtype=wr.dtype, device=wr.device)] if pad else []), 0)
        self.w_ri = ops.conv3x3_bf16_pack(w_ri)
        self.b_ri = torch.cat([brg, bi] + ([torch.zeros(pad, device=brg.device)] if pad else [])).contiguous()
        self._bufs = collections.OrderedDict()

    def __call__(self, feats):
        """feats: per-level (B, Cin, H, W) channels-last bf16 -> (cls[L], reg[L], iou[L])"""
        F = self.F
        feats = list(feats)
        halves = self._halves
        cur = self._acts('a', feats, 2 * F)
        ops.conv3x3_bf16_levels([feats], self.w0, self.b0, 2 * F, [cur], relu=True)
        if self.n_layers == 1:
            cls_feat, reg_feat = [t[:, :F] for t in cur], [t[:, F:].contiguous(memory_format=torch.channels_last) for t in cur]
        for i, (w, b) in enumerate(zip(self.w, self.b)):
            last = i == len(self.w) - 1
            if last:
                # the last tower layer writes two dense F-channel tensors: retina_reg / retina_iou
                # are library convolutions and want a dense input
                cls_feat, reg_feat = self._acts('c', feats, F), self._acts('r', feats, F)
                ops.conv3x3_bf16_levels(halves(cur), w, b, F, [cls_feat, reg_feat], relu=True)
            else:
                nxt = self._acts('b' if cur is self._acts('a', feats, 2 * F) else 'a', feats, 2 * F)
                ops.conv3x3_bf16_levels(halves(cur), w, b, F, halves(nxt), relu=True)
                cur = nxt
        cls = [torch.empty((x.shape[0], self.c_cls, x.shape[2], x.shape[3]), dtype=torch.bfloat16,
                           device=x.device, memory_format=torch.channels_last) for x in feats]
        ops.conv3x3_bf16_levels([cls_feat], self.w_cls, self.b_cls, self.c_cls, [cls], relu=False)
        ri = [torch.empty((x.shape[0], self.c_ri, x.shape[2], x.shape[3]), dtype=torch.bfloat16,
                          device=x.device, memory_format=torch.channels_last) for x in feats]
        ops.conv3x3_bf16_levels([reg_feat], self.w_ri, self.b_ri, self.c_ri, [ri], relu=False)
        cl = torch.channels_last
        reg = [t[:, :self.c_reg].contiguous(memory_format=cl) for t in ri]
        iou = [t[:, self.c_reg:self.c_reg + self.c_iou].contiguous(memory_format=cl) for t in ri]
        return cls, reg, iou


class Bf16ConvFCOSHead(_Bf16Towers):
    """the GN conv towers and output convolutions of an IoUawareFCOSHead or a plain FCOSHead in
    bf16: per tower layer one convolution launch (all levels, both towers; no bias, no ReLU) and
    the bf16 GroupNorm + ReLU pair on the 2F-channel activation (2 x num_groups groups, the two
    towers' affine parameters side by side, fp32); fcos_cls | fcos_centerness on the cls half and
    fcos_reg | fcos_iou (plain head: fcos_reg alone) on the reg half, read in place through the
    pixel stride; then exp(scale_l * reg) per level in place."""

    def __init__(self, head):
        convs_c, convs_r = list(head.cls_convs), list(head.reg_convs)
        if len(convs_c) != len(convs_r) or not convs_c:
            raise NotImplementedError('towers of different depth')
        for m in convs_c + convs_r:
            if not (m.with_norm and m.norm_cfg.get('type') == 'GN' and m.with_activatation
                    and m.conv.bias is None and m.activate_last and _plain3(m.conv)):
                raise NotImplementedError('FCOS towers other than 3x3 conv (no bias) + GN + ReLU')
        F = head.feat_channels
        if head.in_channels % 32 or F % 32:
            raise NotImplementedError('channel counts')
        self.groups = 2 * int(convs_c[0].norm.num_groups)
        self.eps = float(convs_c[0].norm.eps)
        if any(float(m.norm.eps) != self.eps or 2 * int(m.norm.num_groups) != self.groups
               for m in convs_c + convs_r):
            raise NotImplementedError('towers with different GroupNorm settings')
        if (2 * F) & (2 * F - 1) or 2 * F > 1024 or (2 * F // self.groups) % 8:
            raise NotImplementedError('the bf16 GroupNorm takes 2^k <= 1024 channels, 8 k per group')
        outs = [head.fcos_cls, head.fcos_centerness, head.fcos_reg]
        iou = getattr(head, 'fcos_iou', None)
        if not all(_plain3(c) for c in outs + ([iou] if iou is not None else [])):
            raise NotImplementedError('the kernel covers plain 3x3 / stride-1 / pad-1 convolutions')
        self.F, self.cin, self.n_layers = F, head.in_channels, len(convs_c)
        w = lambda m: m.conv.weight.detach()  # noqa: E731
        # layer 0: both towers read the FPN feature -> one group with 2F output channels; layers
        # 1..: two groups on the channel halves
        self.w0 = ops.conv3x3_bf16_pack(torch.cat([w(convs_c[0]), w(convs_r[0])], 0))
        self.w = [ops.conv3x3_bf16_pack(torch.cat([w(mc), w(mr)], 0), groups=2)
                  for mc, mr in zip(convs_c[1:], convs_r[1:])]
        self.gn = [(torch.cat([mc.norm.weight.detach(), mr.norm.weight.detach()]).float().contiguous(),
                    torch.cat([mc.norm.bias.detach(), mr.norm.bias.detach()]).float().contiguous())
                   for mc, mr in zip(convs_c, convs_r)]
        self.c_cls, self.c_ctr = head.fcos_cls.out_channels, head.fcos_centerness.out_channels
        w_cc, self.b_cc, self.n_cc = _joined([head.fcos_cls, head.fcos_centerness], F)
        self.w_cc = ops.conv3x3_bf16_pack(w_cc)
        self.c_reg, self.c_iou = head.fcos_reg.out_channels, (iou.out_channels if iou is not None else 0)
        if self.c_reg % 4:
            raise NotImplementedError('the regression output needs a multiple of 4 channels')
        w_ri, self.b_ri, self.n_ri = _joined([head.fcos_reg] + ([iou] if iou is not None else []), F)
        self.w_ri = ops.conv3x3_bf16_pack(w_ri)
        self.scales = torch.stack([s.scale.detach().float() for s in head.scales]).contiguous()
        self._bufs = collections.OrderedDict()
        self.calls = 0                        # forwards served (tests: the route was taken)

    def usable(self, feats):
        return len(feats) <= self.scales.numel() and super(Bf16ConvFCOSHead, self).usable(feats)

    def __call__(self, feats):
        """feats: per-level (B, Cin, H, W) channels-last bf16 -> (cls[L], bbox[L], centerness[L],
        iou[L]) (plain head: (cls[L], bbox[L], centerness[L])), bf16 channels-last"""
        from .fcos_ops import groupnorm_relu_, scale_exp_
        F = self.F
        feats = list(feats)
        cur = self._acts('a', feats, 2 * F)
        ops.conv3x3_bf16_levels([feats], self.w0, None, 2 * F, [cur], relu=False)
        groupnorm_relu_(cur, self.gn[0][0], self.gn[0][1], self.groups, self.eps, relu=True)
        for i, w in enumerate(self.w):
            nxt = self._acts('b' if cur is self._acts('a', feats, 2 * F) else 'a', feats, 2 * F)
            ops.conv3x3_bf16_levels(self._halves(cur), w, None, F, self._halves(nxt), relu=False)
            g, b = self.gn[i + 1]
            groupnorm_relu_(nxt, g, b, self.groups, self.eps, relu=True)
            cur = nxt
        cls_feat, reg_feat = self._halves(cur)
        cl = torch.channels_last
        cc = self._new(feats, self.n_cc)
        ops.conv3x3_bf16_levels([cls_feat], self.w_cc, self.b_cc, self.n_cc, [cc], relu=False)
        cls = [t[:, :self.c_cls].contiguous(memory_format=cl) for t in cc]
        ctr = [t[:, self.c_cls:self.c_cls + self.c_ctr].contiguous(memory_format=cl) for t in cc]
        ri = self._new(feats, self.n_ri)
        ops.conv3x3_bf16_levels([reg_feat], self.w_ri, self.b_ri, self.n_ri, [ri], relu=False)
        if self.n_ri == self.c_reg:
            reg = ri
        else:
            reg = [t[:, :self.c_reg].contiguous(memory_format=cl) for t in ri]
        scale_exp_(reg, self.scales)
        self.calls += 1
        if not self.c_iou:
            return cls, reg, ctr
        iou = [t[:, self.c_reg:self.c_reg + self.c_iou].contiguous(memory_format=cl) for t in ri]
        return cls, reg, ctr, iou

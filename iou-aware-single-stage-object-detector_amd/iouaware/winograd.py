"""Winograd F(4x4,3x3) inference path for the 3x3 / stride-1 convolutions of the IoU-aware
RetinaNet head (reference iou_aware_retina_head.py:171-219: cls / reg towers, retina_cls,
retina_reg, retina_iou) and of the FPN output convolutions (fpn.py:124-127).

    activations (channels-last, all five levels)  --k_wino_in-->   V  (36 matrices tiles x Cin)
    V . U   (36 [x2 towers] plain fp32 GEMMs: hipBLASLt, strided batched, csrc/gemm.hip)    -->  M
    M  --k_wino_out (+bias, +ReLU)-->  next activations / the head outputs, channels-last
    M  --k_wino_mid (+bias, +ReLU)-->  V of the next tower layer (bias + ReLU towers: no activation tensor)
    activations  --k_wino_in_gemm-->  M  (64 -> 64, ResNet stage 1: transform and products in one launch, no V)

The head's weights are shared by the pyramid levels, so every layer is ONE batched GEMM over the
tiles of all levels; the two towers run side by side (first layer: one GEMM with 512 output
columns on the shared input, later layers: 72 matrices).  36 multiplications per 4x4 output tile
instead of 144: these convolutions are 63 % of the network's multiply-adds.  That tower program is
`_WinogradTowers`; `WinogradHead` (RetinaNet: bias + ReLU inside the output transform) and
`WinogradFCOSHead` (FCOS: GroupNorm + ReLU behind it) add the layer epilogue and their output
convolutions.

Numerics: fp32 throughout; the Winograd transforms reassociate the sums, outputs agree with a
direct convolution to ~1e-5 of the activation scale (tests/test_gpu_winograd.py).  The retina_cls
product of WinogradHead runs on bf16 MFMA through an exact three-way split of both fp32 operands
(ia_batched_gemm_split3, fp32-class error: tests/test_gpu_split_gemm.py).  The weights are
transformed (fp64 -> fp32, and split) once when the runner is built: build it AFTER loading a checkpoint.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream, stream_id

_G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
               [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)


_G_DEV = {}


def transform_weight(w):
    """(Cout, Cin, 3, 3) conv weight -> U (36, Cin, Cout) fp32, U[6i+j] = (G g G^T)[i, j]."""
    if w.dim() != 4 or w.shape[2] != 3 or w.shape[3] != 3:
        raise ValueError('Winograd F(4,3) needs a 3x3 kernel, got %s' % (tuple(w.shape),))
    g = w.detach().to(torch.float64)
    G = _G_DEV.get(g.device)
    if G is None:
        G = _G_DEV[g.device] = torch.from_numpy(_G).to(g.device)
    u = torch.einsum('ik,ockl,jl->ijco', G, g, G)           # (6, 6, Cin, Cout)
    return u.reshape(36, g.shape[1], g.shape[0]).to(torch.float32).contiguous()


def _wino_geom(sizes, batch):
    """ia_wino_geom of per-level (H, W) feature maps (also the GroupNorm kernels' geometry)"""
    g = _lib.WinoGeom()
    g.num_levels, g.batch = len(sizes), int(batch)
    for l, (h, w) in enumerate(sizes):
        g.H[l], g.W[l] = int(h), int(w)
    return g


def _wino_tiles(g):
    tiles = C.c_int32()
    _lib.check(_lib.lib().ia_wino_tiles(C.byref(g), C.byref(tiles)), 'ia_wino_tiles')
    return tiles.value


def _usable(x):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] % 4 == 0
            and x.is_contiguous(memory_format=torch.channels_last))


_SCRATCH = {}


def _scratch(device, name, shape):
    """V / M staging buffers are shared by every Winograd layer of the process: the layers run
    one after the other on one stream, so a buffer is free again when the next layer starts."""
    n = 1
    for d in shape:
        n *= int(d)
    key = (device, stream_id(), name)
    b = _SCRATCH.get(key)
    if b is None or b.numel() < n:
        b = _SCRATCH[key] = torch.empty(n, dtype=torch.float32, device=device)
    return b[:n].view(*shape)


_PLAN_ENTRIES = 4     # plans kept per layer object: the head's plan owns two ping-pong activation sets
                      # (2 x B x 2F x sum(HW) floats: 92 MB at batch 1, 736 MB at batch 8 of 800 x 1344)


def _plan_for(plans, key, make):
    """least-recently-used cache of _Plan objects: evaluation meets many pad shapes (keep-ratio
    resize, padded to /32), and a plan per shape kept for the life of the model pinned its
    activation buffers for good (the growth ADVICE r3 found in the bf16 head's buffers)"""
    plan = plans.get(key)
    if plan is None:
        while len(plans) >= _PLAN_ENTRIES:
            plans.popitem(last=False)
        plan = plans[key] = make()
    else:
        plans.move_to_end(key)
    return plan


class _Plan(object):
    """buffers of one (batch, feature-map sizes) configuration"""

    def __init__(self, sizes, batch, device):
        self.sizes, self.batch = list(sizes), batch
        self.geom = _wino_geom(sizes, batch)
        self.T = _wino_tiles(self.geom)
        self.device = device
        self._bufs = {}

    def buf(self, name, shape):
        return _scratch(self.device, name, shape)

    def acts(self, name, channels):
        """per-level channels-last activation tensors (B, C, H, W)"""
        key = ('acts', name, channels)
        a = self._bufs.get(key)
        if a is None:
            a = [torch.empty((self.batch, channels, h, w), dtype=torch.float32, device=self.device,
                             memory_format=torch.channels_last) for (h, w) in self.sizes]
            self._bufs[key] = a
        return a


# Measurement hook (bench.py): when TIMING is a list, every transform launch appends
# (kind, start event, end event, algorithmic bytes) -- HIP events on the launch stream.  Bytes:
# input transform = the activation read once (16 pixels per tile) + V written (36 per tile);
# output transform = M read (36 per tile) + the activation written (16 per tile), fp32.
TIMING = None


def _timed(kind, nbytes, launch):
    if TIMING is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    TIMING.append((kind, e0, e1, nbytes))


def input_transform(plan, xs, groups, out, pre=None):
    """pre = (scale or None, shift, relu): the input is read as relu?(x * scale + shift)"""
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    ps, pb, pr = pre if pre is not None else (None, None, False)
    ch = int(xs[0].shape[1])
    _timed('in', plan.T * ch * 4 * (16 + 36), lambda: _lib.check(
        _lib.lib().ia_wino_input_transform(C.byref(plan.geom), ptrs, ch, int(groups), _ptr(ps),
                                           _ptr(pb), int(bool(pr)), _ptr(out), _stream()),
        'ia_wino_input_transform'))
    return out


def output_transform(plan, m, channels, groups, bias, relu, segments):
    """segments: list of (c0, n, dst_tensors, dst_offset)"""
    segs = (_lib.WinoSeg * len(segments))()
    for k, (c0, n, dst, off) in enumerate(segments):
        segs[k].c0, segs[k].n = int(c0), int(n)
        segs[k].dst_channels, segs[k].dst_offset = int(dst[0].shape[1]), int(off)
        for l, t in enumerate(dst):
            segs[k].dst[l] = t.data_ptr()
    _timed('out', plan.T * int(channels) * 4 * (36 + 16), lambda: _lib.check(
        _lib.lib().ia_wino_output_transform(C.byref(plan.geom), _ptr(m), int(channels), int(groups),
                                            _ptr(bias), int(bool(relu)), len(segments), segs,
                                            _stream()), 'ia_wino_output_transform'))


MID_CHANNELS = 32     # ia_wino_mid_transform: channels per group in multiples of this


def mid_transform(plan, m, channels, groups_m, bias, relu, out, groups_v):
    """V (groups_v * 36, T, C / groups_v) of the next 3x3 convolution of the same geometry straight
    from this layer's M (groups_m * 36, T, C / groups_m): the bits of output_transform (+bias,
    +ReLU) into activation tensors followed by input_transform of them, without the activation's
    trip through HBM.  Bytes: M read + V written (36 + 36 per tile)."""
    _timed('mid', plan.T * int(channels) * 4 * (36 + 36), lambda: _lib.check(
        _lib.lib().ia_wino_mid_transform(C.byref(plan.geom), _ptr(m), int(channels), int(groups_m),
                                         _ptr(bias), int(bool(relu)), _ptr(out), int(groups_v),
                                         _stream()), 'ia_wino_mid_transform'))
    return out


_LT_WS_BYTES = 128 << 20


STREAM_BMM = True
_STREAM_BMM_SHAPES = ((64, 64),)      # (128, 128) and (256, 48) measured slower than the library: 137 / 148 vs 124 / 139 us


SPLIT_GEMM = True
# (k, n) of the head products that ia_batched_gemm_split3 serves (WinogradHead only): retina_cls (256 -> 720),
# 1.27 x the library on the bench's own data (profiles/split_gemm_isolated_timing.txt).  Layer 0 (256 -> 2 x 256)
# and the tower layers (256 -> 256) are 1.18-1.22 x faster too but stay on the library: they feed the reg tower,
# and the box coordinates of two X-101 e2e fixtures, 0.9 x the 1e-4 bound off their fp64 evaluation on the
# library, moved to 1.13-1.22 x with the split's other (not larger) rounding.  reg | iou
# (256 -> 48) is HBM-bound: nothing to gain.
_SPLIT_SHAPES = ((256, 720),)


def split3_pack_u(u):
    """U (batch, K, N) fp32 -> its exact three-way bf16 split u = h + m + l, packed in the fragment order
    ia_batched_gemm_split3 reads: (batch, K/16, Np/32, 3, 64, 8) bf16, Np = N rounded up to 128, zero
    columns beyond N; packed[b][s][cb][p][32 q + c][e] = piece p of u[b][16 s + 8 q + e][32 cb + c].
    Built once with the weights (build the head AFTER loading a checkpoint)."""
    b, k, n = u.shape
    if k % 32:
        raise ValueError('the split GEMM needs K in multiples of 32')
    npad = (n + 127) // 128 * 128
    u = u.to(torch.float32)
    h = u.to(torch.bfloat16)
    r = u - h.float()                       # exact: at most 16 significant bits
    m = r.to(torch.bfloat16)
    lo = (r - m.float()).to(torch.bfloat16)  # exact, and exactly representable
    p = torch.zeros((b, 3, k, npad), dtype=torch.bfloat16, device=u.device)
    p[:, 0, :, :n], p[:, 1, :, :n], p[:, 2, :, :n] = h, m, lo
    # (b, piece, s, q, e, cb, c) -> (b, s, cb, piece, q, c, e), lane = 32 q + c
    return p.view(b, 3, k // 16, 2, 8, npad // 32, 32).permute(0, 2, 5, 1, 3, 6, 4).contiguous() \
            .view(b, k // 16, npad // 32, 3, 64, 8)


def split_shape(u):
    """the (k, n) of U (batch, k, n) is served by the split GEMM"""
    return (int(u.shape[1]), int(u.shape[2])) in _SPLIT_SHAPES


def batched_gemm(v, u, out, u3=None):
    """out[b] = v[b] @ u[b] through hipBLASLt (csrc/gemm.hip); the kernel of a shape comes from the
    committed tuning table (ops.gemm_table_load: found offline by timing the library's candidates,
    worth ~20 % over the heuristic's pick at these shapes), never from a timing race at run time.
    u3 = split3_pack_u(u): the shapes in _SPLIT_SHAPES run on ia_batched_gemm_split3 (bf16 MFMA, exact
    three-way split of both operands, fp32-class error) while SPLIT_GEMM is on."""
    from . import ops
    ops._ensure_gemm_table()
    batch, rows, k = v.shape
    n = u.shape[2]
    if not (v.is_contiguous() and u.is_contiguous() and out.is_contiguous()):
        raise ValueError('batched_gemm needs contiguous stacks')
    if SPLIT_GEMM and u3 is not None and (k, n) in _SPLIT_SHAPES and v.dtype == torch.float32:
        if u3.dtype != torch.bfloat16 or tuple(u3.shape) != (batch, k // 16, (n + 127) // 128 * 4, 3, 64, 8) \
                or not u3.is_contiguous():
            raise ValueError('u3 is not split3_pack_u of this U')
        _lib.check(_lib.lib().ia_batched_gemm_split3(_ptr(v), _ptr(u3), _ptr(out), int(batch), int(rows),
                                                     int(k), int(n), _stream()), 'ia_batched_gemm_split3')
        return out
    if STREAM_BMM and (k, n) in _STREAM_BMM_SHAPES and rows >= 4096 and v.dtype == torch.float32:
        # HBM-bound products (<= 16 K weights per matrix): this library's streaming MFMA kernel,
        # weights in LDS -- the library's kernels reach 3.4 TB/s on these shapes
        _lib.check(_lib.lib().ia_batched_gemm_stream(_ptr(v), _ptr(u), _ptr(out), int(batch), int(rows),
                                                     int(k), int(n), _stream()), 'ia_batched_gemm_stream')
        return out
    ws = _scratch(v.device, 'lt_ws', (_LT_WS_BYTES // 4,))
    _lib.check(_lib.lib().ia_batched_gemm(_ptr(v), _ptr(u), _ptr(out), int(batch), int(rows), int(k),
                                          int(n), _ptr(ws), _LT_WS_BYTES, _stream()),
               'ia_batched_gemm')
    return out


FUSE_IN_GEMM = True    # False: input_transform + batched_gemm (tests compare the two bit for bit)
FUSE_OUT = True        # False: ia_wino_in_gemm into M + output_transform (the same bits, two launches)
_IN_GEMM_CHANNELS = (64,)      # ia_wino_in_gemm: Cin == Cout in this list


def pack_u_fragments(u):
    """U (36, Cin, Cout) -> the MFMA fragment order ia_wino_in_gemm reads, (36, Cout/16, Cin/16, 64, 4):
    packed[k][nb][j][16 q + p][c] = u[k][16 j + 4 q + c][16 nb + p]"""
    b, k, n = u.shape
    if k % 16 or n % 16:
        raise ValueError('fragment order needs multiples of 16 channels')
    return u.reshape(b, k // 16, 4, 4, n // 16, 16).permute(0, 4, 1, 2, 5, 3).contiguous() \
            .view(b, n // 16, k // 16, 64, 4)


def input_transform_gemm(plan, xs, u_packed, out, pre=None, epilogue=None):
    """out (36, T, C) = input_transform(xs) @ U in one launch (V stays on chip): the bits of
    input_transform followed by ia_batched_gemm_stream.  Not a pure transform, so not `_timed`.
    epilogue = (bias or None, relu, ys), out None: the output transform runs on the accumulators in
    the same launch (ia_wino_conv3x3_c64) and writes the per-level channels-last tensors ys -- the
    bits of output_transform on `out`, M never written.  Returns ys."""
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    ps, pb, pr = pre if pre is not None else (None, None, False)
    if epilogue is not None:
        bias, relu, ys = epilogue
        if out is not None or len(ys) != len(xs):
            raise ValueError('the one-launch form writes ys, one per level, and no M')
        yptrs = (C.c_void_p * len(ys))(*[y.data_ptr() for y in ys])
        _lib.check(_lib.lib().ia_wino_conv3x3_c64(C.byref(plan.geom), ptrs, int(xs[0].shape[1]), _ptr(ps),
                                                  _ptr(pb), int(bool(pr)), _ptr(u_packed), _ptr(bias),
                                                  int(bool(relu)), yptrs, _stream()),
                   'ia_wino_conv3x3_c64')
        return ys
    _lib.check(_lib.lib().ia_wino_in_gemm(C.byref(plan.geom), ptrs, int(xs[0].shape[1]), _ptr(ps), _ptr(pb),
                                          int(bool(pr)), _ptr(u_packed), _ptr(out), _stream()),
               'ia_wino_in_gemm')
    return out


class WinogradConv3x3(object):
    """one 3x3 / stride-1 / pad-1 convolution (+bias, +ReLU) over a list of channels-last level
    tensors that do NOT share the weight with other layers' inputs (FPN output convs: one
    instance per level)."""

    def __init__(self, weight, bias, relu=False):
        self.u = transform_weight(weight)
        self.u_packed = None
        if self.u.shape[1] == self.u.shape[2] and self.u.shape[1] in _IN_GEMM_CHANNELS:
            self.u_packed = pack_u_fragments(self.u)
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous()
        self.relu = relu
        self.cin, self.cout = self.u.shape[1], self.u.shape[2]
        if self.cout % 4:
            raise ValueError('output channels must be a multiple of 4')
        self._plans = collections.OrderedDict()

    def usable(self, x):
        # raw kernels, no autograd graph: grad mode off, or an input that carries no gradient
        # (a frozen stage during training; fuse._fast has checked the parameters)
        return _usable(x) and x.shape[1] == self.cin \
            and not (torch.is_grad_enabled() and x.requires_grad)

    def __call__(self, x, pre=None):
        """pre = (scale, shift, relu): x is the raw output of the convolution in front, its folded
        BatchNorm / ReLU is applied while the input transform loads it"""
        # the plan owns scratch buffers (V, M): one per stream, so forwards on different streams
        # do not share them
        key = (x.shape[0], tuple(x.shape[-2:]), x.device, stream_id())
        plan = _plan_for(self._plans, key, lambda: _Plan([tuple(x.shape[-2:])], x.shape[0], x.device))
        if (FUSE_IN_GEMM and self.u_packed is not None and STREAM_BMM
                and (self.cin, self.cout) in _STREAM_BMM_SHAPES and plan.T >= 4096
                and x.dtype == torch.float32):
            # exactly where batched_gemm takes the streaming kernel: the same bits, V not written
            if FUSE_OUT:
                y = torch.empty((x.shape[0], self.cout) + tuple(x.shape[-2:]), dtype=torch.float32,
                                device=x.device, memory_format=torch.channels_last)
                input_transform_gemm(plan, [x], self.u_packed, None, pre, epilogue=(self.bias, self.relu, [y]))
                return y
            m = input_transform_gemm(plan, [x], self.u_packed, plan.buf('m', (36, plan.T, self.cout)), pre)
        else:
            v = input_transform(plan, [x], 1, plan.buf('v', (36, plan.T, self.cin)), pre)
            m = batched_gemm(v, self.u, plan.buf('m', (36, plan.T, self.cout)))
        y = torch.empty((x.shape[0], self.cout) + tuple(x.shape[-2:]), dtype=torch.float32,
                        device=x.device, memory_format=torch.channels_last)
        output_transform(plan, m, self.cout, 1, self.bias, self.relu, [(0, self.cout, [y], 0)])
        return y


def plain_3x3(conv):
    """3x3 / stride 1 / pad 1 / dilation 1 / groups 1: what F(4x4,3x3) computes.  The callers
    conjoin what else their route needs (channel multiples, bias, module type, padding mode)."""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1)


def _pair(a, b, F, granule):
    """one or two output convolutions on one tower: (U (36, F, n_pad), bias (n_pad,), n_a, n_b);
    b None: n_b = 0.  n_pad = n_a + n_b rounded up to `granule`: the caller's, because N selects
    the GEMM kernel from the committed table."""
    na, nb = a.out_channels, (0 if b is None else b.out_channels)
    n_pad = (na + nb + granule - 1) // granule * granule
    dev = a.weight.device
    u = torch.zeros((36, F, n_pad), dtype=torch.float32, device=dev)
    u[:, :, :na] = transform_weight(a.weight)
    bias = torch.zeros(n_pad, dtype=torch.float32, device=dev)
    bias[:na] = a.bias.detach().float()
    if b is not None:
        u[:, :, na:na + nb] = transform_weight(b.weight)
        bias[na:na + nb] = b.bias.detach().float()
    return u.contiguous(), bias.contiguous(), na, nb


class _WinogradTowers(object):
    """the two conv towers of a head, all levels at once: layer 0 one GEMM with 2F output columns
    on the shared input, layers 1..n-1 72 matrices (cls tower = channels [0,F), reg tower =
    [F,2F)), activations ping-pong between the plan's 'a' / 'b' sets.  A subclass supplies the
    layer epilogue (`_layer_out`) and the output convolutions behind `_towers`.  Where that epilogue
    is plain bias + ReLU the subclass sets `mid_bias` (per layer (2F,)) and the activations between
    the layers stay on chip: `mid_transform` instead of `_layer_out` + `input_transform`."""

    FUSE_MID = True       # False: the two-launch route (tests compare the two bit for bit)
    mid_bias = None
    u0_3 = None           # split3_pack_u of u0 / of each u[i], where a subclass routes the split GEMM
    u_3 = None

    def __init__(self, head):
        convs_c, convs_r = list(head.cls_convs), list(head.reg_convs)
        self.n_layers = len(convs_c)
        F = head.feat_channels
        if head.in_channels % 4 or F % 4:
            raise ValueError('channel counts must be multiples of 4')
        self.F, self.cin = F, head.in_channels
        self.u0 = torch.cat([transform_weight(convs_c[0].conv.weight),
                             transform_weight(convs_r[0].conv.weight)], dim=2).contiguous()  # (36, Cin, 2F)
        self.u = [torch.cat([transform_weight(convs_c[i].conv.weight),
                             transform_weight(convs_r[i].conv.weight)], dim=0).contiguous()  # (72, F, F)
                  for i in range(1, self.n_layers)]
        self._plans = collections.OrderedDict()

    def usable(self, feats):
        return all(_usable(x) and x.shape[1] == self.cin for x in feats) \
            and not torch.is_grad_enabled()

    def _towers(self, feats):
        """-> (plan, V of the towers' last activations (72, T, F): [:36] cls, [36:] reg, new);
        new(c): per-level channels-last (B, c, H, W) output tensors"""
        B, dev = feats[0].shape[0], feats[0].device
        sizes = [tuple(x.shape[-2:]) for x in feats]
        key = (B, tuple(sizes), dev, stream_id())
        plan = _plan_for(self._plans, key, lambda: _Plan(sizes, B, dev))
        T, F = plan.T, self.F
        # layer 0
        u3 = (lambda i: self.u_3[i]) if self.u_3 is not None else (lambda i: None)  # noqa: E731
        v = input_transform(plan, feats, 1, plan.buf('v', (36, T, self.cin)))
        m = batched_gemm(v, self.u0, plan.buf('m', (36, T, 2 * F)), self.u0_3)
        new = lambda c: [torch.empty((B, c, h, w), dtype=torch.float32, device=dev,  # noqa: E731
                                     memory_format=torch.channels_last) for (h, w) in sizes]
        if self.FUSE_MID and self.mid_bias is not None and F % MID_CHANNELS == 0:
            # plain bias + ReLU layers: M of a layer -> V of the next in one launch; the ping-pong
            # activation tensors are not touched (layer 0's M is ONE group of 2F columns)
            groups = 1
            for i, u in enumerate(self.u):
                v = mid_transform(plan, m, 2 * F, groups, self.mid_bias[i], True,
                                  plan.buf('v', (72, T, F)), 2)
                m = batched_gemm(v, u, plan.buf('m', (72, T, F)), u3(i))
                groups = 2
            v = mid_transform(plan, m, 2 * F, groups, self.mid_bias[self.n_layers - 1], True,
                              plan.buf('v', (72, T, F)), 2)
            return plan, v, new
        acts = plan.acts('a', 2 * F)
        self._layer_out(plan, m, 1, 0, acts)
        # layers 1..n-1: groups = 2
        for i, u in enumerate(self.u):
            v = input_transform(plan, acts, 2, plan.buf('v', (72, T, F)))
            m = batched_gemm(v, u, plan.buf('m', (72, T, F)), u3(i))
            nxt = plan.acts('b' if acts is plan.acts('a', 2 * F) else 'a', 2 * F)
            self._layer_out(plan, m, 2, i + 1, nxt)
            acts = nxt
        v = input_transform(plan, acts, 2, plan.buf('v', (72, T, F)))
        return plan, v, new

    @staticmethod
    def _out_conv(plan, v, name, u, bias, segments, u3=None):
        """one tower's output convolutions: a GEMM with u.shape[2] columns, scattered to `segments`"""
        n = u.shape[2]
        m = batched_gemm(v, u, plan.buf(name, (36, plan.T, n)), u3)
        output_transform(plan, m, n, 1, bias, False, segments)


class WinogradHead(_WinogradTowers):
    """the conv towers (bias + ReLU inside the output transform) and output convolutions of an
    IoUawareRetinaHead: retina_cls on the cls tower, retina_reg | retina_iou on the reg tower."""

    def __init__(self, head):
        convs_c, convs_r = list(head.cls_convs), list(head.reg_convs)
        if any(m.with_norm or not m.with_activatation for m in convs_c + convs_r):
            raise NotImplementedError('towers with norm layers / without ReLU')
        super(WinogradHead, self).__init__(head)

        def bias(m):
            conv = m.conv
            b = conv.bias if conv.bias is not None else torch.zeros(conv.out_channels,
                                                                     device=conv.weight.device)
            return b.detach().float()

        # per layer: the two towers' biases side by side (2F,)
        self.b = [torch.cat([bias(mc), bias(mr)]).contiguous() for mc, mr in zip(convs_c, convs_r)]
        self.mid_bias = self.b
        if head.retina_cls.out_channels % 4:
            raise ValueError('A*C must be a multiple of 4')
        # retina_cls goes in unpadded, reg | iou padded to 16 columns
        self.u_cls, self.b_cls, self.c_cls, _ = _pair(head.retina_cls, None, self.F, 1)
        self.u_ri, self.b_ri, self.c_reg, self.c_iou = _pair(head.retina_reg, head.retina_iou,
                                                             self.F, 16)
        # the products in _SPLIT_SHAPES run on the split GEMM: their U split once, here
        pack = lambda u: split3_pack_u(u) if split_shape(u) else None  # noqa: E731
        self.u0_3 = pack(self.u0)
        self.u_3 = [pack(u) for u in self.u]
        self.u_cls3 = pack(self.u_cls)

    def _layer_out(self, plan, m, groups, i, acts):
        output_transform(plan, m, 2 * self.F, groups, self.b[i], True, [(0, 2 * self.F, acts, 0)])

    def __call__(self, feats):
        """feats: per-level (B, Cin, H, W) channels-last fp32 -> (cls[L], reg[L], iou[L])"""
        plan, v, new = self._towers(feats)
        cls, reg, iou = new(self.c_cls), new(self.c_reg), new(self.c_iou)
        # the 548 MB class logits are written FIRST: the (MFMA-bound) reg / iou GEMM behind them
        # gives their write-back time to drain before the row-max kernel streams them back in
        # (round 6, measured again in bench steps, 2 x 20 steps each: class logits LAST -> decode stage 0.133 ms
        # in-step against 0.120-0.121 this way; gpurun_out/r06_ab_clslast.txt)
        self._out_conv(plan, v[:36], 'mc', self.u_cls, self.b_cls, [(0, self.c_cls, cls, 0)], self.u_cls3)
        self._out_conv(plan, v[36:], 'mr', self.u_ri, self.b_ri,
                       [(0, self.c_reg, reg, 0), (self.c_reg, self.c_iou, iou, 0)])
        return cls, reg, iou


class WinogradFCOSHead(_WinogradTowers):
    """the GN conv towers and output convolutions of an IoUawareFCOSHead or a plain FCOSHead:
    every tower layer is a Winograd convolution without bias / ReLU followed by the
    HIP GroupNorm + ReLU over both towers (csrc/groupnorm.hip: 2 x num_groups groups, the two
    towers' affine parameters side by side); outputs fcos_cls | fcos_centerness on the cls tower,
    fcos_reg | fcos_iou (plain head: fcos_reg alone) on the reg tower, then exp(scale_l * reg) per
    level in place."""

    def __init__(self, head):
        convs_c, convs_r = list(head.cls_convs), list(head.reg_convs)
        for m in convs_c + convs_r:
            if not (m.with_norm and m.norm_cfg.get('type') == 'GN' and m.with_activatation
                    and m.conv.bias is None and m.activate_last and plain_3x3(m.conv)):
                raise NotImplementedError('FCOS towers other than 3x3 conv (no bias) + GN + ReLU')
        super(WinogradFCOSHead, self).__init__(head)
        self.groups = 2 * int(convs_c[0].norm.num_groups)
        self.eps = float(convs_c[0].norm.eps)
        if any(float(m.norm.eps) != self.eps or 2 * int(m.norm.num_groups) != self.groups
               for m in convs_c + convs_r):
            raise NotImplementedError('towers with different GroupNorm settings')
        # per layer: the two towers' affine parameters side by side (2F,)
        self.gn = [(torch.cat([mc.norm.weight.detach(), mr.norm.weight.detach()]).float().contiguous(),
                    torch.cat([mc.norm.bias.detach(), mr.norm.bias.detach()]).float().contiguous())
                   for mc, mr in zip(convs_c, convs_r)]
        self.u_cc, self.b_cc, self.c_cls, self.c_ctr = _pair(head.fcos_cls, head.fcos_centerness,
                                                             self.F, 16)
        # the plain FCOSHead has no IoU branch: its reg tower feeds fcos_reg alone (c_iou = 0)
        self.u_ri, self.b_ri, self.c_reg, self.c_iou = _pair(head.fcos_reg,
                                                             getattr(head, 'fcos_iou', None),
                                                             self.F, 16)
        if self.c_reg % 4:
            raise ValueError('the regression output needs a multiple of 4 channels')
        self.scales = torch.stack([s.scale.detach().float() for s in head.scales]).contiguous()
        self.calls = 0                        # forwards served (tests: the route was taken)

    def usable(self, feats):
        return len(feats) <= self.scales.numel() and super(WinogradFCOSHead, self).usable(feats)

    def _layer_out(self, plan, m, groups, i, acts):
        from .fcos_ops import groupnorm_relu_
        output_transform(plan, m, 2 * self.F, groups, None, False, [(0, 2 * self.F, acts, 0)])
        g, b = self.gn[i]
        groupnorm_relu_(acts, g, b, self.groups, self.eps, relu=True)

    def __call__(self, feats):
        """feats: per-level (B, Cin, H, W) channels-last fp32 -> (cls[L], bbox[L], centerness[L],
        iou[L]) (plain head: (cls[L], bbox[L], centerness[L])), channels-last"""
        plan, v, new = self._towers(feats)
        cls, ctr, reg = new(self.c_cls), new(self.c_ctr), new(self.c_reg)
        iou = new(self.c_iou) if self.c_iou else None
        self._out_conv(plan, v[:36], 'mc', self.u_cc, self.b_cc,
                       [(0, self.c_cls, cls, 0), (self.c_cls, self.c_ctr, ctr, 0)])
        segs = [(0, self.c_reg, reg, 0)]
        if iou is not None:
            segs.append((self.c_reg, self.c_iou, iou, 0))
        self._out_conv(plan, v[36:], 'mr', self.u_ri, self.b_ri, segs)
        ptrs = (C.c_void_p * len(reg))(*[t.data_ptr() for t in reg])
        _lib.check(_lib.lib().ia_scale_exp_levels(C.byref(plan.geom), ptrs, self.c_reg,
                                                  _ptr(self.scales), _stream()),
                   'ia_scale_exp_levels')
        self.calls += 1
        if iou is None:
            return cls, reg, ctr
        return cls, reg, ctr, iou

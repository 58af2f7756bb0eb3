"""helpers for the -m gpu parity tests"""
import numpy as np
import torch

import synth


def product_base_anchors(strides=synth.STRIDES, octave_base_scale=4, scales_per_octave=3,
                         ratios=(0.5, 1.0, 2.0)):
    """the base anchors the PRODUCT generates (iouaware/anchors.py, the generator behind
    head.geometry) -- the HIP path must not be fed the checker's anchors"""
    from iouaware.anchors import AnchorGenerator
    scales = np.array([2 ** (i / scales_per_octave) for i in range(scales_per_octave)]) \
        * octave_base_scale
    return np.stack([AnchorGenerator(s, scales, list(ratios)).base_anchors.numpy()
                     for s in strides])


def geometry(pad_h, pad_w, nms_pre, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), softmax=False):
    """-> (HIP geometry built from the product's anchor generator, the ORACLE's base anchors for
    the checker side); the two generators must agree bit for bit"""
    import oracle
    from iouaware import ops
    sizes = synth.level_shapes(pad_h, pad_w)
    base_oracle = oracle.head_base_anchors(synth.STRIDES)
    base = product_base_anchors()
    assert base.dtype == np.float32 and np.array_equal(base, base_oracle)
    return ops.HeadGeometry(sizes, synth.STRIDES, base, synth.C, nms_pre=nms_pre, means=means,
                            stds=stds, softmax=softmax), base_oracle


def to_dev(arrs, dtype=torch.float32):
    return [torch.from_numpy(a).cuda().to(dtype) for a in arrs]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """bitwise equality, except that +0 == -0"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | ((a == 0) & (b == 0))).all())


def close(a, b, tol=1e-4):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return True
    return bool((np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all())


def bf16_round(arrs):
    """round fp32 numpy arrays to bf16 (RNE) and return them as fp32"""
    return [torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy() for a in arrs]


# ------------------------------------------------------------------ the FCOS loss node on channels-last rows
# (ia_point_head_loss_*_nhwc through ctypes; shared by test_gpu_point_loss_nhwc.py and
# test_gpu_fcos_loss_edges.py)
def point_rows(vals, iou_branch, dtype, wc, wr, num_classes, fill=7.0):
    """(cls, reg, ctr, iou) per-level NCHW arrays -> (B, H, W, width) rows [cls | ctr | fill] and
    [reg | iou? | fill] per level, on the device"""
    cc, ri = [], []
    for l in range(len(vals[0])):
        cls, reg, ctr = (torch.from_numpy(np.array(m[l])) for m in vals[:3])
        B, _, h, w = cls.shape
        a = torch.full((B, h, w, wc), fill)
        a[..., :num_classes] = cls.permute(0, 2, 3, 1)
        a[..., num_classes] = ctr[:, 0]
        b = torch.full((B, h, w, wr), fill)
        b[..., :4] = reg.permute(0, 2, 3, 1)
        if iou_branch:
            b[..., 4] = torch.from_numpy(np.array(vals[3][l]))[:, 0]
        cc.append(a.to('cuda:0', dtype))
        ri.append(b.to('cuda:0', dtype))
    return cc, ri


def point_row_ptrs(cc, ri, iou_branch, off_ctr, off_iou=4):
    from iouaware import _lib
    p, st = _lib.PointLevelPtrs(), _lib.PointPixStrides()
    es = cc[0].element_size()
    for l in range(len(cc)):
        p.cls[l], p.ctr[l] = cc[l].data_ptr(), cc[l].data_ptr() + off_ctr * es
        p.reg[l] = ri[l].data_ptr()
        p.iou[l] = ri[l].data_ptr() + off_iou * es if iou_branch else None
        st.cls[l] = st.ctr[l] = cc[l].shape[-1]
        st.reg[l] = st.iou[l] = ri[l].shape[-1]
    return p, st


def point_row_maps(grads, iou_branch, num_classes):
    """gradient rows (g_cc, g_ri, g_sc) -> {kind: [L] (B, ch, H, W) float64 arrays}, 'scale': (L,)"""
    g_cc, g_ri, g_sc = grads
    f = lambda t: t.detach().double().cpu().permute(0, 3, 1, 2).numpy()   # noqa: E731
    C = num_classes
    m = dict(cls=[f(t[..., :C]) for t in g_cc], ctr=[f(t[..., C:C + 1]) for t in g_cc],
             reg=[f(t[..., :4]) for t in g_ri])
    if iou_branch:
        m['iou'] = [f(t[..., 4:5]) for t in g_ri]
    if g_sc is not None:
        m['scale'] = g_sc.double().cpu().numpy()
    return m


class PointRowsNode(object):
    """the node on rows of `vals`, targets from the HIP assigner: forward once, backward per upstream
    vector, through ctypes.  scales None: the reg row holds the distances"""

    def __init__(self, sizes, strides, num_classes, ranges, gb, gl, iou_branch, vals, dtype, wc, wr,
                 scales=None, cfg=(2.0, 0.25, 1, 0)):
        import ctypes as C
        from iouaware import _lib, fcos_ops
        self.C_, self.NL, self.nc = C, len(sizes), num_classes
        dev = lambda xs: [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]   # noqa: E731
        self.L, self.iou, self.B = _lib.lib(), iou_branch, len(gb)
        self.geom = fcos_ops.PointGeometry(sizes, strides, num_classes)
        self.lab, self.tgt, self.counts = fcos_ops.point_targets(self.geom, dev(gb), dev(gl), ranges)
        self.cc, self.ri = point_rows(vals, iou_branch, dtype, wc, wr, num_classes)
        self.dt = _lib.IA_BF16 if dtype == torch.bfloat16 else _lib.IA_F32
        self.p, self.st = point_row_ptrs(self.cc, self.ri, iou_branch, num_classes)
        self.pt = _lib.PointTargets()
        for l in range(self.NL):
            self.pt.labels[l], self.pt.bbox_targets[l] = self.lab[l].data_ptr(), self.tgt[l].data_ptr()
        self.pt.counts = self.counts.data_ptr()
        self.cfg = _lib.PointLossCfg(*cfg)
        self.sc = torch.from_numpy(np.asarray(scales, np.float32)).cuda() if scales is not None else None
        self.nbytes = self.L.ia_point_head_loss_nhwc_workspace_bytes(self.geom.ref(), self.B)
        assert self.nbytes > 0
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device='cuda:0')
        self.res = torch.full((6,), -7.0, device='cuda:0')

    def _p(self, t):
        return self.C_.c_void_p(t.data_ptr()) if t is not None else None

    def fwd(self, **kw):
        C = self.C_
        a = dict(geom=self.geom, p=self.p, st=self.st, dt=self.dt, B=self.B, sc=self.sc, ws=self.ws, n=self.nbytes)
        a.update(kw)
        return self.L.ia_point_head_loss_fwd_nhwc(
            a['geom'].ref(), C.byref(a['p']), C.byref(a['st']), a['dt'], a['B'], C.byref(self.pt),
            C.byref(self.cfg), self._p(a['sc']), self._p(a['ws']), a['n'], self._p(self.res), None)

    def new_grads(self, fill=float('nan')):
        return ([torch.full_like(t, fill) for t in self.cc], [torch.full_like(t, fill) for t in self.ri],
                torch.full((self.NL,), fill, device='cuda:0') if self.sc is not None else None)

    def bwd(self, gin, grads, packed=1, **kw):
        C = self.C_
        g_cc, g_ri, g_sc = grads
        gp, gst = point_row_ptrs(g_cc, g_ri, self.iou, self.nc)
        a = dict(p=self.p, st=self.st, dt=self.dt, sc=self.sc, gp=gp, gst=gst, g_sc=g_sc, n=self.nbytes)
        a.update(kw)
        return self.L.ia_point_head_loss_bwd_nhwc(
            self.geom.ref(), C.byref(a['p']), C.byref(a['st']), a['dt'], self.B, C.byref(self.pt),
            C.byref(self.cfg), self._p(a['sc']), self._p(self.ws), a['n'], self._p(self.res),
            self._p(gin), C.byref(a['gp']), C.byref(a['gst']), packed, self._p(a['g_sc']), None)

    def run_upstream(self, upstream):
        """-> the six result floats, gradient rows for the upstream vector (4 floats)"""
        assert self.fwd() == 0
        grads = self.new_grads()
        assert self.bwd(torch.tensor(list(upstream), dtype=torch.float32, device='cuda:0'), grads) == 0
        torch.cuda.synchronize()
        return self.res.cpu().numpy(), grads

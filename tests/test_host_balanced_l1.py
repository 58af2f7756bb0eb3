"""CPU side of BalancedL1Loss: the reference configs build with it through the registry, the new C
struct and the header <-> ctypes agreement, the argument checks of the *_box entries that need no device,
the yardstick (tests/balanced_l1_ref.py) against the reference's recorded numbers, and the table E_ref
-- a plain float32 torch evaluation against the yardstick on the edge data of
tests/test_gpu_balanced_l1.py -- on which the GPU bars rest."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import balanced_l1_ref as BL
import synth
import test_gpu_balanced_l1 as E
from test_gpu_loss_edges import rel, share_of_max

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, 'golden')
HEADER = os.path.join(ROOT, 'include', 'iouaware.h')
IA_E_ARG = -1

CONFIGS = [('ref_configs.json', 'iou_aware_retinanet_r50_fpn_1x_4gpu'),
           ('ref_configs.json', 'iou_aware_retinanet_r50_fpn_1x_2gpu'),
           ('retina_plain_ref.json', 'retinanet_r50_fpn_1x_2gpu'),
           ('retina_plain_ref.json', 'retinanet_r50_fpn_1x_4gpu')]


# ------------------------------------------------------------------ 1: registry
@pytest.mark.parametrize('fixture,config', CONFIGS)
def test_reference_configs_build_with_balanced_l1(fixture, config):
    import iouaware
    from iouaware.config import ConfigDict
    from iouaware.losses import BalancedL1Loss
    with open(os.path.join(GOLD, fixture)) as fh:
        rec = json.load(fh)[config]
    rec['model']['pretrained'] = None
    rec['model']['bbox_head']['loss_bbox'] = dict(type='BalancedL1Loss', alpha=0.75, gamma=1.25, beta=0.11,
                                                  loss_weight=2.0)
    model = iouaware.build_detector(ConfigDict(rec['model']), train_cfg=ConfigDict(rec['train_cfg']),
                                    test_cfg=ConfigDict(rec['test_cfg']))
    lb = model.bbox_head.loss_bbox
    assert type(lb) is BalancedL1Loss and iouaware.LOSSES.get('BalancedL1Loss') is BalancedL1Loss
    assert (lb.alpha, lb.gamma, lb.beta, lb.loss_weight) == (0.75, 1.25, 0.11, 2.0)
    d = BalancedL1Loss()
    assert (d.alpha, d.gamma, d.beta, d.loss_weight) == (0.5, 1.5, 1.0, 1.0)
    # the switch of the all-levels node admits it, on both heads, without fuse_balanced
    class _FakeMap(object):
        is_cuda = True
        dtype = torch.float32
    assert model.bbox_head.fuse_balanced is False
    # (the _2gpu / _4gpu plain configs name the IoU-balanced focal loss, which RetinaHead does not train)
    plain_focal = type(model.bbox_head.loss_cls).__name__ == 'FocalLoss'
    assert bool(model.bbox_head._fused_loss_ok([_FakeMap()] * 5)) == plain_focal
    assert not model.bbox_head._fused_loss_ok([torch.zeros(1, 1, 1, 1)])
    from iouaware import compat
    compat.install()
    import mmdet.models.losses as ml
    assert ml.BalancedL1Loss is BalancedL1Loss


# ------------------------------------------------------------------ 2: struct and bindings
def test_box_loss_cfg_layout_and_header():
    from iouaware import _lib
    S = _lib.BoxLossCfg
    assert [f[0] for f in S._fields_] == ['struct_size', 'kind', 'alpha', 'gamma']
    assert C.sizeof(S) == 16
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12]
    assert [t for _, t in S._fields_] == [C.c_int32, C.c_int32, C.c_float, C.c_float]
    txt = open(HEADER).read()
    body = re.search(r'typedef struct ia_box_loss_cfg \{(.*?)\} ia_box_loss_cfg;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    got = []
    for typ, names in re.findall(r'\b(float|int32_t)\s+([^;]+);', body):
        got += [(n.strip(), typ) for n in names.split(',')]
    assert got == [(n, 'float' if t is C.c_float else 'int32_t') for n, t in S._fields_]
    assert re.search(r'#define IA_BOX_SMOOTH_L1 0\b', txt) and re.search(r'#define IA_BOX_BALANCED_L1 1\b', txt)
    assert (_lib.IA_BOX_SMOOTH_L1, _lib.IA_BOX_BALANCED_L1) == (0, 1)
    # ia_head_loss_cfg is untouched
    assert C.sizeof(_lib.HeadLossCfg) == 48


def test_new_entries_are_declared_bound_and_exported():
    from iouaware import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = C.CDLL(_lib.SO_PATH)
    for old in ('ia_head_loss_fwd', 'ia_head_loss_bwd', 'ia_head_loss_fwd_nhwc', 'ia_head_loss_bwd_nhwc'):
        new = old + '_box'
        assert new in _lib.SIGNATURES and hasattr(h, new)
        # the arguments of the old entry plus one pointer to the struct, behind cfg
        a_old, a_new = list(_lib.SIGNATURES[old][1]), list(_lib.SIGNATURES[new][1])
        assert a_new[:6] == a_old[:6] and a_new[7:] == a_old[6:]
        assert a_new[6] is C.POINTER(_lib.BoxLossCfg)
        decl = re.search(r'int %s\((.*?)\);' % new, txt, re.S).group(1)
        assert re.search(r'const ia_head_loss_cfg \*cfg,\s*const ia_box_loss_cfg \*box,', decl)
        assert decl.count(',') + 1 == len(a_new)
    for name, n in (('ia_balanced_l1_fwd', 12), ('ia_balanced_l1_bwd', 14)):
        assert name in _lib.SIGNATURES and hasattr(h, name) and len(_lib.SIGNATURES[name][1]) == n
        decl = re.search(r'int %s\((.*?)\);' % name, txt, re.S).group(1)
        assert decl.count(',') + 1 == n and re.search(r'float beta, float alpha, float gamma', decl)


# ------------------------------------------------------------------ 3: argument checks without a device
class _Call(object):
    """the four *_box entries on a valid geometry and non-NULL (never dereferenced) pointers: a refused
    struct returns IA_E_ARG before anything else is looked at or enqueued"""

    def __init__(self):
        import gpu_util as G
        from iouaware import _lib, ops
        self._lib, self.lib = _lib, _lib.lib()
        sizes = synth.level_shapes(64, 96)
        self.L = len(sizes)
        self.geoms = {ib: ops.HeadGeometry(sizes, synth.STRIDES, G.product_base_anchors(), synth.C, iou_branch=ib)
                      for ib in (True, False)}
        self.buf = (C.c_char * 4096)()                   # host memory: an aligned stand-in for every pointer
        self.ptr = (C.addressof(self.buf) + 255) // 256 * 256

    def cfg(self, beta=0.11, bal_cls=0, bal_loc=0):
        return self._lib.HeadLossCfg(2.0, 0.25, 1.0, beta, 1.0, 1, 0, 0, 1.5, 1.5, bal_cls, bal_loc)

    def box(self, kind=1, alpha=0.5, gamma=1.5, size=None):
        S = self._lib.BoxLossCfg
        return S(C.sizeof(S) if size is None else size, kind, alpha, gamma)

    def __call__(self, entry, hc, bc, iou_branch=True):
        _lib = self._lib
        p, st, ht = _lib.LevelPtrs(), _lib.LevelPixStrides(), _lib.HeadTargets()
        for l in range(self.L):
            p.cls[l] = p.reg[l] = self.ptr
            p.iou[l] = self.ptr if iou_branch else None
            st.cls[l], st.reg[l], st.iou[l] = synth.A * synth.C, synth.A * 4, synth.A
            ht.labels[l] = ht.label_weights[l] = ht.bbox_targets[l] = ht.bbox_weights[l] = self.ptr
        ht.avg_factor = 1.0
        g = self.geoms[iou_branch].ref()
        b = None if bc is None else C.byref(bc)
        v = self.ptr
        if entry == 'fwd':
            return self.lib.ia_head_loss_fwd_box(g, C.byref(p), _lib.IA_F32, 2, C.byref(ht), C.byref(hc), b,
                                                 v, 1 << 30, v, None)
        if entry == 'bwd':
            return self.lib.ia_head_loss_bwd_box(g, C.byref(p), _lib.IA_F32, 2, C.byref(ht), C.byref(hc), b,
                                                 v, v, v, C.byref(p), None)
        if entry == 'fwd_nhwc':
            return self.lib.ia_head_loss_fwd_nhwc_box(g, C.byref(p), C.byref(st), 2, C.byref(ht), C.byref(hc),
                                                      b, v, 1 << 30, v, None)
        return self.lib.ia_head_loss_bwd_nhwc_box(g, C.byref(p), C.byref(st), 2, C.byref(ht), C.byref(hc), b,
                                                  v, v, C.byref(p), C.byref(st), None)


@pytest.mark.parametrize('entry', ['fwd', 'bwd', 'fwd_nhwc', 'bwd_nhwc'])
def test_box_entries_refuse_a_bad_struct_before_anything_is_enqueued(entry):
    """no device is touched: every call below returns from the struct check"""
    c = _Call()
    ok = c.cfg()
    for iou_branch in (True, False):
        assert c(entry, ok, c.box(size=12), iou_branch) == IA_E_ARG          # a wrong struct_size
        assert c(entry, ok, c.box(size=0), iou_branch) == IA_E_ARG
        assert c(entry, ok, c.box(size=20, kind=0), iou_branch) == IA_E_ARG  # whatever the kind
        assert c(entry, ok, c.box(kind=2), iou_branch) == IA_E_ARG           # an unknown kind
        assert c(entry, ok, c.box(kind=-1), iou_branch) == IA_E_ARG
        for bad in (0.0, -0.5, float('nan')):                                # alpha, gamma, beta not > 0
            assert c(entry, ok, c.box(alpha=bad), iou_branch) == IA_E_ARG
            assert c(entry, ok, c.box(gamma=bad), iou_branch) == IA_E_ARG
            assert c(entry, c.cfg(beta=bad), c.box(), iou_branch) == IA_E_ARG
        assert c(entry, ok, c.box(alpha=1e-3, gamma=1.0), iou_branch) == IA_E_ARG   # e^1000: no fp32 b
    # kind 1 together with the IoU-balanced smooth-L1 weighting
    assert c(entry, c.cfg(bal_loc=1), c.box()) == IA_E_ARG
    assert c(entry, c.cfg(bal_cls=1, bal_loc=1), c.box()) == IA_E_ARG


def test_the_per_level_entries_refuse_bad_parameters_without_a_device():
    from iouaware import _lib
    lib = _lib.lib()
    buf = (C.c_char * 64)()
    v = C.addressof(buf)
    for beta, alpha, gamma in ((0.0, 0.5, 1.5), (0.11, 0.0, 1.5), (0.11, 0.5, 0.0), (-1.0, 0.5, 1.5),
                               (0.11, float('nan'), 1.5), (0.11, 1e-3, 1.0)):
        assert lib.ia_balanced_l1_fwd(v, _lib.IA_F32, v, v, 1, 1, 1, beta, alpha, gamma, v, None) == IA_E_ARG
        assert lib.ia_balanced_l1_bwd(v, _lib.IA_F32, v, v, 1, 1, 1, beta, alpha, gamma, 1.0, None, v,
                                      None) == IA_E_ARG
    assert lib.ia_balanced_l1_fwd(v, 99, v, v, 1, 1, 1, 0.11, 0.5, 1.5, v, None) == IA_E_ARG
    assert lib.ia_balanced_l1_fwd(None, _lib.IA_F32, v, v, 1, 1, 1, 0.11, 0.5, 1.5, v, None) == IA_E_ARG


def test_head_loss_refuses_delta_with_balanced_l1_and_cpu_tensors():
    from iouaware import _lib, ops
    from iouaware.losses import BalancedL1Loss
    with pytest.raises(_lib.IouAwareLibraryError):
        BalancedL1Loss()(torch.zeros(3, 4), torch.zeros(3, 4), torch.ones(3, 4), avg_factor=1.0)
    with pytest.raises(ValueError):
        ops._box_loss_cfg(('huber', 1.0, 1.0))
    bc = ops._box_loss_cfg(('balanced_l1', 0.25, 1.0))
    assert (bc.struct_size, bc.kind, bc.alpha, bc.gamma) == (16, 1, 0.25, 1.0)
    assert ops._box_loss_cfg(None) is None


# ------------------------------------------------------------------ 4: yardstick == recorded reference
def _as_map(v):
    """(n,) -> the (B = n, A*4 = 4, 1, 1) map and (n, 1, 4) rows of balanced_l1_ref, the value in coordinate 0"""
    v = np.asarray(v, np.float32)
    m = np.zeros((v.size, 4, 1, 1), np.float32)
    m[:, 0, 0, 0] = v
    return m


def test_yardstick_reproduces_the_recorded_reference_numbers():
    f = np.load(os.path.join(GOLD, 'balanced_l1.npz'))
    alpha, gamma = float(f['alpha']), float(f['gamma'])
    assert (alpha, gamma, float(f['beta'])) == (0.5, 1.5, float(np.float32(0.11)))
    # the eight elements of the issue's table
    pred = f['el_unit_pred']
    w = np.zeros((pred.size, 1, 4), np.float32)
    w[:, 0, 0] = 1.0
    ref = BL.balanced_l1(_as_map(pred), np.zeros_like(w), w, 1, 0.11, alpha, gamma)
    g = ref['grad'].numpy()[:, 0, 0, 0]
    table = np.array([0, 1.5, 1.7014115, -1.5, 1.5, -1.5, 3.9850621, 0])
    assert np.allclose(f['el_unit_grad'], table, rtol=2e-7, atol=0) and abs(float(f['el_unit_sum']) - 15005.113) < 2e-3
    assert np.abs(g - f['el_unit_grad']).max() <= 1e-6 * np.abs(g).max()
    assert rel(ref['sum'], float(f['el_unit_sum'])) <= 1e-6
    assert g[0] == 0 and g[7] == 0 and g[1] == 1.5 and g[3] == -1.5     # 0 at pred == target; linear at d == beta
    # the planted list, both betas
    for i, beta in enumerate(f['betas']):
        pred, wt = f['el_pred_%d' % i], f['el_weight_%d' % i]
        w = np.zeros((pred.size, 1, 4), np.float32)
        w[:, 0, 0] = wt
        ref = BL.balanced_l1(_as_map(pred), np.zeros_like(w), w, 1, float(beta), alpha, gamma)
        g = ref['grad'].numpy()[:, 0, 0, 0]
        print('beta %g: sum %.9g recorded %.9g, gradient error %.3g' %
              (beta, ref['sum'], float(f['el_sum_%d' % i]), np.abs(g - f['el_grad_%d' % i]).max()))
        assert rel(ref['sum'], float(f['el_sum_%d' % i])) <= 1e-6
        assert np.abs(g - f['el_grad_%d' % i]).max() <= 1e-6 * np.abs(g).max()
        assert bool((g[(wt == 0) | (pred == 0)] == 0).all())
    # the heads' recorded per-level losses are those the issue quotes
    assert np.allclose(f['plain_loss_bbox_0'], [0.8422, 1.1421, 0.5926, 0, 0], atol=5e-5)
    assert np.allclose(f['plain_loss_bbox_1'], [2.9095, 0, 0, 0, 0], atol=5e-5)
    for k in (0, 1):
        assert np.allclose(f['iou_loss_bbox_%d' % k], f['plain_loss_bbox_%d' % k], rtol=1e-6)
    assert os.path.getsize(os.path.join(GOLD, 'balanced_l1.npz')) < 1000000


# ------------------------------------------------------------------ 5: E_ref
def _edge_levels(beta):
    for bf16 in (False, True):
        for name, (h, w) in sorted(E.LEVELS.items()):
            yield bf16, 'level %s' % name, E.bl_level(h, w, beta, 11, bf16=bf16)
        for l, d in enumerate(E.node_data(beta, bf16)[1]):
            yield bf16, 'node level %d' % l, d


@pytest.mark.parametrize('ag', E.AGS, ids=['a.5g1.5', 'a.25g1'])
@pytest.mark.parametrize('beta', E.BETAS)
def test_e_ref_table(beta, ag):
    """float32 torch against the float64 yardstick on the edge data: the measurement the GPU bars rest on.
    The data has what the issue asks for (check_coverage), the yardstick is finite everywhere, and the
    measured errors stay within the table of tests/test_gpu_balanced_l1.py (E_REF)"""
    E.check_coverage([d for bf16, _, d in _edge_levels(beta) if not bf16 and _.startswith('level')], beta)
    E.check_coverage(E.node_data(beta)[1], beta)
    E.check_coverage(E.node_data(beta, True)[1], beta, bf16=True)
    worst_g = worst_s = 0.0
    for bf16, name, d in _edge_levels(beta):
        ref = BL.evaluate(d['reg'], d['bt'], d['bw'], E.A, beta, ag[0], ag[1], E.GS, torch.float64)
        f32 = BL.evaluate(d['reg'], d['bt'], d['bw'], E.A, beta, ag[0], ag[1], E.GS, torch.float32)
        assert f32['grad'].dtype == torch.float32
        assert np.isfinite(ref['sum']) and bool(torch.isfinite(ref['grad']).all())
        g64 = ref['grad'].numpy()
        assert bool((g64[E.weight0_mask(d)] == 0).all()) and bool((g64[E.equal_mask(d)] == 0).all())
        eg, es = share_of_max(f32['grad'].numpy(), g64), rel(f32['sum'], ref['sum'])
        worst_g, worst_s = max(worst_g, eg), max(worst_s, es)
    print('E_ref beta %-5g (alpha, gamma) %-12s gradient %.2g of max   sum %.2g relative'
          % (beta, ag, worst_g, worst_s))
    eg, es = E.E_REF[(beta, ag)]
    # (the table was measured with one CPU's vectorised float32 log; another's may round a little differently)
    assert worst_g <= 1.25 * eg and worst_s <= 1.25 * es

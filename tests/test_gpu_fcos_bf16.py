"""GPU: the bf16 inference path of the FCOS heads -- the bf16 GroupNorm + ReLU pair, the bf16
exp(scale * x), the bf16 instances of the point decode, the head runner
(conv3x3_bf16.Bf16ConvFCOSHead) and the detector end to end.

Yardsticks: fp64 GroupNorm (tests/gn_ref.py) on the same bf16-rounded inputs; the fp32 entries on
the widened tensors (bit for bit: a bf16 value converts exactly and everything behind the load is the
fp32 arithmetic); the fp32 module forward on bf16-rounded weights with torch's own bf16 forward as
the comparator (the project's bf16 contract of test_config3_r101_bf16_whole_network)."""
import copy
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import gn_ref
import synth_fcos
import synth_fcos_plain

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
DEV = torch.device('cuda:0')
BF = torch.bfloat16
CL = torch.channels_last
# GroupNorm: |err| <= 2^-8 |want| + bar * max|want| -- one round-to-nearest-even rounding to bf16
# (half an ulp = 2^-9 of the binade, at most 2^-8 of the value) on top of the fp32 kernels' bars of
# tests/test_gpu_fcos.py (what the fp64 statistics and the fp32 x * s + t leave)
BF16_RNE = 2.0 ** -8
GN_BAR = {0.0: 2e-5, 200.0: 2e-4}
PAD = (128, 192)              # levels (16, 24), (8, 12), (4, 6), (2, 3), (1, 2)


def _levels(pad=PAD):
    return synth_fcos.level_shapes(*pad)


def _acts(seed, B, sizes, ch, mean_over_std=0.0):
    """bf16-rounded activations (as fp32 tensors); every group: std 0.007, mean 0.007 * mean_over_std
    where that is given"""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for (h, w) in sizes:
        x = torch.randn((B, ch, h, w), generator=g) * 0.7
        if mean_over_std:
            x = x * 0.01 + 0.007 * mean_over_std
        xs.append(x.to(BF).float())
    return xs


def _affine(seed, ch):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(ch, generator=g) + 0.5, torch.randn(ch, generator=g) * 0.3


def _gn_run(xs, gamma, beta, groups, relu=True):
    from iouaware import fcos_ops
    dev = [x.to(DEV).to(BF).contiguous(memory_format=CL) for x in xs]
    fcos_ops.groupnorm_relu_(dev, gamma.to(DEV), beta.to(DEV), groups, relu=relu)
    torch.cuda.synchronize()
    assert all(d.dtype == BF for d in dev)
    return [d.cpu() for d in dev]


GN_CASES = {
    # batch, channels, groups, level sizes: level 0 of 'pyramid' is one full chunk of 256 pixels
    # plus a partial one, the others are below a chunk
    'pyramid': (2, 512, 64, _levels()),
    'narrow': (1, 64, 8, [(20, 30)]),
    'odd': (1, 256, 32, [(17, 13)]),
}


@pytest.mark.parametrize('mean_over_std', [0.0, 200.0])
@pytest.mark.parametrize('case', sorted(GN_CASES))
def test_groupnorm_bf16_against_fp64(case, mean_over_std):
    B, ch, groups, sizes = GN_CASES[case]
    xs = _acts(1, B, sizes, ch, mean_over_std)
    gamma, beta = _affine(2, ch)
    want = gn_ref.forward(xs, gamma, beta, groups, dtype=torch.float64)
    got = _gn_run(xs, gamma, beta, groups)
    bar = GN_BAR[mean_over_std]
    for l, (o, r) in enumerate(zip(got, want)):
        err = (o.double() - r).abs()
        bound = BF16_RNE * r.abs() + bar * float(r.abs().max())
        worst = float((err / bound).max())
        print('%s, |mean|/std %g, level %d: worst error / bound %.3f' % (case, mean_over_std, l, worst))
        assert worst <= 1.0, (case, l, worst)


def test_groupnorm_bf16_without_relu():
    B, ch, groups, sizes = GN_CASES['odd']
    xs = _acts(4, B, sizes, ch)
    gamma, beta = _affine(5, ch)
    want = gn_ref.forward(xs, gamma, beta, groups, relu=False, dtype=torch.float64)
    got = _gn_run(xs, gamma, beta, groups, relu=False)
    for o, r in zip(got, want):
        assert float(o.min()) < 0.0
        bound = BF16_RNE * r.abs() + GN_BAR[0.0] * float(r.abs().max())
        assert bool(((o.double() - r).abs() <= bound).all())


def test_groupnorm_bf16_refuses_four_channels_per_group():
    from iouaware import _lib, fcos_ops
    xs = [torch.zeros((1, 256, 4, 4), dtype=BF, device=DEV).contiguous(memory_format=CL)]
    g = fcos_ops._wino_geom(xs)
    L = _lib.lib()
    assert L.ia_groupnorm_workspace_bytes_dt(ctypes.byref(g), 256, 64, _lib.IA_BF16) == 0
    assert L.ia_groupnorm_workspace_bytes_dt(ctypes.byref(g), 256, 64, _lib.IA_F32) > 0
    with pytest.raises(_lib.IouAwareLibraryError):
        fcos_ops.groupnorm_relu_(xs, torch.ones(256, device=DEV), torch.zeros(256, device=DEV), 64)
    # the training node keeps its fp32-only contract
    with pytest.raises(ValueError):
        fcos_ops.groupnorm_relu(xs, torch.ones(256, device=DEV), torch.zeros(256, device=DEV), 32)


def test_groupnorm_bf16_bits_repeat_and_do_not_depend_on_the_batch():
    xs = _acts(3, 3, _levels(), 512, mean_over_std=10.0)
    gamma, beta = _affine(6, 512)
    a = _gn_run(xs, gamma, beta, 64)
    b = _gn_run(xs, gamma, beta, 64)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    alone = _gn_run([x[1:2] for x in xs], gamma, beta, 64)
    assert all(torch.equal(u[1:2], v) for u, v in zip(a, alone))


def test_scale_exp_bf16_is_the_fp32_entry_rounded_once():
    from iouaware import fcos_ops
    g = torch.Generator().manual_seed(7)
    sizes = [(16, 24), (5, 7), (1, 3)]            # 768 / 70 / 6 groups of four: several blocks, odd
    xs = [((torch.rand((2, 4, h, w), generator=g) * 12 - 6).to(BF)).to(DEV).contiguous(memory_format=CL)
          for (h, w) in sizes]
    scales = torch.tensor([0.5, 1.0, 2.3], device=DEV)
    wide = [x.float().contiguous(memory_format=CL) for x in xs]
    fcos_ops.scale_exp_(wide, scales)
    got = [x.clone(memory_format=CL) for x in xs]
    fcos_ops.scale_exp_(got, scales)
    torch.cuda.synchronize()
    for l, (o, w) in enumerate(zip(got, wide)):
        assert o.dtype == BF
        assert torch.equal(o, w.to(BF)), l
        assert not torch.equal(o, xs[l])


# ------------------------------------------------------------------ point decode
VIEWS = ('rowmax', 'cand_idx', 'boxes', 'scores_t', 'best_score')
SHAPES = [(PAD[0] - 20, PAD[1] - 7, 3), (PAD[0], PAD[1] - 48, 3)]
FACTORS = [0.75, 1.5]


def _maps(kind, nhwc, dtype):
    sizes = _levels()
    if kind == 'iou':
        cls, reg, _, third = synth_fcos.head_outputs(31, 2, sizes)
    else:
        cls, reg, third = synth_fcos_plain.head_outputs(31, 2, sizes)
    out = []
    for ts in (cls, reg, third):
        ts = [torch.from_numpy(t).to(DEV).to(BF).to(dtype) for t in ts]
        out.append([t.contiguous(memory_format=CL) for t in ts] if nhwc else ts)
    return out


def _decode(kind, nhwc, dtype, nms_pre, rescale):
    from iouaware import fcos_ops
    geom = fcos_ops.PointGeometry(_levels(), synth_fcos.STRIDES, 80, nms_pre, 0.3)
    cls, reg, third = _maps(kind, nhwc, dtype)
    entry = fcos_ops.point_get_bboxes if kind == 'iou' else fcos_ops.point_ctr_get_bboxes
    dets, labels, rows, num, views = entry(geom, cls, reg, third, SHAPES, FACTORS, rescale, 0.05,
                                           0.5, 100, debug=True)
    torch.cuda.synchronize()
    out = dict((k, views[k].clone()) for k in VIEWS)
    out.update(dets=dets, labels=labels, rows=rows, num=num)
    return out


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('nms_pre', [50, 1000])          # below / above the level sizes (384 ... 2)
@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('kind', ['iou', 'ctr'])
def test_point_decode_bf16_gives_the_bits_of_the_fp32_entries(kind, nhwc, nms_pre, rescale):
    want = _decode(kind, nhwc, torch.float32, nms_pre, rescale)
    got = _decode(kind, nhwc, BF, nms_pre, rescale)
    assert int(want['num'].min()) > 0
    for k in VIEWS + ('num', 'labels', 'rows', 'dets'):
        a, b = got[k], want[k]
        if k in ('labels', 'rows', 'dets'):              # rows past num are not written
            for i in range(2):
                n = int(want['num'][i])
                assert torch.equal(a[i, :n], b[i, :n]), (k, i)
        elif k == 'scores_t':
            R = got['cand_idx'].shape[1]
            assert torch.equal(a[:, :, :R], b[:, :, :R]), k
        else:
            assert torch.equal(a, b), k


def test_point_decode_refuses_mixed_dtypes():
    from iouaware import fcos_ops
    geom = fcos_ops.PointGeometry(_levels(), synth_fcos.STRIDES, 80, 50, 0.3)
    cls, reg, iou = _maps('iou', False, BF)
    reg = [r.float() for r in reg]
    with pytest.raises(TypeError):
        fcos_ops.point_get_bboxes(geom, cls, reg, iou, SHAPES, FACTORS, True, 0.05, 0.5, 100)
    with pytest.raises(TypeError):
        fcos_ops.point_ctr_decode_stage(geom, cls, reg, iou, SHAPES, FACTORS, True, 0.05)


# ------------------------------------------------------------------ model level
def _config(kind):
    if kind == 'iou':
        with open(os.path.join(GOLD, 'fcos_ref.json')) as fh:
            cfg = json.load(fh)['config']
    else:
        with open(os.path.join(GOLD, 'fcos_plain_ref.json')) as fh:
            rec = json.load(fh)['fcos_r50_caffe_fpn_gn_1x_4gpu']
        cfg = dict((k, rec[k]) for k in ('model', 'train_cfg', 'test_cfg'))
    return cfg


def _model(kind, seed):
    """the detector of the config with seeded weights ROUNDED TO bf16 (fp32 storage), eval mode"""
    import iouaware
    from iouaware.config import Config
    cfg = _config(kind)
    with tempfile.NamedTemporaryFile('w', suffix='.py', delete=False) as fh:
        fh.write('\n'.join('%s = %r' % (k, v) for k, v in sorted(cfg.items())) + '\n')
    try:
        cfg = Config.fromfile(fh.name)
    finally:
        os.unlink(fh.name)
    cfg.model['pretrained'] = None
    m = iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    state = m.state_dict()
    synth_fcos.fill_state(state, seed)
    m.load_state_dict(state)
    m = m.to(DEV).eval()
    with torch.no_grad():
        for t in list(m.parameters()) + [b for b in m.buffers() if b.dtype == torch.float32]:
            t.copy_(t.to(BF).float())
    return m


def _bf16(m):
    from iouaware.fuse import fuse_inference
    fuse_inference(m, winograd=True)
    return m.to(memory_format=CL).to(BF)


def _feats(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((2, 256, h, w), generator=g).to(BF).float().to(DEV) for (h, w) in _levels()]


def _rms_rel(a, r):
    return float((a.float() - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp(min=1e-12))


@pytest.mark.parametrize('kind', ['iou', 'ctr'])
def test_bf16_head_route_against_the_fp32_module(kind, monkeypatch):
    m = _model(kind, 5)
    head = m.bbox_head
    feats = _feats(12)
    names = ('cls', 'bbox', 'ctr', 'iou') if kind == 'iou' else ('cls', 'bbox', 'ctr')
    with torch.no_grad():
        ref = head(feats)
        eager = copy.deepcopy(head).to(BF)
        eag = eager([f.to(BF) for f in feats])
        del eager
        _bf16(m)
        entered = []
        real = torch.nn.functional.group_norm
        monkeypatch.setattr(torch.nn.functional, 'group_norm',
                            lambda *a, **k: (entered.append(1), real(*a, **k))[1])
        out = head([f.to(BF).contiguous(memory_format=CL) for f in feats])
        torch.cuda.synchronize()
        monkeypatch.undo()
    runner = head._ia_c3
    assert runner and runner.calls == 1, 'the bf16 FCOS runner was not used'
    assert not entered, 'torch group_norm ran on the fused route'
    assert len(out) == len(ref) == len(names)
    for name, os_, es, rs in zip(names, out, eag, ref):
        for l, (o, e, r) in enumerate(zip(os_, es, rs)):
            assert o.dtype == BF and o.shape == r.shape and o.is_contiguous(memory_format=CL)
            e_route, e_eager = _rms_rel(o, r), _rms_rel(e, r)
            line = '%s %-4s level %d: route %.2e  torch-bf16 %.2e' % (kind, name, l, e_route, e_eager)
            print(line)
            assert e_route <= 1.5 * e_eager + 1e-3, line


def _box_iou(a, b):
    x1, y1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    x2, y2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.clip(x2 - x1 + 1, 0, None) * np.clip(y2 - y1 + 1, 0, None)
    return inter / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) +
                    (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1) - inter)


def _twins(ref, mine, best=25):
    """of the `best` highest-scoring detections of every image of `ref`: how many have a twin (same
    class, IoU > 0.85) in `mine` -> (strong, found)"""
    strong = found = 0
    for r, d in zip(ref, mine):
        rows = sorted(((box[4], c, k) for c in range(80) for k, box in enumerate(r[c])), reverse=True)
        assert len(rows) >= best, 'the fp32 result has %d detections, %d needed' % (len(rows), best)
        for _, c, k in rows[:best]:
            strong += 1
            found += int(len(d[c]) > 0 and float(_box_iou(r[c][k], d[c]).max()) > 0.85)
    return strong, found


META = [dict(ori_shape=(120, 150, 3), img_shape=(120, 150, 3), pad_shape=(128, 160, 3),
             scale_factor=1.0, flip=False)] * 2


@pytest.mark.parametrize('kind', ['iou', 'ctr'])
def test_bf16_detector_keeps_the_fp32_detections(kind):
    """config -> build_detector -> fuse_inference(winograd=True) -> channels-last bf16 ->
    simple_test_batch, against the fp32 modules and torch's own bf16 modules on the same weights"""
    m = _model(kind, 5)
    x = torch.from_numpy(synth_fcos.image(6, 2, 128, 160, 120, 150)).to(DEV).to(BF).float()
    with torch.no_grad():
        ref = m.simple_test_batch(x, META, rescale=True)
        eager = copy.deepcopy(m).to(BF)
        eager_res = eager.simple_test_batch(x.to(BF), META, rescale=True)
        del eager
        mb = _bf16(m)
        res = mb.simple_test_batch(x.to(BF).contiguous(memory_format=CL), META, rescale=True)
    runner = mb.bbox_head._ia_c3
    assert runner and runner.calls == 1, 'the bf16 FCOS runner was not used'
    assert len(res) == 2 and all(len(r) == 80 for r in res)
    assert all(a.ndim == 2 and a.shape[1] == 5 and a.dtype == np.float32 for r in res for a in r)
    strong, found = _twins(ref, res)
    _, found_eager = _twins(ref, eager_res)
    print('%s: %d fp32 detections; with a twin in the bf16 route %d, in torch\'s own bf16 %d'
          % (kind, strong, found, found_eager))
    # the slack of test_config3_r101_bf16_whole_network, for its reason: the library's bf16
    # convolutions in the backbone are not reproducible from run to run
    assert found >= found_eager - strong // 12, (strong, found, found_eager)


def test_bf16_runner_refolds_when_a_gamma_or_a_scale_changes():
    m = _model('iou', 5)
    head = m.bbox_head
    feats = [f.to(BF).contiguous(memory_format=CL) for f in _feats(13)]
    with torch.no_grad():
        _bf16(m)
        a = head(feats)
        first = head._ia_c3
        assert first and first.calls == 1
        head.cls_convs[0].norm.weight.mul_(1.5)
        b = head(feats)
        assert head._ia_c3 is not first and head._ia_c3.calls == 1
        assert not torch.equal(a[0][0], b[0][0])            # class logits moved
        assert torch.equal(a[1][0], b[1][0])                # the reg tower did not
        head.scales[0].scale.mul_(1.25)
        c = head(feats)
        torch.cuda.synchronize()
        assert not torch.equal(b[1][0], c[1][0])
        assert torch.equal(b[1][1], c[1][1]) and torch.equal(b[0][0], c[0][0])

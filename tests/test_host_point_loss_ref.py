"""CPU: the float64 yardstick of the FCOS heads' loss (tests/point_loss_ref.py)

  * held to synth_fcos_loss.yardstick (the head's torch `_loss` body in fp64) on S.SMALL: the losses and
    every gradient of every loss, 1e-12 relative, and on the whole edge set of
    tests/test_gpu_fcos_loss_edges.py (ties included: both split them half and half);
  * held to the reference fixture tests/golden/fcos_loss.npz with the bar of
    test_gpu_fcos_loss.py::test_loss_against_the_reference_fixture;
  * the edge set's conditions, asserted before anything runs on a GPU;
  * E_cpu32, the error of the head's torch body in fp32 on the CPU against the yardstick per form, kind
    and spec group: measured, printed (`pytest -s`) and held below the table recorded in
    test_gpu_fcos_loss_edges.E_CPU32 / E_CPU32_LOSS, from which the GPU bars are formed."""
import os

import numpy as np
import pytest
import torch

import point_loss_ref as R
import synth_fcos_loss as S
import test_gpu_fcos_loss_edges as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _rel_max(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = np.abs(ref).max()
    return 0.0 if m == 0.0 and not np.any(got) else float(np.abs(got - ref).max() / m)


# ------------------------------------------------------------------ against the head's torch body, fp64
@pytest.mark.parametrize('with_iou,attach', E.MODES, ids=['iou-attached', 'iou-detached', 'plain'])
def test_yardstick_is_the_torch_body_on_small(with_iou, attach):
    sizes, gb, gl, outs = S.case_inputs(S.SMALL)
    lab, tgt = S.np_targets(sizes, gb, gl, np.float64)       # the body forms its targets in fp64 too
    v, g, _, _ = R.yardstick_maps(sizes, lab, tgt, outs, None, attach, with_iou)
    for key in R.KEYS[:4 if with_iou else 3]:
        v64, g64 = S.yardstick(with_iou, outs, gb, gl, detach_iou_target=not attach, grad_of=key)
        assert abs(v[key] - v64[key]) <= 1e-12 * abs(v64[key]), key
        for kind in g64:
            for l in range(len(sizes)):
                assert _rel_max(g[key][kind][l], g64[kind][l]) <= 1e-12, (key, kind, l)


@pytest.mark.parametrize('cid', E.ALL_CASES, ids=str)
def test_yardstick_is_the_torch_body_on_the_edge_set(cid):
    """ties, containment, saturation, exp(scale x): the same conventions, to fp64 rounding"""
    case = E.edge_case(*cid)
    for with_iou, attach in E.MODES:
        v, g, _, _ = E.yardstick(case, with_iou, attach)
        v64, g64 = E.torch_body(case, with_iou, attach, torch.float64)
        for key in v64:
            assert abs(v[key] - v64[key]) <= 1e-12 * max(abs(v64[key]), 1e-300), key
            for kind in g64[key]:
                if kind == 'scale':
                    terms = np.maximum(E.scale_terms(case, g64[key]), 1e-300)
                    assert (np.abs(g[key]['scale'] - g64[key]['scale']) <= 1e-12 * terms).all(), key
                    continue
                for l in range(E.NL):
                    assert _rel_max(g[key][kind][l], g64[key][kind][l]) <= 1e-11, (key, kind, l)


@pytest.mark.parametrize('tag', ['iou', 'plain'])
def test_yardstick_against_the_reference_fixture(tag):
    g = np.load(os.path.join(GOLD, 'fcos_loss.npz'))
    for k, case in enumerate((S.SMALL, S.MAIN1)):
        sizes, gb, gl, outs = S.case_inputs(case)
        lab, tgt = S.np_targets(sizes, gb, gl)
        v, grads, _, _ = R.yardstick_maps(sizes, lab, tgt, outs, None, True, tag == 'iou', float(g['gamma']),
                                          float(g['alpha']))
        total = R.combine(grads, (1.0, 1.0, 1.0, 1.0))
        ref = g['loss_%s_%d' % (tag, k)]
        for key, r in zip(R.KEYS, ref):
            assert abs(v[key] - r) <= 1e-4 * max(1.0, abs(r)), (tag, k, key, v[key], r)
        for kind in ('cls', 'reg', 'ctr', 'iou')[:len(ref)]:
            for l in range(len(sizes)):
                idx = g['g_%s_%d_%s_%d_idx' % (tag, k, kind, l)]
                r = g['g_%s_%d_%s_%d' % (tag, k, kind, l)].astype(np.float64)
                got = total[kind][l].reshape(-1)[idx]
                scale = float(np.abs(r).max())
                if scale == 0.0:
                    assert not np.any(got)
                else:
                    assert float(np.abs(got - r).max()) / scale <= 2e-4, (tag, k, kind, l)


# ------------------------------------------------------------------ the edge set's conditions
def _corners(case, dtype):
    """per positive: predicted and target corners (P, 4) evaluated in `dtype`, as point_elem does"""
    pos, _, _ = R.gather(case['sizes'], case['labels'], case['targets'], case['outs'])
    d = pos['reg'].astype(dtype)
    if case['raw']:
        d = np.exp((E.SCALES[pos['level']].astype(dtype)[:, None] * d).astype(dtype)).astype(dtype)
    sgn = np.array([-1, -1, 1, 1], dtype)
    pt = pos['pts'].astype(dtype)[:, [0, 1, 0, 1]]
    return pos, d, (pt + sgn * d).astype(dtype), (pt + sgn * pos['tgt'].astype(dtype)).astype(dtype)


def _is_bf16(a):
    a = np.asarray(a, np.float32)
    return torch.from_numpy(a.copy()).to(torch.bfloat16).to(torch.float32).numpy() == a


@pytest.mark.parametrize('cid', E.ALL_CASES, ids=str)
def test_edge_set_conditions(cid):
    from iouaware import fcos_ops
    case = E.edge_case(*cid)
    geom, raw, bf16, single = cid
    sizes, groups, spec = case['sizes'], case['groups'], case['spec']
    assert fcos_ops.point_loss_supported(fcos_ops.PointGeometry(sizes, S.STRIDES, S.C), E.B)
    if geom == 'odd':
        assert all((h * w) % 4 for h, w in sizes)
    for b in case['gb']:
        assert (b * 8 == np.round(b * 8)).all(), 'gt boxes on the 1/8 px grid'
    npos = S.check_conditions(sizes, case['gb'], case['gl'])
    # the groups partition the positives: nothing is left out of a comparison
    members = [m for v in groups.values() for m in v]
    assert len(members) == len(set(members)) == sum(npos) == len(spec)
    pos, d32, p32, t32 = _corners(case, np.float32)
    _, d64, p64, t64 = _corners(case, np.float64)
    names = np.array([E.group_of(spec[(int(l), int(b), int(p))]) for l, b, p in zip(pos['level'], pos['b'], pos['p'])])
    if single:
        assert npos == [0, 0, 0, 0, 1] and not any((a[1] > 0).any() for a in case['labels'])
        assert case['targets'][4][0, 0].max() > 512
    else:
        assert min(npos) >= 4, npos
        used = np.concatenate([a[a > 0] for a in case['labels']])
        assert 1 in used and S.C in used
        assert max(float(t[a > 0].max()) for a, t in zip(case['labels'], case['targets'])) > 512
        assert sum(b.min() < 0 or b.max() > 160 for b in case['gb']) >= 2      # boxes outside the padded image
        want = set(E.group_of(s) for s in E.ROT) | {'centre', 'corner', 'raw_tie'}
        have = set(names)
        assert have == want, have ^ want
        for l in range(3):                       # the levels with enough positives carry every planted spec
            assert set(names[pos['level'] == l]) >= set(E.group_of(s) for s in E.ROT), l
        for l in range(E.NL):                    # and every level keeps a random positive
            assert 'random' in set(names[pos['level'] == l]), l
    # fp32 and fp64 see the same ordering of every pair of edges, on every positive
    assert np.array_equal(np.sign(p32 - t32), np.sign(p64 - t64))
    ties = p64 == t64
    planted = np.isin(names, E.TIE_FAMILY + ('pred_inside', 'target_inside', 'mixed'))
    if not raw:
        # the corners of the specs that plant an ordering are exact in fp32 (`zero` and `raw_tie` keep random
        # distances beside theirs, and 2^20 t leaves the 24 bits: their ordering is the assertion above)
        assert np.array_equal(p32[planted].astype(np.float64), p64[planted])
        assert np.array_equal(t32.astype(np.float64), t64)
        if not bf16 and not single:
            assert (ties[names == 'tie_x'] == [True, False, True, False]).all()
            assert (ties[names == 'tie_y'] == [False, True, False, True]).all()
            near = np.abs(d64 - pos['tgt'])[names == 'near_tie'].min(1)
            assert (near == 2.0 ** -12).all() and not ties[names == 'near_tie'].any()
        if bf16:                                 # a tie only where the target distance is a bf16 number
            assert _is_bf16(pos['tgt'][ties]).all() and (not single and ties.sum() >= 8)
        for g, sel in (('equal', names == 'equal'),):
            in_group = np.zeros(len(names), bool)
            idx = {(int(l), int(b), int(p)): i for i, (l, b, p) in enumerate(zip(pos['level'], pos['b'], pos['p']))}
            for m in groups.get('equal', ()):
                in_group[idx[m]] = True
            assert ties[in_group].all() and (single == 'random' or in_group.sum() >= 1)
            assert not ties[~in_group & sel].all(1).any()
    else:
        # no accidental near-tie: the raw form's distances stay clear of the targets, but for the exact ones
        clear = np.abs(d64 - pos['tgt']) > 1e-4 * pos['tgt']
        exact = (pos['reg'] == 0.0) & (pos['tgt'] == 1.0)
        assert (clear | exact).all() and (single or exact.sum() >= 4)
        assert (d32[(pos['reg'] * E.SCALES[pos['level']][:, None]) < -104.0] == 0.0).all()
    if not single:
        zero = d32[names == 'zero'] == 0.0
        assert zero.all(1).any() and (zero.sum(1) == 1).any()
        if not bf16 or not raw:
            assert (d64[names == 'huge'] >= 2.0 ** 19.9 * pos['tgt'][names == 'huge']).all()
        # saturated logits: every value on a positive's centerness / IoU / labelled class, and on negatives
        sat = names == 'sat'
        assert set(pos['ctr'][sat]) == set(E.SAT) and set(pos['iou'][sat]) == set(E.SAT)
        _, fc, fl = R.gather(sizes, case['labels'], case['targets'], case['outs'])
        on_lab = fc[np.nonzero(fl > 0)[0], fl[fl > 0] - 1]
        assert set(E.SAT) <= set(on_lab) and set(E.SAT) <= set(fc[fl == 0].ravel())
        other = fc[fl > 0].copy()
        other[np.arange(len(other)), fl[fl > 0] - 1] = 0.5
        assert set(E.SAT) <= set(other.ravel())
    # the yardstick and the fp32 torch body are finite on every element
    for with_iou, attach in E.MODES:
        v, g, _, r = E.yardstick(case, with_iou, attach)
        v32, g32 = E.torch_body(case, with_iou, attach, torch.float32)
        for vals, grads in ((v, g), (v32, g32)):
            assert np.isfinite(list(vals.values())).all()
            for key in grads:
                for kind, m in grads[key].items():
                    assert all(np.isfinite(x).all() for x in (m if isinstance(m, list) else [m])), (key, kind)
        if not raw:
            eq = np.array([(int(l), int(b), int(p)) in set(groups.get('equal', ())) for l, b, p in
                           zip(pos['level'], pos['b'], pos['p'])])
            assert (r['u'][eq] == 1.0).all()
            total = R.combine(g, E.UP)
            for l, b, p in groups.get('equal', ()):
                m = total['reg'][l].reshape(E.B, 4, -1)
                assert np.abs(m[b, :, p]).max() <= 1e-12 * np.abs(m).max(), 'the yardstick: zero at pred == target'
        if not single:
            assert (r['c'][names == 'centre'] == 1.0).all() and (r['c'][names == 'corner'] < 0.1).all()


# ------------------------------------------------------------------ E_cpu32
def _measure():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                 # the fp32 sums in one order, whatever the machine
    try:
        return _measure_single()
    finally:
        torch.set_num_threads(threads)


def _measure_single():
    box, loss = {}, {}
    for cid in E.ALL_CASES:
        case = E.edge_case(*cid)
        f = E.form(case)
        for with_iou, attach in E.MODES:
            v, g, _, _ = E.yardstick(case, with_iou, attach)
            v32, g32 = E.torch_body(case, with_iou, attach, torch.float32)
            for key in v:
                if v[key] != 0.0:
                    e = abs(v32[key] - v[key]) / abs(v[key])
                    loss[(f, key)] = max(loss.get((f, key), 0.0), e)
            ref, got = R.combine(g, E.UP), R.combine(g32, E.UP)
            kinds = ('reg', 'ctr', 'iou')[:3 if with_iou else 2]
            for k, e in E.group_errors(case, got, ref, kinds).items():
                box[(f,) + k] = max(box.get((f,) + k, 0.0), e)
            if case['raw']:
                terms = E.scale_terms(case, ref)
                for l in range(E.NL):
                    if terms[l] > 0.0:
                        e = abs(got['scale'][l] - ref['scale'][l]) / terms[l]
                        box[('raw', 'scale', 'all')] = max(box.get(('raw', 'scale', 'all'), 0.0), e)
    return box, loss


def test_e_cpu32_table():
    box, loss = _measure()
    print('\nE_CPU32 = {')
    for k in sorted(box):
        print('    %r: %.1e,' % (k, box[k]))
    print('}\nE_CPU32_LOSS = {')
    for k in sorted(loss):
        print('    %r: %.1e,' % (k, loss[k]))
    print('}')
    assert set(box) == set(E.E_CPU32) and set(loss) == set(E.E_CPU32_LOSS), 'the recorded table has other entries'
    for k, e in box.items():
        assert e <= E.E_CPU32[k], (k, e, E.E_CPU32[k])
    for k, e in loss.items():
        assert e <= E.E_CPU32_LOSS[k], (k, e, E.E_CPU32_LOSS[k])

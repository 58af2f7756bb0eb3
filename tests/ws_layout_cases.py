"""The fixed table of inputs behind tests/golden/workspace_layout.json: every size, layout and
status-offset query of the post-conv workspaces, and the calls the entries refuse before they touch
the device.  record(lib) evaluates the whole table against a loaded library and returns
{'layout': {case: answer}, 'refusal': {case: return code}}; tools/record_workspace_layout.py writes
that to the golden file, tests/test_host_workspace_layout.py compares a fresh evaluation with it.

Nothing here reaches a launch: every refusal case fails a host-side check first, so fabricated
addresses stand in for device memory and are never dereferenced."""
import ctypes as C

from iouaware import _lib

NCHW, NHWC = _lib.IA_LAYOUT_NCHW, _lib.IA_LAYOUT_NHWC
PYRAMID = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]        # the BASELINE head at 800 x 1344
SMALL = [(8, 10), (4, 5), (2, 3)]
ADDR = 0x7f0000000000               # fabricated, 256-byte aligned
ERRORS = (-1, -2, -3, -4, -5)       # IA_E_*: what a refusal on the host can answer


def head_geom(sizes, A, C_, nms_pre, layout=NCHW):
    g = _lib.HeadGeom()
    g.num_levels, g.num_anchors, g.num_classes, g.nms_pre = len(sizes), A, C_, nms_pre
    for l, (h, w) in enumerate(sizes):
        g.H[l], g.W[l], g.stride[l] = h, w, 8 << l
    for k in range(4):
        g.stds[k] = 1.0
    g.layout, g.cls_activation = layout, _lib.IA_CLS_SIGMOID
    return g


def point_geom(sizes, C_, nms_pre, layout=NCHW, score_alpha=0.4):
    g = _lib.PointHeadGeom()
    g.num_levels, g.num_classes, g.nms_pre = len(sizes), C_, nms_pre
    for l, (h, w) in enumerate(sizes):
        g.H[l], g.W[l], g.stride[l] = h, w, 8 << l
    g.layout, g.score_alpha = layout, score_alpha
    return g


def guided_geom(sizes, C_, nms_pre):
    g = _lib.GuidedGeom()
    g.head = head_geom(sizes, 1, C_, nms_pre)
    for k in range(4):
        g.anchoring_stds[k] = 1.0
    g.loc_filter_thr, g.use_loc_filter = 0.01, 1
    return g


def ssd_geom(sizes, anchors, C_):
    g = _lib.SsdGeom()
    g.num_levels, g.num_classes = len(sizes), C_
    for l, (s, a) in enumerate(zip(sizes, anchors)):
        g.H[l], g.W[l], g.stride[l], g.num_anchors[l] = s, s, 8 << l, a
    for k in range(4):
        g.stds[k] = 1.0
    return g


def wino_geom(sizes, batch):
    g = _lib.WinoGeom()
    g.num_levels, g.batch = len(sizes), batch
    for l, (h, w) in enumerate(sizes):
        g.H[l], g.W[l] = h, w
    return g


ANCHOR_GEOMS = {                     # name -> (geometry, batches)
    'baseline_nchw': (head_geom(PYRAMID, 9, 80, 1000), (1, 8, 16)),          # N, R, Rs = 201600, 4693, 4736
    'baseline_nhwc': (head_geom(PYRAMID, 9, 80, 1000, NHWC), (1, 8, 16)),
    'one_by_one': (head_geom([(1, 1)], 1, 1, 1000), (1,)),
    'small_all_rows': (head_geom(SMALL, 3, 4, -1), (1, 2)),
    'r8192': (head_geom([(64, 64), (64, 64)], 1, 80, 4096), (1, 2)),
    'r8193': (head_geom([(64, 64), (64, 64), (1, 1)], 1, 80, 4096), (1,)),  # one above IA_MAX_CANDIDATES
}
POINT_GEOMS = {
    'pyramid_nchw': (point_geom(PYRAMID, 80, 1000), (1, 8)),
    'pyramid_nhwc': (point_geom(PYRAMID, 80, 1000, NHWC), (1, 8)),
    'alpha_out_of_range': (point_geom(PYRAMID, 80, 1000, score_alpha=1.5), (1,)),
}
GUIDED_GEOMS = {'pyramid_a1': (guided_geom(PYRAMID, 80, 1000), (1, 8))}
SSD_GEOMS = {
    'ssd300': (ssd_geom([38, 19, 10, 5, 3, 1], [4, 6, 6, 6, 4, 4], 81), (1, 8)),         # R = 8732 > Rk = 8192
    'ssd512': (ssd_geom([64, 32, 16, 8, 4, 2, 1], [4, 6, 6, 6, 6, 4, 4], 81), (1, 8)),   # R = 24564
    'toy': (ssd_geom([3, 1], [4, 6], 4), (1, 8)),
}
NMS_R = (1, 63, 64, 65, 4693, 8192, 8193)
GN_GEOMS = {'pyramid': PYRAMID, 'small': SMALL}


def _layout(fn, g, batch, n):
    out = (C.c_size_t * n)()
    rc = fn(C.byref(g), batch, C.byref(out))
    return dict(rc=rc, offsets=list(out) if rc == 0 else None)


def layouts(lib):
    r = {}
    for name, (g, batches) in ANCHOR_GEOMS.items():
        N, R, Rs = C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.ia_geom_sizes(C.byref(g), C.byref(N), C.byref(R), C.byref(Rs)) == 0
        r['anchor/%s/sizes' % name] = [N.value, R.value, Rs.value]
        for b in batches:
            d = _layout(lib.ia_get_bboxes_workspace_layout, g, b, 8)
            d['bytes'] = lib.ia_get_bboxes_workspace_bytes(C.byref(g), b)
            d['status_offset'] = lib.ia_get_bboxes_status_offset(C.byref(g), b)
            d['select_bytes'] = lib.ia_select_topk_workspace_bytes(C.byref(g), b)
            r['anchor/%s/b%d' % (name, b)] = d
    for name, (g, batches) in POINT_GEOMS.items():
        for b in batches:
            d = _layout(lib.ia_point_workspace_layout, g, b, 8)
            d['bytes'] = lib.ia_point_workspace_bytes(C.byref(g), b)
            r['point/%s/b%d' % (name, b)] = d
    for name, (g, batches) in GUIDED_GEOMS.items():
        for b in batches:
            d = _layout(lib.ia_guided_workspace_layout, g, b, 8)
            d['bytes'] = lib.ia_guided_get_bboxes_workspace_bytes(C.byref(g), b)
            r['guided/%s/b%d' % (name, b)] = d
    for name, (g, batches) in SSD_GEOMS.items():
        for b in batches:
            d = _layout(lib.ia_ssd_workspace_layout, g, b, 8)
            d['bytes'] = lib.ia_ssd_get_bboxes_workspace_bytes(C.byref(g), b)
            r['ssd/%s/b%d' % (name, b)] = d
            d = _layout(lib.ia_ssd_head_loss_workspace_layout, g, b, 5)
            d['bytes'] = lib.ia_ssd_head_loss_workspace_bytes(C.byref(g), b)
            r['ssd_loss/%s/b%d' % (name, b)] = d
    for R in NMS_R:
        for C_ in (1, 80):
            for b in (1, 8):
                r['nms/R%d/C%d/b%d' % (R, C_, b)] = dict(
                    full=lib.ia_multiclass_nms_workspace_bytes(b, R, C_),
                    lazy=lib.ia_multiclass_nms_lazy_workspace_bytes(b, R, C_),
                    soft=lib.ia_multiclass_soft_nms_workspace_bytes(b, R, C_))
    # (not ia_nms_f64_workspace_bytes: it asks the sort library, which asks the device)
    for n in NMS_R + (0, 20000):
        r['nms_single/n%d' % n] = lib.ia_nms_workspace_bytes(n)
    for name, sizes in GN_GEOMS.items():
        for b in (1, 8):
            g = wino_geom(sizes, b)
            for ch, groups in ((256, 32), (64, 8)):
                r['groupnorm/%s/b%d/c%d' % (name, b, ch)] = [
                    [lib.ia_groupnorm_workspace_bytes_dt(C.byref(g), ch, groups, dt),
                     lib.ia_groupnorm_saved_bytes_dt(C.byref(g), ch, groups, dt),
                     lib.ia_groupnorm_bwd_workspace_bytes_dt(C.byref(g), ch, groups, dt)]
                    for dt in (_lib.IA_F32, _lib.IA_BF16)]
    return r


def _ptrs(cls, fields):
    p = cls()
    for f in fields:
        for l in range(_lib.IA_MAX_LEVELS):
            getattr(p, f)[l] = ADDR
    return p


def _workspace_cases(need):
    """(case, workspace address, workspace_bytes) of the refusals every entry shares"""
    return (('null_workspace', None, need), ('one_byte_short', ADDR, need - 1), ('unaligned', ADDR + 4, need))


def refusals(lib):
    r = {}
    A = ADDR                                                       # stands for any device buffer
    g, b = ANCHOR_GEOMS['baseline_nchw'][0], 2
    need = lib.ia_get_bboxes_workspace_bytes(C.byref(g), b)
    p = _lib.LevelPtrs()
    big = ANCHOR_GEOMS['r8193'][0]

    def anchor(entry, gg, pp, ws, nbytes, cand=0):
        ga = C.byref(gg) if gg is not None else None
        pa = C.byref(pp) if pp is not None else None
        if entry == 'ia_decode_stage':
            return lib.ia_decode_stage(ga, pa, b, 0, A, A, 0, ws, nbytes, None)
        if entry == 'ia_get_bboxes':
            return lib.ia_get_bboxes(ga, pa, b, 0, A, A, 0, 0.05, 0.5, 100, ws, nbytes, A, A, A, A, None)
        return lib.ia_get_bboxes_lazy(ga, pa, b, 0, A, A, 0, 0.05, 0.5, 100, cand, ws, nbytes, A, A, A, A, None)

    for e in ('ia_decode_stage', 'ia_get_bboxes', 'ia_get_bboxes_lazy'):
        r[e + '/null_geom'] = anchor(e, None, p, A, need)
        r[e + '/null_p'] = anchor(e, g, None, A, need)
        r[e + '/null_p_and_short'] = anchor(e, g, None, A, need - 1)
        r[e + '/too_many_candidates'] = anchor(e, big, p, A, 1 << 40)
        for case, ws, n in _workspace_cases(need):
            r['%s/%s' % (e, case)] = anchor(e, g, p, ws, n)
        r[e + '/short_and_unaligned'] = anchor(e, g, p, A + 4, need - 1)
    r['ia_get_bboxes_lazy/negative_candidates'] = anchor('ia_get_bboxes_lazy', g, p, A, need, cand=-1)

    pg = POINT_GEOMS['pyramid_nchw'][0]
    pneed = lib.ia_point_workspace_bytes(C.byref(pg), b)
    bad_alpha = POINT_GEOMS['alpha_out_of_range'][0]

    def point(entry, gg, pp, ws, nbytes, dets=A, cand=0):
        ga = C.byref(gg) if gg is not None else None
        pa = C.byref(pp) if pp is not None else None
        if entry == 'ia_point_decode_stage':
            return lib.ia_point_decode_stage(ga, pa, b, A, A, 0, ws, nbytes, None)
        if entry == 'ia_point_ctr_decode_stage':
            return lib.ia_point_ctr_decode_stage(ga, pa, b, A, A, 0, 0.05, ws, nbytes, None)
        if entry.endswith('_dt'):
            return getattr(lib, entry)(ga, pa, b, _lib.IA_BF16, A, A, 0, 0.05, 0.5, 100, cand, ws, nbytes, dets, A, A, A,
                                       None)
        return getattr(lib, entry)(ga, pa, b, A, A, 0, 0.05, 0.5, 100, cand, ws, nbytes, dets, A, A, A, None)

    for e in ('ia_point_decode_stage', 'ia_point_ctr_decode_stage', 'ia_point_get_bboxes', 'ia_point_get_bboxes_dt',
              'ia_point_ctr_get_bboxes', 'ia_point_ctr_get_bboxes_dt'):
        r[e + '/null_geom'] = point(e, None, p, A, pneed)
        r[e + '/alpha_out_of_range'] = point(e, bad_alpha, p, A, pneed)
        r[e + '/null_p'] = point(e, pg, None, A, pneed)
        r[e + '/null_p_and_short'] = point(e, pg, None, A, pneed - 1)
        for case, ws, n in _workspace_cases(pneed):
            r['%s/%s' % (e, case)] = point(e, pg, p, ws, n)
        r[e + '/short_and_unaligned'] = point(e, pg, p, A + 4, pneed - 1)
        if 'get_bboxes' in e:
            r[e + '/null_dets'] = point(e, pg, p, A, pneed, dets=None)
            r[e + '/null_dets_and_null_geom'] = point(e, None, p, A, pneed, dets=None)

    gg = GUIDED_GEOMS['pyramid_a1'][0]
    gneed = lib.ia_guided_get_bboxes_workspace_bytes(C.byref(gg), b)
    gp = _ptrs(_lib.GuidedLevelPtrs, ('cls', 'reg', 'iou', 'shape', 'loc'))
    gbig = guided_geom([(64, 64), (64, 64), (1, 1)], 80, 4096)

    def guided(geom, pp, ws, nbytes, score_thr=0.05, dets=A):
        return lib.ia_guided_get_bboxes(C.byref(geom), C.byref(pp) if pp is not None else None, b, A, A, 0, score_thr,
                                        0.5, 100, ws, nbytes, dets, A, A, A, None)

    e = 'ia_guided_get_bboxes'
    r[e + '/null_p'] = guided(gg, None, A, gneed)
    r[e + '/null_level_pointer'] = guided(gg, _lib.GuidedLevelPtrs(), A, gneed)
    r[e + '/negative_score_thr'] = guided(gg, gp, A, gneed, score_thr=-0.1)
    r[e + '/negative_score_thr_and_null_workspace'] = guided(gg, gp, None, gneed, score_thr=-0.1)
    r[e + '/null_dets'] = guided(gg, gp, A, gneed, dets=None)
    r[e + '/too_many_candidates'] = guided(gbig, gp, A, 1 << 40)
    for case, ws, n in _workspace_cases(gneed):
        r['%s/%s' % (e, case)] = guided(gg, gp, ws, n)
    r[e + '/short_and_unaligned'] = guided(gg, gp, A + 4, gneed - 1)

    sp = _ptrs(_lib.SsdLevelPtrs, ('cls', 'reg'))
    for name in ('ssd300', 'toy'):
        sg = SSD_GEOMS[name][0]
        sneed = lib.ia_ssd_get_bboxes_workspace_bytes(C.byref(sg), b)

        def ssd(pp, ws, nbytes, score_thr=0.02, max_per_img=200, dtype=0, dets=A):
            return lib.ia_ssd_get_bboxes(C.byref(sg), C.byref(pp) if pp is not None else None, b, dtype, A, A, 0,
                                         score_thr, 0.45, max_per_img, ws, nbytes, dets, A, A, A, A, None)

        e = 'ia_ssd_get_bboxes/' + name
        r[e + '/null_p'] = ssd(None, A, sneed)
        r[e + '/null_level_pointer'] = ssd(_lib.SsdLevelPtrs(), A, sneed)
        r[e + '/bf16'] = ssd(sp, A, sneed, dtype=_lib.IA_BF16)
        r[e + '/negative_score_thr'] = ssd(sp, A, sneed, score_thr=-0.1)
        r[e + '/null_dets'] = ssd(sp, A, sneed, dets=None)
        r[e + '/max_per_img_0'] = ssd(sp, A, sneed, max_per_img=0)
        r[e + '/max_per_img_1025'] = ssd(sp, A, sneed, max_per_img=1025)
        r[e + '/max_per_img_1025_and_short'] = ssd(sp, A, sneed - 1, max_per_img=1025)
        r[e + '/max_per_img_0_and_unaligned'] = ssd(sp, A + 4, sneed, max_per_img=0)
        for case, ws, n in _workspace_cases(sneed):
            r['%s/%s' % (e, case)] = ssd(sp, ws, n)
        r[e + '/short_and_unaligned'] = ssd(sp, A + 4, sneed - 1)

        lneed = lib.ia_ssd_head_loss_workspace_bytes(C.byref(sg), b)
        for case, ws, n in _workspace_cases(lneed) + (('batch_above_limit', A, 1 << 40),):
            bb = 65536 if case == 'batch_above_limit' else b        # batch * levels <= 65535 (grid.y)
            r['ia_ssd_head_loss_fwd/%s/%s' % (name, case)] = lib.ia_ssd_head_loss_fwd(
                C.byref(sg), C.byref(sp), bb, 0, A, A, A, A, None, 4.0, 3, 1.0, ws, n, A, None)
            r['ia_ssd_head_loss_bwd/%s/%s' % (name, case)] = lib.ia_ssd_head_loss_bwd(
                C.byref(sg), C.byref(sp), bb, 0, A, A, A, A, None, 4.0, 1.0, ws, n, A, C.byref(sp), None)

    # stage-level NMS: data pointers null where the stages' own checks have to answer
    for R, C_ in ((4693, 80), (65, 1)):
        tag = 'R%d_C%d' % (R, C_)
        for e, bytes_fn in (('ia_multiclass_nms', lib.ia_multiclass_nms_workspace_bytes),
                            ('ia_multiclass_nms_lazy', lib.ia_multiclass_nms_lazy_workspace_bytes),
                            ('ia_multiclass_soft_nms', lib.ia_multiclass_soft_nms_workspace_bytes)):
            nneed = bytes_fn(b, R, C_)

            def nms(ws, nbytes, data=None, RR=R, max_per_img=100, cand=0, batch=b):
                if e == 'ia_multiclass_nms':
                    return lib.ia_multiclass_nms(data, data, data, batch, RR, C_, 0.05, 0.5, max_per_img, ws, nbytes, A,
                                                 A, A, A, A, A, None)
                if e == 'ia_multiclass_nms_lazy':
                    return lib.ia_multiclass_nms_lazy(data, data, data, batch, RR, C_, 0.05, 0.5, max_per_img, cand, ws,
                                                      nbytes, A, A, A, A, None)
                return lib.ia_multiclass_soft_nms(data, data, batch, RR, C_, 0.05, 0.5, 1, 0.5, 0.001, max_per_img, ws,
                                                  nbytes, A, A, A, A, A, A, None)

            k = '%s/%s' % (e, tag)
            r[k + '/null_workspace'] = nms(None, nneed)
            r[k + '/one_byte_short'] = nms(A, nneed - 1)
            r[k + '/zero_bytes'] = nms(A, 0)
            r[k + '/too_many_rows'] = nms(A, 1 << 40, RR=8193)
            r[k + '/batch_0'] = nms(A, 1 << 40, batch=0)
            r[k + '/null_boxes'] = nms(A, nneed)                   # refused by the first stage's own check
            r[k + '/null_boxes_unaligned'] = nms(A + 4, nneed)
            r[k + '/null_boxes_max_per_img_1025'] = nms(A, nneed, max_per_img=1025)
            r[k + '/null_boxes_max_per_img_0'] = nms(A, nneed, max_per_img=0)
            if e == 'ia_multiclass_nms_lazy':
                r[k + '/negative_candidates'] = nms(A, nneed, data=A, cand=-1)
                r[k + '/negative_candidates_and_short'] = nms(A, nneed - 1, data=A, cand=-1)
    assert all(v in ERRORS for v in r.values()), {k: v for k, v in r.items() if v not in ERRORS}
    return r


def record(lib):
    return dict(layout=layouts(lib), refusal=refusals(lib))

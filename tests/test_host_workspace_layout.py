"""CPU: the post-conv workspaces keep every byte.  tests/golden/workspace_layout.json holds what the
library answered, before the host code that sizes and slices these workspaces was folded into one
carve function per layout, to the fixed table of tests/ws_layout_cases.py: the size, layout and
status-offset queries of the anchor, point, guided and SSD whole-path workspaces, of the SSD loss
node and of the stage-level NMS entries, and the return code of every call those entries refuse
before they reach the device (tools/record_workspace_layout.py writes the file).  Callers cache
workspaces by size and tests read stage outputs through these offsets, so each answer of the
current build has to equal the recorded one."""
import json
import os

import pytest

import ws_layout_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_layout.json')


@pytest.fixture(scope='module')
def recorded():
    with open(GOLD) as fh:
        return json.load(fh)


@pytest.fixture(scope='module')
def current():
    from iouaware import _lib
    # through JSON, so both sides hold the same types
    return json.loads(json.dumps(ws_layout_cases.record(_lib.lib())))


@pytest.mark.parametrize('kind', ['layout', 'refusal'])
def test_every_recorded_answer_is_reproduced(recorded, current, kind):
    assert sorted(current[kind]) == sorted(recorded[kind])
    wrong = {k: (current[kind][k], v) for k, v in recorded[kind].items() if current[kind][k] != v}
    assert not wrong, wrong


def test_the_table_covers_what_it_is_for(recorded):
    lay, ref = recorded['layout'], recorded['refusal']
    assert lay['anchor/baseline_nchw/sizes'] == [201600, 4693, 4736]
    for b in (1, 8, 16):
        for name in ('baseline_nchw', 'baseline_nhwc'):
            d = lay['anchor/%s/b%d' % (name, b)]
            assert d['rc'] == 0 and d['bytes'] > d['status_offset'] > d['offsets'][7] > 0
            assert all(o % 256 == 0 for o in d['offsets'])
    assert lay['anchor/one_by_one/sizes'] == [1, 1, 64] and lay['anchor/one_by_one/b1']['bytes'] > 0
    assert lay['anchor/small_all_rows/sizes'][0] == lay['anchor/small_all_rows/sizes'][1] == 3 * (80 + 20 + 6)
    assert lay['anchor/r8192/sizes'][1] == 8192 and lay['anchor/r8192/b1']['bytes'] > 0
    assert lay['anchor/r8193/sizes'][1] == 8193
    assert lay['anchor/r8193/b1'] == dict(rc=-3, offsets=None, bytes=0, status_offset=0,
                                          select_bytes=lay['anchor/r8193/b1']['select_bytes'])
    assert lay['point/alpha_out_of_range/b1']['bytes'] == 0 and lay['point/alpha_out_of_range/b1']['rc'] == -1
    # the point and guided heads run on the anchor workspace of their A = 1 geometry
    assert lay['point/pyramid_nchw/b8']['offsets'] == lay['guided/pyramid_a1/b8']['offsets']
    assert lay['point/pyramid_nhwc/b1']['bytes'] > 0 and lay['guided/pyramid_a1/b1']['bytes'] > 0
    for name in ('ssd300', 'ssd512', 'toy'):
        for b in (1, 8):
            assert lay['ssd/%s/b%d' % (name, b)]['bytes'] > 0 and lay['ssd_loss/%s/b%d' % (name, b)]['bytes'] > 0
    # SSD300 keeps R = 8732 row scores per image, the stages behind run on Rk = 8192 rows
    o = lay['ssd/ssd300/b1']['offsets']
    assert o[1] - o[0] == 8732 * 4 + (-8732 * 4) % 256 and o[4] - o[3] == 8192 * 16
    for R in (1, 63, 64, 65, 4693, 8192):
        for c in (1, 80):
            for b in (1, 8):
                d = lay['nms/R%d/C%d/b%d' % (R, c, b)]
                assert d['lazy'] > d['full'] > 0 and d['soft'] > 0
    assert all(lay['nms/R8193/C%d/b%d' % (c, b)] == dict(full=0, lazy=0, soft=0) for c in (1, 80) for b in (1, 8))
    # refusals: the codes are the recording's alone; here only that each entry has its cases, and that
    # every one of them is a refusal by the library (IA_E_*), not an error of a runtime it reached
    for e in ('ia_get_bboxes', 'ia_get_bboxes_lazy', 'ia_point_get_bboxes', 'ia_point_get_bboxes_dt',
              'ia_point_ctr_get_bboxes', 'ia_point_ctr_get_bboxes_dt', 'ia_guided_get_bboxes',
              'ia_ssd_get_bboxes/ssd300', 'ia_ssd_get_bboxes/toy', 'ia_multiclass_nms/R4693_C80',
              'ia_multiclass_nms_lazy/R4693_C80', 'ia_multiclass_soft_nms/R65_C1'):
        cases = ('null_workspace', 'one_byte_short') + (() if 'multiclass' in e else ('null_p', 'unaligned'))
        assert all('%s/%s' % (e, c) in ref for c in cases), e
    for k in ('ia_ssd_get_bboxes/ssd300/max_per_img_0', 'ia_ssd_get_bboxes/ssd300/max_per_img_1025',
              'ia_guided_get_bboxes/negative_score_thr', 'ia_ssd_get_bboxes/toy/negative_score_thr',
              'ia_get_bboxes_lazy/negative_candidates', 'ia_multiclass_nms_lazy/R65_C1/negative_candidates'):
        assert k in ref
    assert all(v in ws_layout_cases.ERRORS for v in ref.values())

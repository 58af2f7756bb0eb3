"""CPU: the instruments of tests/test_gpu_conv3x3_bf16_edges.py (tests/conv3_edges_ref.py) -- the shift
probe's expectation against the convolution's definition, what each emulated kernel fault does to it on the
GPU case lists, the ties of the integer cases -- and, through the host-only entry ia_conv3x3_bf16_plan, which
tile shapes and kernel variants those lists reach."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv3_edges_ref as E
from test_capi_symbols import declared_functions


def _plan():
    from iouaware import ops
    return ops.conv3x3_bf16_plan


def _route(monkeypatch, force):
    if force is None:
        monkeypatch.delenv(E.ENV, raising=False)
    else:
        monkeypatch.setenv(E.ENV, force)


def _entries(monkeypatch, force, cout):
    _route(monkeypatch, force)
    return E.class_maps(_plan(), cout)


# ------------------------------------------------------------------ the plan entry
def test_plan_entry_is_declared_and_checks_its_arguments(monkeypatch):
    from iouaware import _lib
    assert 'ia_conv3x3_bf16_plan' in declared_functions() and 'ia_conv3x3_bf16_plan' in _lib.SIGNATURES
    lib = _lib.lib()
    _route(monkeypatch, None)

    def desc(cin=32, cout=64, levels=1, groups=1, xs=None, ys=None, hw=(5, 7)):
        d = _lib.Conv3x3Desc()
        d.num_levels, d.batch, d.groups = levels, 2, groups
        d.cin, d.cout, d.x_stride, d.y_stride = cin, cout, cin if xs is None else xs, cout if ys is None else ys
        for l in range(min(levels, _lib.IA_MAX_LEVELS)):
            d.H[l], d.W[l] = hw
        return d

    def call(d):
        out = [(C.c_int32 * _lib.IA_MAX_LEVELS)(*([-7] * _lib.IA_MAX_LEVELS)) for _ in range(5)]
        return lib.ia_conv3x3_bf16_plan(C.byref(d), *out), [list(o) for o in out]

    rc, out = call(desc(levels=3))                  # no pointer is set: the entry does not look at them
    assert rc == 0 and [o[:4] for o in out] == [[141] * 3 + [-7], [5] * 3 + [-7], [7] * 3 + [-7], [1] * 3 + [-7], [1] * 3 + [-7]]
    assert lib.ia_conv3x3_bf16_plan(C.byref(desc()), None, None, None, None, None) == 0
    for what, d in (('Cin 48', desc(cin=48)), ('Cin 16', desc(cin=16)), ('odd Cout', desc(cout=65)), ('Cout 0', desc(cout=0)),
                    ('x_stride < cin', desc(cin=64, xs=56)), ('x_stride % 8', desc(xs=36)), ('y_stride < cout', desc(ys=62)),
                    ('odd y_stride', desc(ys=67)), ('9 levels', desc(levels=9)), ('0 levels', desc(levels=0)),
                    ('3 groups', desc(groups=3)), ('0 groups', desc(groups=0)), ('empty map', desc(hw=(0, 7)))):
        rc, out = call(d)
        assert rc == -1, what                       # IA_E_ARG
        assert all(v == -7 for o in out for v in o), what
    assert lib.ia_conv3x3_bf16_plan(None, None, None, None, None, None) == -1


def test_plan_follows_the_launchers_routes(monkeypatch):
    plan = _plan()
    _route(monkeypatch, None)
    # the head tower at config 3's batch: P3 on (4, 1, 4) in a launch of its own, the rest on (2, 1, 4)
    got = plan([(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)], 256, 256, batch=16)
    assert [p[0] for p in got] == [414, 214, 214, 214, 214]
    for (h, w), (v, th, tw, ty, tx) in zip([(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)], got):
        assert th * tw <= E.tile_pixels(v) and ty == -(-h // th) and tx == -(-w // tw)
    assert plan([(100, 168)], 256, 256, batch=1)[0][0] == 214
    assert [plan([(40, 56)], 64, co)[0][0] for co in (2, 64, 66, 128, 130, 600)] == [141, 141, 222, 222, 214, 214]
    # the environment variable is read on every call
    for force, want in (('41', [141, 222, 414]), ('21', [141, 222, 214]), ('22', [222, 222, 214]), ('12', [141, 122, 214])):
        _route(monkeypatch, force)
        assert [plan([(9, 9)], 32, co)[0][0] for co in (64, 128, 256)] == want, force
    _route(monkeypatch, '21')
    assert plan([(100, 168)], 256, 256, batch=16)[0][0] == 214
    # every route of the GPU tests reaches its variant
    for variant, force, couts in E.ROUTES:
        _route(monkeypatch, force)
        for co in couts:
            assert {p[0] for p in E.plan_maps(plan, E.ENUM_MAPS, co)} == {variant}, (variant, force, co)


# ------------------------------------------------------------------ coverage
def test_case_lists_cover_every_class_of_tile_shape(monkeypatch):
    counts = {}
    for variant, force, couts in E.ROUTES:
        px = E.tile_pixels(variant)
        lists = [_entries(monkeypatch, force, co) for co in couts]
        assert all(l == lists[0] for l in lists)                  # the tile shape does not depend on Cout
        entries = lists[0]
        counts[(variant, force)] = len(entries)
        shapes = [(p[1], p[2]) for _, p in entries]
        assert len(set(shapes)) == len(shapes)
        every = {(p[1], p[2]) for p in E.plan_maps(_plan(), E.ENUM_MAPS, couts[0])}
        assert set(shapes) == every                               # one map of EVERY shape the library returns
        for (h, w), (v, th, tw, ty, tx) in entries:
            assert v == variant and th * tw <= px and 4 <= tw and 2 <= th
        classes = E.tile_classes(entries)
        for name, maps in classes.items():
            if name in E.UNREACHABLE[px]:
                assert not maps, (variant, name)
                assert max(tw for _, tw in every) < 32            # q32 >= 1 everywhere: nothing left to reach
            else:
                assert maps, (variant, force, name)
        assert (1, 1) in classes['th2_h1'] and (1, 1) in classes['below32']
        # the maps with several tiles: a tile with all four neighbours, partial tiles right and bottom
        multi = list(zip(E.MULTI_TILE_MAPS, E.plan_maps(_plan(), E.MULTI_TILE_MAPS, couts[0])))
        inner, right, bottom = E.neighbour_classes(multi)
        assert inner and right and bottom, (variant, inner, right, bottom)
        six = E.chunk_maps(entries)
        assert len(set(six)) == 6
    # DESIGN.md section 3.24 quotes these
    assert counts == {(414, '41'): 190, (214, None): 88, (222, None): 190, (222, '22'): 190, (122, '12'): 88,
                      (141, None): 190}


def test_weight_sets_read_every_tap_and_channel():
    for cin in E.CHUNK_CINS:
        for cout in (2, 34, 64, 66, 128, 130, 258):
            pairs, ns = set(), E.num_sets(cout, cin)
            for s in range(ns):
                taps, cis = E.onehot(cout, cin, s)
                assert taps.shape == (cout,) and int(cis.max()) < cin and int(taps.max()) < 9
                pairs |= set(zip(taps.tolist(), cis.tolist()))
                w = E.onehot_weight(taps, cis, cin)
                assert bool((w.flatten(1).sum(1) == 1).all())    # every output channel (column slot) carries a 1
            if cout >= 32:
                assert len(pairs) == 9 * cin, (cin, cout)
                assert ns >= 2
            else:
                assert {(t, c // 8) for t, c in pairs} == {(t, k) for t in range(9) for k in range(cin // 8)}, (cin, cout)
    taps, _ = E.onehot(130, 32, 0)
    assert taps.tolist() == [co % 9 for co in range(130)]


# ------------------------------------------------------------------ the reference against the definition
SMALL_MAPS = ((1, 1), (1, 2), (2, 1), (1, 5), (3, 1), (2, 2), (3, 3), (4, 7), (5, 4), (7, 6), (9, 13), (6, 11))


def test_shift_expectation_is_the_convolution():
    for i, (h, w) in enumerate(SMALL_MAPS):
        cin, cout = (32, 64)[i % 2], (34, 2, 66)[i % 3]
        x = E.shift_x(h, w, cin)
        assert x.min() >= -128 and x.max() <= 127 and torch.equal(x, x.to(torch.bfloat16).float())
        for s in range(E.num_sets(cout, cin)):
            taps, cis = E.onehot(cout, cin, s)
            want = F.conv2d(x.double(), E.onehot_weight(taps, cis, cin).double(), None, 1, 1)
            got = E.shift_expected(x, taps, cis)
            assert torch.equal(got.double(), want), (h, w, s, E.describe_shift_mismatch(got, want, taps, cis))
    # a mismatch names its source
    x = E.shift_x(4, 7)
    taps, cis = E.onehot(34, 32, 1)
    good = E.shift_expected(x, taps, cis)
    bad = good.clone()
    bad[1, 20, 2, 5] += 1
    text = E.describe_shift_mismatch(bad, good, taps, cis)
    assert 'image 1, co 20 (tap %d' % int(taps[20]) in text and 'ci %d)' % int(cis[20]) in text and 'pixel (2, 5)' in text


def test_nan_mask_is_what_the_definition_gives():
    w, bias = E.int_weight(34, 32)
    for (h, wd), (b, py, px) in (((5, 4), (0, 0, 0)), ((5, 4), (1, 4, 3)), ((7, 6), (1, 3, 3)), ((1, 1), (0, 0, 0))):
        x = E.int_x(h, wd)
        x[b, 9, py, px] = float('nan')
        y, _ = E.int_reference(x, w, bias, False)
        assert torch.equal(torch.isnan(y), E.nan_mask(y.shape, b, py, px))
    assert bool(torch.isnan(torch.relu(torch.tensor(float('nan')))))


# ------------------------------------------------------------------ what the faults do to the shift probe
# (fault, map) pairs where the fault CANNOT show, with the reason; beyond these, by construction:
#   chunks_swapped   needs two chunks: shows on the Cin >= 64 cases (test_chunk_counts) only
#   groups_swapped   needs two groups (test_slices_groups_and_guards, the NaN probes, test_same_bits_twice)
BLIND = {('taps_transposed', (1, 1)): 'on a 1 x 1 map only the centre tap reads the map, and it is its own transpose',
         ('taps_flipped', (1, 1)): 'as above: the centre tap is its own flip'}


def _shows(fault, x, cout, cin):
    for s in range(E.num_sets(cout, cin)):
        taps, cis = E.onehot(cout, cin, s)
        if not torch.equal(E.shift_expected(x, taps, cis), E.shift_expected(x, taps, cis, fault)):
            return True
    return False


def test_every_fault_changes_the_expectation_on_every_gpu_case(monkeypatch):
    single = [f for f in E.FAULTS if f not in ('chunks_swapped', 'groups_swapped')]
    seen, blind = set(), set()
    for variant, force, couts in E.ROUTES:
        entries = _entries(monkeypatch, force, couts[0])
        maps = [m for m, _ in entries] + list(E.MULTI_TILE_MAPS)
        for cout in couts:
            for m in maps:
                if (m, cout) in seen:
                    continue
                seen.add((m, cout))
                x = E.shift_x(*m)
                for fault in single:
                    if not _shows(fault, x, cout, E.CIN):
                        blind.add((fault, m))
                if m == (17, 23):
                    assert not _shows('chunks_swapped', x, cout, E.CIN)       # one chunk: nothing to swap
        # the chunk-count cases: every fault, chunks_swapped included, from two chunks up
        cout = couts[-1]
        for cin in E.CHUNK_CINS[1:]:
            for m in E.chunk_maps(entries):
                x = E.shift_x(m[0], m[1], cin)
                for fault in single + ['chunks_swapped']:
                    assert _shows(fault, x, cout, cin), (fault, m, cin, cout)
    assert blind == set(BLIND), blind ^ set(BLIND)
    # two groups: each group's weights on the other's input
    for m in ((1, 1), (1, 2), (17, 23)):
        xs = [E.shift_x(m[0], m[1], E.CIN, g) for g in range(2)]
        sets = [E.onehot(34, E.CIN, s) for s in (0, 1)]
        good, bad = E.shift_expected_groups(xs, sets), E.shift_expected_groups(xs, sets, 'groups_swapped')
        assert not torch.equal(good[0], bad[0]) and not torch.equal(good[1], bad[1]), m


# ------------------------------------------------------------------ ties of the integer cases
def test_tie_count_counts_ties():
    assert E.tie_count(torch.tensor([257.0, 258.0, 259.0, 192.5, 193.0, 0.5, 3.0, -385.0, 0.0, 511.0, 513.0, 514.0]).double()) == 6


def test_integer_cases_hold_ties(monkeypatch):
    """an integer CASE is one launch: at most eight levels (conv3_edges_ref.pack_launches), one Cout, one
    Cin; at least TIE_FLOOR of its reference elements are bf16 ties, with and without ReLU"""
    done = set()
    lowest = None
    for variant, force, couts in E.ROUTES:
        entries = _entries(monkeypatch, force, couts[0])
        launches = [(l, E.CIN, co) for co in couts
                    for l in E.pack_launches([m for m, _ in entries]) + E.pack_launches(list(E.MULTI_TILE_MAPS))]
        launches += [(E.chunk_maps(entries), cin, couts[-1]) for cin in E.CHUNK_CINS]
        if variant in (414, 214):
            launches.append((E.chunk_maps(entries), 64, 258))
        for maps, cin, cout in launches:
            key = (tuple(maps), cin, cout)
            if key in done:
                continue
            done.add(key)
            w, bias = E.int_weight(cout, cin)
            ties = [0, 0]
            for m in maps:
                y, yb = E.int_reference(E.int_x(m[0], m[1], cin), w, bias, False)
                assert float(y.abs().max()) < 2 ** 24 and torch.equal(yb, y.to(torch.bfloat16))
                ties[0] += E.tie_count(y)
                ties[1] += E.tie_count(y.clamp(min=0))
            assert min(ties) >= E.TIE_FLOOR, (variant, maps, cin, cout, ties)
            lowest = min(ties) if lowest is None else min(lowest, min(ties))
    print('  fewest ties in an integer case: %d' % lowest)

"""GPU: k_conv3x3_bf16 (csrc/conv3x3_bf16.hip, epilogue csrc/ia_conv3.hpp) at every tile shape and in every
template variant, EXACTLY.  tests/test_gpu_conv3x3_bf16.py holds the kernel to a tolerance on random data
at the shapes the models use; here every comparison is torch.equal, a bit pattern or a NaN set:

  shift probe   integer x, one-hot weights: the output is an index shift of x, and a wrong element names its
                (co, tap, ci, pixel) -- all weight sets of a case (tests/conv3_edges_ref.py)
  integer case  x in -3..3, w in -2..2, biases that put the sums on bf16 ties: equal to F.conv2d in fp64 on
                the CPU rounded once, with and without ReLU
  guards        NaN around the input slices, a bit pattern around the output slices
  NaN probes    one NaN in x reaches its 3 x 3 neighbourhood and nothing else

The case lists come from the library itself: ia_conv3x3_bf16_plan says which variant and tile shape a
map gets (conv3_edges_ref.class_maps keeps the smallest map of every distinct (TH, TW));
tests/test_host_conv3_edges.py shows on the CPU that the lists hold every class of tile shape and that
nine kinds of index error change the expectation on them.  The (1, 2, 2) variant and (2, 2, 2) at
Cout <= 64 are reached through IA_CONV3_VARIANT only, (4, 1, 4) at these sizes as well; one case at batch 16
takes the product's own route to it, the call split into two launches.  B = 2 everywhere else.
"""
import ctypes as C

import pytest
import torch

import conv3_edges_ref as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
PATTERN = 0x7FA5                        # bf16 bits of the output prefill (a NaN with a payload)
GUARD = 64                              # elements behind an output


def _ops():
    from iouaware import ops
    return ops


def _route(monkeypatch, force):
    if force is None:
        monkeypatch.delenv(E.ENV, raising=False)
    else:
        monkeypatch.setenv(E.ENV, force)


def _entries(monkeypatch, force, cout):
    _route(monkeypatch, force)
    return E.class_maps(_ops().conv3x3_bf16_plan, cout)


def _assert_variant(maps, cin, cout, variant, groups=1, shapes=None):
    """through the plan entry: this launch runs `variant` (and these tile shapes) on every level"""
    got = _ops().conv3x3_bf16_plan(list(maps), cin, cout, batch=E.B, groups=groups)
    assert [p[0] for p in got] == [variant] * len(maps), (variant, got)
    if shapes is not None:
        assert [(p[1], p[2]) for p in got] == list(shapes), (got, shapes)
    return got


# ------------------------------------------------------------------ tensors
def _nhwc(ts):
    """CPU (B, C, H, W) tensors -> one flat bf16 device tensor, level after level, pixels x channels"""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1) for t in ts]).to(BF).to(DEV)


def _views(flat, maps, c, batch=E.B):
    """the (batch, c, H, W) channels-last views of a flat buffer, level after level"""
    out, off = [], 0
    for h, w in maps:
        n = batch * h * w * c
        out.append(flat[off:off + n].view(batch, h, w, c).permute(0, 3, 1, 2))
        off += n
    assert off == flat.numel()
    return out


def _conv(maps, xs, w, bias, cout, relu, cin, batch=E.B):
    """one launch: xs a flat device buffer per group, w (groups * cout, cin, 3, 3) on the CPU -> the flat
    outputs per group"""
    ops, groups = _ops(), len(xs)
    wp = ops.conv3x3_bf16_pack(w.to(BF).to(DEV), groups=groups)
    ys = [torch.full((x.numel() // cin * cout,), PATTERN, dtype=torch.int16, device=DEV).view(BF) for x in xs]
    ops.conv3x3_bf16_levels([_views(x, maps, cin, batch) for x in xs], wp, None if bias is None else bias.to(DEV), cout,
                            [_views(y, maps, cout, batch) for y in ys], relu=relu, cin=cin)
    return ys


def _shift_case(maps, cout, cin=E.CIN):
    """all weight sets of the shift probe on one launch's maps"""
    x_cpu = [E.shift_x(h, w, cin) for h, w in maps]
    x = _nhwc(x_cpu)
    for s in range(E.num_sets(cout, cin)):
        taps, cis = E.onehot(cout, cin, s)
        want_cpu = [E.shift_expected(t, taps, cis) for t in x_cpu]
        got = _conv(maps, [x], E.onehot_weight(taps, cis, cin), None, cout, False, cin)[0]
        if not torch.equal(got, _nhwc(want_cpu)):
            for m, g, t in zip(maps, _views(got.cpu().float(), maps, cout), want_cpu):
                assert torch.equal(g, t), 'map %s Cout %d Cin %d set %d: %s' % (m, cout, cin, s, E.describe_shift_mismatch(g, t, taps, cis))
            raise AssertionError('unreachable')


def _int_case(maps, cout, cin=E.CIN):
    """the integer case on one launch's maps: equal to the fp64 convolution rounded once, without and with ReLU"""
    w, bias = E.int_weight(cout, cin)
    x_cpu = [E.int_x(h, wd, cin) for h, wd in maps]
    x = _nhwc(x_cpu)
    ref = [E.int_reference(t, w, bias, False)[0] for t in x_cpu]
    for relu in (False, True):
        want = [(r.clamp(min=0) if relu else r).to(BF) for r in ref]
        got = _conv(maps, [x], w, bias, cout, relu, cin)[0]
        if not torch.equal(got, _nhwc(want)):
            for m, g, t in zip(maps, _views(got.cpu(), maps, cout), want):
                bad = torch.nonzero(g.float() != t.float())
                assert bad.numel() == 0, ('map %s Cout %d Cin %d relu %d: %d wrong, first (b, co, h, w) = %s: got %s want %s'
                                          % (m, cout, cin, relu, bad.shape[0], bad[0].tolist(), float(g[tuple(bad[0])]), float(t[tuple(bad[0])])))
            raise AssertionError('unreachable')


# ------------------------------------------------------------------ every tile shape
@pytest.mark.parametrize('variant', E.VARIANTS)
def test_every_tile_shape(variant, monkeypatch):
    """the smallest map of every (TH, TW) the library picks, eight levels to a launch: shift probe and
    integer case, in the variant the plan entry confirms"""
    ran = 0
    for _, force, couts in E.routes_of(variant):
        for cout in couts:
            entries = _entries(monkeypatch, force, cout)
            shape_of = {m: (p[1], p[2]) for m, p in entries}
            for maps in E.pack_launches([m for m, _ in entries]):
                _assert_variant(maps, E.CIN, cout, variant, shapes=[shape_of[m] for m in maps])
                _shift_case(maps, cout)
                _int_case(maps, cout)
                ran += len(maps)
    assert ran >= 88


@pytest.mark.parametrize('variant', E.VARIANTS)
def test_multi_tile_maps(variant, monkeypatch):
    """maps of several tiles: tiles with all four neighbours, partial tiles on the right and bottom edges"""
    for _, force, couts in E.routes_of(variant):
        _route(monkeypatch, force)
        for cout in couts:
            plan = E.plan_maps(_ops().conv3x3_bf16_plan, E.MULTI_TILE_MAPS, cout)
            assert {p[0] for p in plan} == {variant}
            inner, right, bottom = E.neighbour_classes(list(zip(E.MULTI_TILE_MAPS, plan)))
            assert inner and right and bottom, (inner, right, bottom)
            for maps in E.pack_launches(list(E.MULTI_TILE_MAPS)):
                _assert_variant(maps, E.CIN, cout, variant)
                _shift_case(maps, cout)
                _int_case(maps, cout)


@pytest.mark.parametrize('variant', E.VARIANTS)
def test_chunk_counts(variant, monkeypatch):
    """1, 2, 3 and 5 chunks of 32 input channels: the first patch buffer alone, both, the first one reused, the
    `chunk + 1 < nchunk` and `step + 2 < nsteps` clamps at the end of the K loop; on the WN = 4 variants
    also Cout = 258: two column tiles, the second with one channel pair"""
    for _, force, couts in E.routes_of(variant):
        maps = E.chunk_maps(_entries(monkeypatch, force, couts[-1]))
        for cin in E.CHUNK_CINS:
            _assert_variant(maps, cin, couts[-1], variant)
            _shift_case(maps, couts[-1], cin)
            _int_case(maps, couts[-1], cin)
        if variant in (414, 214):
            _assert_variant(maps, 64, 258, variant)
            _shift_case(maps, 258, 64)
            _int_case(maps, 258, 64)


def test_large_and_small_maps_split_into_two_launches(monkeypatch):
    """the product's own route to (4, 1, 4): a map with 2048 or more 128-pixel tiles in the batch goes to a launch
    of its own, the other levels of the call to (2, 1, 4) -- here the large map BETWEEN two small ones, so that
    both launches renumber their levels.  Shift probe, one weight set, the expectation built on the device."""
    _route(monkeypatch, None)
    batch, cout, maps = 16, 130, [(7, 11), (100, 168), (13, 21)]
    plan = _ops().conv3x3_bf16_plan(maps, E.CIN, cout, batch=batch)
    assert [p[0] for p in plan] == [214, 414, 214] and batch * plan[1][3] * plan[1][4] >= 2048
    x_dev = [E.shift_x(h, w, batch=batch).to(DEV) for h, w in maps]
    taps, cis = E.onehot(cout, E.CIN, 1)
    got = _conv(maps, [_nhwc(x_dev)], E.onehot_weight(taps, cis, E.CIN), None, cout, False, E.CIN, batch=batch)[0]
    for m, g, x in zip(maps, _views(got, maps, cout, batch), x_dev):
        want = E.shift_expected(x, taps, cis)
        assert torch.equal(g.float(), want), (m, E.describe_shift_mismatch(g.float().cpu(), want.cpu(), taps, cis))


# ------------------------------------------------------------------ slices, groups, guards
def _sliced_x(x_cpu, cin):
    """two groups' (B, cin, H, W) inputs as the channel slices [32, 32 + cin) and [32 + cin, 32 + 2 cin) of one
    NaN-filled channels-last tensor -> (the wide tensor, [slice 0, slice 1])"""
    Bn, _, h, w = x_cpu[0].shape
    wide = torch.full((Bn, h, w, 64 + 2 * cin), float('nan'), dtype=BF, device=DEV)
    for g in range(2):
        wide[..., 32 + g * cin:32 + (g + 1) * cin] = x_cpu[g].permute(0, 2, 3, 1).to(BF).to(DEV)
    wide = wide.permute(0, 3, 1, 2)
    return wide, [wide[:, 32 + g * cin:32 + (g + 1) * cin] for g in range(2)]


def _sliced_y(h, w, cout):
    """-> (flat buffer, wide (B, 2 cout + 8, H, W) view, [slice 0, slice 1]): the two groups' outputs are the
    channel slices [2, 2 + cout) and [2 + cout, 2 + 2 cout) of a pattern-filled tensor with GUARD elements behind
    it: bases 4-byte aligned, not 16"""
    cw = 2 * cout + 8
    n = E.B * h * w * cw
    flat = torch.full((n + GUARD,), PATTERN, dtype=torch.int16, device=DEV).view(BF)
    wide = flat[:n].view(E.B, h, w, cw).permute(0, 3, 1, 2)
    sl = [wide[:, 2 + g * cout:2 + (g + 1) * cout] for g in range(2)]
    assert all(s.data_ptr() % 4 == 0 for s in sl) and sl[0].data_ptr() % 16 == 4
    return flat, wide, sl


def _run_sliced(maps, x_cpu, w, bias, cout, relu, cin=E.CIN):
    """one two-group launch on sliced tensors; checks the guards; -> [group][level] outputs on the CPU"""
    ops = _ops()
    xin = [_sliced_x([x_cpu[0][l], x_cpu[1][l]], cin) for l in range(len(maps))]
    yout = [_sliced_y(h, wd, cout) for h, wd in maps]
    wp = ops.conv3x3_bf16_pack(w.to(BF).to(DEV), groups=2)
    ops.conv3x3_bf16_levels([[xi[1][g] for xi in xin] for g in range(2)], wp, None if bias is None else bias.to(DEV),
                            cout, [[yo[2][g] for yo in yout] for g in range(2)], relu=relu, cin=cin)
    torch.cuda.synchronize()
    for m, (flat, wide, sl) in zip(maps, yout):
        inside = wide[:, 2:2 + 2 * cout].contiguous().view(torch.int16)
        assert not bool((inside == PATTERN).any()), ('an element inside the slices was not written', m)
        chk = flat.clone().view(torch.int16)
        chk[:wide.numel()].view(E.B, m[0], m[1], 2 * cout + 8)[..., 2:2 + 2 * cout] = PATTERN
        assert bool((chk == PATTERN).all()), ('an element outside the slices was written', m)
    return [[yo[2][g].cpu() for yo in yout] for g in range(2)]


@pytest.mark.parametrize('variant', E.VARIANTS)
def test_slices_groups_and_guards(variant, monkeypatch):
    """two groups in one launch on channel slices: x between NaN channels, y at channel 2 of a pattern-filled
    tensor; every element inside written, every element outside untouched, the groups' results the two
    single-group results.  With the 1 x 1 and 1 x 2 maps, whose pixel stride is the image stride."""
    for _, force, couts in E.routes_of(variant):
        cout = couts[0]
        maps = [(1, 1), (1, 2)] + E.chunk_maps(_entries(monkeypatch, force, cout))[:4]
        _assert_variant(maps, E.CIN, cout, variant, groups=2)
        # shift probe: group g on weight set s + g
        x_cpu = [[E.shift_x(h, w, E.CIN, g) for h, w in maps] for g in range(2)]
        ns = E.num_sets(cout)
        for s in range(ns):
            sets = [E.onehot(cout, E.CIN, (s + g) % ns) for g in range(2)]
            w = torch.cat([E.onehot_weight(t, c, E.CIN) for t, c in sets])
            got = _run_sliced(maps, x_cpu, w, None, cout, False)
            for g in range(2):
                alone = _conv(maps, [_nhwc(x_cpu[g])], w[g * cout:(g + 1) * cout], None, cout, False, E.CIN)[0]
                assert torch.equal(_nhwc(got[g]), alone), (variant, s, g)
                for l, m in enumerate(maps):
                    want = E.shift_expected(x_cpu[g][l], *sets[g])
                    assert torch.equal(got[g][l].float(), want), (m, s, g, E.describe_shift_mismatch(got[g][l].float(), want, *sets[g]))
        # integer case, bias and ReLU
        w, bias = E.int_weight(cout, E.CIN, groups=2)
        x_cpu = [[E.int_x(h, wd, E.CIN, g) for h, wd in maps] for g in range(2)]
        got = _run_sliced(maps, x_cpu, w, bias, cout, True)
        for g in range(2):
            wg, bg = w[g * cout:(g + 1) * cout], bias[g * cout:(g + 1) * cout]
            alone = _conv(maps, [_nhwc(x_cpu[g])], wg, bg, cout, True, E.CIN)[0]
            assert torch.equal(_nhwc(got[g]), alone), (variant, g)
            for l, m in enumerate(maps):
                assert torch.equal(got[g][l], E.int_reference(x_cpu[g][l], wg, bg, True)[1]), (m, g)


# ------------------------------------------------------------------ NaN containment
@pytest.mark.parametrize('variant', E.VARIANTS)
def test_nan_stays_in_its_neighbourhood(variant, monkeypatch):
    """one NaN in x per launch: without ReLU isnan(y) is the definition's set (the 3 x 3 neighbourhood, every
    output channel, that image and group) and every other element keeps the clean run's value -- a NaN at a
    clamped border address does not reach the padding taps (the AND mask), the idle rows that read the tile's last
    pixel store nothing.  With ReLU the same positions hold +0.0: the epilogue computes v > 0 ? v : 0, which
    sends NaN to 0 where torch.relu keeps it."""
    assert bool(torch.isnan(torch.relu(torch.tensor(float('nan'), device=DEV))))
    for _, force, couts in E.routes_of(variant):
        _route(monkeypatch, force)
        cout, maps = couts[0], [(17, 23), (5, 7)]
        plan = _assert_variant(maps, E.CIN, cout, variant, groups=2)
        th, tw = plan[0][1], plan[0][2]
        assert plan[0][3] >= 2 and plan[0][4] >= 2
        w, bias = E.int_weight(cout, E.CIN, groups=2)
        x_cpu = [[E.int_x(h, wd, E.CIN, g) for h, wd in maps] for g in range(2)]
        # (group, image, channel, y, x) in level 0: a corner; an interior pixel whose neighbourhood lies in four
        # tiles; the last pixel of the last image; one channel of group 1 only
        probes = ((0, 0, 1, 0, 0), (0, 0, 14, th, tw), (0, E.B - 1, 31, 16, 22), (1, 1, 17, 3, 5))
        for relu in (False, True):
            clean = _conv(maps, [_nhwc(x) for x in x_cpu], w, bias, cout, relu, E.CIN)
            assert not any(bool(torch.isnan(c).any()) for c in clean)
            for (g, b, c, py, px) in probes:
                xn = [[t.clone() for t in x] for x in x_cpu]
                xn[g][0][b, c, py, px] = float('nan')
                got = _conv(maps, [_nhwc(x) for x in xn], w, bias, cout, relu, E.CIN)
                mask = [torch.zeros_like(cl, dtype=torch.bool) for cl in clean]
                mask[g] = _nhwc([E.nan_mask((E.B, cout) + maps[0], b, py, px).float(), torch.zeros((E.B, cout) + maps[1])]) != 0
                for k in range(2):
                    if relu:
                        assert not bool(torch.isnan(got[k]).any()), (variant, relu, g, b, c, py, px)
                        assert bool((got[k].view(torch.int16)[mask[k]] == 0).all()), (variant, g, b, c, py, px)
                    else:
                        assert torch.equal(torch.isnan(got[k]), mask[k]), (variant, g, b, c, py, px, k)
                    assert torch.equal(got[k][~mask[k]], clean[k][~mask[k]]), (variant, relu, g, b, c, py, px, k)


# ------------------------------------------------------------------ the same bits on every run
@pytest.mark.parametrize('variant', E.VARIANTS)
def test_same_bits_twice(variant, monkeypatch):
    for _, force, couts in E.routes_of(variant):
        _route(monkeypatch, force)
        cout, cin, maps = couts[-1], 96, [(25, 37), (13, 21), (7, 11), (3, 70), (1, 1)]
        _assert_variant(maps, cin, cout, variant, groups=2)
        g = torch.Generator().manual_seed(variant)
        xs = [_nhwc([torch.randn(E.B, cin, h, w, generator=g) for h, w in maps]) for _ in range(2)]
        w = torch.randn(2 * cout, cin, 3, 3, generator=g) * 0.05
        bias = torch.randn(2 * cout, generator=g)
        a = _conv(maps, xs, w, bias, cout, True, cin)
        b = _conv(maps, xs, w, bias, cout, True, cin)
        for k in range(2):
            assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), (variant, k)
            assert not bool((a[k].view(torch.int16) == PATTERN).any())


# ------------------------------------------------------------------ the adjoint pack (input gradient of bf16 training)
@pytest.mark.parametrize('variant,cin', [(414, 160), (214, 160), (222, 96), (122, 96), (141, 64)])
@pytest.mark.parametrize('cout0', [45, 64, 80])
def test_adjoint_pack_probe(variant, cin, cout0, monkeypatch):
    """ops.conv3x3_bf16_pack(w_fp32, adjoint=True) of a one-hot weight (cout0, cin, 3, 3), run through the kernel
    on dy: dx[b, ci, h, w] = sum over the co with cis[co] = ci of dy[b, co, h - dy + 1, w - dx + 1], the
    FLIPPED-tap shift of dy (at most two terms of -128..127 per element: exact in bf16).  The kernel reads
    P = cout0 rounded up to 32 channels per pixel; the packed weight has zero rows for the padding.
    Contract (include/iouaware.h, ia_conv3x3_bf16_pack_f32): the padding channels of dy must be FINITE, no more;
    iouaware/conv3x3_bf16_train.py hands in buffers whose padding it zeroed once (`_zeroed_levels`), which is
    inside that contract.  Here the padding holds 77 and must not show in dx."""
    ops = _ops()
    force = {414: '41', 122: '12'}.get(variant)
    _route(monkeypatch, force)
    P = (cout0 + 31) // 32 * 32
    maps = [(1, 1), (5, 7), (17, 23)]
    _assert_variant(maps, P, cin, variant)                      # the kernel's Cin = P, its Cout = cin
    q = torch.arange(cout0)
    taps, cis = q % 9, (q * 7 + 3) % cin                        # injective up to cout0 = cin; two co per ci at (80, 64)
    assert int(torch.bincount(cis, minlength=cin).max()) <= 2
    wt = ops.conv3x3_bf16_pack(E.onehot_weight(taps, cis, cin).to(DEV), adjoint=True)
    dy_cpu = [torch.randint(-128, 128, (E.B, cout0, h, w), generator=torch.Generator().manual_seed(h * w + cout0)).float()
              for h, w in maps]
    padded = [torch.cat([t, torch.full((E.B, P - cout0) + t.shape[2:], 77.0)], 1) for t in dy_cpu]
    dy = _nhwc(padded)
    dx = torch.full((dy.numel() // P * cin,), PATTERN, dtype=torch.int16, device=DEV).view(BF)
    ops.conv3x3_bf16_levels([_views(dy, maps, P)], wt, None, cin, [_views(dx, maps, cin)], relu=False, cin=P)
    for m, t, got in zip(maps, dy_cpu, _views(dx.cpu().float(), maps, cin)):
        want = torch.zeros(E.B, cin, m[0], m[1])
        want.index_add_(1, cis, E.shift_expected(t, 8 - taps, torch.arange(cout0)))
        assert float(want.abs().max()) <= 256
        assert torch.equal(got, want), (variant, cout0, m, int((got != want).sum()))


# ------------------------------------------------------------------ rejections
def test_bad_arguments_leave_the_output_untouched():
    from iouaware import _lib
    ops, lib = _ops(), _lib.lib()
    h, w, cin, cout = 5, 7, 64, 66
    x = torch.zeros(E.B * h * w * cin + 64, dtype=BF, device=DEV)
    wp = ops.conv3x3_bf16_pack(torch.zeros(2 * cout, cin, 3, 3, dtype=BF, device=DEV), groups=2)
    bias = torch.zeros(2 * cout, device=DEV)
    outs = []

    def call(levels=1, groups=1, cin=cin, cout=cout, xs=cin, ys=cout, x_off=0):
        y = torch.full((E.B * h * w * 2 * cout + GUARD,), PATTERN, dtype=torch.int16, device=DEV)
        outs.append(y)
        d = _lib.Conv3x3Desc()
        d.num_levels, d.batch, d.groups = levels, E.B, groups
        d.cin, d.cout, d.x_stride, d.y_stride = cin, cout, xs, ys
        for l in range(min(levels, _lib.IA_MAX_LEVELS)):
            d.H[l], d.W[l] = h, w
            for g in range(2):
                d.x[g][l], d.y[g][l] = x.data_ptr() + 2 * x_off, y.data_ptr()
        return lib.ia_conv3x3_bf16_levels(C.byref(d), C.c_void_p(wp.data_ptr()), C.c_void_p(bias.data_ptr()), 1, ops._stream())

    assert call() == 0                                              # the descriptor itself is a good one
    torch.cuda.synchronize()
    assert not bool((outs.pop()[:E.B * h * w * cout] == PATTERN).any())
    bad = [('Cin 48', call(cin=48, xs=48)), ('odd Cout', call(cout=65)), ('x_stride < cin', call(xs=56)),
           ('x_stride % 8', call(xs=68)), ('x slice at channel 4', call(x_off=4)), ('9 levels', call(levels=9)),
           ('3 groups', call(groups=3))]
    torch.cuda.synchronize()
    assert [what for what, rc in bad if rc != -1] == []             # IA_E_ARG
    assert len(outs) == 7
    for y in outs:
        assert bool((y == PATTERN).all())

"""CPU helpers of tests/test_gpu_conv3x3_bf16_edges.py and tests/test_host_conv3_edges.py: the bf16 3x3
implicit-GEMM convolution (csrc/conv3x3_bf16.hip, epilogue csrc/ia_conv3.hpp) written from its definition
in plain torch.  Test-only: nothing imported from the project; the functions that need the library's launch
geometry take `plan` = iouaware.ops.conv3x3_bf16_plan as an argument.

    y[b, co, h, w] = relu?(bias[co] + sum_{ci, dy, dx} w[co, ci, dy, dx] * x[b, ci, h + dy - 1, w + dx - 1])
    (x = 0 outside the map), x / w / y bf16, one rounding (nearest even) at the end.

Two exact instruments:

  * SHIFT PROBE (`shift_x`, `onehot`, `shift_expected`): x = integers in -128..127 (exact in bf16), a
    ONE-HOT weight -- output channel co holds a single 1 at (ci, tap) = `onehot(...)[co]`, for weight set 0
    tap = co % 9 -- so the expected output is a pure index shift, built with F.pad and slicing, no
    convolution.  Over the `num_sets` weight sets of a case every (tap, input channel) pair is read by some
    output channel (from 32 output channels up; with fewer the sets cover every tap with every
    8-channel k-group, see `num_sets`), and every output channel carries a 1, i.e. every column slot of
    the kernel (n mod 64, both j halves, every wavefront column below Cout) stores a value that names its
    source.  `describe_shift_mismatch` names (co, tap, ci, pixel) of the first wrong element.
  * INTEGER CASE (`int_x`, `int_weight`, `int_reference`): x in -3..3, w in -2..2, bias[co] = BIASES[co % 8], which puts
    the sums on bf16 TIES: 384.0 -> sums in 256..512, where bf16 has a spacing of 2 and every odd value is
    a tie; 192.5 -> n + 0.5 in 128..256 (spacing 1).  9 * Cin * 3 * 2 + |bias| < 2^24 (`int_bound`, asserted),
    so every fp32 partial sum is exact in any order and the kernel must EQUAL F.conv2d in fp64 on the CPU
    rounded once with .to(torch.bfloat16).  `tie_count` counts the tie elements of a reference.

`FAULTS` are the nearest WRONG results of the shift probe (tests/test_host_conv3_edges.py shows that each
changes the expected tensor on the GPU case lists).

The case lists come from the library: `class_maps` replays ia_conv3x3_bf16_plan over `ENUM_MAPS` and keeps
the smallest map of every distinct tile shape (TH, TW); `ROUTES` says how each kernel variant is reached.
"""
import torch
import torch.nn.functional as F

B = 2                       # images per case: image offsets count
CIN = 32                    # unless stated
LEVELS = 8                  # levels per launch (IA_MAX_LEVELS)

# (variant = 100 * MB + 10 * WM + WN, IA_CONV3_VARIANT or None for the default route, Cout per group)
#   130: a partial third wavefront column, nothing in the fourth; 66: one channel pair in the second
#   column; 64 under "22": the second wavefront column multiplies zeros
ROUTES = ((414, '41', (130,)), (214, None, (130,)), (222, None, (66, 128)), (222, '22', (64,)),
          (122, '12', (66, 128)), (141, None, (2, 34, 64)))
VARIANTS = (414, 214, 222, 122, 141)
ENV = 'IA_CONV3_VARIANT'

# the maps with several tiles.  The first nine are too small for a 128-pixel tile with all four neighbours
# (the shape search takes the FEWEST tiles); (25, 37) is the smallest-but-four map with 3 x 3 of them
MULTI_TILE_MAPS = ((17, 23), (9, 41), (13, 21), (25, 42), (33, 3), (3, 70), (31, 31), (16, 64), (20, 30), (25, 37))
ENUM_MAPS = tuple((h, w) for h in range(1, 13) for w in range(1, 37)) + MULTI_TILE_MAPS
CHUNK_CINS = (32, 64, 96, 160)          # 1, 2, 3, 5 chunks of 32 input channels

BIASES = (384.0, 192.5, -384.0, 0.5, -192.5, 0.0, 3.0, -0.5)
TIE_FLOOR = 64


def routes_of(variant):
    return [r for r in ROUTES if r[0] == variant]


def tile_pixels(variant):
    """pixels of a workgroup's tile: 32 * MB * WM"""
    return 32 * (variant // 100) * (variant // 10 % 10)


# ------------------------------------------------------------------ case lists (through the plan entry)
def plan_maps(plan, maps, cout, cin=CIN, groups=1):
    """-> [(variant, TH, TW, tiles_y, tiles_x)] per map, asked LEVELS maps at a time"""
    out = []
    for i in range(0, len(maps), LEVELS):
        out += plan(list(maps[i:i + LEVELS]), cin, cout, batch=B, groups=groups)
    return out


def class_maps(plan, cout, maps=ENUM_MAPS):
    """-> [((H, W), (variant, TH, TW, tiles_y, tiles_x))]: the smallest map (area, then H, then W) of every
    distinct (TH, TW) the library returns over `maps`, sorted by map.  The caller has set ENV."""
    best = {}
    for m, p in zip(maps, plan_maps(plan, maps, cout)):
        key = (p[1], p[2])
        if key not in best or (m[0] * m[1], m) < (best[key][0][0] * best[key][0][1], best[key][0]):
            best[key] = (m, p)
    return sorted(best.values(), key=lambda e: (e[0][0] * e[0][1], e[0]))


def tile_classes(entries):
    """-> {class name: [(H, W), ...]} of a class_maps list.  The walks these classes are about:
      tw4_th3     TW = 4 (and TW = 5: `tw5`): the epilogue's +6 row walk wraps twice
      tw_odd32    32 % TW != 0: the a_off walk over q32 / r32 wraps inside a 32-pixel block
      tw32, tw_gt32   q32 = 1 / 0 (128-pixel tiles only: a 64-pixel tile is at most 30 wide, below)
      th2_h1      TH = 2 on an H = 1 map: the tile's second row is all overhang
      below32     TH * TW < 32: whole 32-pixel accumulator blocks are idle
      full        TH * TW = the whole tile: no idle row"""
    out = {k: [] for k in ('tw4_th3', 'tw5', 'tw_odd32', 'tw32', 'tw_gt32', 'th2_h1', 'below32', 'full')}
    for (h, w), (v, th, tw, _, _) in entries:
        for name, hit in (('tw4_th3', tw == 4 and th >= 3), ('tw5', tw == 5), ('tw_odd32', 32 % tw != 0),
                          ('tw32', tw == 32), ('tw_gt32', tw > 32), ('th2_h1', th == 2 and h == 1),
                          ('below32', th * tw < 32), ('full', th * tw == tile_pixels(v))):
            if hit:
                out[name].append((h, w))
    return out


# classes a variant cannot reach, with the reason
UNREACHABLE = {
    64: {'tw32': 'a 64-pixel tile stages (TH + 2) * (TW + 2) <= 128 patch pixels: TH >= 2 caps TW at 30',
         'tw_gt32': 'as tw32: q32 = 32 / TW is at least 1 on every 64-pixel variant'},
    128: {},
}


def neighbour_classes(entries):
    """of [((H, W), plan)]: maps with a tile that has all four neighbours, with partial tiles on the right,
    with partial tiles at the bottom"""
    return ([m for m, p in entries if p[3] >= 3 and p[4] >= 3],
            [m for m, p in entries if m[1] % p[2]],
            [m for m, p in entries if m[0] % p[1]])


def pack_launches(maps):
    """the maps dealt round-robin (in their order: callers pass them sorted by area) onto the fewest
    launches of at most LEVELS levels: every launch gets small and large maps"""
    n = (len(maps) + LEVELS - 1) // LEVELS
    return [list(maps[i::n]) for i in range(n)]


def chunk_maps(entries):
    """six maps for the chunk-count cases: of a class_maps list the first TW = 4 / TH >= 3 map, the first
    32 % TW != 0 map with two rows or more, the widest tile's map; and three of MULTI_TILE_MAPS"""
    c = tile_classes(entries)
    widest = max(entries, key=lambda e: (e[1][2], e[1][1]))[0]
    odd = [m for m in c['tw_odd32'] if m[0] >= 2 and m not in (c['tw4_th3'][0], widest)][0]
    return [c['tw4_th3'][0], odd, widest, (17, 23), (9, 41), (33, 3)]


# ------------------------------------------------------------------ data
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * m for v, m in zip(key, (1, 37, 1009, 65537, 7, 131))) + 5)


def shift_x(h, w, cin=CIN, group=0, batch=B):
    """(batch, cin, h, w) integers in -128..127 as fp32 (exact in bf16)"""
    return torch.randint(-128, 128, (batch, cin, h, w), generator=_gen(h, w, cin, group, 1)).float()


def num_sets(cout, cin=CIN):
    """weight sets of a (cout, cin) case.  9 * cin (tap, channel) pairs, cout of them per set: all pairs from
    32 output channels up (at most 9 * cin / 32 sets); below that every tap with every 8-channel k-group
    (what one lane feeds into one MFMA), 9 * cin / 8 pairs -- all pairs would take 144 sets at Cout = 2,
    and the wider cases of the same variant run the same maps.  At least two, so that the two groups of
    a launch can hold different sets."""
    if cout >= 32:
        return max(2, (9 * cin + cout - 1) // cout)
    return (9 * (cin // 8) + cout - 1) // cout


def onehot(cout, cin, s):
    """weight set s -> (taps, cis): LongTensors (cout), output channel co reads input channel cis[co] at
    tap taps[co] = 3 * dy + dx.  With q = s * cout + co: tap = q % 9 (set 0: tap = co % 9); from 32
    output channels up ci = perm[q // 9 mod cin] with a seeded permutation, below that ci walks the
    8-channel k-groups, q // 9 mod cin / 8, at a changing place inside the group."""
    q = s * cout + torch.arange(cout)
    if cout >= 32:
        perm = torch.randperm(cin, generator=_gen(cin, 0, 0, 0, 9))
        return q % 9, perm[(q // 9) % cin]
    return q % 9, ((q // 9) % (cin // 8)) * 8 + (q * 3) % 8


def onehot_weight(taps, cis, cin):
    """(cout, cin, 3, 3) fp32"""
    cout = taps.numel()
    w = torch.zeros(cout, cin, 9)
    w[torch.arange(cout), cis, taps] = 1.0
    return w.view(cout, cin, 3, 3)


FAULTS = ('taps_transposed', 'taps_flipped', 'kk_halves_swapped', 'chunks_swapped', 'pad_clamped',
          'row_wrap_missing', 'image_off_by_one', 'groups_swapped', 'channel_pair_swapped')


def shift_expected(x, taps, cis, fault=None):
    """x (B, cin, H, W), one-hot weight (taps, cis) -> y (B, cout, H, W) = x[b, cis[co], h + dy - 1, w + dx - 1],
    0 outside the map: F.pad and nine slices.  `fault`: one of FAULTS (not groups_swapped: see
    shift_expected_groups), the result a kernel with that index error would give."""
    Bn, cin, H, W = x.shape
    taps, cis = taps.clone().to(x.device), cis.clone().to(x.device)
    if fault == 'taps_transposed':
        taps = (taps % 3) * 3 + taps // 3
    elif fault == 'taps_flipped':
        taps = 8 - taps
    elif fault == 'kk_halves_swapped':              # the two 16-wide halves of a 32-channel chunk
        cis = cis ^ 16
    elif fault == 'chunks_swapped':                 # chunks c and c + 1 (c even, where c + 1 exists)
        c = cis // 32
        partner = c ^ 1
        cis = torch.where(partner < cin // 32, partner * 32 + cis % 32, cis)
    elif fault == 'image_off_by_one':
        x = x.roll(-1, 0)
    if fault == 'pad_clamped':
        xp = F.pad(x, (1, 1, 1, 1), mode='replicate')
    else:
        xp = F.pad(x, (1, 1, 1, 1))
    if fault == 'row_wrap_missing':
        # flat addressing: the pixel right of a row's end is the next row's first, left of its start the
        # previous row's last
        xq = xp.clone()
        xq[:, :, :-1, W + 1] = xp[:, :, 1:, 1]
        xq[:, :, 1:, 0] = xp[:, :, :-1, W]
        xp = xq
    y = torch.zeros(Bn, taps.numel(), H, W, dtype=x.dtype, device=x.device)
    for t in range(9):
        cos = torch.nonzero(taps == t).flatten()
        if cos.numel():
            dy, dx = t // 3, t % 3
            y[:, cos] = xp[:, cis[cos], dy:dy + H, dx:dx + W]
    if fault == 'channel_pair_swapped':
        y = y[:, torch.arange(y.shape[1], device=x.device) ^ 1]
    return y


def shift_expected_groups(xs, sets, fault=None):
    """two groups: xs[g] and sets[g] = (taps, cis) -> [y_0, y_1]; groups_swapped: each group's weights on
    the other group's input"""
    if fault == 'groups_swapped':
        xs = xs[::-1]
        fault = None
    return [shift_expected(x, t, c, fault) for x, (t, c) in zip(xs, sets)]


def describe_shift_mismatch(got, want, taps, cis):
    """first wrong element of a shift-probe output (B, cout, H, W) -> text naming (co, tap, ci, pixel)"""
    bad = torch.nonzero(got.double() != want.double())
    if bad.numel() == 0:
        return 'equal'
    b, co, h, w = (int(v) for v in bad[0])
    t = int(taps[co])
    return ('%d wrong of %d; first: image %d, co %d (tap %d = (dy %d, dx %d), ci %d), pixel (%d, %d) of %d x %d: '
            'got %s, want %s' % (bad.shape[0], want.numel(), b, co, t, t // 3, t % 3, int(cis[co]), h, w,
                                 want.shape[2], want.shape[3], float(got[b, co, h, w]), float(want[b, co, h, w])))


# ------------------------------------------------------------------ the integer case
def int_bound(cin, bias):
    return 9 * cin * 3 * 2 + (float(bias.abs().max()) if bias is not None else 0.0)


def int_weight(cout, cin, groups=1):
    """-> w (groups * cout, cin, 3, 3) in -2..2 and bias (groups * cout) = BIASES[co % 8], both fp32"""
    g = _gen(cout, cin, groups, 0, 3)
    w = torch.randint(-2, 3, (groups * cout, cin, 3, 3), generator=g).float()
    bias = torch.tensor(BIASES)[torch.arange(groups * cout) % len(BIASES)].float()
    assert int_bound(cin, bias) < 2 ** 24
    return w, bias


def int_x(h, w, cin=CIN, group=0):
    """(B, cin, h, w) integers in -3..3 as fp32"""
    return torch.randint(-3, 4, (B, cin, h, w), generator=_gen(h, w, cin, group, 2)).float()


def int_reference(x, w, bias, relu):
    """F.conv2d in fp64 on the CPU, rounded ONCE to bf16"""
    assert x.device.type == 'cpu' and int_bound(x.shape[1], bias) < 2 ** 24
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), 1, 1)
    if relu:
        y = y.clamp(min=0)
    return y, y.to(torch.bfloat16)


def tie_count(y64):
    """elements of an fp64 tensor that lie exactly between two neighbouring bf16 values"""
    near = y64.to(torch.bfloat16).double()
    _, e = torch.frexp(y64)                         # |y| = m * 2^e, m in [0.5, 1): bf16 spacing 2^(e - 8)
    return int((((y64 - near).abs() * 2 == torch.ldexp(torch.ones_like(y64), e - 8)) & (y64 != 0)).sum())


# ------------------------------------------------------------------ NaN containment
def nan_mask(shape, b, h, w):
    """(B, cout, H, W) bool: the outputs a NaN at x[b, :, h, w] reaches by the definition -- the 3 x 3
    neighbourhood, every output channel (NaN * 0 = NaN), that image"""
    m = torch.zeros(shape, dtype=torch.bool)
    m[b, :, max(h - 1, 0):h + 2, max(w - 1, 0):w + 2] = True
    return m

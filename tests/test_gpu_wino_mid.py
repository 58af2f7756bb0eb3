"""GPU (MI355X): ia_wino_mid_transform (csrc/wino.hip k_wino_mid: the output transform of a tower
layer and the input transform of the next in one launch, the activation in LDS) against
output_transform -> input_transform: the same bits (torch.equal), every element of V written and
nothing beside it, and the whole WinogradHead on the fused route against the two-launch route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BENCH_PYRAMID = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
E2E_PYRAMID = [(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)]                 # a 256 x 320 image

GUARD = 4096          # floats on either side of V


def _both(sizes, batch, channels, groups_m, groups_v, with_bias, relu=True, seed=0):
    """-> (V of the two launches, V of the fused launch inside its guard bands, the bands)"""
    from iouaware import winograd as wg
    dev = torch.device('cuda')
    plan = wg._Plan(sizes, batch, dev)
    T = plan.T
    g = torch.Generator(device='cuda').manual_seed(seed)
    m = torch.randn(groups_m * 36, T, channels // groups_m, device=dev, generator=g)     # both signs
    bias = torch.randn(channels, device=dev, generator=g) if with_bias else None
    acts = [torch.full((batch, channels, h, w), float('nan'), device=dev)
            .contiguous(memory_format=torch.channels_last) for (h, w) in sizes]
    wg.output_transform(plan, m, channels, groups_m, bias, relu, [(0, channels, acts, 0)])
    ref = torch.full((groups_v * 36, T, channels // groups_v), float('nan'), device=dev)
    wg.input_transform(plan, acts, groups_v, ref)
    n = ref.numel()
    # the destination starts as NaN (every element must be written), the guard bands as a pattern
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev)
    buf[:GUARD] = 12345.0
    buf[GUARD + n:] = 12345.0
    got = buf[GUARD:GUARD + n].view_as(ref)
    assert got.data_ptr() % 16 == 0
    wg.mid_transform(plan, m, channels, groups_m, bias, relu, got, groups_v)
    torch.cuda.synchronize()
    return ref, got, (buf[:GUARD], buf[GUARD + n:])


def _check(sizes, batch, channels, groups_m, groups_v, with_bias, relu=True, seed=0):
    ref, got, bands = _both(sizes, batch, channels, groups_m, groups_v, with_bias, relu, seed)
    assert not bool(torch.isnan(ref).any())
    assert not bool(torch.isnan(got).any()), 'elements of V left unwritten'
    assert torch.equal(got, ref), 'differs in %d of %d elements' % (int((got != ref).sum()), ref.numel())
    for band in bands:
        assert bool((band == 12345.0).all()), 'written outside V'


@pytest.mark.parametrize('batch', [8, 1])
@pytest.mark.parametrize('groups_m,groups_v', [(1, 2), (2, 2)])
def test_bench_pyramid(batch, groups_m, groups_v):
    """the head's tower transitions at the bench shape: 512 channels, layer 0 -> 1 (one group of 2F
    columns in, two groups out) and the later ones (two groups both sides)"""
    _check(BENCH_PYRAMID, batch, 512, groups_m, groups_v, True, seed=batch)


@pytest.mark.parametrize('batch', [2, 1])
def test_small_e2e_pyramid(batch):
    _check(E2E_PYRAMID, batch, 512, 2, 2, True, seed=3 + batch)
    _check(E2E_PYRAMID, batch, 512, 1, 2, True, seed=5 + batch)


@pytest.mark.parametrize('sizes', [
    [(30, 32)],                       # partial tiles in y
    [(32, 27)],                       # ... in x
    [(33, 35)], [(37, 70)],           # ... in both; more than one block per side
    [(3, 2)], [(1, 1)],               # a level smaller than one tile
    [(4, 4)], [(32, 32)], [(36, 36)],  # exact tiles; exactly one block; one tile more than a block
    [(65, 9), (2, 67), (5, 5)],       # several levels, blocks clipped on every side
])
@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('with_bias', [True, False])
def test_edges_groups_bias(sizes, groups, with_bias):
    _check(sizes, 3, 64, groups, groups, with_bias, seed=len(sizes) + groups)


def test_without_relu_and_group_change():
    _check([(33, 35), (9, 6)], 2, 128, 1, 2, True, relu=False, seed=11)
    _check([(33, 35), (9, 6)], 2, 128, 2, 1, False, relu=False, seed=12)
    _check([(33, 35), (9, 6)], 2, 128, 4, 2, True, relu=True, seed=13)


def test_rejects_what_it_cannot_split():
    from iouaware import winograd as wg, _lib
    plan = wg._Plan([(8, 8)], 1, torch.device('cuda'))
    m = torch.zeros(36, plan.T, 48, device='cuda')
    v = torch.zeros(36, plan.T, 48, device='cuda')
    with pytest.raises(_lib.IouAwareLibraryError):
        wg.mid_transform(plan, m, 48, 1, None, True, v, 1)              # 48 % 32 != 0
    m = torch.zeros(72, plan.T, 16, device='cuda')
    with pytest.raises(_lib.IouAwareLibraryError):
        wg.mid_transform(plan, m, 32, 2, None, True, v, 1)              # 16 channels per group


def _head(seed):
    import iouaware
    from iouaware.config import ConfigDict
    from iouaware.fuse import fuse_inference
    import bench
    torch.manual_seed(seed)
    m = iouaware.build_detector(ConfigDict(bench.MODEL), test_cfg=ConfigDict(bench.TEST_CFG)).cuda().eval()
    with torch.no_grad():
        for p in m.bbox_head.parameters():
            if p.dim() == 4:
                p.normal_(0, (2.0 / (9 * p.shape[1])) ** 0.5)
            else:
                p.normal_(0, 0.5)                                       # biases of both signs
    fuse_inference(m, winograd=True)
    return m.bbox_head


@pytest.mark.parametrize('batch,sizes', [(8, BENCH_PYRAMID), (2, E2E_PYRAMID)])
def test_whole_head_fused_route_equals_two_launch_route(batch, sizes):
    """all 15 head outputs bit-equal, and the fused route is the one the head takes"""
    from iouaware import winograd as wg
    head = _head(7)
    w = head._ia_wino
    assert isinstance(w, wg.WinogradHead) and w.FUSE_MID and w.mid_bias is not None
    g = torch.Generator(device='cuda').manual_seed(batch)
    feats = [torch.randn(batch, 256, h, wd, device='cuda', generator=g)
             .contiguous(memory_format=torch.channels_last) for (h, wd) in sizes]
    with torch.no_grad():
        assert w.usable(feats)
        wg.TIMING = []
        try:
            fused = w(feats)
            kinds = [k for (k, _, _, _) in wg.TIMING]
        finally:
            wg.TIMING = None
        assert kinds == ['in'] + ['mid'] * 4 + ['out'] * 2, kinds
        fused = [[t.clone() for t in ts] for ts in fused]
        w.FUSE_MID = False
        try:
            wg.TIMING = []
            two = w(feats)
            kinds = [k for (k, _, _, _) in wg.TIMING]
        finally:
            wg.TIMING = None
            del w.FUSE_MID
        assert kinds == ['in', 'out'] + ['in', 'out'] * 3 + ['in'] + ['out'] * 2, kinds
    torch.cuda.synchronize()
    n = 0
    for a, b in zip(fused, two):
        for u, v in zip(a, b):
            assert u.shape == v.shape and torch.equal(u, v)
            n += 1
    assert n == 15


def test_fcos_head_keeps_the_two_launch_route():
    """GroupNorm sits between the transforms of the FCOS towers: no mid_bias, no fused launch"""
    from iouaware import winograd as wg
    assert wg.WinogradFCOSHead.mid_bias is None

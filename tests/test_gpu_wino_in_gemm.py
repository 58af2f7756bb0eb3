"""GPU (MI355X): ia_wino_in_gemm (csrc/wino.hip k_wino_in_gemm: the input transform of a 64 -> 64
Winograd convolution and its 36 products in one launch, V in LDS) against ia_wino_input_transform
followed by ia_batched_gemm_stream: the same bits (torch.equal), every element of M written and
nothing beside it; and WinogradConv3x3 on the fused route against the two-launch route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096          # floats on either side of M
C64 = 64

EDGES = [
    [(30, 32)],                       # partial tiles in y
    [(32, 27)],                       # ... in x
    [(33, 35)],                       # ... in both
    [(3, 2)], [(1, 1)],               # a level smaller than one tile (T = 3: one group, 13 idle rows)
    [(4, 4)],                         # exact tiles
    [(65, 9)],                        # tall and narrow
    [(65, 9), (2, 67), (5, 5)],       # three levels: T = 216, no multiple of 16, groups span two levels
]


def _inputs(sizes, batch, pre_kind, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    xs = [torch.randn(batch, C64, h, w, device='cuda', generator=g).contiguous(memory_format=torch.channels_last)
          for (h, w) in sizes]
    u = torch.randn(36, C64, C64, device='cuda', generator=g) * 0.1
    pre = None
    if pre_kind == 'full':
        pre = (torch.randn(C64, device='cuda', generator=g), torch.randn(C64, device='cuda', generator=g), True)
    elif pre_kind == 'shift':
        pre = (None, torch.randn(C64, device='cuda', generator=g), False)
    return xs, u, pre


def _both(sizes, batch, pre_kind, seed):
    """-> (M of the two launches, M of the fused launch inside its guard bands, the bands)"""
    from iouaware import winograd as wg, _lib
    from iouaware.ops import _ptr, _stream
    xs, u, pre = _inputs(sizes, batch, pre_kind, seed)
    plan = wg._Plan(sizes, batch, torch.device('cuda'))
    T = plan.T
    v = torch.full((36, T, C64), float('nan'), device='cuda')
    wg.input_transform(plan, xs, 1, v, pre)
    ref = torch.full((36, T, C64), float('nan'), device='cuda')
    # called directly: batched_gemm takes the library below 4096 rows
    _lib.check(_lib.lib().ia_batched_gemm_stream(_ptr(v), _ptr(u), _ptr(ref), 36, T, C64, C64, _stream()),
               'ia_batched_gemm_stream')
    n = ref.numel()
    # the destination starts as NaN (every element must be written), the guard bands as a pattern
    buf = torch.full((n + 2 * GUARD,), float('nan'), device='cuda')
    buf[:GUARD] = 12345.0
    buf[GUARD + n:] = 12345.0
    got = buf[GUARD:GUARD + n].view_as(ref)
    assert got.data_ptr() % 16 == 0
    wg.input_transform_gemm(plan, xs, wg.pack_u_fragments(u), got, pre)
    torch.cuda.synchronize()
    return ref, got, (buf[:GUARD], buf[GUARD + n:])


def _check(sizes, batch, pre_kind, seed):
    ref, got, bands = _both(sizes, batch, pre_kind, seed)
    assert not bool(torch.isnan(ref).any())
    assert not bool(torch.isnan(got).any()), 'elements of M left unwritten'
    assert torch.equal(got, ref), 'differs in %d of %d elements' % (int((got != ref).sum()), ref.numel())
    for band in bands:
        assert bool((band == 12345.0).all()), 'written outside M'


@pytest.mark.parametrize('sizes', EDGES)
@pytest.mark.parametrize('pre_kind', ['full', 'shift', 'none'])
def test_edges_levels_preactivation(sizes, pre_kind):
    _check(sizes, 3, pre_kind, seed=len(sizes) + sizes[0][0])


def test_pack_u_fragments_layout():
    """packed[k][nb][j][16 q + p][c] = u[k][16 j + 4 q + c][16 nb + p], on distinct integers"""
    from iouaware import winograd as wg
    u = torch.arange(2 * 64 * 64, dtype=torch.float32, device='cuda').view(2, 64, 64)
    pk = wg.pack_u_fragments(u)
    assert pk.shape == (2, 4, 4, 64, 4) and pk.is_contiguous()
    for (k, nb, j, q, p, c) in [(0, 0, 0, 0, 0, 0), (1, 3, 2, 1, 7, 3), (0, 1, 3, 3, 15, 2), (1, 2, 0, 2, 9, 1)]:
        assert float(pk[k, nb, j, 16 * q + p, c]) == float(u[k, 16 * j + 4 * q + c, 16 * nb + p])


def test_rejects_other_channel_counts():
    from iouaware import winograd as wg, _lib
    plan = wg._Plan([(8, 8)], 1, torch.device('cuda'))
    x = torch.zeros(1, 128, 8, 8, device='cuda').contiguous(memory_format=torch.channels_last)
    u = wg.pack_u_fragments(torch.zeros(36, 128, 128, device='cuda'))
    with pytest.raises(_lib.IouAwareLibraryError):
        wg.input_transform_gemm(plan, [x], u, torch.zeros(36, plan.T, 128, device='cuda'))


def test_conv_takes_the_fused_route_with_the_same_bits(monkeypatch):
    """WinogradConv3x3(64 -> 64, bias, ReLU) on (1, 64, 200, 336), T = 4200 >= 4096: FUSE_IN_GEMM on and off
    give equal outputs, and on means ia_wino_in_gemm instead of the transform + streaming products"""
    from iouaware import winograd as wg
    g = torch.Generator(device='cuda').manual_seed(21)
    wt = torch.randn(64, 64, 3, 3, device='cuda', generator=g) * (2.0 / (9 * 64)) ** 0.5
    bias = torch.randn(64, device='cuda', generator=g)
    x = torch.randn(1, 64, 200, 336, device='cuda', generator=g).contiguous(memory_format=torch.channels_last)
    pre = (torch.rand(64, device='cuda', generator=g) + 0.5, torch.randn(64, device='cuda', generator=g), True)
    layer = wg.WinogradConv3x3(wt, bias, relu=True)
    assert wg.FUSE_IN_GEMM and layer.u_packed is not None
    calls = []
    real_fused, real_in, real_bmm = wg.input_transform_gemm, wg.input_transform, wg.batched_gemm
    monkeypatch.setattr(wg, 'input_transform_gemm', lambda *a, **k: (calls.append('fused'), real_fused(*a, **k))[1])
    monkeypatch.setattr(wg, 'input_transform', lambda *a, **k: (calls.append('in'), real_in(*a, **k))[1])
    monkeypatch.setattr(wg, 'batched_gemm', lambda *a, **k: (calls.append('bmm'), real_bmm(*a, **k))[1])
    with torch.no_grad():
        assert layer.usable(x)
        on = [layer(x).clone(), layer(x, pre).clone()]
        assert calls == ['fused', 'fused'], calls
        del calls[:]
        monkeypatch.setattr(wg, 'FUSE_IN_GEMM', False)
        off = [layer(x), layer(x, pre)]
        assert calls == ['in', 'bmm', 'in', 'bmm'], calls
        # below 4096 tiles the library route stays, fused flag or not
        monkeypatch.setattr(wg, 'FUSE_IN_GEMM', True)
        del calls[:]
        layer(x[:, :, :64, :64].contiguous(memory_format=torch.channels_last))
        assert calls == ['in', 'bmm'], calls
    torch.cuda.synchronize()
    for a, b in zip(on, off):
        assert not bool(torch.isnan(a).any())
        assert torch.equal(a, b), 'differs in %d elements' % int((a != b).sum())

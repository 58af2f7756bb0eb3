"""GPU (MI355X): ia_wino_conv3x3_c64 (csrc/wino.hip k_wino_conv: input transform, the 36 products and the
output transform of a 64 -> 64 Winograd convolution in one launch, V in LDS, M in registers) against the
two launches it replaces, ia_wino_in_gemm into M followed by ia_wino_output_transform: the same bits
(torch.equal), every pixel of y written and nothing beside it; and the route through WinogradConv3x3 and
through a fused ResNet-50 stage 1."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096          # floats on either side of y
BAND = 12345.0
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

_CASES = {}


def _inputs(sizes, batch, pre_kind, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    xs = [torch.randn(batch, C64, h, w, device='cuda', generator=g).contiguous(memory_format=torch.channels_last)
          for (h, w) in sizes]
    u = torch.randn(36, C64, C64, device='cuda', generator=g) * 0.1
    bias = torch.randn(C64, device='cuda', generator=g)
    pre = None
    if pre_kind == 'full':
        pre = (torch.randn(C64, device='cuda', generator=g), torch.randn(C64, device='cuda', generator=g), True)
    elif pre_kind == 'shift':
        pre = (None, torch.randn(C64, device='cuda', generator=g), False)
    return xs, u, bias, pre


def _levels(sizes, batch, fill):
    """every level's y (B, 64, H, W) channels-last as a view into ONE flat buffer filled with `fill`,
    between guard bands -> (buffer, views)"""
    n = sum(batch * h * w * C64 for (h, w) in sizes)
    buf = torch.full((n + 2 * GUARD,), fill, device='cuda')
    buf[:GUARD] = BAND
    buf[GUARD + n:] = BAND
    ys, off = [], GUARD
    for (h, w) in sizes:
        k = batch * h * w * C64
        ys.append(buf[off:off + k].view(batch, h, w, C64).permute(0, 3, 1, 2))
        assert ys[-1].data_ptr() % 16 == 0
        off += k
    return buf, ys


def _case(sizes, batch, pre_kind):
    """inputs and the M of ia_wino_in_gemm, once per (sizes, pre_kind): shared by the bias / relu cases"""
    from iouaware import winograd as wg
    key = (tuple(sizes), batch, pre_kind)
    if key not in _CASES:
        xs, u, bias, pre = _inputs(sizes, batch, pre_kind, seed=len(sizes) + sizes[0][0])
        plan = wg._Plan(sizes, batch, torch.device('cuda'))
        up = wg.pack_u_fragments(u)
        m = torch.full((36, plan.T, C64), float('nan'), device='cuda')
        wg.input_transform_gemm(plan, xs, up, m, pre)
        torch.cuda.synchronize()
        _CASES[key] = (xs, up, bias, pre, plan, m)
    return _CASES[key]


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('pre_kind', ['full', 'shift', 'none'])
@pytest.mark.parametrize('sizes', EDGES)
def test_edges_levels_preactivation_bias_relu(sizes, pre_kind, with_bias, relu):
    from iouaware import winograd as wg
    batch = 3
    xs, up, bias, pre, plan, m = _case(sizes, batch, pre_kind)
    b = bias if with_bias else None
    n = sum(batch * h * w * C64 for (h, w) in sizes)
    # the yardstick: the two launches, also into NaN-filled tensors
    rbuf, ref = _levels(sizes, batch, float('nan'))
    wg.output_transform(plan, m, C64, 1, b, relu, [(0, C64, ref, 0)])
    buf, got = _levels(sizes, batch, float('nan'))
    wg.input_transform_gemm(plan, xs, up, None, pre, epilogue=(b, relu, got))
    torch.cuda.synchronize()
    r, g = rbuf[GUARD:GUARD + n], buf[GUARD:GUARD + n]
    assert not bool(torch.isnan(r).any()), 'the two-launch reference left pixels unwritten'
    assert not bool(torch.isnan(g).any()), 'pixels of y left unwritten'
    assert torch.equal(g, r), 'differs in %d of %d elements' % (int((g != r).sum()), n)
    for band in (buf[:GUARD], buf[GUARD + n:]):
        assert bool((band == BAND).all()), 'written outside y'


def _direct(plan, x, channels, up, y):
    from iouaware import _lib
    from iouaware.ops import _ptr, _stream
    xp = (C.c_void_p * 1)(x.data_ptr())
    yp = (C.c_void_p * 1)(y)
    _lib.check(_lib.lib().ia_wino_conv3x3_c64(C.byref(plan.geom), xp, channels, None, None, 0, _ptr(up), None, 0,
                                              yp, _stream()), 'ia_wino_conv3x3_c64')


def test_rejections():
    """128 channels, a y that is not 16-byte aligned, no packed weights"""
    from iouaware import winograd as wg, _lib
    plan = wg._Plan([(8, 8)], 1, torch.device('cuda'))
    x = torch.zeros(1, C64, 8, 8, device='cuda').contiguous(memory_format=torch.channels_last)
    up = wg.pack_u_fragments(torch.zeros(36, C64, C64, device='cuda'))
    ybuf = torch.zeros(8 * 8 * C64 + 4, device='cuda')
    _direct(plan, x, C64, up, ybuf.data_ptr())            # the well-formed call passes
    with pytest.raises(_lib.IouAwareLibraryError):
        _direct(plan, x, C64, up, ybuf.data_ptr() + 4)
    with pytest.raises(_lib.IouAwareLibraryError):
        _direct(plan, x, C64, None, ybuf.data_ptr())
    x128 = torch.zeros(1, 128, 8, 8, device='cuda').contiguous(memory_format=torch.channels_last)
    up128 = wg.pack_u_fragments(torch.zeros(36, 128, 128, device='cuda'))
    y128 = torch.zeros(8 * 8 * 128, device='cuda')
    with pytest.raises(_lib.IouAwareLibraryError):
        _direct(plan, x128, 128, up128, y128.data_ptr())
    with pytest.raises(_lib.IouAwareLibraryError):
        wg.input_transform_gemm(plan, [x128], up128, None, epilogue=(None, False, [y128.view(1, 8, 8, 128).permute(0, 3, 1, 2)]))
    torch.cuda.synchronize()


def test_conv_takes_the_one_launch_route_with_the_same_bits(monkeypatch):
    """WinogradConv3x3(64 -> 64, bias, ReLU) on (1, 64, 200, 336), T = 4200 >= 4096: FUSE_OUT on and off give
    equal outputs; on means one call of input_transform_gemm and no output_transform; below 4096 tiles the
    library route stays"""
    from iouaware import winograd as wg
    g = torch.Generator(device='cuda').manual_seed(22)
    wt = torch.randn(64, 64, 3, 3, device='cuda', generator=g) * (2.0 / (9 * 64)) ** 0.5
    bias = torch.randn(64, device='cuda', generator=g)
    x = torch.randn(1, 64, 200, 336, device='cuda', generator=g).contiguous(memory_format=torch.channels_last)
    pre = (torch.rand(64, device='cuda', generator=g) + 0.5, torch.randn(64, device='cuda', generator=g), True)
    layer = wg.WinogradConv3x3(wt, bias, relu=True)
    assert wg.FUSE_IN_GEMM and layer.u_packed is not None
    calls = []

    def spy(name):
        real = getattr(wg, name)
        monkeypatch.setattr(wg, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])
    for name in ('input_transform_gemm', 'input_transform', 'batched_gemm', 'output_transform'):
        spy(name)
    with torch.no_grad():
        assert layer.usable(x)
        monkeypatch.setattr(wg, 'FUSE_OUT', True)
        on = [layer(x).clone(), layer(x, pre).clone()]
        assert calls == ['input_transform_gemm'] * 2, calls
        del calls[:]
        monkeypatch.setattr(wg, 'FUSE_OUT', False)
        off = [layer(x), layer(x, pre)]
        assert calls == ['input_transform_gemm', 'output_transform'] * 2, calls
        monkeypatch.setattr(wg, 'FUSE_OUT', True)
        del calls[:]
        layer(x[:, :, :64, :64].contiguous(memory_format=torch.channels_last))
        assert calls == ['input_transform', 'batched_gemm', 'output_transform'], calls
    torch.cuda.synchronize()
    for a, b in zip(on, off):
        assert not bool(torch.isnan(a).any())
        assert torch.equal(a, b), 'differs in %d elements' % int((a != b).sum())


def test_stage1_one_launch_equals_two(monkeypatch):
    """a fused ResNet-50 at batch 1 of 800 x 1344 (stage 1: 200 x 336, T = 4200): the three 3x3 convolutions of
    stage 1 take the one-launch form, and FUSE_OUT on and off give the same stage outputs"""
    from iouaware import winograd as wg
    from iouaware.backbones import ResNet
    from iouaware.fuse import fuse_inference
    torch.manual_seed(5)
    net = ResNet(depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1, style='pytorch').cuda().eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.1)
    fuse_inference(net, winograd=True)
    x = torch.randn(1, 3, 800, 1344, device='cuda').contiguous(memory_format=torch.channels_last)
    calls = []
    real = wg.input_transform_gemm
    monkeypatch.setattr(wg, 'input_transform_gemm',
                        lambda *a, **k: (calls.append(k.get('epilogue') is not None), real(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setattr(wg, 'FUSE_OUT', True)
        a = net(x)
        assert calls == [True] * 3, calls
        del calls[:]
        monkeypatch.setattr(wg, 'FUSE_OUT', False)
        b = net(x)
        assert calls == [False] * 3, calls
    torch.cuda.synchronize()
    assert tuple(a[0].shape) == (1, 256, 200, 336)
    for u, v in zip(a, b):
        assert not bool(torch.isnan(u).any())
        assert torch.equal(u, v)

"""GPU (MI355X): ia_batched_gemm_split3 (csrc/wino_split_gemm.hip: D[b] = V[b] . U[b] on bf16 MFMA through
the exact three-way split x = h + m + l of both fp32 operands, six of the nine product terms) against fp64,
with the library's fp32 batched GEMM on the same operands as the comparator (tests/wino_ref.py gate A and
gate B); every element written and nothing beside it; NaN / Inf only where an operand carries one; the
same bits in every run; and the whole WinogradHead on the split route against the library route.
The CPU side of the numerics (the split is exact, the six-term scheme passes both gates, a two-piece
split fails gate B) is tests/test_host_split_gemm.py."""
import importlib.util
import os

import pytest
import torch

import wino_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GUARD = 4096          # floats on either side of D
K = 256
ROWS = (1, 17, 129)   # 129: one past the kernel's 128-row tile


def _split_gemm(v, u3, out, n):
    from iouaware import _lib
    from iouaware.ops import _ptr, _stream
    b, rows, k = v.shape
    _lib.check(_lib.lib().ia_batched_gemm_split3(_ptr(v), _ptr(u3), _ptr(out), b, rows, k, n, _stream()),
               'ia_batched_gemm_split3')
    return out


def _library(v, u):
    from iouaware import winograd as wg
    out = torch.empty(v.shape[0], v.shape[1], u.shape[2], device='cuda')
    return wg.batched_gemm(v, u, out)           # no u3: the library's fp32 GEMM


def _operands(batch, rows, n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    v = torch.randn(batch, rows, K, device='cuda', generator=g)
    u = torch.randn(batch, K, n, device='cuda', generator=g) * 0.05
    return v, u


def _guarded(batch, rows, n):
    """D inside guard bands: D NaN (every element must be written), the bands a pattern"""
    cnt = batch * rows * n
    buf = torch.full((cnt + 2 * GUARD,), float('nan'), device='cuda')
    buf[:GUARD] = 12345.0
    buf[GUARD + cnt:] = 12345.0
    return buf, buf[GUARD:GUARD + cnt].view(batch, rows, n)


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [2, 72])
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('n', [48, 256, 512, 720])
def test_split_gemm_within_the_gates_every_element_written(n, rows, batch):
    from iouaware import winograd as wg
    v, u = _operands(batch, rows, n, seed=n + rows + batch)
    u3 = wg.split3_pack_u(u)
    buf, d = _guarded(batch, rows, n)
    _split_gemm(v, u3, d, n)
    lib = _library(v, u)
    torch.cuda.synchronize()
    assert torch.all(buf[:GUARD] == 12345.0) and torch.all(buf[GUARD + d.numel():] == 12345.0)
    assert bool(torch.isfinite(d).all()), 'elements left unwritten (NaN) or not finite'
    ref = torch.bmm(v.double(), u.double())
    e, h, ratio = R.gates(d, lib, ref)
    print('split3 n=%d rows=%d batch=%d: error %.3e, library %.3e, ratio %.2f' % (n, rows, batch, e, h, ratio))
    assert e <= R.GATE_A, e
    assert ratio <= R.GATE_B, (e, h, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [256, 720])
def test_non_finite_operands_reach_exactly_the_affected_entries(n):
    from iouaware import winograd as wg
    batch, rows = 3, 129
    v, u = _operands(batch, rows, n, seed=7)
    v[0, 5, 17] = float('nan')
    v[2, 128, 200] = float('inf')
    u[1, 31, n - 1] = float('nan')
    u[2, 0, 100] = float('-inf')
    d = _split_gemm(v, wg.split3_pack_u(u), torch.empty(batch, rows, n, device='cuda'), n)
    want = torch.zeros(batch, rows, n, dtype=torch.bool, device='cuda')
    want[0, 5, :] = True
    want[2, 128, :] = True
    want[1, :, n - 1] = True
    want[2, :, 100] = True
    assert torch.equal(~torch.isfinite(d), want)
    # the library on the same operands marks the same entries
    assert torch.equal(~torch.isfinite(_library(v, u)), want)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    from iouaware import winograd as wg
    v, u = _operands(72, 300, 256, seed=11)
    u3 = wg.split3_pack_u(u)
    a = _split_gemm(v, u3, torch.empty(72, 300, 256, device='cuda'), 256)
    b = _split_gemm(v, u3, torch.empty(72, 300, 256, device='cuda'), 256)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    from iouaware import _lib, winograd as wg
    v, u = _operands(2, 17, 720, seed=1)
    u3 = wg.split3_pack_u(u)
    out = torch.empty(2, 17, 720, device='cuda')
    from iouaware.ops import _ptr, _stream
    L = _lib.lib()
    assert L.ia_batched_gemm_split3(_ptr(v), _ptr(u3), _ptr(out), 2, 17, 48, 720, _stream()) != 0    # k % 32
    assert L.ia_batched_gemm_split3(_ptr(v), None, _ptr(out), 2, 17, 256, 720, _stream()) != 0
    assert L.ia_batched_gemm_split3(_ptr(v), _ptr(u3), _ptr(out), 2, 0, 256, 720, _stream()) != 0
    assert (256, 720) in wg._SPLIT_SHAPES                                # the route the check below is on
    with pytest.raises(ValueError):
        wg.batched_gemm(v, u, out, u3[:1].contiguous())                # not the split of this U


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


@pytest.mark.gpu
def test_whole_head_split_route_against_the_library_route():
    """WinogradHead at batch 2 on the 224 x 288 pyramid: all 15 outputs of the split route within gate A of
    the library route (SPLIT_GEMM = False), and the split route is the one the head takes"""
    from iouaware import winograd as wg
    w = _head(5)._ia_wino
    assert isinstance(w, wg.WinogradHead)
    # layer 0, three tower layers, retina_cls: those in _SPLIT_SHAPES carry a split U (retina_cls at least)
    routed = [u is not None for u in [w.u0_3] + list(w.u_3) + [w.u_cls3]]
    assert routed[-1] and routed == [wg.split_shape(u) for u in [w.u0] + list(w.u) + [w.u_cls]]
    sizes = [(28, 36), (14, 18), (7, 9), (4, 5), (2, 3)]               # a 224 x 288 image
    g = torch.Generator(device='cuda').manual_seed(2)
    feats = [torch.randn(2, 256, h, wd, device='cuda', generator=g)
             .contiguous(memory_format=torch.channels_last) for (h, wd) in sizes]
    calls = []
    real = wg._lib.lib().ia_batched_gemm_split3

    def counting(*a):
        calls.append(a[5:7])
        return real(*a)
    with torch.no_grad():
        assert wg.SPLIT_GEMM and w.usable(feats)
        L = wg._lib.lib()
        L.ia_batched_gemm_split3 = counting
        try:
            split = [[t.clone() for t in ts] for ts in w(feats)]
        finally:
            L.ia_batched_gemm_split3 = real
        wg.SPLIT_GEMM = False
        try:
            lib = w(feats)
        finally:
            wg.SPLIT_GEMM = True
    torch.cuda.synchronize()
    assert len(calls) == sum(routed), calls
    worst = 0.0
    for a, b in zip(split, lib):
        for x, y in zip(a, b):
            assert x.shape == y.shape
            e = R.rel_err(x, y)
            worst = max(worst, e)
            assert e <= R.GATE_A, e
    print('whole head, split against library route: worst %.3e of the maximum' % worst)


def test_split_gemm_kernel_does_not_spill():
    """CPU: the kernel's code object: no VGPR spill, no scratch"""
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    import __graft_entry__ as g
    g.build()
    if not os.path.exists(os.path.join(t.LLVM, 'llvm-readelf')):
        pytest.skip('no llvm-readelf in this image')
    rows = [r for r in t.kernels() if 'k_gemm_split3' in r['name']]
    assert len(rows) == 1, [r['name'] for r in rows]
    assert rows[0]['vgpr_spill'] == 0 and rows[0]['scratch'] == 0, rows[0]

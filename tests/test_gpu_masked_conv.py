"""GPU: the masked convolution (csrc/masked_conv.hip, iouaware/masked_conv.py) against
F.conv2d in fp64 (tests/ga_ref.masked_conv2d).

Gates, those of tests/test_gpu_deform_conv.py: as max|got - ref| / max|ref| against the fp64
evaluation of the same fp32 tensors,
    gate A  <= 1e-4, and
    gate B  <= 4 x the same figure of a plain fp32 evaluation on the CPU -- the largest over ORDERS
            evaluations that differ only in the order of the input channels, i.e. of their sums (the
            reasoning stands next to dcn_ref.GATE_B: one order's figure is luck at these sizes).
Where the mask is false the output is +0.0f to the bit.

Cases: maps 7 x 11 and 13 x 21 (odd, smaller and larger than a wavefront, 2 compaction workgroups
at batch 2), C = 16 and 256, n = 80 / 4 / 1 (the widths of the three layers: a padded GEMM width
each), 1x1 and 3x3 kernels; masks: all false (no GEMM), all true (the dense convolution), one kept
pixel in a corner per image (batch 4, a corner each: every border tap), 37 scattered pixels, batch
2 with an empty image.  The output, the GEMM result and the column buffer are handed over full of
NaN; NaN is planted in every input pixel that no kept receptive field touches and the result must
be finite; two runs give equal bits.
"""
import numpy as np
import pytest
import torch

import dcn_ref as R
import ga_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
ORDERS = 4
MASKS = ('none', 'all', 'corners', 'scattered', 'batch2_empty')


def _mask(kind, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    scattered = torch.zeros(H * W, dtype=torch.bool)
    scattered[torch.randperm(H * W, generator=g)[:37]] = True
    scattered = scattered.view(H, W)
    if kind == 'none':
        return torch.zeros(1, H, W, dtype=torch.bool)
    if kind == 'all':
        return torch.ones(1, H, W, dtype=torch.bool)
    if kind == 'corners':
        m = torch.zeros(4, H, W, dtype=torch.bool)
        for b, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            m[b, y, x] = True
        return m
    if kind == 'scattered':
        return scattered[None].clone()
    return torch.stack([scattered, torch.zeros(H, W, dtype=torch.bool)])


def _data(H, W, Cc, ks, kind):
    seed = 7 * H + 3 * Cc + ks + 11 * MASKS.index(kind)
    mask = _mask(kind, H, W, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(mask.shape[0], Cc, H, W, generator=g)
    # the input pixels some kept receptive field touches
    touched = mask.clone()
    if ks == 3:
        touched = torch.nn.functional.max_pool2d(mask[:, None].float(), 3, 1, 1)[:, 0] > 0
    ws = {n: (torch.randn(n, Cc, ks, ks, generator=g) / np.sqrt(Cc * ks * ks), torch.randn(n, generator=g))
          for n in (80, 4, 1)}
    return mask, x, touched, ws


def _fp32_figure(x, mask, w, b, pad, ref):
    """the largest rel_err over ORDERS plain fp32 CPU evaluations with permuted input channels"""
    figs = []
    for o in range(ORDERS):
        perm = torch.arange(x.shape[1]) if o == 0 else torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(o))
        figs.append(R.rel_err(ga_ref.masked_conv2d(x[:, perm], mask, w[:, perm], b, pad, torch.float32), ref))
    return max(figs)


def _run(x_dev, comp, packed, ks, n, shape):
    """the operator with its output, GEMM result and column buffer full of NaN"""
    from iouaware import masked_conv, ops
    B, H, W = shape
    out = torch.full((B, n, H, W), NAN, device=DEV).contiguous(memory_format=torch.channels_last)
    rows_pad = max(1, (comp.n + masked_conv.ROW_GRANULE - 1) // masked_conv.ROW_GRANULE) * masked_conv.ROW_GRANULE
    y = torch.full((rows_pad, packed[0].shape[1]), NAN, device=DEV)
    k = int(packed[0].shape[0])
    ops._col_buffer(x_dev.device, rows_pad * k * 4)[:rows_pad * k * 4].view(torch.float32).fill_(NAN)
    got = masked_conv.masked_conv_packed(x_dev, comp, packed, ks, y_out=y, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got


@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('ks', [1, 3])
@pytest.mark.parametrize('Cc', [16, 256])
@pytest.mark.parametrize('H,W', [(7, 11), (13, 21)])
def test_masked_conv_against_fp64(H, W, Cc, ks, kind):
    from iouaware import masked_conv
    mask, x, touched, ws = _data(H, W, Cc, ks, kind)
    B, pad = mask.shape[0], (ks - 1) // 2
    x_nan = x.clone()
    x_nan.permute(0, 2, 3, 1)[~touched] = NAN
    # (37 scattered pixels of a 7 x 11 map touch all of it with a 3x3 kernel: nothing to plant there)
    assert kind in ('all', 'scattered') or bool(torch.isnan(x_nan).any())
    x_dev = x_nan.to(DEV).contiguous(memory_format=torch.channels_last)
    comp = masked_conv.compact_mask(mask.to(DEV))
    assert comp.n == int(mask.sum())
    for n, (w, b) in ws.items():
        packed = masked_conv.pack_weight(w.to(DEV), b.to(DEV))
        got = _run(x_dev, comp, packed, ks, n, (B, H, W))
        again = _run(x_dev, comp, packed, ks, n, (B, H, W))
        torch.cuda.synchronize()
        assert got.shape == (B, n, H, W) and got.is_contiguous(memory_format=torch.channels_last)
        g = got.cpu()
        assert bool(torch.isfinite(g).all()), (n, 'NaN / inf in the result')
        assert torch.equal(g.view(torch.int32), again.cpu().view(torch.int32)), 'two runs differ'
        # +0.0f to the bit where the mask is false
        off = g.permute(0, 2, 3, 1)[~mask]
        assert bool((off.contiguous().view(torch.int32) == 0).all())
        if comp.n == 0:
            continue
        ref = ga_ref.masked_conv2d(x, mask, w, b, pad, torch.float64)
        e = R.rel_err(g, ref)
        h = _fp32_figure(x, mask, w, b, pad, ref)
        print('  %dx%d C%d k%d %-12s n%-2d  %.2e (%.2f x the fp32 figure %.2e)' % (H, W, Cc, ks, kind, n, e, e / h, h))
        assert h > 0
        assert e <= R.GATE_A, 'gate A: %.3e' % e
        assert e <= R.GATE_B * h, 'gate B: HIP %.3e vs fp32 %.3e = %.2f x' % (e, h, e / h)


def test_public_op_layouts_and_mask_forms():
    """masked_conv2d / MaskedConv2d: an NCHW input gives an NCHW output, a channels-last one a
    channels-last output, the (1, H, W) mask of the reference and the per-image (B, H, W) form; a
    column cap of one granule of rows (the chunked path) passes the same gate"""
    from iouaware import MaskedConv2d, masked_conv2d
    H, W, Cc = 13, 21, 16
    mask, x, _, ws = _data(H, W, Cc, 3, 'scattered')
    w, b = ws[4]
    ref = ga_ref.masked_conv2d(x, mask, w, b, 1, torch.float64)
    y = masked_conv2d(x.to(DEV), mask.to(DEV), w.to(DEV), b.to(DEV), padding=1)
    assert y.is_contiguous() and R.rel_err(y, ref) <= R.GATE_A
    ycl = masked_conv2d(x.to(DEV).contiguous(memory_format=torch.channels_last), mask.to(DEV), w.to(DEV), None,
                        padding=1)
    assert ycl.is_contiguous(memory_format=torch.channels_last)
    assert R.rel_err(ycl, ga_ref.masked_conv2d(x, mask, w, None, 1, torch.float64)) <= R.GATE_A
    m = MaskedConv2d(Cc, 4, 3, padding=1).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        assert torch.equal(m(x.to(DEV), mask.to(DEV)), y)
        dense = m(x.to(DEV))
    assert R.rel_err(dense, torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1)) <= R.GATE_A
    # batch 8, all kept: 2184 rows = 3 granules; a column cap of one granule of rows -> three chunks
    xb = torch.randn(8, Cc, H, W, generator=torch.Generator().manual_seed(5))
    mb = torch.ones(8, H, W, dtype=torch.bool)
    one = masked_conv2d(xb.to(DEV), mb.to(DEV), w.to(DEV), b.to(DEV), padding=1)
    chunked = masked_conv2d(xb.to(DEV), mb.to(DEV), w.to(DEV), b.to(DEV), padding=1, col_cap=1024 * 9 * Cc * 4)
    refb = torch.nn.functional.conv2d(xb.double(), w.double(), b.double(), padding=1)
    assert R.rel_err(chunked, refb) <= R.GATE_A          # (another GEMM shape: maybe another library kernel)
    assert R.rel_err(one, torch.nn.functional.conv2d(xb.double(), w.double(), b.double(), padding=1)) <= R.GATE_A


@pytest.mark.parametrize('shape,frac', [((1, 7, 11), 0.5), ((2, 13, 21), 0.1), ((5, 120, 130), 0.3),
                                        ((1, 100, 168), 0.01)])
def test_compaction(shape, frac):
    """idx = the ascending kept flat indices, rank = row or -1, count; more workgroups than one scan
    round holds ((5, 120, 130): 305); the same bits in two runs"""
    from iouaware import masked_conv
    g = torch.Generator().manual_seed(shape[1])
    mask = torch.rand(shape, generator=g) < frac
    want = torch.nonzero(mask.reshape(-1))[:, 0].to(torch.int32)
    rank = torch.full((mask.numel(),), -1, dtype=torch.int32)
    rank[want.long()] = torch.arange(len(want), dtype=torch.int32)
    for _ in range(2):
        c = masked_conv.compact_mask(mask.to(DEV))
        assert c.n == len(want)
        assert torch.equal(c.idx[:c.n].cpu(), want)
        assert torch.equal(c.rank.cpu().reshape(-1), rank)
    # a uint8 mask and a caller's count slot
    counts = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    c = masked_conv.compact_mask(mask.to(torch.uint8).to(DEV) * 7, counts[1:2])
    assert counts.tolist() == [-5, len(want), -5] and torch.equal(c.idx[:len(want)].cpu(), want)


@pytest.mark.parametrize('shape', [(1, 7, 11), (2, 13, 21), (5, 120, 130)])
def test_logit_compaction(shape):
    """compact_logits = compact_mask of (the library's sigmoid >= thr), the keep decision of the
    guided decode: logits spread around the threshold's logit, some exactly on it, NaN never kept"""
    from iouaware import masked_conv, ops
    g = torch.Generator().manual_seed(shape[2])
    thr = 0.01
    x = torch.randn(shape, generator=g) * 2 + float(np.log(thr / (1 - thr)))
    x.view(-1)[::7] = float(np.log(thr / (1 - thr)))
    x.view(-1)[3::11] = NAN
    xd = x.to(DEV)
    want = masked_conv.compact_mask(ops.test_math(2, xd) >= thr)
    got = masked_conv.compact_logits(xd, thr)
    assert 0 < got.n == want.n < x.numel()
    assert torch.equal(got.idx[:got.n], want.idx[:want.n]) and torch.equal(got.rank, want.rank)
    assert not bool(torch.isnan(x.view(-1)[got.idx[:got.n].cpu().long()]).any())


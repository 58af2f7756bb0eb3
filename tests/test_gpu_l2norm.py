"""-m gpu: the L2Norm kernel (csrc/l2norm.hip, ia_l2norm_nchw) against the reference expression
weight[c] * x / (sqrt(sum_c x^2) + eps) evaluated in fp64 on the same fp32 inputs.

Gate (both must hold): absolute error <= 1e-4 * max|y|, and <= 4 x the error of torch's own fp32
evaluation of the expression on the CPU.  |x| <= 1e4 throughout; the cases with more than one pixel and
more than one channel carry a pixel whose channels are all zero (its own test below)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-10
GUARD = 4096                                  # floats in front of and behind the output
# (B, C, H, W): conv4_3 of SSD300 at batch 2; one pixel; a pixel count that is no multiple of 64
SHAPES = [(2, 512, 38, 38), (1, 4, 1, 1), (1, 512, 5, 7), (3, 1, 9, 9)]


def _inputs(shape, seed):
    rng = np.random.RandomState(seed)
    B, Cn, H, W = shape
    x = rng.randn(*shape) * 10.0 ** rng.uniform(-2, 3.5, size=(B, 1, H, W))      # magnitudes differ per pixel
    x = np.clip(x, -1e4, 1e4).astype(np.float32)
    if H * W > 1:
        x[0, :, H // 2, W // 3] = 0.0                                             # an all-zero pixel
        x[-1, :, 0, 0] = 1e4                                                      # the largest allowed values
    w = (20.0 + rng.uniform(-5, 5, size=Cn)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(w)


def _expr(x, w, eps=EPS):
    norm = x.pow(2).sum(1, keepdim=True).sqrt() + eps
    return w[None, :, None, None].expand_as(x) * x / norm


def _run(x, w, eps=EPS):
    """the kernel into a NaN-filled buffer with guards -> (y on the host, guards intact)"""
    from iouaware import ssd_ops
    xd, wd = x.cuda(), w.cuda()
    buf = torch.full((2 * GUARD + x.numel(),), float('nan'), device='cuda')
    y = buf[GUARD:GUARD + x.numel()].view(x.shape)
    ssd_ops.l2norm_into(xd, wd, eps, y)
    torch.cuda.synchronize()
    host = buf.cpu()
    guards = bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[-GUARD:]).all())
    return host[GUARD:GUARD + x.numel()].view(x.shape).clone(), guards


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_l2norm_against_fp64(shape):
    x, w = _inputs(shape, 11 + shape[1] + shape[2])
    assert float(x.abs().max()) <= 1e4
    want = _expr(x.double(), w.double())
    y, guards = _run(x, w)
    assert guards, 'wrote outside the output'
    assert not bool(torch.isnan(y).any())
    err = float((y.double() - want).abs().max())
    err_torch = float((_expr(x, w).double() - want).abs().max())
    ymax = float(want.abs().max())
    print('l2norm %s: error %.3e, torch fp32 on the CPU %.3e, max|y| %.3e' % (shape, err, err_torch, ymax))
    assert err <= 1e-4 * ymax
    assert err <= 4 * err_torch


def test_all_zero_pixel_gives_zero_not_nan():
    x, w = _inputs((1, 512, 5, 7), 5)
    y, _ = _run(x, w)
    assert float(x[0, :, 2, 2].abs().max()) == 0
    assert bool((y[0, :, 2, 2] == 0).all())
    y0, _ = _run(torch.zeros(2, 8, 3, 3), torch.ones(8))
    assert bool((y0 == 0).all())


def test_two_runs_give_the_same_bits():
    x, w = _inputs(SHAPES[0], 7)
    a, _ = _run(x, w)
    b, _ = _run(x, w)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_in_place_and_bad_arguments_are_refused():
    from iouaware import _lib, ssd_ops
    x = torch.randn(1, 8, 4, 4, device='cuda')
    w = torch.ones(8, device='cuda')
    keep = x.clone()
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    assert L.ia_l2norm_nchw(p(x), p(w), EPS, 1, 8, 4, 4, p(x), None) == -1            # IA_E_ARG
    assert L.ia_l2norm_nchw(p(x), p(w), EPS, 1, 0, 4, 4, p(keep), None) == -1
    assert L.ia_l2norm_nchw(p(x), p(w), EPS, 0, 8, 4, 4, p(keep), None) == -1
    assert L.ia_l2norm_nchw(p(x), None, EPS, 1, 8, 4, 4, p(keep), None) == -1
    with pytest.raises(_lib.IouAwareLibraryError, match='argument'):
        ssd_ops.l2norm_into(x, w, EPS, x)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


def test_module_eval_route_is_the_kernel_and_training_route_the_expression():
    from iouaware.ssd_vgg import L2Norm
    x, w = _inputs((1, 512, 5, 7), 9)
    m = L2Norm(512).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
    y, _ = _run(x, w)
    with torch.no_grad():
        assert torch.equal(m.eval()(x.cuda()).cpu(), y)
        # channels-last input: converted, same values
        assert torch.equal(m(x.cuda().contiguous(memory_format=torch.channels_last)).cpu(), y)
        t = m.train()(x.cuda()).cpu()
    assert float((t - y).abs().max()) <= 1e-4 * float(y.abs().max())

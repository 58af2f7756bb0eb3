"""bf16 3x3 tower convolution (256 -> 256, batch 16, the five pyramid levels of 800x1344): the
library's own MFMA implicit-GEMM kernel (csrc/conv3x3_bf16.hip, bias + ReLU fused) against
MIOpen / CK's convolution + the separate bias + ReLU pass.

    python tools/time_conv3x3_bf16.py [B]
    python tools/time_conv3x3_bf16.py --wgrad [B]    the backward of bf16 training (csrc/conv3x3_bf16_bwd.hip):
        the weight-gradient launch (MFMA kernel + the split-K reduce), the input-gradient launch (the
        forward kernel on the adjoint weight) and the two weight packs, for the tower shape (256 -> 256,
        two groups) and the class output (256 -> 720), all five levels in one launch, batch 4.  Kernel
        times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_conv3x3_bf16.py --wgrad`."""
import os, sys, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
import torch, torch.nn.functional as F
from iouaware import ops
torch.backends.cudnn.benchmark = True
WGRAD = '--wgrad' in sys.argv
ARGS = [a for a in sys.argv[1:] if a != '--wgrad']
B = int(ARGS[0]) if ARGS else (4 if WGRAD else 16)
def bench(fn, n=20):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
if WGRAD:
    BF, CL = torch.bfloat16, torch.channels_last
    PX = B * sum(h * w for h, w in SIZES)
    print('batch %d, %d pixels over %d levels' % (B, PX, len(SIZES)))
    for name, groups, cout in (('tower 256 -> 256, both towers', 2, 256), ('cls output 256 -> 720', 1, 720)):
        P = (cout + 31) // 32 * 32
        acts = [torch.randn(B, groups * 256, h, w, device='cuda').clamp(min=0).to(BF).contiguous(memory_format=CL) for h, w in SIZES]
        gbuf = [(torch.randn(B, groups * P, h, w, device='cuda') * (torch.rand(B, groups * P, h, w, device='cuda') > 0.5))
                .to(BF).contiguous(memory_format=CL) for h, w in SIZES]
        for t in gbuf:
            for k in range(groups):
                t[:, k * P + cout:(k + 1) * P] = 0
        xs = [[a[:, k * 256:(k + 1) * 256] for a in acts] for k in range(groups)]
        gs = [[t[:, k * P:k * P + cout] for t in gbuf] for k in range(groups)]
        gin = [[t[:, k * P:(k + 1) * P] for t in gbuf] for k in range(groups)]
        w = torch.randn(groups * cout, 256, 3, 3, device='cuda') * 0.03
        dxb = [torch.empty_like(a) for a in acts]
        dxs = [[t[:, k * 256:(k + 1) * 256] for t in dxb] for k in range(groups)]
        wt = ops.conv3x3_bf16_pack(w, groups=groups, adjoint=True)
        tiles, st, n = ops.conv3x3_bf16_wgrad_plan(xs, gs, 256, cout)
        fl = 2.0 * groups * PX * 256 * cout * 9
        t_w = bench(lambda: ops.conv3x3_bf16_wgrad_levels(xs, gs, 256, cout))
        t_x = bench(lambda: ops.conv3x3_bf16_levels(gin, wt, None, 256, dxs, cin=P))
        t_p = bench(lambda: ops.conv3x3_bf16_pack(w, groups=groups))
        t_a = bench(lambda: ops.conv3x3_bf16_pack(w, groups=groups, adjoint=True))
        print('%-30s %d tiles, %d slices of %d: dW (kernel + reduce) %.3f ms (%.0f TF/s)   dx %.3f ms (%.0f TF/s)   '
              'pack %.3f ms, adjoint pack %.3f ms' % (name, tiles, n, st, t_w, fl / t_w / 1e9, t_x, fl / t_x / 1e9, t_p, t_a), flush=True)
    sys.exit(0)
tot = [0.0, 0.0]
for (H, W) in [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]:
    x = torch.randn(B, 256, H, W, device='cuda')
    kind = os.environ.get('IA_BENCH_INPUT', 'randn')        # randn | relu (what a tower layer really reads) | zeros
    x = x.clamp(min=0) if kind == 'relu' else (x * 0 if kind == 'zeros' else x)
    x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(256, 256, 3, 3, device='cuda') * 0.03).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(256, device='cuda')
    wp = ops.conv3x3_bf16_pack(w)
    def lib():
        y = F.conv2d(x, w, None, 1, 1)
        return ops.channel_affine_act_(y, None, b, relu=True)
    def mine():
        return ops.conv3x3_bf16(x, wp, b, 256, relu=True)
    t0, t1 = bench(lib), bench(mine)
    fl = 2.0 * B * H * W * 256 * 256 * 9
    tot[0] += t0; tot[1] += t1
    var = ''
    for v in ('41', '21'):                      # forced variants (4, 1, 4) / (2, 1, 4): 128- / 64-pixel tiles
        os.environ['IA_CONV3_VARIANT'] = v
        tv = bench(mine)
        var += '  %s: %.3f (%.0f)' % (v, tv, fl / tv / 1e9)
    del os.environ['IA_CONV3_VARIANT']
    print('%3dx%3d  library conv + epilogue %.3f ms (%.0f TF)   own kernel %.3f ms (%.0f TF) |%s' % (H, W, t0, fl / t0 / 1e9, t1, fl / t1 / 1e9, var), flush=True)
print('all levels: library %.3f ms, own %.3f ms' % tuple(tot))

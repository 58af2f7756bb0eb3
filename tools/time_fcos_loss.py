"""Loss part of one FCOS training iteration (B images of 800x1344, fixed synthetic head outputs and
gts of tests/synth_fcos_loss.py): point targets + the three / four losses of all levels forward +
their sum + backward, on the HIP node (`fused`) or on the torch transcription of the reference
(`torch`, `fuse_loss = False`).  Prints wall time per iteration (HIP events around --iters
iterations after 5 warm-up iterations) for --runs runs; with both routes in --route they alternate.

    python tools/time_fcos_loss.py --head {iou_aware,plain} --route {torch,fused,both} [--batch 4]
                                   [--iters 400] [--runs 3]

Under `rocprofv3 --kernel-trace --stats -- python tools/time_fcos_loss.py --route fused --iters 20
--runs 1` (one route per run, a run of its own) the per-kernel times and the launches per
iteration come from the kernel statistics divided by 5 + iters iterations.
"""
import argparse
import os
import sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import synth_fcos_loss as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--head', choices=('iou_aware', 'plain'), default='iou_aware')
ap.add_argument('--route', choices=('torch', 'fused', 'both'), default='both')
ap.add_argument('--batch', type=int, default=4)
ap.add_argument('--iters', type=int, default=400)
ap.add_argument('--runs', type=int, default=3)
a = ap.parse_args()

iou = a.head == 'iou_aware'
case = S.MAIN[:5] + (a.batch,) + S.MAIN[6:]
sizes, gb, gl, maps = S.case_inputs(case)
outs = [[torch.from_numpy(t).cuda().requires_grad_(True) for t in m] for m in maps[:4 if iou else 3]]
leaves = [t for m in outs for t in m]
gtb = [torch.from_numpy(x).cuda() for x in gb]
gtl = [torch.from_numpy(x).cuda() for x in gl]
head = S.make_head(iou, True).cuda()


def it(fused):
    head.fuse_loss = fused
    for t in leaves:
        t.grad = None
    losses = S.head_loss(head, outs, gtb, gtl)
    sum(v.sum() for v in losses.values()).backward()


def run(fused):
    for _ in range(5):
        it(fused)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        it(fused)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters


routes = ('torch', 'fused') if a.route == 'both' else (a.route,)
for r in range(a.runs):
    ms = {name: run(name == 'fused') for name in routes}
    line = '  '.join('%s %.3f ms' % (k, v) for k, v in ms.items())
    if len(ms) == 2:
        line += '  torch / fused %.2f' % (ms['torch'] / ms['fused'])
    print('B=%d %s run %d: targets + loss fwd + sum + bwd per iteration: %s' % (a.batch, a.head, r, line))
n = sum(h * w for h, w in sizes) * a.batch
print('focal algorithmic bytes per iteration: fwd %.1f MB (logits + int32 labels + weights), bwd %.1f MB '
      '(+ the gradient)' % (n * (S.C * 4 + 8) / 1e6, n * (2 * S.C * 4 + 8) / 1e6))

"""Loss part of one training iteration (BASELINE config 5 shapes: B images of 800x1344, fixed head
outputs): device target assignment + the three losses of all levels forward + parse_losses +
backward.  Prints wall per iteration (HIP events); under rocprofv3 the kernel trace is reduced by
tools/summarize_trace.py with the marker `k_box_ml<float, true` (last kernel of an iteration).

    python tools/time_headloss.py [B] [per_level | nhwc] [plain | balanced | --head {iou_aware,plain}]
                                  [balanced_l1] [--iters N]

`plain` (or `--head plain`): the plain RetinaHead built from the same settings, the IoU maps
dropped -- FocalLoss + SmoothL1Loss alone, on the same three routes (the all-levels node without
the IoU term, the per-level kernels, the channels-last kernels with reg as its own tensor, as its
training head produces it).  The focal part, and with it the algorithmic-bytes line, is shared.

`balanced`: the IoU-aware head with IOUbalancedSigmoidFocalLoss(eta = 1.5) + IoUbalancedSmoothL1Loss
(delta = 1.5), `fuse_balanced` set: the all-levels node with its IoU-balanced instances (markers
`k_box_ml<float, true, true, true>` / `k_box_nhwc<true, true, true>`), or with `per_level` the route such
a head takes without the switch.

`balanced_l1`: loss_bbox = BalancedL1Loss(alpha = 0.5, gamma = 1.5) with the configuration's beta and
loss_weight, on either head (combine with `plain`) and on all three routes: the node's LOC = 1 instances
(markers `k_box_ml<float, true, true, false, 1>` / `k_box_nhwc<true, true, false, 1>`, `.., false, false, 1>`
without the IoU term), or with `per_level` the per-level kernels `k_smooth_l1<.., 1>`.
"""
import os
import sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import synth  # noqa: E402
from iouaware.config import ConfigDict  # noqa: E402
from iouaware.head import IoUawareRetinaHead, RetinaHead  # noqa: E402
from iouaware.train import parse_losses  # noqa: E402
import bench  # noqa: E402

args = sys.argv[1:]
plain = 'plain' in args
if '--head' in args:
    k = args.index('--head')
    if k + 1 >= len(args) or args[k + 1] not in ('iou_aware', 'plain'):
        sys.exit('--head takes iou_aware or plain')
    plain = args[k + 1] == 'plain'
    del args[k:k + 2]
n = 20                                   # timed iterations (--iters: a longer window, less host noise)
if '--iters' in args:
    k = args.index('--iters')
    n = int(args[k + 1])
    del args[k:k + 2]
balanced = 'balanced' in args
if balanced and plain:
    sys.exit('the IoU-balanced losses need the IoU-aware head')
balanced_l1 = 'balanced_l1' in args
if balanced and balanced_l1:
    sys.exit('balanced (the IoU-balanced smooth-L1) and balanced_l1 both replace loss_bbox')
args = [a for a in args if a not in ('plain', 'balanced', 'balanced_l1')]
B = int(args[0]) if args else 4
per_level = len(args) > 1 and args[1] == 'per_level'
nhwc = len(args) > 1 and args[1] == 'nhwc'              # channels-last outputs, reg | iou as slices of one
                                                         # 48-channel tensor: what the training head produces
TRAIN_CFG = ConfigDict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4,
                                     min_pos_iou=0, ignore_iof_thr=-1), allowed_border=-1,
                       pos_weight=-1, debug=False)
kw = dict(bench.MODEL['bbox_head'])
kw.pop('type')
if plain:
    for k in ('loss_iou', 'attach_iou_target'):
        kw.pop(k, None)
if balanced:
    kw['loss_cls'] = dict(type='IOUbalancedSigmoidFocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
                          eta=1.5, loss_weight=1.0)
    kw['loss_bbox'] = dict(type='IoUbalancedSmoothL1Loss', beta=kw['loss_bbox'].get('beta', 0.11), delta=1.5,
                           loss_weight=kw['loss_bbox'].get('loss_weight', 1.0))
if balanced_l1:
    kw['loss_bbox'] = dict(type='BalancedL1Loss', alpha=0.5, gamma=1.5, beta=kw['loss_bbox'].get('beta', 0.11),
                           loss_weight=kw['loss_bbox'].get('loss_weight', 1.0))
head = (RetinaHead if plain else IoUawareRetinaHead)(**kw).cuda()
head.fuse_levels = not per_level
head.fuse_balanced = balanced
cls, reg, iou = synth.head_outputs(3, B, 800, 1344, 'A')
outs = [[torch.from_numpy(t).cuda().requires_grad_(True) for t in x]
        for x in ((cls, reg) if plain else (cls, reg, iou))]
leaves = [t for x in outs for t in x]
if nhwc and plain:
    outs = [[t.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in x]
            for x in outs]
    leaves = [t for x in outs for t in x]
elif nhwc:
    cl = torch.channels_last
    c = [t.detach().contiguous(memory_format=cl).requires_grad_(True) for t in outs[0]]
    ri = [torch.cat([r.detach(), i.detach(), r.detach()[:, :3] * 0], 1).contiguous(memory_format=cl)
          .requires_grad_(True) for r, i in zip(outs[1], outs[2])]
    n_reg, n_iou = outs[1][0].shape[1], outs[2][0].shape[1]
    outs = [c, [t[:, :n_reg] for t in ri], [t[:, n_reg:n_reg + n_iou] for t in ri]]
    leaves = c + ri
gts, gls = synth.train_targets(5, B, 800, 1333, max_gt=20)
gtb = [torch.from_numpy(x).cuda() for x in gts]
gtl = [torch.from_numpy(x).cuda() for x in gls]
metas = [synth.img_meta(800, 1333, 800, 1344) for _ in range(B)]


FWD_ONLY = os.environ.get('FWD_ONLY')


def it():
    if FWD_ONLY:
        with torch.no_grad():
            head.loss(*outs, gtb, gtl, metas, TRAIN_CFG)
        return
    for t in leaves:
        t.grad = None
    losses = head.loss(*outs, gtb, gtl, metas, TRAIN_CFG)
    loss, _ = parse_losses(losses)
    loss.backward()


for _ in range(5):
    it()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
e0.record()
for _ in range(n):
    it()
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / n
print('B=%d %s%s: targets + losses fwd + bwd  %.3f ms per iteration' %
      (B, 'plain RetinaHead, ' if plain else ('IoU-balanced losses, ' if balanced else ''),
       ('BalancedL1Loss, ' if balanced_l1 else '') +
       ('per-level kernels' if per_level else 'all-levels kernels'), ms))
print('focal algorithmic bytes: fwd %.1f MB, bwd %.1f MB per iteration' %
      (66931200 * B / 1e6, 131443200 * B / 1e6))

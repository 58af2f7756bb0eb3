"""Scratch: BASELINE config 5 on one GPU -- training iterations of R-50 IoU-aware RetinaNet at
800x1344, B images, HIP target assignment + loss kernels (no data-parallel all-reduce here).

    python tools/time_train.py [B]
    MODEL=fcos|fcos_plain python tools/time_train.py [B]     the two FCOS detectors (R-50 caffe, GN
                                                             towers): tools/time_fcos.py's own
                                                             config, or CONFIG=<an mmdet config file
                                                             with model / train_cfg / test_cfg>
    TRAIN_WINOGRAD=0    the head's module route (bbox_head.train_winograd = False)
    TRAIN_BF16=1        the heads' bf16 route (bbox_head.train_bf16 = True: bf16 activations on the MFMA
                        convolutions -- and, in the FCOS towers, the bf16 GroupNorm node --, fp32 master
                        weights; iouaware/conv3x3_bf16_train.py)
    TRAIN_STRIDED=1     the stride-2 3x3 convolutions (conv2 of the first block of stages 2-4, P6 / P7) on
                        the im2col / col2im node (backbone.train_strided = neck.train_strided = True;
                        needs FUSE=1); 0: the framework's convolution
    FUSE_HEAD_LOSS=1    the FCOS heads' forward + loss as one call (bbox_head.fuse_head_loss = True: on the
                        bf16 / Winograd tower routes the packed channels-last outputs go straight into the loss
                        node, exp(scale * x) inside it); the route is then named <route>+packed
    BACKBONE=x101-32x4d|x101-64x4d   (MODEL=retina) the ResNeXt-101 backbones of the reference's
                        iou_aware_retinanet_x101_*_fpn_1x configs instead of R-50
    TRAIN_GCONV=1       the grouped 3x3 conv2 of the ResNeXt blocks on csrc/gconv.hip / csrc/gconv_bwd.hip
                        (backbone.train_gconv = True; needs FUSE=1); 0: the blocks' module route
The result line names the head route that ran (bf16 / winograd / module), the TRAIN_STRIDED setting and
the TRAIN_GCONV setting with the calls of the grouped node per iteration (the route that ran).
    ITERS=n             timed iterations (default 5)"""
import sys, os, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'iou-aware-single-stage-object-detector_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch, bench, synth, iouaware
from iouaware.config import ConfigDict
from iouaware.train import build_optimizer, train_step
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
torch.backends.cudnn.benchmark = not os.environ.get('NOFIND')
TRAIN_CFG = ConfigDict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0,
                                     ignore_iof_thr=-1), allowed_border=-1, pos_weight=-1, debug=False)
torch.manual_seed(0)
MODEL = os.environ.get('MODEL', 'retina')
BACKBONE = os.environ.get('BACKBONE', '')
if MODEL == 'retina':
    MODEL_CFG = dict(bench.MODEL)
    if BACKBONE:
        if BACKBONE not in ('x101-32x4d', 'x101-64x4d'):
            sys.exit('BACKBONE=%s: x101-32x4d or x101-64x4d (unset: R-50)' % BACKBONE)
        groups, base_width = dict([('x101-32x4d', (32, 4)), ('x101-64x4d', (64, 4))])[BACKBONE]
        MODEL_CFG['backbone'] = dict(type='ResNeXt', depth=101, groups=groups, base_width=base_width, num_stages=4,
                                     out_indices=(0, 1, 2, 3), frozen_stages=1, style='pytorch')
    model = iouaware.build_detector(ConfigDict(MODEL_CFG), train_cfg=TRAIN_CFG, test_cfg=ConfigDict(bench.TEST_CFG)).cuda().train()
else:
    TRAIN_CFG = ConfigDict(gamma=2.0, alpha=0.25)
    if os.environ.get('CONFIG'):
        from iouaware.config import Config
        cfg = Config.fromfile(os.environ['CONFIG'])
        cfg.model['pretrained'] = None
        TRAIN_CFG = cfg.train_cfg
        model = iouaware.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().train()
    else:
        import time_fcos
        model = time_fcos.build(head=dict(fcos='iou_aware', fcos_plain='plain')[MODEL]).train()
        model.train_cfg = TRAIN_CFG
if os.environ.get('TRAIN_WINOGRAD') is not None:
    model.bbox_head.train_winograd = bool(int(os.environ['TRAIN_WINOGRAD']))
if os.environ.get('TRAIN_BF16') is not None:
    model.bbox_head.train_bf16 = bool(int(os.environ['TRAIN_BF16']))
if os.environ.get('FUSE_HEAD_LOSS') is not None:
    model.bbox_head.fuse_head_loss = bool(int(os.environ['FUSE_HEAD_LOSS']))
STRIDED = bool(int(os.environ.get('TRAIN_STRIDED', '0')))
if STRIDED:
    model.backbone.train_strided = model.neck.train_strided = True      # the backbone's is read by fuse_inference below
GCONV = bool(int(os.environ.get('TRAIN_GCONV', '0')))
if GCONV:
    if not os.environ.get('FUSE'):
        sys.exit('TRAIN_GCONV=1 needs FUSE=1: the switch is read by fuse_inference')
    model.backbone.train_gconv = True                                   # read by fuse_inference below
print('model %s  head %s  train_winograd %s  train_bf16 %s' % (MODEL, type(model.bbox_head).__name__, model.bbox_head.train_winograd,
                                                               getattr(model.bbox_head, 'train_bf16', False)))
# which head route runs: count the calls of the route functions
from iouaware import conv3x3_bf16_train, winograd_train
ROUTE = []
def _count(mod, name, tag):
    real = getattr(mod, name)
    def spy(*a, **k):
        ROUTE.append(tag)
        return real(*a, **k)
    setattr(mod, name, spy)
for _name in ('head_forward', 'fcos_head_forward'):
    _count(conv3x3_bf16_train, _name, 'bf16')
    _count(winograd_train, _name, 'winograd')
_count(conv3x3_bf16_train, 'fcos_head_forward_packed', 'bf16+packed')
_count(winograd_train, 'fcos_head_forward_packed', 'winograd+packed')
from iouaware import train_fuse
GCONV_CALLS = []
_real_gconv = train_fuse.grouped_conv3x3_train
def _gconv_spy(*a, **k):
    GCONV_CALLS.append(1)
    return _real_gconv(*a, **k)
train_fuse.grouped_conv3x3_train = _gconv_spy
opt = build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001))
img = torch.randn(B, 3, 800, 1344, device='cuda')
if os.environ.get('FUSE'):
    from iouaware.fuse import fuse_inference
    print('fused modules', fuse_inference(model, winograd=True, train=True))
    os.environ['CL'] = '1'
if os.environ.get('CL'):
    model = model.to(memory_format=torch.channels_last); img = img.contiguous(memory_format=torch.channels_last)
gts, gls = synth.train_targets(5, B, 800, 1333, max_gt=20)
gtb = [torch.from_numpy(x).cuda() for x in gts]; gtl = [torch.from_numpy(x).cuda() for x in gls]
metas = [synth.img_meta(800, 1333, 800, 1344) for _ in range(B)]
for _ in range(3): lv = train_step(model, opt, img, metas, gtb, gtl, grad_clip=dict(max_norm=35, norm_type=2))
torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); t = time.time(); n = int(os.environ.get('ITERS', 5))
del ROUTE[:]; del GCONV_CALLS[:]
for _ in range(n): lv = train_step(model, opt, img, metas, gtb, gtl, grad_clip=dict(max_norm=35, norm_type=2))
torch.cuda.synchronize(); dt = (time.time() - t) / n
route = '+'.join(sorted(set(ROUTE))) if ROUTE else 'module'
print('B=%d  backbone %s  head route %s  train_strided %d  train_gconv %d (%d node calls per iteration)  %.1f ms/iter  %.1f img/s  loss %s  mem %.2f GB' % (B, BACKBONE or 'r50', route, STRIDED, GCONV, len(GCONV_CALLS) // n, dt * 1e3, B / dt, {k: round(v, 4) for k, v in lv.items()}, torch.cuda.max_memory_allocated() / 1e9))
if os.environ.get('TRAIN_ONLY'):
    sys.exit(0)
# loss part alone (targets + 3 losses fwd + bwd) on fixed head outputs
with torch.no_grad():
    outs = model.bbox_head(model.extract_feat(img))
outs = [[t.detach().requires_grad_(True) for t in o] for o in outs]
def loss_only():
    losses = model.bbox_head.loss(*outs, gtb, gtl, metas, TRAIN_CFG)
    sum(sum(v) for v in losses.values()).backward()
for _ in range(3): loss_only()
torch.cuda.synchronize(); t = time.time()
for _ in range(10): loss_only()
torch.cuda.synchronize(); print('targets + losses fwd+bwd: %.2f ms' % ((time.time() - t) / 10 * 1e3))

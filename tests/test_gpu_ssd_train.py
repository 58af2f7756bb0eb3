"""-m gpu: SSD300 built from the recorded ssd300_coco config with the recorded train_cfg, batch 2 at
300 x 300: forward_train -> parse_losses -> backward on the fused loss node and on the torch route, the
loss dict and the head convolutions' gradient norms under the training gate; one optimizer step; the
mmdet.* alias takes the same route."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def ssd300():
    import iouaware
    from iouaware.config import ConfigDict
    with open(os.path.join(GOLD, 'ssd_ref.json')) as fh:
        cfg = json.load(fh)['configs']['ssd300_coco']
    train_cfg = json.loads(str(np.load(os.path.join(GOLD, 'ssd_loss.npz'))['train_cfg']))
    torch.manual_seed(0)
    det = iouaware.build_detector(ConfigDict(dict(cfg['model'], pretrained=None)), train_cfg=ConfigDict(train_cfg),
                                  test_cfg=ConfigDict(cfg['test_cfg']))
    det = det.cuda().train()
    torch.manual_seed(5)
    img = torch.randn(2, 3, 300, 300, device='cuda') * 10
    metas = [dict(ori_shape=(300, 300, 3), img_shape=(300, 300, 3), pad_shape=(300, 300, 3), scale_factor=1.0,
                  flip=False)] * 2
    gts = [torch.tensor([[20., 30., 120., 160.], [150., 40., 290., 200.], [60., 180., 110., 260.], [200., 220., 228., 246.]], device='cuda'),
           torch.tensor([[5., 5., 280., 290.], [100., 100., 140., 150.]], device='cuda')]
    gls = [torch.tensor([3, 17, 80, 9], device='cuda'), torch.tensor([1, 44], device='cuda')]
    return dict(det=det, img=img, metas=metas, gts=gts, gls=gls)


def _step(s, fuse):
    from iouaware.train import parse_losses
    det = s['det']
    det.bbox_head.fuse_loss = fuse
    det.zero_grad()
    losses = det.forward_train(s['img'], s['metas'], s['gts'], s['gls'])
    loss, log_vars = parse_losses(losses)
    loss.backward()
    det.bbox_head.fuse_loss = type(det.bbox_head).fuse_loss
    norms = {n: float(p.grad.double().norm()) for n, p in det.bbox_head.named_parameters()}
    return losses, {k: float(v.detach()) for k, v in log_vars.items()}, norms


def test_forward_train_on_both_routes(ssd300):
    """the torch route in fp32 is the twin; the gate against it: <= 1e-4 of the largest magnitude (the
    convolutions' gradients come from torch's library kernels on both sides)"""
    lf, vf, nf = _step(ssd300, True)
    lt, vt, nt = _step(ssd300, False)
    assert sorted(lf) == sorted(lt) == ['loss_bbox', 'loss_cls']
    assert all(len(lf[k]) == 2 and all(tuple(t.shape) == (1,) for t in lf[k]) for k in lf)
    assert 'SsdHeadLossFn' in type(lf['loss_cls'][0].grad_fn).__name__ or \
        'SsdHeadLossFn' in str(lf['loss_cls'][0].grad_fn.next_functions)          # the native node ran
    for k in ('loss_cls', 'loss_bbox', 'loss'):
        print('%s: fused %.6f torch %.6f' % (k, vf[k], vt[k]))
        assert np.isfinite(vf[k]) and abs(vf[k] - vt[k]) <= 1e-4 * abs(vt[k])
    scale = max(nt.values())
    assert scale > 0 and len(nf) == 24
    for n in nt:
        print('%s: gradient norm fused %.6e torch %.6e' % (n, nf[n], nt[n]))
        assert np.isfinite(nf[n]) and abs(nf[n] - nt[n]) <= 1e-4 * scale
    assert all(p.grad is not None for p in ssd300['det'].backbone.parameters() if p.requires_grad)


def test_one_optimizer_step_and_the_mmdet_alias(ssd300):
    from iouaware import compat, ssd_head
    from iouaware.train import build_optimizer, train_step
    compat.install()
    import mmdet.models as mm
    det = ssd300['det']
    assert mm.SSDHead is ssd_head.SSDHead and isinstance(det.bbox_head, mm.SSDHead)
    state = {k: v.clone() for k, v in det.state_dict().items()}
    det.bbox_head.fuse_loss = True
    try:
        opt = build_optimizer(det, dict(type='SGD', lr=1e-4, momentum=0.9, weight_decay=5e-4))
        out = train_step(det, opt, ssd300['img'], ssd300['metas'], ssd300['gts'], ssd300['gls'],
                         grad_clip=dict(max_norm=35, norm_type=2))
    finally:
        det.bbox_head.fuse_loss = type(det.bbox_head).fuse_loss
    assert list(out) == ['loss_cls', 'loss_bbox', 'loss'] and all(np.isfinite(v) for v in out.values())
    assert all(bool(torch.isfinite(p).all()) for p in det.parameters())
    assert any(not torch.equal(p, state[k]) for k, p in det.state_dict().items())
    det.load_state_dict(state)

"""-m gpu: SSD's training loss on the HIP node (csrc/ssdloss.hip) -- the cross-entropy rows, the
hard-negative mining and the whole node with its backward against tests/ssd_loss_ref.py in fp64.

Geometries (tests/ssd_loss_ref.py, CASES): `small` 192 rows x 6 logits, batch 3 (the 4 / 6-anchor
boundary, three 1 x 1 levels); `mid` 2 268 rows x 81; `ssd300` SSD300's own 8 732 rows x 81 (keys in LDS);
`big` SSD512's 24 564 rows x 3 logits, above the LDS budget of the mining kernel
(ia_ssd_mine_lds_rows() = 12 288 rows): keys re-read from global memory.

The training gate of this project: error <= 1e-4 of the yardstick's largest magnitude and <= 4 x the
error of the plain fp32 torch evaluation (ssd_loss_ref in fp32 on the CPU), where that is non-zero.
Selections are compared exactly: the fixtures' margins (tests/test_host_ssd_loss.py) make a mismatch a
bug and not rounding."""
import numpy as np
import pytest
import torch

import ssd_loss_ref as R

pytestmark = pytest.mark.gpu

LDS_ROWS = 12288
AVG_DEV = 'device scalar'


@pytest.fixture(scope='module')
def data():
    """{name: dict(inp, head, geom, dev tensors, r64, r32)} built on first use, shared and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            from iouaware.ssd_head import SSDHead
            case = R.CASES[name]
            inp = R.inputs(name)
            head = SSDHead(num_classes=case['num_classes'], **case['head'])
            geom = head.geometry(case['sizes'])
            go = np.stack([np.linspace(0.5, 1.5, inp['B']), np.linspace(2.0, 1.0, inp['B'])], 1)
            tg = inp['targets']
            r64 = R.loss([c.double() for c in inp['cls']], [r.double() for r in inp['reg']], *tg, grad_out=go)
            r32 = R.loss(inp['cls'], inp['reg'], *tg, grad_out=go)
            # what makes a selection mismatch a bug: fp32 selects what fp64 selects, and outside the tie
            # images the k-th and (k + 1)-th largest negative loss differ by >= 1e-4
            assert torch.equal(r32['sel'], r64['sel'])
            for b, kind in enumerate(case['kinds']):
                m = R.margins(inp, b)
                assert m['iou'] >= 1e-5 and m['best'] >= 1e-5 and (kind != 'few' or m['gap'] >= 1e-4), (name, b, m)
            cache[name] = dict(inp=inp, head=head, geom=geom, go=go, r64=r64, r32=r32,
                               cls=[c.cuda() for c in inp['cls']], reg=[r.cuda() for r in inp['reg']],
                               tg=[t.cuda() for t in tg[:4]], avg=float(tg[4]))
        return cache[name]
    return get


def gate(got, want64, torch32, what):
    got, want = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    err = float(np.abs(got - want).max())
    err_t = float(np.abs(np.asarray(torch32, np.float64) - want).max())
    scale = float(np.abs(want).max())
    print('%s: error %.3e, fp32 torch %.3e (ratio %s), largest magnitude %.3e'
          % (what, err, err_t, '%.2f' % (err / err_t) if err_t > 0 else 'n/a', scale))
    assert err <= 1e-4 * scale, what
    if err_t > 0:
        assert err <= 4 * err_t, what
    return err, err_t


def _rows_of(maps, ch):
    return R.rows([m.cpu() for m in maps], ch).numpy()


# ------------------------------------------------------------------ stage 1
@pytest.mark.parametrize('name', ['small', 'mid', 'ssd300'])
def test_rows_ce_and_lse_against_fp64(data, name):
    from iouaware import ssd_ops
    d = data(name)
    assert d['geom'].R == d['inp']['R']
    ce, lse, parts = ssd_ops.ssd_loss_rows(d['geom'], d['cls'], d['reg'], *d['tg'])
    nc = d['inp']['num_classes']
    labels = d['inp']['targets'][0]
    want, want32 = {}, {}
    for dt, out in ((torch.float64, want), (torch.float32, want32)):
        x = R.rows([c.to(dt) for c in d['inp']['cls']], nc)
        out['lse'] = torch.stack([R.cross_entropy(x[b], torch.zeros_like(labels[b])) + x[b, :, 0] for b in range(len(x))])
        out['ce'] = torch.stack([R.cross_entropy(x[b], labels[b]) for b in range(len(x))])
    gate(ce.cpu(), want['ce'], want32['ce'], name + ' ce')
    gate(lse.cpu(), want['lse'], want32['lse'], name + ' lse')
    # the box partials: their sum per image is the smooth-L1 sum
    box = parts.sum(1).cpu().numpy() / d['avg']
    r64 = R.loss([c.double() for c in d['inp']['cls']], [r.double() for r in d['inp']['reg']], *d['inp']['targets'])
    assert np.abs(box - r64['loss_bbox'].numpy()).max() <= 1e-6 * np.abs(r64['loss_bbox'].numpy()).max()


def test_rows_large_logits_and_zero_weights(data):
    from iouaware import ssd_ops
    d = data('small')
    nc, B, Rn = d['inp']['num_classes'], d['inp']['B'], d['inp']['R']
    rng = np.random.RandomState(7)
    logits = rng.choice(np.asarray([-80.0, 80.0, 0.0, 3.5], np.float32), size=(B, Rn, nc))
    logits[:, ::5] = -80.0                                     # whole rows at -80 and at +80
    logits[:, 1::5] = 80.0
    cls = [torch.from_numpy(c).cuda() for c in R.to_maps(logits, R.CASES['small']['sizes'], d['inp']['A'])]
    labels = torch.from_numpy(rng.randint(0, nc, size=(B, Rn))).cuda()
    lw = torch.from_numpy((rng.rand(B, Rn) < 0.5).astype(np.float32)).cuda()
    ce, lse, _ = ssd_ops.ssd_loss_rows(d['geom'], cls, d['reg'], labels, lw, d['tg'][2], d['tg'][3])
    x = torch.from_numpy(logits)
    want = torch.stack([R.cross_entropy(x[b].double(), labels[b].cpu()) * lw[b].cpu().double() for b in range(B)])
    want32 = torch.stack([R.cross_entropy(x[b], labels[b].cpu()) * lw[b].cpu() for b in range(B)])
    assert bool(torch.isfinite(ce).all()) and bool(torch.isfinite(lse).all())
    gate(ce.cpu(), want, want32, 'ce at logits of +-80')
    assert float(want.max()) >= 159.0
    off = (lw == 0)
    assert bool(off.any()) and bool((ce[off].view(torch.int32) == 0).all())      # weight 0: exactly +0.0


# ------------------------------------------------------------------ mining
def _mine_check(ce, labels, ratio, avg=1.0):
    """ssd_mine on (B, R) numpy inputs against ssd_loss_ref.mine -> (sel, counts) numpy"""
    from iouaware import ssd_ops
    t_ce, t_lab = torch.from_numpy(ce), torch.from_numpy(labels)
    sel, counts, losses = ssd_ops.ssd_mine(t_ce.cuda(), t_lab.cuda(), ratio, avg)
    sel, counts, losses = sel.cpu().numpy(), counts.cpu().numpy(), losses.cpu().numpy()
    for b in range(ce.shape[0]):
        want, npos, k = R.mine(t_ce[b], t_lab[b], ratio)
        assert counts[b].tolist() == [npos, k], (b, counts[b], npos, k)
        assert np.array_equal(sel[b].astype(bool), want.numpy()), 'image %d: selection differs' % b
        s = float(ce[b].astype(np.float64)[want.numpy()].sum() / avg)
        assert abs(losses[b, 0] - s) <= 1e-6 * max(abs(s), 1e-30), (b, losses[b, 0], s)
        assert losses[b, 1] == 0.0
    return sel, counts


def _labels(rng, Rn, npos, nign=0):
    lab = np.zeros(Rn, np.int64)
    idx = rng.permutation(Rn)
    lab[idx[:npos]] = rng.randint(1, 81, size=npos)
    lab[idx[npos:npos + nign]] = -1
    return lab


@pytest.mark.parametrize('Rn', [1000, LDS_ROWS, LDS_ROWS + 1])
def test_mine_counts_and_k_edges(Rn):
    """num_pos = 0 (k = 0), 1, 3 * num_pos > num_neg, and k at 63 / 64 / 65 and 255 / 256 / 257 (ratio 1),
    on both sides of the LDS budget; rows with a negative label are neither positive nor negative"""
    from iouaware import ssd_ops
    assert ssd_ops.ssd_mine_lds_rows() == LDS_ROWS
    rng = np.random.RandomState(Rn)
    npos = [0, 1, Rn // 3, 63, 64, 65, 255, 256, 257]
    labels = np.stack([_labels(rng, Rn, n, nign=17) for n in npos])
    ce = np.abs(rng.randn(len(npos), Rn)).astype(np.float32)
    sel, counts = _mine_check(ce, labels, 3, avg=7.0)
    assert counts[0].tolist() == [0, 0] and not sel[0].any()
    assert counts[1].tolist() == [1, 3]
    assert counts[2, 1] == Rn - 17 - Rn // 3 < 3 * (Rn // 3)            # every negative is taken
    sel, counts = _mine_check(ce, labels, 1)
    assert counts[3:, 1].tolist() == [63, 64, 65, 255, 256, 257]
    _mine_check(ce, labels, 0)                                          # ratio 0: positives only


@pytest.mark.parametrize('Rn', [2268, LDS_ROWS + 1000])
def test_mine_ties_zero_runs_and_digit_edges(Rn):
    rng = np.random.RandomState(Rn + 1)
    cases = []
    # (0) exact ties at the threshold: 40 bit-identical rows, 10 rows above them, k = 30
    lab = _labels(rng, Rn, 10)
    ce = (rng.rand(Rn) * 0.5).astype(np.float32)
    neg = np.nonzero(lab == 0)[0]
    tie = np.sort(rng.choice(neg, 40, replace=False))
    ce[tie] = np.float32(0.7501)
    ce[rng.choice(np.setdiff1d(neg, tie), 10, replace=False)] += np.float32(1.0)
    cases.append((lab, ce))
    # (1) a run of ce == 0 reached by k: 20 non-zero negatives, the rest +0.0 and -0.0, k = 60
    lab = _labels(rng, Rn, 20)
    ce = np.zeros(Rn, np.float32)
    neg = np.nonzero(lab == 0)[0]
    ce[neg[1::2]] = -0.0
    ce[rng.choice(neg, 20, replace=False)] = rng.rand(20).astype(np.float32) + 0.1
    ce[lab > 0] = 2.0
    cases.append((lab, ce))
    # (2) keys that differ only in the lowest byte, (3) only in the highest byte (both signs)
    lab = _labels(rng, Rn, 30)
    low = (np.uint32(0x3f800000) + rng.randint(0, 256, size=Rn).astype(np.uint32)).view(np.float32)
    cases.append((lab, low))
    top = rng.choice(np.concatenate([np.arange(0x30, 0x50), np.arange(0xb0, 0xd0)]), size=Rn).astype(np.uint32)
    cases.append((lab, ((top << np.uint32(24)) | np.uint32(0x00123456)).view(np.float32)))
    # (4) negative losses (a negative label weight): the order of the keys holds across the sign
    cases.append((lab, rng.randn(Rn).astype(np.float32)))
    labels, ce = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    sel, counts = _mine_check(ce, labels, 3)
    # the tie winners are the lowest row ids, exactly k - #(ce > t) of them
    assert counts[0, 1] == 30
    assert sel[0][tie].tolist() == [1] * 20 + [0] * 20
    zero_neg = np.nonzero((labels[1] == 0) & (ce[1] == 0))[0]
    assert sel[1][zero_neg].tolist() == [1] * 40 + [0] * (len(zero_neg) - 40)


# ------------------------------------------------------------------ the node
GUARD = 64


def _guarded(shapes, dev):
    """contiguous tensors of these shapes inside one NaN-filled buffer, GUARD floats around each"""
    n = sum(int(np.prod(s)) + GUARD for s in shapes) + GUARD
    buf = torch.full((n,), float('nan'), dtype=torch.float32, device=dev)
    out, off = [], GUARD
    for s in shapes:
        k = int(np.prod(s))
        out.append(buf[off:off + k].view(*s))
        off += k + GUARD
    return buf, out


def _run_node(d, avg, guard=False):
    from iouaware import _lib, ssd_ops
    geom, B = d['geom'], d['inp']['B']
    cls = [c.clone().requires_grad_(True) for c in d['cls']]
    reg = [r.clone().requires_grad_(True) for r in d['reg']]
    kw, extra = {}, None
    if guard:
        nbytes = _lib.lib().ia_ssd_head_loss_workspace_bytes(geom.ref(), B)
        wsbuf = torch.full((nbytes + 512,), 0xFF, dtype=torch.uint8, device='cuda')
        gbuf, grads = _guarded([tuple(t.shape) for t in cls + reg], 'cuda')
        kw = dict(workspace=wsbuf[256:256 + nbytes], grads=grads)
        extra = (wsbuf, nbytes, gbuf, grads)
    lc, lb = ssd_ops.ssd_head_loss(geom, cls, reg, *d['tg'], avg, R.NEG_POS_RATIO, R.BETA, **kw)
    go = torch.from_numpy(d['go']).float().cuda()
    ((lc * go[:, 0]).sum() + (lb * go[:, 1]).sum()).backward()
    return lc.detach(), lb.detach(), [c.grad for c in cls], [r.grad for r in reg], extra


@pytest.mark.parametrize('name,avg_kind', [('small', 'host'), ('mid', AVG_DEV), ('ssd300', 'host'), ('big', 'host')])
def test_node_losses_and_gradients_against_fp64(data, name, avg_kind):
    from iouaware import ssd_ops
    d = data(name)
    B, nc, r64, r32 = d['inp']['B'], d['inp']['num_classes'], d['r64'], d['r32']
    assert (d['geom'].R > LDS_ROWS) == (name == 'big')
    avg = torch.tensor([d['avg']], device='cuda') if avg_kind == AVG_DEV else d['avg']
    lc, lb, gc, gr, (wsbuf, nbytes, gbuf, grads) = _run_node(d, avg, guard=True)
    views = ssd_ops.ssd_loss_workspace_views(d['geom'], B, wsbuf[256:256 + nbytes])
    # selection and counts: identical to the yardstick
    assert np.array_equal(views['sel'].cpu().numpy().astype(bool), r64['sel'].numpy())
    assert np.array_equal(views['counts'].cpu().numpy(), r64['counts'])
    gate(lc.cpu(), r64['loss_cls'], r32['loss_cls'], name + ' loss_cls')
    gate(lb.cpu(), r64['loss_bbox'], r32['loss_bbox'], name + ' loss_bbox')
    g_cls, g_reg = _rows_of(gc, nc), _rows_of(gr, 4)
    gate(g_cls, r64['grad_cls'], r32['grad_cls'], name + ' grad_cls')
    gate(g_reg, r64['grad_reg'], r32['grad_reg'], name + ' grad_reg')
    # unselected rows: exactly +0.0 in every class gradient; rows without box weight: +0.0
    off = ~r64['sel'].numpy()
    assert off.any() and (g_cls.view(np.int32)[off] == 0).all()
    assert (g_reg.view(np.int32)[d['inp']['targets'][3].numpy() == 0] == 0).all()
    # every element written (no NaN left inside), nothing outside: the guards keep their fill
    inside = torch.zeros_like(gbuf, dtype=torch.bool)
    for g in grads:
        assert not bool(torch.isnan(g).any())
        start = (g.data_ptr() - gbuf.data_ptr()) // 4
        inside[start:start + g.numel()] = True
    assert bool(torch.isnan(gbuf[~inside]).all()) and int((~inside).sum()) == GUARD * (len(grads) + 1)
    assert bool((wsbuf[:256] == 0xFF).all()) and bool((wsbuf[256 + nbytes:] == 0xFF).all())


def test_node_gives_the_same_bits_in_every_run(data):
    d = data('mid')
    a, b = _run_node(d, d['avg']), _run_node(d, d['avg'])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize('name', ['small', 'mid'])
def test_head_loss_fused_against_the_torch_route_on_the_device(data, name):
    import json
    import os
    from iouaware.config import ConfigDict
    d = data(name)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssd_loss.npz'))
    cfg = ConfigDict(json.loads(str(gold['train_cfg'])))
    head, inp, nc = d['head'], d['inp'], d['inp']['num_classes']
    gts, gls = [g.cuda() for g in inp['gt_bboxes']], [l.cuda() for l in inp['gt_labels']]
    res = {}
    for fuse in (True, False):
        head.fuse_loss = fuse
        cls = [c.clone().requires_grad_(True) for c in d['cls']]
        reg = [r.clone().requires_grad_(True) for r in d['reg']]
        out = head.loss(cls, reg, gts, gls, inp['metas'], cfg)
        assert all(len(v) == inp['B'] and all(tuple(t.shape) == (1,) for t in v) for v in out.values())
        (sum(v.sum() for v in out['loss_cls']) + sum(v.sum() for v in out['loss_bbox'])).backward()
        res[fuse] = (torch.cat(out['loss_cls']).detach().cpu().numpy(), torch.cat(out['loss_bbox']).detach().cpu().numpy(),
                     _rows_of([c.grad for c in cls], nc), _rows_of([r.grad for r in reg], 4))
    head.fuse_loss = type(head).fuse_loss
    ones = np.ones((inp['B'], 2))
    r64 = R.loss([c.double() for c in inp['cls']], [r.double() for r in inp['reg']], *inp['targets'], grad_out=ones)
    # the tie rows carry equal gradients on whichever of them the route picked: compared by their number
    for b, tie in enumerate(inp['tie_rows']):
        n = [int((np.abs(res[f][2][b, tie]).max(1) > 0).sum()) for f in (True, False)]
        assert n[0] == n[1]
        for arr in (res[True][2], res[False][2], r64['grad_cls'].numpy()):
            arr[b, tie] = 0
    for f in (True, False):
        assert np.array_equal(np.abs(res[f][2]).max(2) > 0, np.abs(r64['grad_cls'].numpy()).max(2) > 0)   # the selection
    for i, (what, key) in enumerate((('loss_cls', 'loss_cls'), ('loss_bbox', 'loss_bbox'), ('grad_cls', 'grad_cls'),
                                     ('grad_reg', 'grad_reg'))):
        gate(res[True][i], r64[key], res[False][i], '%s fused %s against the torch route' % (name, what))

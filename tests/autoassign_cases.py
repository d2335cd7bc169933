"""Generated AutoAssign cases off the fixture geometry (in the manner of tests/fovea_cases.py): inputs for dsl_aa_assign / dsl_aa_loss
whose expected outputs come from tests/autoassign_ref.py, the model that test_autoassign_cpu.py pins to the reference's own head.

Box edges lie a quarter pixel off the half-pixel grid, so no edge comes near a point coordinate (a multiple of 8) and the inside mask
is decided far from rounding.  A case is redrawn (next seed) unless, in float64, every R_g of a box with inside points lies in
(1e-6, 1 - 1e-6) and every q <= 1 - 1e-6: the fixtures' conditions.
  four_images   batch 4 on a 256 x 320 canvas - level 0 holds 4 * 32 * 40 locations, twenty workgroups of the per-point pass - with an
                empty third image
  many_boxes    the fixture geometry, 70 boxes in the first image (more than a wavefront's lanes, two chunks), 3 in the second
  fewer         many_boxes' first five boxes per image: what a reused plan sees in its next step
  many_boxes_80 many_boxes' geometry with 80 classes: two classes per lane together with more boxes than a wavefront has lanes
  four_images_18  four_images' geometry with 18 classes (a class count that is no multiple of 4, off the fixture canvas)
  one_class     a single class: every box shares the one class, so the same-class rule decides every shared point"""
import functools

import numpy as np
import torch

import autoassign_ref as AR


def _boxes(rs, n, H, W, lo=6.0, hi=None):
    hi = hi or 0.9 * max(H, W)
    out = []
    while len(out) < n:
        w, h = np.exp(rs.uniform(np.log(lo), np.log(hi), 2))
        x, y = rs.uniform(-4, W - 4), rs.uniform(-4, H - 4)
        b = (np.round(np.array([x, y, min(x + w, W + 6), min(y + h, H + 6)]) * 2) / 2 + 0.25).astype(np.float32)
        if b[2] - b[0] < 1 or b[3] - b[1] < 1:
            continue
        out.append(b)
    return torch.from_numpy(np.stack(out))


def _make(seed, sizes, counts, H, W, C):
    for t in range(20):
        rs = np.random.RandomState(seed + 100 * t)
        gts = [_boxes(rs, k, H, W) if k else torch.zeros(0, 4) for k in counts]
        gls = [torch.from_numpy(rs.randint(0, C, len(b)).astype('int64')) for b in gts]
        n, M = len(counts), len(counts) * sum(h * w for h, w in sizes)
        g = torch.Generator().manual_seed(int(rs.randint(1 << 30)))
        c = dict(n=n, B=n, C=C, sizes=sizes, gts=gts, gls=gls, cls=torch.randn(M, C, generator=g) * 1.5 - 2.0,
                 raw=torch.randn(M, 4, generator=g) * 1.2 + 1.0, obj=torch.randn(M, 1, generator=g), scales=1.0 + 0.2 * torch.randn(5, generator=g),
                 mean=0.4 * torch.randn(C, 2, generator=g), sigma=1.0 + 0.6 * torch.rand(C, 2, generator=g), pos_w=0.25, neg_w=0.75,
                 center_w=0.75, bbox_weight=5.0)
        if _clean(c):
            return c
    raise RuntimeError('no clean draw')


def _clean(c):
    out = compute(c)[0]
    for R, ins in zip(out['R'], out['inside']):
        has = ins.any(0)
        if len(R) and not bool(((R[has] > 1e-6) & (R[has] < 1 - 1e-6)).all()):
            return False
    pts, lvl, img = AR.flat_points(c['sizes'], c['n'])
    pc, po = c['cls'].double().sigmoid(), c['obj'].double().reshape(-1).sigmoid()
    for i in range(c['n']):
        idx = torch.as_tensor(np.nonzero(img == i)[0])
        if not bool((pc[idx] * po[idx][:, None] * out['negw'][i] <= 1 - 1e-6).all()):
            return False
    return True


def compute(c, world=None):
    """autoassign_ref in float64 with autograd: (out dict, d cls, d raw, d obj, d scales, d mean, d sigma)."""
    leaf = lambda t: t.double().clone().requires_grad_()      # noqa: E731
    cls, raw, obj, sc, mean, sigma = (leaf(c[k]) for k in ('cls', 'raw', 'obj', 'scales', 'mean', 'sigma'))
    out = AR.loss(cls, raw, obj, sc, mean, sigma, c['gts'], c['gls'], c['sizes'], c['C'], c['pos_w'], c['neg_w'], c['center_w'], c['bbox_weight'],
                  world=world)
    (out['loss_pos'] + out['loss_neg'] + out['loss_center']).backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)      # noqa: E731
    return out, z(cls), z(raw), z(obj), z(sc), z(mean), z(sigma)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'four_images':
        return _make(11, [(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)], (9, 14, 0, 6), 256, 320, 20)
    if name == 'many_boxes':
        return _make(12, AR.SIZES, (70, 3), 128, 160, 20)
    if name == 'fewer':
        c = dict(case('many_boxes'))
        c['gts'], c['gls'] = [b[:5] for b in c['gts']], [l[:5] for l in c['gls']]
        return c
    if name == 'many_boxes_80':
        return _make(14, AR.SIZES, (70, 3), 128, 160, 80)
    if name == 'four_images_18':
        return _make(15, [(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)], (9, 14, 0, 6), 256, 320, 18)
    if name == 'one_class':
        return _make(13, AR.SIZES, (6, 4), 128, 160, 1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    """autoassign_ref's losses and gradients of the case: computed once, shared by the tests, left unchanged."""
    return compute(case(name))

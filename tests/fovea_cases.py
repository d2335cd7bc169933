"""Generated Fovea cases off the fixture geometry (in the manner of tests/head_cases.py): inputs for dsl_fovea_assign / dsl_fovea_loss
whose expected outputs come from tests/fovea_ref.py, the model that test_fovea_cpu.py pins to the reference's own FoveaHead.

Boxes lie on the half-pixel grid and have pairwise distinct fp32 sqrt-areas within an image, so that the one order the reference
leaves open (equal areas) does not occur.  The kernel and the model then perform the same fp32 operations in the same order: the
comparison is exact.
  four_images   batch 4 on a 256 x 320 canvas - level 0 holds 4 * 32 * 40 locations, twenty workgroups - with an empty third image
  many_boxes    the fixture geometry, 70 boxes in the first image (more than a wavefront's worth, two LDS chunks), 3 in the second
  fewer         many_boxes' first five boxes per image: what a reused plan sees in its next step"""
import functools

import numpy as np
import torch

import fovea_ref as FR

C = 20


def _boxes(rs, n, H, W, lo=4.0, hi=None):
    """n boxes on the half-pixel grid inside (and slightly beyond) the canvas, pairwise distinct fp32 sqrt-areas."""
    hi = hi or 0.9 * max(H, W)
    out, areas = [], set()
    while len(out) < n:
        w, h = np.exp(rs.uniform(np.log(lo), np.log(hi), 2))
        x, y = rs.uniform(-4, W - 4), rs.uniform(-4, H - 4)
        b = (np.round(np.array([x, y, min(x + w, W + 6), min(y + h, H + 6)]) * 2) / 2).astype(np.float32)
        if b[2] - b[0] < 1 or b[3] - b[1] < 1:
            continue
        a = float(np.sqrt((b[2] - b[0]) * (b[3] - b[1])))
        if a in areas:
            continue
        areas.add(a)
        out.append(b)
    return torch.from_numpy(np.stack(out))


def _make(rs, sizes, counts, H, W):
    gts = [_boxes(rs, k, H, W) if k else torch.zeros(0, 4) for k in counts]
    gls = [torch.from_numpy(rs.randint(0, C, len(b)).astype('int64')) for b in gts]
    n, M = len(counts), len(counts) * sum(h * w for h, w in sizes)
    g = torch.Generator().manual_seed(int(rs.randint(1 << 30)))
    cls = torch.randn(M, C, generator=g) * 1.5 - 2.5
    raw = torch.randn(M, 4, generator=g) * 1.5
    return dict(n=n, C=C, sizes=sizes, gts=gts, gls=gls, cls=cls, raw=raw, sigma=0.4, base=FR.BASE, ranges=FR.RANGES, beta=0.11, gamma=1.5,
                alpha=0.4)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'four_images':
        return _make(np.random.RandomState(11), [(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)], (9, 14, 0, 6), 256, 320)
    if name == 'many_boxes':
        return _make(np.random.RandomState(12), FR.SIZES, (70, 3), 128, 160)
    if name == 'fewer':
        c = dict(case('many_boxes'))
        c['gts'], c['gls'] = [b[:5] for b in c['gts']], [l[:5] for l in c['gls']]
        return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    """fovea_ref's assignment of the case: computed once, shared by the tests, left unchanged."""
    c = case(name)
    return FR.assign(c['gts'], c['gls'], c['sizes'], c['C'], c['sigma'], c['base'], c['ranges'])

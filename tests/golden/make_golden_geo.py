"""Generates geo_transforms.json: RandomShift, RandomCrop, Expand, MinIoURandomCrop and CutOut run from the reference file itself.

    python tests/golden/make_golden_geo.py <reference checkout>

The five classes are compiled out of mmdet/datasets/pipelines/transforms.py's source (the module imports cv2 / torchvision / mmcv,
none needed by these classes) and bbox_overlaps out of mmdet/core/evaluation/bbox_overlaps.py; in that file `random` is
numpy.random.  Only data is stored: per case the seed, the chain's constructor arguments, the input (an index into a shared pool of
hex images; boxes as the hex of their float32 bytes; labels), the reference's output (the image's shape and the SHA-256 of its bytes - equal
digests are equal images, and the file stays reviewable -, boxes, labels), the number of np.random draws the chain made, the last
four of them (name, value) and the stream's next draw.  `img_shape` is the shape of the output IMAGE: Expand leaves the reference's results['img_shape']
stale, the transforms behind it read results['img'].shape as well.  The generator asserts its own coverage before it writes."""
import ast
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ('RandomShift', 'RandomCrop', 'Expand', 'MinIoURandomCrop', 'CutOut')
MEAN_RGB = (123.675, 116.28, 103.53)


class DrawLog:
    """numpy.random with every call written down."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        f = getattr(np.random, name)

        def logged(*a, **k):
            v = f(*a, **k)
            self.calls.append([name, np.asarray(v).tolist()])
            return v
        return logged


class NumpyWithLog:
    def __init__(self, log):
        self.random = log

    def __getattr__(self, name):
        return getattr(np, name)


def load_reference(root, log):
    g = dict(np=NumpyWithLog(log), random=log)
    path = os.path.join(root, 'mmdet/core/evaluation/bbox_overlaps.py')
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'bbox_overlaps']
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), g)
    path = os.path.join(root, 'mmdet/datasets/pipelines/transforms.py')
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in NAMES]
    assert len(keep) == len(NAMES)
    for n in keep:
        n.decorator_list = []
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), g)
    return {n: g[n] for n in NAMES}


def f32hex(a):
    """float32 values as the hex of their bytes: exact and short."""
    return np.asarray(a, np.float32).tobytes().hex()


def jsonable(kw):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}


def make_args(name, rng, h, w):
    """Constructor arguments of one transform of a chain, sized for an h x w image."""
    if name == 'RandomShift':
        return dict(shift_ratio=[0.5, 0.9, 1.0][rng.randint(3)], max_shift_px=int(rng.randint(2, 10)), filter_thr_px=int(rng.randint(1, 3)))
    if name == 'RandomCrop':
        kind = ('absolute', 'absolute_range', 'relative', 'relative_range')[rng.randint(4)]
        if kind == 'absolute':
            size = [(16, 20), (24, 18), (30, 30)][rng.randint(3)]
        elif kind == 'absolute_range':
            size = [(14, 28), (20, 36)][rng.randint(2)]
        else:
            size = [(0.6, 0.7), (0.8, 0.5), (0.75, 0.75)][rng.randint(3)]
        return dict(crop_size=size, crop_type=kind, allow_negative_crop=bool(rng.randint(4) == 0), bbox_clip_border=bool(rng.randint(4) != 0))
    if name == 'Expand':
        mean = MEAN_RGB if rng.randint(2) else (127.5, 127.5, 127.5)
        return dict(mean=mean, to_rgb=bool(rng.randint(2)), ratio_range=(1, 1.4) if rng.randint(4) else (1.1, 1.7), prob=[0.5, 0.8][rng.randint(2)])
    if name == 'MinIoURandomCrop':
        return dict(min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=[0.3, 0.5][rng.randint(2)], bbox_clip_border=bool(rng.randint(4) != 0))
    if rng.randint(2):
        shape = [(6, 9), [(4, 4), (12, 7), (9, 30)]][rng.randint(2)]
        kw = dict(cutout_shape=shape)
    else:
        kw = dict(cutout_ratio=[(0.3, 0.2), [(0.1, 0.5), (0.45, 0.25)]][rng.randint(2)])
    return dict(n_holes=[2, (1, 4), (0, 3)][rng.randint(3)], fill_in=[(0, 0, 0), (114, 114.9, 7)][rng.randint(2)], **kw)


def build(cls, kw):
    kw = dict(kw)
    for k in ('crop_size', 'mean', 'ratio_range', 'min_ious', 'fill_in'):
        if k in kw:
            kw[k] = tuple(kw[k])
    if isinstance(kw.get('n_holes'), list):
        kw['n_holes'] = tuple(kw['n_holes'])
    for k in ('cutout_shape', 'cutout_ratio'):
        if k in kw:
            v = kw[k]
            kw[k] = [tuple(x) for x in v] if isinstance(v[0], (list, tuple)) else tuple(v)
    return cls(**kw)


def main(root):
    log = DrawLog()
    ref = load_reference(root, log)
    rng = np.random.RandomState(2026)
    pool, cases = [], []
    for _ in range(12):
        h, w = int(rng.randint(12, 41)), int(rng.randint(12, 41))
        pool.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
    cov = dict(modes=set(), no_box_crop=0, expand=set(), shift=set(), shift_early=0, crop_types=set(), cut=set(), cut_right=0, cut_bottom=0,
               rejected=0, random_crop=0)
    plan = [((n,), None) for n in NAMES for _ in range(16)]
    plan += [(('MinIoURandomCrop',), 'none' if q % 2 else 'big') for q in range(20)]      # the high thresholds need one large box (or none)
    plan += [(('RandomShift',), 'none')] * 4                  # no gt box: the early return
    while len(plan) < 104 + 64:
        plan.append((tuple(NAMES[i] for i in rng.randint(0, 5, int(rng.randint(2, 6)))), None))
    for ci, (chain, box_mode) in enumerate(plan):
        pi = int(rng.randint(len(pool)))
        img = pool[pi]
        h, w = img.shape[:2]
        n, k = int(rng.randint(0, 5)), int(rng.randint(0, 3))

        def boxes(m):
            x1, y1 = rng.uniform(0, w * 0.6, m), rng.uniform(0, h * 0.6, m)
            x2, y2 = x1 + rng.uniform(3, w * 0.7, m), y1 + rng.uniform(3, h * 0.7, m)
            return np.stack([x1, y1, np.minimum(x2, w), np.minimum(y2, h)], 1).astype(np.float32).reshape(-1, 4)
        if box_mode is not None:
            n, k = int(box_mode == 'big'), 0
        gtb, gtl, ign = boxes(n), rng.randint(0, 80, n).astype(np.int64), boxes(k)
        if box_mode == 'big':
            gtb = np.array([[w * 0.04, h * 0.05, w * 0.97, h * 0.96]], np.float32)
        args = [jsonable(make_args(name, rng, h, w)) for name in chain]
        seed = 5000 + ci
        res = dict(img=img.copy(), img_shape=img.shape, gt_bboxes=gtb.copy(), gt_labels=gtl.copy(), gt_bboxes_ignore=ign.copy(),
                   bbox_fields=['gt_bboxes_ignore', 'gt_bboxes'])
        np.random.seed(seed)
        log.calls = []
        modes, marks = [], []
        for name, kw in zip(chain, args):
            t = build(ref[name], kw)
            before, shape_in = len(log.calls), res['img'].shape
            res = t(res)
            mine = log.calls[before:]
            if name == 'MinIoURandomCrop':
                modes.append(float(t.mode))
                marks.append(('mode', float(t.mode)))
                if n + k == 0 and len(chain) == 1 and t.mode != 1:
                    marks.append(('no_box_crop', 1))
            if name == 'Expand':
                marks.append(('expand', (len(mine) > 1, len(set(kw['mean'])) == 1)))
            if name == 'RandomShift' and len(mine) == 3:
                dx, dy = mine[1][1], mine[2][1]
                moved = res['img'].shape == shape_in and not np.array_equal(res['img'], img) if len(chain) == 1 else None
                if len(chain) == 1 and dx and dy:
                    marks.append(('shift' if moved else 'shift_early', (dx > 0, dy > 0)))
            if name == 'RandomCrop':
                marks.append(('crop_type', kw['crop_type']))
            if name == 'CutOut':
                marks.append(('cut', 'ratio' if 'cutout_ratio' in kw else 'shape'))
                hh, ww = shape_in[:2]
                for q in range(1, len(mine) - 2, 3):
                    x1, y1, idx = mine[q][1], mine[q + 1][1], mine[q + 2][1]
                    cand = kw.get('cutout_shape', kw.get('cutout_ratio'))
                    cand = cand if isinstance(cand[0], (list, tuple)) else [cand]
                    cw, ch = (int(cand[idx][0] * ww), int(cand[idx][1] * hh)) if 'cutout_ratio' in kw else cand[idx]
                    marks.append(('cut_right', int(x1 + cw > ww)))
                    marks.append(('cut_bottom', int(y1 + ch > hh)))
            if res is None:
                break
        has_rc = 'RandomCrop' in chain
        if res is None and cov['rejected'] >= 10:
            continue                   # enough rejected cases: keep them a small share of the RandomCrop cases
        cov['random_crop'] += int(has_rc)
        cov['rejected'] += int(res is None)
        for key, v in marks:
            if key == 'mode':
                cov['modes'].add(v)
            elif key in ('expand', 'shift'):
                cov[key].add(v)
            elif key == 'crop_type':
                cov['crop_types'].add(v)
            elif key == 'cut':
                cov['cut'].add(v)
            else:
                cov[key] += 1 if key in ('no_box_crop', 'shift_early') else v
        next_draw = float(np.random.random())
        out = dict(none=res is None, next_draw=next_draw, modes=modes, n_draws=len(log.calls), last_draws=list(log.calls[-4:]))
        if res is not None:
            oi = np.ascontiguousarray(res['img'])
            assert oi.dtype == np.uint8
            assert res['gt_bboxes'].dtype == np.float32 and res['gt_bboxes_ignore'].dtype == np.float32
            out.update(img_sha256=hashlib.sha256(oi.tobytes()).hexdigest(), img_shape=list(oi.shape), gt_bboxes=f32hex(res['gt_bboxes']),
                       gt_labels=np.asarray(res['gt_labels']).tolist(), gt_bboxes_ignore=f32hex(res['gt_bboxes_ignore']))
        cases.append(dict(seed=seed, chain=[[name, kw] for name, kw in zip(chain, args)],
                          input=dict(image=pi, gt_bboxes=f32hex(gtb), gt_labels=gtl.tolist(), gt_bboxes_ignore=f32hex(ign)), output=out))
    # coverage
    assert cov['modes'] == {1.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.0}, cov['modes']
    assert cov['no_box_crop'] >= 1
    assert cov['expand'] == {(a, b) for a in (True, False) for b in (True, False)}, cov['expand']
    assert cov['shift'] == {(a, b) for a in (True, False) for b in (True, False)} and cov['shift_early'] >= 1, cov
    assert cov['crop_types'] == {'absolute', 'absolute_range', 'relative', 'relative_range'}
    assert cov['cut'] == {'shape', 'ratio'} and cov['cut_right'] >= 1 and cov['cut_bottom'] >= 1
    assert 8 <= cov['rejected'] <= cov['random_crop'] // 4, (cov['rejected'], cov['random_crop'])
    assert any(len(c['chain']) == m for c in cases for m in (5,)) and sum(len(c['chain']) == 1 for c in cases) >= 80
    doc = dict(pool=[dict(shape=list(p.shape), hex=p.tobytes().hex()) for p in pool], cases=cases)
    path = os.path.join(HERE, 'geo_transforms.json')
    with open(path, 'w') as f:           # one pool image / one case per line
        f.write('{"pool":[\n' + ',\n'.join(json.dumps(p, separators=(',', ':')) for p in doc['pool']) + '\n],"cases":[\n' +
                ',\n'.join(json.dumps(c, separators=(',', ':')) for c in cases) + '\n]}\n')
    print('wrote', path, len(cases), 'cases,', cov['rejected'], 'rejected of', cov['random_crop'], 'RandomCrop cases,',
          os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ['DSL_REFERENCE'])

"""dsl_image_geo on the GPU against the numpy model tests/geo_ref.py, bit for bit, through the C ABI; then the golden chains of the
reference's own transforms (tests/golden/geo_transforms.json) rendered by the kernel, and GpuBatchPipeline with the geometric
transforms in front of Resize and behind RandomFlip against the same composition on the host models."""
import ctypes
import random

import numpy as np
import pytest
import torch

import geo_ref
from geo_ref import CROP, CUTOUT, EXPAND, SHIFT
from oracle import datapath_oracle as DO

pytestmark = pytest.mark.gpu
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def run_geo(jobs):
    """jobs: dicts(img, steps[, dst_hw, src_ld, dst_ld]).  One dsl_image_geo launch; every destination is pre-filled with 7 and checked
    against geo_ref inside its dst_h x dst_w rectangle (zero margin included) and for being untouched beyond it."""
    from dsl_amd import _lib as L
    n = len(jobs)
    its = (L.GeoItem * n)()
    keep = []
    for it, j in zip(its, jobs):
        img = j['img']
        h, w = img.shape[:2]
        oh, ow = L.geo_out_size(j['steps'], h, w)
        dh, dw = j.get('dst_hw', (oh, ow))
        sld, dld = j.get('src_ld', w), j.get('dst_ld', dw)
        src = np.full((h, sld, 3), 201, np.uint8)
        src[:, :w] = img
        ts, td = torch.from_numpy(src).cuda(), torch.full((dh + 1, dld, 3), 7, dtype=torch.uint8, device='cuda')
        keep.append((ts, td, dh, dw))
        L.geo_fill_item(it, j['steps'], ts.data_ptr(), h, w, sld, td.data_ptr(), dh, dw, dld)
    tab = torch.frombuffer(bytearray(bytes(its)), dtype=torch.uint8).cuda()
    L.check(L.lib.dsl_image_geo(ctypes.cast(its, ctypes.c_void_p), L.ptr(tab), n, max(k[2] for k in keep), max(k[3] for k in keep),
                                L.stream_ptr()), 'dsl_image_geo')
    torch.cuda.synchronize()
    for q, (j, (_, td, dh, dw)) in enumerate(zip(jobs, keep)):
        got = td.cpu().numpy()
        want = geo_ref.render_into(j['img'], j['steps'], dh, dw)
        assert np.array_equal(got[:dh, :dw], want), (q, j['steps'], j['img'].shape)
        assert (got[:dh, dw:] == 7).all() and (got[dh:] == 7).all(), (q, 'written outside the dst rectangle')


def edge_lists(h, w):
    """The step lists of the issue for an h x w image."""
    f1, f2 = (11, 22, 33), (250, 0, 128)
    lists = [[],                                                                     # a copy
             [(CROP, (w - 1, h - 1, 1, 1))], [(CROP, (w // 2, h // 3, 1, 1))],       # to a single pixel
             [(EXPAND, (0, 0, w + 3, h + 2), f1)], [(EXPAND, (5, 4, w + 5, h + 4), f2)],      # at the origin, at the far corner
             [(SHIFT, (w - 1, h - 1))], [(SHIFT, (-(w - 1), -(h - 1)))], [(SHIFT, (w - 1, -(h - 1)))], [(SHIFT, (-(w - 1), h - 1))],
             [(SHIFT, (0, 0))],
             # cutouts touching every edge, overlapping each other; a later fill wins
             [(CUTOUT, (0, 0, max(w // 2, 1), 1), f1), (CUTOUT, (0, 0, 1, h), f2), (CUTOUT, (w - 1, 0, w, h), f1), (CUTOUT, (0, h - 1, w, h), f2),
              (CUTOUT, (w // 3, h // 3, w, h), f1), (CUTOUT, (w // 2, h // 2, w, h), f2), (CUTOUT, (0, 0, w, h // 4), (0, 0, 0))],
             # every kind in one walk, sizes changing in between
             [(CUTOUT, (0, 0, (w + 1) // 2, (h + 1) // 2), f1), (EXPAND, (2, 1, w + 4, h + 3), f2), (SHIFT, (1, -1)),
              (CROP, (1, 0, w + 2, h + 2)), (CUTOUT, (w, h, w + 2, h + 2), f1), (SHIFT, (-(w + 1), 0)), (EXPAND, (0, 3, w + 2, h + 5), f1)]]
    return lists


@pytest.mark.parametrize('h, w', [(1, 1), (7, 5), (19, 27), (40, 23)])
def test_steps_match_the_model(h, w):
    rng = np.random.RandomState(h * 100 + w)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    jobs = [dict(img=img, steps=s) for s in edge_lists(h, w)]
    # dst larger than the output (the zero margin), and row pitches wider than the images
    jobs += [dict(img=img, steps=s, dst_hw=(L0 + 3, L1 + 6), src_ld=w + 5, dst_ld=L1 + 11)
             for s in edge_lists(h, w) for (L0, L1) in [geo_size(s, h, w)]]
    run_geo(jobs)


def geo_size(steps, h, w):
    from dsl_amd import _lib as L
    return L.geo_out_size(steps, h, w)


def test_more_than_one_block_per_row():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (7, 5, 3)).astype(np.uint8)
    wide = rng.randint(0, 256, (3, 700, 3)).astype(np.uint8)
    run_geo([dict(img=img, steps=[(EXPAND, (258, 1, 530, 9), (1, 2, 3)), (CUTOUT, (250, 0, 262, 4), (9, 8, 7))]),
             dict(img=wide, steps=[(SHIFT, (-300, 1)), (CROP, (100, 0, 520, 3))], dst_hw=(4, 600)),
             dict(img=wide, steps=[], src_ld=701, dst_ld=777)])


def test_full_list_and_refusal_of_a_longer_one():
    from dsl_amd import _lib as L
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (19, 27, 3)).astype(np.uint8)
    steps, h, w = [], 19, 27
    for k in range(32):          # 32 steps: crops and expands alternate around shifts and cutouts, the size keeps changing
        kind = (CUTOUT, SHIFT, EXPAND, CROP)[k % 4]
        if kind == CUTOUT:
            x1, y1 = int(rng.randint(0, w)), int(rng.randint(0, h))
            steps.append((CUTOUT, (x1, y1, min(x1 + 5, w), min(y1 + 4, h)), tuple(int(v) for v in rng.randint(0, 256, 3))))
        elif kind == SHIFT:
            steps.append((SHIFT, (int(rng.randint(-3, 4)), int(rng.randint(-3, 4)))))
        elif kind == EXPAND:
            steps.append((EXPAND, (int(rng.randint(0, 3)), int(rng.randint(0, 3)), w + 4, h + 3), (k, 2 * k, 255 - k)))
            h, w = h + 3, w + 4
        else:
            steps.append((CROP, (int(rng.randint(0, 4)), int(rng.randint(0, 3)), w - 3, h - 2)))
            h, w = h - 2, w - 3
    assert len(steps) == L.GEO_MAX_STEPS
    run_geo([dict(img=img, steps=steps), dict(img=img, steps=[(CUTOUT, (k % 27, k % 19, 27, 19), (k, k, k)) for k in range(32)])])
    # one step more: refused through dsl_last_error(), nothing is launched
    it = (L.GeoItem * 1)()
    src, dst = torch.from_numpy(img).cuda(), torch.full((19, 27, 3), 7, dtype=torch.uint8, device='cuda')
    L.geo_fill_item(it[0], [(CUTOUT, (0, 0, 1, 1), (1, 1, 1))] * 33, src.data_ptr(), 19, 27, 27, dst.data_ptr(), 19, 27, 27)
    tab = torch.frombuffer(bytearray(bytes(it)), dtype=torch.uint8).cuda()
    rc = L.lib.dsl_image_geo(ctypes.cast(it, ctypes.c_void_p), L.ptr(tab), 1, 19, 27, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b'nsteps' in L.lib.dsl_last_error() and (dst == 7).all()


def test_batch_of_different_sizes_and_list_lengths():
    rng = np.random.RandomState(5)
    imgs = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((7, 5), (40, 23), (19, 27))]
    run_geo([dict(img=imgs[0], steps=[], dst_hw=(9, 9)),
             dict(img=imgs[1], steps=edge_lists(40, 23)[-1]),
             dict(img=imgs[2], steps=[(CROP, (3, 2, 20, 10)), (CUTOUT, (0, 0, 4, 10), (5, 6, 7))], src_ld=31, dst_ld=64, dst_hw=(12, 33))])


def test_golden_chains_rendered_by_the_kernel():
    """Every chain of the reference's own transforms: the steps the product recorded, rendered by the kernel, give the reference's image."""
    from dsl_amd import _lib as L
    from test_geo_transforms_cpu import all_results, golden, same_image
    doc = golden()
    its, want, keep = [], [], []
    for case, (r, _, _, _) in zip(doc['cases'], all_results()):
        if r is None:
            continue
        img = doc['images'][case['input']['image']]
        o = case['output']
        want.append(o)
        oh, ow = o['img_shape'][:2]
        ts, td = torch.from_numpy(img.copy()).cuda(), torch.full((oh, ow, 3), 7, dtype=torch.uint8, device='cuda')
        keep.append((ts, td))
        its.append((r.get('_geo', []), ts.data_ptr(), img.shape[0], img.shape[1], img.shape[1], td.data_ptr(), oh, ow, ow))
    tab_h = (L.GeoItem * len(its))()
    for it, a in zip(tab_h, its):
        L.geo_fill_item(it, *a)
    tab = torch.frombuffer(bytearray(bytes(tab_h)), dtype=torch.uint8).cuda()
    L.check(L.lib.dsl_image_geo(ctypes.cast(tab_h, ctypes.c_void_p), L.ptr(tab), len(its), max(a[6] for a in its), max(a[7] for a in its),
                                L.stream_ptr()), 'dsl_image_geo')
    torch.cuda.synchronize()
    bad = [q for q, ((_, td), w) in enumerate(zip(keep, want)) if not same_image(td.cpu().numpy(), w)]
    assert len(want) >= 140 and not bad, bad


def _samples(rng, sizes):
    out = []
    for i, (h, w) in enumerate(sizes):
        n = int(rng.randint(1, 5))
        x1, y1 = rng.uniform(0, w * 0.4, n), rng.uniform(0, h * 0.4, n)
        b = np.stack([x1, y1, x1 + rng.uniform(w * 0.3, w * 0.6, n), y1 + rng.uniform(h * 0.3, h * 0.6, n)], 1).astype(np.float32)
        out.append(dict(img=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_bboxes=b, gt_labels=rng.randint(0, 80, n),
                        gt_bboxes_ignore=b[:1] + 1, filename=f'im{i}.jpg'))
    return out


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_chain_in_front_of_resize(seed):
    """Expand -> MinIoURandomCrop -> Resize -> RandomFlip -> Normalize -> Pad: the oracle's resize / flip / normalize / pad applied to the
    model's rendering of the recorded steps, bit for bit."""
    from dsl_amd.datapath import GpuBatchPipeline
    pipe = GpuBatchPipeline([dict(type='Expand', mean=NORM['mean'], to_rgb=True, ratio_range=(1, 2.5)), dict(type='MinIoURandomCrop'),
                             dict(type='Resize', img_scale=[(200, 120), (200, 150)], multiscale_mode='value', keep_ratio=True),
                             dict(type='RandomFlip', flip_ratio=0.5), dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32)])
    samples = _samples(np.random.RandomState(seed), [(97, 131), (64, 64), (120, 50), (33, 77)])
    np.random.seed(40 + seed)
    random.seed(50 + seed)
    batch = pipe(samples)
    torch.cuda.synchronize()
    spec, stepped = [], 0
    for s, m, (pre, post) in zip(samples, batch['img_metas'], pipe.last_geo):
        assert post == []
        stepped += len(pre)
        spec.append(dict(img=geo_ref.render(s['img'], pre), scale=(200, 120) if m['scale_idx'] == 0 else (200, 150), ps=None, flip=m['flip']))
    want, shapes = DO.prepare_batch(spec, NORM['mean'], NORM['std'], True, 32)
    got = batch['img'].cpu().numpy()
    assert stepped >= 2 and got.shape == want.shape and [m['img_shape'][:2] for m in batch['img_metas']] == [tuple(s) for s in shapes]
    assert np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_chain_behind_random_flip(seed):
    """Resize -> PatchShuffle -> RandomFlip -> RandomCrop -> CutOut -> UBAug -> Normalize -> Pad(size=): the same composition on the host
    models, the augmentation passes replayed as tests/test_augment_gpu.py does (equal outside UBAug's erased rectangles)."""
    from test_augment_gpu import _replay
    from dsl_amd.datapath import GpuBatchPipeline
    pipe = GpuBatchPipeline([dict(type='Resize', img_scale=[(200, 120), (200, 150)], multiscale_mode='value', keep_ratio=True),
                             dict(type='PatchShuffle', ratio=0.5, ranges=[0.0, 1.0], mode=['flip', 'flop']),
                             dict(type='RandomFlip', flip_ratio=0.5),
                             dict(type='RandomCrop', crop_size=(90, 110), allow_negative_crop=True),
                             dict(type='CutOut', n_holes=(2, 6), cutout_shape=[(10, 14), (31, 7)], fill_in=(114, 114, 114)),
                             dict(type='UBAug'), dict(type='Normalize', **NORM), dict(type='Pad', size=(96, 128))])
    samples = _samples(np.random.RandomState(10 + seed), [(97, 131), (64, 64), (120, 50), (150, 200)])
    np.random.seed(60 + seed)
    random.seed(70 + seed)
    batch = pipe(samples)
    torch.cuda.synchronize()
    got = batch['img'].cpu().numpy()
    assert got.shape == (4, 3, 96, 128)
    n_pass = 0
    for i, (s, m) in enumerate(zip(samples, batch['img_metas'])):
        scale = (200, 120) if m['scale_idx'] == 0 else (200, 150)
        img = DO.resize_bilinear_u8(s['img'], DO.rescale_size((s['img'].shape[1], s['img'].shape[0]), scale))
        if m['PS']:
            img = DO.patch_shuffle_image(img, m['PS_place'], m['PS_mode'])
        if m['flip']:
            img = img[:, ::-1]
        pre, post = pipe.last_geo[i]
        assert pre == [] and any(st[0] == CUTOUT for st in post)
        img = geo_ref.render(np.ascontiguousarray(img), post)
        h, w = img.shape[:2]
        assert m['img_shape'] == (h, w, 3) and m['pad_shape'] == (96, 128, 3) and h <= 90 and w <= 110
        n_pass += len(pipe.last_passes[i])
        img, erased = _replay(img, pipe.last_passes[i])
        want = DO.imnormalize(img, NORM['mean'], NORM['std'], NORM['to_rgb']).transpose(2, 0, 1)
        g = got[i, :, :h, :w]
        assert np.array_equal(g[:, ~erased], want[:, ~erased]), (i, post)
        assert (got[i, :, h:] == 0).all() and (got[i, :, :, w:] == 0).all()
    assert n_pass > 0


def test_lists_longer_than_one_launch():
    """More steps than DSL_GEO_MAX_STEPS on both sides of Resize: successive launches over two buffers, sizes changing in between."""
    from dsl_amd.datapath import GpuBatchPipeline
    holes = dict(type='CutOut', n_holes=30, cutout_shape=[(5, 3), (2, 9)], fill_in=(1, 2, 3))
    pipe = GpuBatchPipeline([holes, dict(type='Expand', mean=(10, 20, 30), prob=1.0, ratio_range=(1.2, 1.6)), holes,
                             dict(type='RandomCrop', crop_size=(0.8, 0.8), crop_type='relative', allow_negative_crop=True), holes,
                             dict(type='Resize', img_scale=(120, 90), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
                             holes, dict(type='RandomShift', shift_ratio=1.0, max_shift_px=6), holes,
                             dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32)])
    samples = _samples(np.random.RandomState(21), [(50, 70), (64, 40)])
    samples.append(dict(samples[0], gt_bboxes=np.zeros((0, 4), np.float32), gt_labels=np.zeros((0,), np.int64)))
    np.random.seed(22)
    batch = pipe(samples)
    torch.cuda.synchronize()
    got = batch['img'].cpu().numpy()
    assert max(len(pre) for pre, _ in pipe.last_geo) > 64 and max(len(post) for _, post in pipe.last_geo) > 32
    for i, (s, m) in enumerate(zip(samples, batch['img_metas'])):
        pre, post = pipe.last_geo[i]
        img = geo_ref.render(s['img'], pre)
        img = DO.resize_bilinear_u8(img, DO.rescale_size((img.shape[1], img.shape[0]), (120, 90)))
        img = geo_ref.render(np.ascontiguousarray(img[:, ::-1] if m['flip'] else img), post)
        h, w = img.shape[:2]
        want = DO.imnormalize(img, NORM['mean'], NORM['std'], True).transpose(2, 0, 1)
        assert m['img_shape'] == (h, w, 3) and np.array_equal(got[i, :, :h, :w], want), i
        assert (got[i, :, h:] == 0).all() and (got[i, :, :, w:] == 0).all()


def test_pipeline_without_geometric_transforms_is_untouched():
    from dsl_amd.datapath import GpuBatchPipeline
    pipe = GpuBatchPipeline([dict(type='Resize', img_scale=(120, 90), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
                             dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32)])
    assert pipe._geo_split is None
    np.random.seed(1)
    pipe(_samples(np.random.RandomState(2), [(50, 70)]))
    torch.cuda.synchronize()
    assert pipe.last_geo == [([], [])] and len(pipe._keep[0]) == 1      # the upload alone: no canvas, no table but dsl_image_prep's


def test_geometric_batch_feeds_the_training_step():
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.datapath import GpuBatchPipeline
    from dsl_amd.registry import build_detector
    from util import fcos_model_cfg
    from oracle import fcos_oracle as O
    pipe = [dict(type='Expand', mean=NORM['mean'], ratio_range=(1, 2)), dict(type='MinIoURandomCrop', min_crop_size=0.5),
            dict(type='Resize', img_scale=[(200, 120), (200, 150)], multiscale_mode='value', keep_ratio=True),
            dict(type='PatchShuffle', ratio=0.5, ranges=[0.0, 1.0], mode=['flip', 'flop']), dict(type='RandomFlip', flip_ratio=0.5),
            dict(type='RandomShift', max_shift_px=8), dict(type='CutOut', n_holes=(1, 3), cutout_ratio=(0.1, 0.1)),
            dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32)]
    np.random.seed(3)
    random.seed(4)
    gp = GpuBatchPipeline(pipe)
    batch = gp(_samples(np.random.RandomState(9), [(96, 128), (120, 90)]))
    assert sum(len(a) + len(b) for a, b in gp.last_geo) > 0
    model = build_detector(fcos_model_cfg())
    model.load_state_dict(O.synth_state_dict(0))
    model = model.cuda()
    losses = model.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'], batch['gt_bboxes_ignore'])
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v.detach())) for v in losses.values()) and torch.isfinite(model.store.grad).all()

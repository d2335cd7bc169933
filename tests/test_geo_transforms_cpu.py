"""RandomShift, RandomCrop, Expand, MinIoURandomCrop and CutOut (dsl_amd/datapath.py) against the reference's own classes
(tests/golden/geo_transforms.json, written by tests/golden/make_golden_geo.py): seeded the same way, the product's transforms give
the reference's boxes, labels, image shape, rejection and np.random draws with ==, and the step list they record renders - on the
numpy model tests/geo_ref.py - to the reference's image byte for byte.  Plus the position rules of GpuBatchPipeline, Pad(size=),
the resample / SampleRejected protocol and dsl_image_geo's host-side refusals.  No GPU."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import geo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
_CACHE = {}


def golden():
    if 'doc' not in _CACHE:
        doc = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'geo_transforms.json')))
        doc['images'] = [np.frombuffer(bytes.fromhex(p['hex']), np.uint8).reshape(p['shape']) for p in doc['pool']]
        _CACHE['doc'] = doc
    return _CACHE['doc']


def f32(hexed):
    """Boxes are stored as the hex of their float32 bytes."""
    return np.frombuffer(bytes.fromhex(hexed), np.float32).reshape(-1, 4)


def same_image(img, o):
    return list(img.shape) == o['img_shape'] and hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == o['img_sha256']


def ctor_args(kw):
    """JSON lists back to the tuples the constructors test for (n_holes pair, candidate lists of pairs)."""
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
    return kw


def build_chain(chain):
    from dsl_amd.datapath import PIPELINES
    return [PIPELINES.build(dict(type=name, **ctor_args(kw))) for name, kw in chain]


class Draws:
    """np.random's drawing functions wrapped to write every call down (name, value), as the generator did for the reference."""
    NAMES = ('random', 'randint', 'uniform', 'choice', 'rand')

    def __enter__(self):
        self.calls, self.saved = [], {n: getattr(np.random, n) for n in self.NAMES}
        for n, f in self.saved.items():
            def logged(*a, _f=f, _n=n, **k):
                v = _f(*a, **k)
                self.calls.append([_n, np.asarray(v).tolist()])
                return v
            setattr(np.random, n, logged)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(np.random, n, f)


def run_product(case):
    """The product's transforms on one golden case: (result or None, modes, draws, next draw)."""
    doc = golden()
    img = doc['images'][case['input']['image']]
    r = dict(img_shape=tuple(img.shape), gt_bboxes=f32(case['input']['gt_bboxes']).copy(),
             gt_labels=np.asarray(case['input']['gt_labels'], np.int64).reshape(-1), gt_bboxes_ignore=f32(case['input']['gt_bboxes_ignore']).copy(),
             bbox_fields=['gt_bboxes_ignore', 'gt_bboxes'])
    ts = build_chain(case['chain'])
    np.random.seed(case['seed'])
    modes = []
    with Draws() as d:
        for t in ts:
            r = t(r)
            if type(t).__name__ == 'MinIoURandomCrop':
                modes.append(float(t.mode))
            if r is None:
                break
    return r, modes, d.calls, float(np.random.random())


def all_results():
    if 'runs' not in _CACHE:
        _CACHE['runs'] = [run_product(c) for c in golden()['cases']]
    return _CACHE['runs']


def test_golden_file_covers_what_it_should():
    cases = golden()['cases']
    assert len(cases) >= 150 and sum(c['output']['none'] for c in cases) >= 8
    assert {len(c['chain']) for c in cases} >= {1, 2, 3, 4, 5}
    assert {n for c in cases for n, _ in c['chain']} == {'RandomShift', 'RandomCrop', 'Expand', 'MinIoURandomCrop', 'CutOut'}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'geo_transforms.json')) < 1 << 20


def test_transforms_match_the_reference():
    bad = []
    for ci, (case, (r, modes, draws, nxt)) in enumerate(zip(golden()['cases'], all_results())):
        o = case['output']
        ok = (r is None) == o['none'] and modes == o['modes'] and len(draws) == o['n_draws'] and draws[-4:] == o['last_draws'] \
            and nxt == o['next_draw']
        if ok and r is not None:
            ok = list(r['img_shape']) == o['img_shape'] and r['gt_labels'].tolist() == o['gt_labels'] \
                and all(r[k].dtype == np.float32 and r[k].tolist() == f32(o[k]).tolist() for k in ('gt_bboxes', 'gt_bboxes_ignore'))
        if not ok:
            bad.append((ci, [n for n, _ in case['chain']]))
    assert not bad, bad


def test_recorded_steps_render_the_reference_image():
    doc = golden()
    bad, rendered = [], 0
    for ci, (case, (r, _, _, _)) in enumerate(zip(doc['cases'], all_results())):
        if r is None:
            continue
        img = doc['images'][case['input']['image']]
        rendered += int(len(r.get('_geo', [])) > 0)
        if not same_image(geo_ref.render(img, r.get('_geo', [])), case['output']):
            bad.append(ci)
    assert not bad and rendered >= 80, (bad, rendered)


def test_expand_fill_is_the_mean_in_bgr_truncated():
    from dsl_amd.datapath import Expand
    np.random.seed(0)
    r = Expand(mean=(123.675, 116.28, 103.53), to_rgb=True, prob=1.0)(dict(img_shape=(10, 10, 3), bbox_fields=[]))
    assert r['_geo'][0][2] == (103, 116, 123)
    r = Expand(mean=(123.675, 116.28, 103.53), to_rgb=False, prob=1.0)(dict(img_shape=(10, 10, 3), bbox_fields=[]))
    assert r['_geo'][0][2] == (123, 116, 103)


def test_random_shift_refuses_a_shift_of_the_image_size():
    from dsl_amd.datapath import RandomShift
    t = RandomShift(shift_ratio=1.0, max_shift_px=64, filter_thr_px=-100)      # (the threshold keeps the clipped boxes: no early return)
    hit = 0
    for seed in range(20):
        np.random.seed(seed)
        r = dict(img_shape=(8, 8, 3), gt_bboxes=np.array([[1, 1, 5, 5]], np.float32), gt_labels=np.array([1]), bbox_fields=['gt_bboxes'])
        try:
            t(r)
        except ValueError:
            hit += 1
            assert '_geo' not in r
    assert hit >= 10


def test_constructor_assertions():
    from dsl_amd.datapath import CutOut, RandomCrop, RandomShift
    with pytest.raises(ValueError):
        RandomCrop((10, 10), crop_type='nope')
    with pytest.raises(AssertionError):
        RandomCrop((0.5, 10), crop_type='absolute')
    with pytest.raises(AssertionError):
        RandomCrop((1.5, 0.5), crop_type='relative')
    with pytest.raises(AssertionError):
        CutOut(1, cutout_shape=(2, 2), cutout_ratio=(0.1, 0.1))
    with pytest.raises(AssertionError):
        CutOut((3, 2), cutout_shape=(2, 2))
    with pytest.raises(AssertionError):
        RandomShift(shift_ratio=1.5)


# ---- GpuBatchPipeline: positions, Pad(size=), rejection -------------------------------------------------------------------------
RESIZE = dict(type='Resize', img_scale=(64, 48), keep_ratio=True)
FLIP = dict(type='RandomFlip', flip_ratio=0.5)
CROP = dict(type='RandomCrop', crop_size=(16, 20))
CUT = dict(type='CutOut', n_holes=2, cutout_shape=(4, 4))
NORMALIZE = dict(type='Normalize', **NORM)


def test_supported_positions_build():
    from dsl_amd.datapath import GpuBatchPipeline
    p = GpuBatchPipeline([dict(type='Expand', mean=NORM['mean']), dict(type='MinIoURandomCrop'), RESIZE, FLIP, NORMALIZE,
                          dict(type='Pad', size_divisor=32)], device='cpu')
    assert p._geo_split == 2
    p = GpuBatchPipeline([RESIZE, dict(type='PatchShuffle', ratio=0.5), FLIP, CROP, CUT, dict(type='RandomShift'), dict(type='UBAug'),
                          NORMALIZE, dict(type='Pad', size=(32, 32))], device='cpu')
    assert p._geo_split == 0
    assert GpuBatchPipeline([RESIZE, CROP, NORMALIZE], device='cpu')._geo_split == 0          # behind Resize, no flip at all
    assert GpuBatchPipeline([RESIZE, FLIP, NORMALIZE], device='cpu')._geo_split is None


@pytest.mark.parametrize('pipe, name, where', [
    ([RESIZE, CROP, FLIP, NORMALIZE], 'RandomCrop', 'between Resize and RandomFlip'),
    ([RESIZE, CUT, dict(type='PatchShuffle', ratio=0.5), NORMALIZE], 'CutOut', 'between Resize and PatchShuffle'),
    ([RESIZE, FLIP, NORMALIZE, CUT], 'CutOut', 'after Normalize'),
    ([RESIZE, FLIP, dict(type='UBAug'), dict(type='RandomShift'), NORMALIZE], 'RandomShift', 'after the augmentation passes'),
    ([CROP, RESIZE, FLIP, RESIZE, NORMALIZE], 'Resize', 'second Resize'),
    ([FLIP, CROP, RESIZE, NORMALIZE], 'Resize', 'position 2'),
])
def test_other_positions_are_refused_at_construction(pipe, name, where):
    from dsl_amd.datapath import GpuBatchPipeline
    with pytest.raises(NotImplementedError) as e:
        GpuBatchPipeline(pipe, device='cpu')
    assert str(e.value).startswith(name + ' at position') and where in str(e.value), str(e.value)


def test_pad_to_a_fixed_size():
    from dsl_amd.datapath import Pad
    r = Pad(size=(40, 64))(dict(img_shape=(33, 50, 3)))
    assert r['pad_shape'] == (40, 64, 3) and r['pad_fixed_size'] == (40, 64) and r['pad_size_divisor'] is None
    with pytest.raises(AssertionError):
        Pad(size=(32, 64))(dict(img_shape=(33, 50, 3)))
    with pytest.raises(AssertionError):
        Pad(size=(32, 32), size_divisor=32)
    with pytest.raises(AssertionError):
        Pad(size=(32, 32), pad_val=1)
    assert Pad(size_divisor=32)(dict(img_shape=(33, 50, 3)))['pad_shape'] == (64, 64, 3)


def _sample(h, w, boxes):
    return dict(img=np.zeros((h, w, 3), np.uint8), gt_bboxes=np.asarray(boxes, np.float32).reshape(-1, 4),
                gt_labels=np.arange(len(boxes)), filename=f'{h}x{w}.jpg')


def test_rejection_resample_and_sample_rejected():
    from dsl_amd.datapath import GpuBatchPipeline, SampleRejected, META_KEYS
    pipe = GpuBatchPipeline([RESIZE, FLIP, CROP, CUT, NORMALIZE, dict(type='Pad', size=(32, 32))], device='cpu')
    good, empty = _sample(48, 64, [[0, 0, 64, 48]]), _sample(48, 64, [])
    np.random.seed(1)
    assert pipe.draw(empty, 48, 64) is None
    with pytest.raises(SampleRejected) as e:
        pipe.draw_batch([good, empty, good])
    assert e.value.index == 1
    asked = []

    def resample(i):
        asked.append(i)
        return empty if len(asked) < 3 else good
    imgs, results = pipe.draw_batch([good, empty], resample)
    assert asked == [1, 1, 1] and len(results) == 2 and all(r is not None for r in results)
    r = results[1]
    assert r['img_shape'] == (16, 20, 3) and r['_prep_shape'] == (48, 64, 3) and r['pad_shape'] == (32, 32, 3)
    assert r['_geo'][0][0] == geo_ref.CROP and r['_geo_pre'] == []
    meta = pipe.meta(r, 32, 32)
    assert not any(k.startswith('_') for k in meta) and '_geo' not in META_KEYS and meta['img_shape'] == (16, 20, 3)


def test_steps_in_front_of_resize_are_kept_apart():
    from dsl_amd.datapath import GpuBatchPipeline
    pipe = GpuBatchPipeline([dict(type='Expand', mean=NORM['mean'], prob=1.0, ratio_range=(1.5, 2)), RESIZE, FLIP, CUT, NORMALIZE,
                             dict(type='Pad', size_divisor=32)], device='cpu')
    np.random.seed(3)
    r = pipe.draw(_sample(30, 40, [[5, 5, 20, 20]]), 30, 40)
    assert [s[0] for s in r['_geo_pre']] == [geo_ref.EXPAND] and [s[0] for s in r['_geo']] == [geo_ref.CUTOUT] * 2
    big_w, big_h = r['_geo_pre'][0][1][2:]
    assert r['ori_shape'] == (30, 40, 3) and r['_prep_shape'] == r['img_shape']
    sf = min(64 / max(big_h, big_w), 48 / min(big_h, big_w))
    assert r['img_shape'][:2] == (int(big_h * sf + 0.5), int(big_w * sf + 0.5))


# ---- the C ABI of dsl_image_geo ---------------------------------------------------------------------------------------------
def test_geo_structs_match_the_header(tmp_path):
    from dsl_amd import _lib as L
    pairs = [('dsl_geo_step', L.GeoStep, 'fill'), ('dsl_geo_item', L.GeoItem, 'steps'), ('dsl_geo_item', L.GeoItem, 'dst')]
    body = ''.join(f'  printf("%zu %zu\\n", sizeof({c}), offsetof({c}, {f}));\n' for c, _, f in pairs)
    src = tmp_path / 'sizes.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsl_hip.h"\nint main(void) {\n' + body +
                   '  printf("%d %d %d %d %d\\n", DSL_GEO_CROP, DSL_GEO_EXPAND, DSL_GEO_SHIFT, DSL_GEO_CUTOUT, DSL_GEO_MAX_STEPS);\n  return 0;\n}\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    for i, (c, t, f) in enumerate(pairs):
        assert ctypes.sizeof(t) == int(out[2 * i]) and getattr(t, f).offset == int(out[2 * i + 1]), (c, f)
    assert [int(v) for v in out[6:]] == [L.GEO_CROP, L.GEO_EXPAND, L.GEO_SHIFT, L.GEO_CUTOUT, L.GEO_MAX_STEPS]
    assert (geo_ref.CROP, geo_ref.EXPAND, geo_ref.SHIFT, geo_ref.CUTOUT) == (L.GEO_CROP, L.GEO_EXPAND, L.GEO_SHIFT, L.GEO_CUTOUT)


def _refused(L, steps, src=0x1000, dst=0x2000, src_hw=(10, 12), dst_hw=None, src_ld=None, dst_ld=None, tab=0x3000, n=1, fix=None):
    """dsl_image_geo on a table the host-side check must refuse: nothing is launched (the addresses are never touched)."""
    it = (L.GeoItem * 1)()
    oh, ow = L.geo_out_size(steps, *src_hw)
    dh, dw = dst_hw or (oh, ow)
    L.geo_fill_item(it[0], steps, src, src_hw[0], src_hw[1], src_ld or src_hw[1], dst, dh, dw, dst_ld or dw)
    if fix:
        fix(it[0])
    rc = L.lib.dsl_image_geo(ctypes.cast(it, ctypes.c_void_p), ctypes.c_void_p(tab), n, max(dh, 1), max(dw, 1), None)
    assert rc != 0
    return L.lib.dsl_last_error().decode()


def test_entry_refuses_bad_tables_on_the_host():
    from dsl_amd import _lib as L
    cut = (L.GEO_CUTOUT, (1, 1, 3, 3), (9, 9, 9))
    assert 'nsteps' in _refused(L, [cut] * 33)
    assert 'null' in _refused(L, [cut], src=0)
    assert 'null' in _refused(L, [cut], dst=0)
    assert 'src == dst' in _refused(L, [cut], dst=0x1000)
    assert 'bad arguments' in _refused(L, [cut], tab=0)
    assert 'bad arguments' in _refused(L, [cut], n=0)
    assert 'non-positive' in _refused(L, [cut], fix=lambda it: setattr(it, 'src_h', 0))
    assert 'pitch' in _refused(L, [cut], src_ld=11)
    assert 'pitch' in _refused(L, [cut], dst_ld=11)
    assert 'smaller than the output' in _refused(L, [cut], dst_hw=(9, 12))
    assert 'CROP outside' in _refused(L, [(L.GEO_CROP, (5, 0, 8, 10))])
    assert 'CROP outside' in _refused(L, [(L.GEO_CROP, (0, -1, 8, 10))])
    assert 'EXPAND' in _refused(L, [(L.GEO_EXPAND, (3, 0, 14, 10), (0, 0, 0))])
    assert 'SHIFT' in _refused(L, [(L.GEO_SHIFT, (12, 0))])
    assert 'SHIFT' in _refused(L, [(L.GEO_SHIFT, (0, -10))])
    assert 'CUTOUT' in _refused(L, [(L.GEO_CUTOUT, (1, 1, 13, 3), (0, 0, 0))])
    assert 'unknown' in _refused(L, [(7, (0, 0, 0, 0))])
    assert 'in_h' in _refused(L, [cut, cut], fix=lambda it: setattr(it.steps[1], 'in_w', 11))
    assert 'out_h' in _refused(L, [cut], dst_hw=(12, 14), fix=lambda it: setattr(it, 'out_w', 13))

"""Test-time augmentation, host side (no GPU): MultiScaleFlipAug's views, the forward_test dispatch, the C entry points'
refusals, and the tests' fp32 restatement of aug_test_bboxes against the reference's recorded outputs."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import aug_ref as A

TRANSFORMS = A.TRANSFORMS


def test_multi_scale_flip_aug_views_in_reference_order():
    """test_time_aug.py:95-107: scales outer, [no flip, flip] inner; every meta carries its view's geometry."""
    from dsl_amd.datapath import PIPELINES, rescale_size
    aug = PIPELINES.build(dict(type='MultiScaleFlipAug', img_scale=[(128, 96), (96, 64)], flip=True, transforms=TRANSFORMS))
    h, w = 100, 150
    metas = aug.views(h, w, filename='a.jpg')
    assert len(metas) == 4
    assert [m['flip'] for m in metas] == [False, True, False, True]
    assert [m['flip_direction'] for m in metas] == [None, 'horizontal', None, 'horizontal']
    for m, scale in zip(metas, [(128, 96), (128, 96), (96, 64), (96, 64)]):
        nw, nh = rescale_size((w, h), scale)
        assert m['img_shape'] == (nh, nw, 3) and m['ori_shape'] == (h, w, 3)
        assert m['pad_shape'] == ((nh + 31) // 32 * 32, (nw + 31) // 32 * 32, 3)
        assert m['scale_factor'].dtype == np.float32
        np.testing.assert_array_equal(m['scale_factor'], np.array([nw / w, nh / h, nw / w, nh / h], np.float32))
    assert metas[0]['img_shape'] != metas[2]['img_shape']


def test_multi_scale_flip_aug_direction_list_and_no_flip():
    from dsl_amd.datapath import MultiScaleFlipAug
    aug = MultiScaleFlipAug(TRANSFORMS, img_scale=[(128, 96), (96, 64)], flip=True, flip_direction=['horizontal', 'vertical', 'diagonal'])
    metas = aug.views(96, 128)
    assert [(m['flip'], m['flip_direction']) for m in metas] == 2 * [(False, None), (True, 'horizontal'), (True, 'vertical'), (True, 'diagonal')]
    with pytest.warns(UserWarning, match='flip_direction has no effect'):          # test_time_aug.py:76-78
        one = MultiScaleFlipAug(TRANSFORMS, img_scale=(128, 96), flip=False, flip_direction=['vertical']).views(96, 128)
    assert len(one) == 1 and one[0]['flip'] is False and one[0]['flip_direction'] is None
    with pytest.warns(UserWarning, match='RandomFlip is not in transforms'):       # :79-82
        MultiScaleFlipAug([t for t in TRANSFORMS if t['type'] != 'RandomFlip'], img_scale=(128, 96), flip=True)
    # scales a config loader turned into lists
    lists = MultiScaleFlipAug(TRANSFORMS, img_scale=[[128, 96], [96, 64]]).views(96, 128)
    assert [m['img_shape'] for m in lists] == [m['img_shape'] for m in metas[0::4]]
    assert MultiScaleFlipAug(TRANSFORMS, img_scale=[128, 96]).views(96, 128)[0]['img_shape'] == metas[0]['img_shape']


def test_forward_test_dispatches_on_the_number_of_views():
    """detectors/base.py:116-153.  Four views reach aug_test (this stopped at 'test-time augmentation is out of scope'), one view
    still goes to simple_test, and unequal list lengths are refused."""
    from dsl_amd.detectors import FCOS
    calls = []

    class Probe(FCOS):
        def aug_test(self, imgs, img_metas, rescale=False):
            calls.append(('aug', len(imgs), rescale))
            return 'aug'

        def simple_test(self, img, img_metas, rescale=False):
            calls.append(('simple', tuple(img.shape), rescale))
            return 'simple'

    det = Probe.__new__(Probe)
    imgs = [torch.zeros(1, 3, 32, 32) for _ in range(4)]
    metas = [[dict(flip=False)] for _ in range(4)]
    assert Probe.forward_test(det, imgs, metas, rescale=True) == 'aug'
    assert Probe.forward(det, imgs[:1], metas[:1], return_loss=False) == 'simple'
    assert calls == [('aug', 4, True), ('simple', (1, 3, 32, 32), False)]
    with pytest.raises(ValueError, match='num of augmentations'):
        Probe.forward_test(det, imgs, metas[:3])
    assert list(inspect.signature(FCOS.aug_test).parameters) == ['self', 'imgs', 'img_metas', 'rescale']
    assert inspect.signature(FCOS.aug_test).parameters['rescale'].default is False


def _desc(n=1):
    from dsl_amd import _lib as L
    d = L.DetDesc()
    d.nlvl, d.n, d.num_classes, d.nms_pre, d.max_per_img = 5, n, 80, 50, 100
    return d


def test_more_than_dsl_max_aug_views_are_refused_with_a_message():
    from dsl_amd import _lib as L
    from dsl_amd.sweep import AugMerge
    d = _desc()
    assert L.MAX_AUG == 16
    assert L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), 16) > 0
    assert L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), 17) == 0
    assert b'17 views' in L.lib.dsl_last_error() and b'DSL_MAX_AUG' in L.lib.dsl_last_error()
    for call in (lambda: L.lib.dsl_fcos_detect_collect(C.byref(d), C.byref(d), 0, 17, 0, None, 0, None),
                 lambda: L.lib.dsl_fcos_detect_finish(C.byref(d), 17, 1, None, 0, None)):
        assert call() != 0 and b'DSL_MAX_AUG' in L.lib.dsl_last_error()
    with pytest.raises(ValueError, match='17 views'):
        AugMerge(17, 5, 'cpu')


def test_two_images_per_view_are_refused_with_a_message():
    from dsl_amd import _lib as L
    d = _desc(n=2)
    assert L.lib.dsl_fcos_detect_collect(C.byref(d), C.byref(_desc()), 0, 2, 0, None, 0, None) != 0
    assert b'one image per view' in L.lib.dsl_last_error()
    assert L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), 2) == 0


def test_a_view_that_is_not_the_pools_is_refused_at_its_collect():
    """The pool is laid out by its own nlvl / nms_pre / num_classes: collect names the view that differs, before any launch."""
    from dsl_amd import _lib as L
    for field, value in (('nms_pre', 40), ('num_classes', 3), ('nlvl', 4)):
        v = _desc()
        setattr(v, field, value)
        assert L.lib.dsl_fcos_detect_collect(C.byref(v), C.byref(_desc()), 1, 2, 0, None, 0, None) != 0
        msg = L.lib.dsl_last_error()
        assert b'view 1' in msg and field.encode() in msg, msg


def test_each_refused_field_is_named():
    from dsl_amd import _lib as L
    for field, value, word in (('num_classes', 0, b'num_classes'), ('nms_pre', 0, b'nms_pre')):
        d = _desc()
        setattr(d, field, value)
        assert L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), 2) == 0 and word in L.lib.dsl_last_error()
    d = _desc()
    d.max_per_img = 2000          # the pool does not depend on it: finish refuses it
    assert L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), 2) > 0
    assert L.lib.dsl_fcos_detect_finish(C.byref(d), 2, 1, None, 0, None) != 0 and b'max_per_img' in L.lib.dsl_last_error()


def test_pool_size_follows_the_documented_layout():
    """include/dsl_hip.h: per-view records and counts, scale factors, nviews * nlvl * nms_pre rows of 5 + num_classes floats, the pair scores of finish and
    its 16 384 candidate slots; every part rounded up to 256 bytes."""
    from dsl_amd import _lib as L
    d = _desc()
    r256 = lambda b: (b + 255) // 256 * 256
    for v in (1, 4, 16):
        rows = v * 5 * 50
        want = (r256(v * (4 + 5) * 4) + r256(v * 16) + r256(rows * 85 * 4) + r256(rows * 80 * 4) + r256(16384 * 16) + 2 * r256(16384 * 4)
                + r256(4 * 65))
        assert L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), v) == want


@pytest.mark.parametrize('name', ['c80_tricks', 'c3_plain'])
@pytest.mark.parametrize('rescale', [True, False])
def test_restatement_reproduces_the_reference(golden, name, rescale):
    """aug_ref.aug_test_bboxes - what the GPU pool-cap test compares with - gives the reference's recorded detections; with the
    project's cap (c80: 21 764 valid pairs > 16 384) they are the same, as 100 boxes survive among the best 16 384."""
    d = golden('aug_test_small.npz')
    views, metas, _, exp_decode = A.fixture_views(d, name)
    cfg = dict(score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']))
    ref_b = d[f'{name}_det_rescale' if rescale else f'{name}_det_norescale']
    for cap in (None, 16384):
        dets, labels, nvalid = A.aug_test_bboxes(views, metas, int(d['nms_pre']), exp_decode, rescale=rescale, cap=cap, **cfg)
        A.match(dets, labels, ref_b, d[f'{name}_lab'])
    assert (nvalid > 16384) == (name == 'c80_tricks')

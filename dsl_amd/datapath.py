"""GPU data path: the per-sample stages of the reference's training pipelines and the loader's
merge/pad, with the image work as ONE HIP launch per batch (csrc/datapath.hip, dsl_image_prep) and the box arithmetic - a few
dozen numbers per image - on the host, exactly as the reference computes it.

Mirrors, by name and argument meaning (configs/fcos_semi/RLA_*.py:68-82; mmdet/datasets/pipelines/transforms.py):
  Resize(img_scale, multiscale_mode='value'|'range', keep_ratio=True)   :41-332
  PatchShuffle(ratio, ranges, mode)                                     :2143-2248
  RandomFlip(flip_ratio)  (drawn: horizontal; forced: any direction)    :334-470
  Normalize(mean, std, to_rgb)                                          :652-690
  Pad(size_divisor)                                                     :581-650
  MultiDataLoader._merge_data2one_batch (pad to the batch's largest)    mmdet/datasets/builder.py:236-267
  RandomAugmentBBox_Fast(aug_type='affine'|'default')                  mmdet/datasets/pipelines/semi_aug.py:344-531
  UBAug()                                                               :2098-2140
  MultiScaleFlipAug(transforms, img_scale, flip, flip_direction)        mmdet/datasets/pipelines/test_time_aug.py:10-120
  RandomShift(shift_ratio, max_shift_px, filter_thr_px)                 :491-577
  Pad(size=(h, w))                                                      :581-650
  RandomCrop(crop_size, crop_type, allow_negative_crop, bbox_clip_border)   :693-873
  Expand(mean, to_rgb, ratio_range, prob)                               :1021-1109
  MinIoURandomCrop(min_ious, min_crop_size, bbox_clip_border)           :1113-1249
  CutOut(n_holes, cutout_shape | cutout_ratio, fill_in)                 :1850-1920
The last five are integer geometry: they draw from np.random in the reference's call order (pinned to the reference's own classes,
tests/golden/geo_transforms.json) and append (kind, a[, fill]) steps to r['_geo']; GpuBatchPipeline renders a sample's list with
dsl_image_geo (one launch per batch, a list longer than 32 steps over successive launches) in one of two places: in front of Resize
(SSD style: Expand -> MinIoURandomCrop -> Resize; the rendered images become dsl_image_prep's sources) or behind Resize / PatchShuffle
/ RandomFlip and in front of the augmentations and Normalize (uint8 canvas -> uint8 canvas); any other position is refused at
construction.  RandomCrop may reject a sample (None): __call__(samples, resample) asks for a replacement, SampleRejected otherwise.
A transform's __call__(results) only DRAWS its random parameters and updates boxes / meta; `GpuBatchPipeline` then renders all
images of the batch: one launch for the labeled stream, and for the unlabeled stream (the last two transforms) one launch per
augmentation pass over uint8 canvases (dsl_image_prep_u8 -> dsl_image_aug ... -> dsl_image_normalize).  UBAug's colour,
grayscale and blur passes are Pillow's 8-bit arithmetic, pinned to Pillow's outputs; imgaug's Affine follows its documentation
(unpinned: imgaug is not in this image); RandomErasing's noise is this library's own stream.
Fails loudly without the HIP library: there is no CPU rendering path in the product (the CPU restatement is oracle/datapath_oracle.py,
test infrastructure).
"""
import ctypes as C
import random
import warnings

import numpy as np
import torch

from . import _lib as L
from .registry import Registry

PIPELINES = Registry('pipeline')


def rescale_size(old_wh, scale):
    """mmcv.rescale_size (call site transforms.py:221-226)."""
    w, h = old_wh
    if isinstance(scale, (float, int)):
        sf = float(scale)
    else:
        sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(sf) + 0.5), int(h * float(sf) + 0.5)


@PIPELINES.register_module()
class Resize:
    def __init__(self, img_scale=None, multiscale_mode='range', ratio_range=None, keep_ratio=True, bbox_clip_border=True, **kw):
        self.img_scale = [img_scale] if isinstance(img_scale, tuple) else list(img_scale or [])
        assert multiscale_mode in ('value', 'range') and ratio_range is None and keep_ratio, 'configs use keep_ratio Resize'
        self.multiscale_mode, self.bbox_clip_border = multiscale_mode, bbox_clip_border

    def _random_scale(self):
        """:185-216."""
        if len(self.img_scale) == 1:
            return self.img_scale[0], 0
        if self.multiscale_mode == 'value':                    # random_select (:107-124)
            idx = np.random.randint(len(self.img_scale))
            return self.img_scale[idx], idx
        longs, shorts = [max(s) for s in self.img_scale], [min(s) for s in self.img_scale]      # random_sample (:126-150)
        return (np.random.randint(min(longs), max(longs) + 1), np.random.randint(min(shorts), max(shorts) + 1)), None

    def __call__(self, r):
        if 'scale' not in r:
            r['scale'], r['scale_idx'] = self._random_scale()
        h, w = r['img_shape'][:2]
        new_w, new_h = rescale_size((w, h), r['scale'])
        sf = np.array([new_w / w, new_h / h, new_w / w, new_h / h], dtype=np.float32)
        r['img_shape'] = r['pad_shape'] = (new_h, new_w, 3)
        r['scale_factor'], r['keep_ratio'] = sf, True
        for key in r.get('bbox_fields', []):
            b = r[key] * sf
            if self.bbox_clip_border:
                b[:, 0::2] = np.clip(b[:, 0::2], 0, new_w)
                b[:, 1::2] = np.clip(b[:, 1::2], 0, new_h)
            r[key] = b
        return r


@PIPELINES.register_module()
class PatchShuffle:
    def __init__(self, ratio=0.5, ranges=(0.2, 0.8), mode=('flip', 'flop')):
        assert isinstance(ratio, float)
        self.ratio, self.ranges, self.mode = ratio, list(ranges), list(mode)

    def __call__(self, r):
        if np.random.rand(1) > self.ratio:
            r['PS'], r['PS_place'], r['PS_mode'] = False, None, None
            return r
        r['PS'] = True
        h, w = r['img_shape'][:2]
        place = np.random.rand(1)[0] * abs(self.ranges[1] - self.ranges[0]) + self.ranges[0]
        mode = random.choice(self.mode)
        r['PS_place'], r['PS_mode'] = place, mode
        if mode == 'flip':
            crop_h, crop_w = h, min(int(round(w * place)), w)
            if crop_w == w or crop_w == 0:
                return r
        elif mode == 'flop':
            crop_h, crop_w = min(int(round(h * place)), h), w
            if crop_h == h or crop_h == 0:
                return r
        else:
            raise NotImplementedError
        r['_ps'] = (1, crop_w) if mode == 'flip' else (2, crop_h)       # what the launch needs: mode, split
        for key in r.get('bbox_fields', []):
            if len(r[key]) == 0:
                continue
            bb, out, lab = r[key], [], []
            for i in range(bb.shape[0]):
                x1, y1, x2, y2 = bb[i]
                if (x1 - crop_w + 1) * (x2 - crop_w + 1) >= 0 and (y1 - crop_h + 1) * (y2 - crop_h + 1) >= 0:
                    if mode == 'flip':
                        if x1 - crop_w + 1 < 0:
                            x1, x2 = x1 + w - crop_w, x2 + w - crop_w
                        if x2 - crop_w + 1 > 0:
                            x1, x2 = x1 - crop_w, x2 - crop_w
                    else:
                        if y1 - crop_h + 1 < 0:
                            y1, y2 = y1 + h - crop_h, y2 + h - crop_h
                        if y2 - crop_h + 1 > 0:
                            y1, y2 = y1 - crop_h, y2 - crop_h
                    out.append([x1, y1, x2, y2])
                    if key == 'gt_bboxes':
                        lab.append(r['gt_labels'][i])
                elif mode == 'flip':
                    out += [[x1 + w - crop_w, y1, w - 1, y2], [0, y1, x2 - crop_w, y2]]
                    if key == 'gt_bboxes':
                        lab += [r['gt_labels'][i]] * 2
                else:
                    out += [[x1, y1 + h - crop_h, x2, h - 1], [x1, 0, x2, y2 - crop_h]]
                    if key == 'gt_bboxes':
                        lab += [r['gt_labels'][i]] * 2
            r[key] = np.array(out).astype(np.float32)
            if key == 'gt_bboxes':
                r['gt_labels'] = np.array(lab).astype(np.int64)
        return r


FLIP_BITS = {'horizontal': 1, 'vertical': 2, 'diagonal': 3}      # dsl_image_prep_item.flip: bit 0 mirrors x, bit 1 mirrors y


@PIPELINES.register_module()
class RandomFlip:
    def __init__(self, flip_ratio=None, direction='horizontal'):
        assert direction == 'horizontal', 'the configs flip horizontally'
        self.flip_ratio = flip_ratio

    def __call__(self, r):
        if 'flip' not in r:
            r['flip'] = bool(self.flip_ratio is not None and np.random.rand() < self.flip_ratio)
            r['flip_direction'] = 'horizontal' if r['flip'] else None
        elif r.get('flip_direction') is None:         # forced (MultiScaleFlipAug gives the direction as well)
            r['flip_direction'] = 'horizontal' if r['flip'] else None
        if r['flip']:
            d = r['flip_direction']
            assert d in FLIP_BITS, f'flip_direction {d!r}'
            h, w = r['img_shape'][:2]
            for key in r.get('bbox_fields', []):          # bbox_flip (:401-432)
                b = r[key]
                f = b.copy()
                if FLIP_BITS[d] & 1:
                    f[..., 0::4] = w - b[..., 2::4]
                    f[..., 2::4] = w - b[..., 0::4]
                if FLIP_BITS[d] & 2:
                    f[..., 1::4] = h - b[..., 3::4]
                    f[..., 3::4] = h - b[..., 1::4]
                r[key] = f
        return r


@PIPELINES.register_module()
class Normalize:
    def __init__(self, mean, std, to_rgb=True):
        self.mean, self.std, self.to_rgb = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32), to_rgb

    def __call__(self, r):
        r['img_norm_cfg'] = dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)
        return r


@PIPELINES.register_module()
class Pad:
    def __init__(self, size=None, size_divisor=None, pad_val=0):
        assert (size is None) != (size_divisor is None) and pad_val == 0, 'pads with zeros, to a multiple or to a fixed (h, w)'
        self.size, self.size_divisor = (None if size is None else (int(size[0]), int(size[1]))), size_divisor

    def __call__(self, r):
        h, w = r['img_shape'][:2]
        if self.size is not None:              # mmcv.impad(shape=size): the image must fit
            assert self.size[0] >= h and self.size[1] >= w, f'Pad(size={self.size}) is smaller than the image {(h, w)}'
            r['pad_shape'] = (self.size[0], self.size[1], 3)
            r['pad_fixed_size'], r['pad_size_divisor'] = self.size, None
            return r
        d = self.size_divisor
        r['pad_shape'] = (int(np.ceil(h / d)) * d, int(np.ceil(w / d)) * d, 3)
        r['pad_size_divisor'] = d
        return r


# ---- the general geometric transforms (transforms.py:491-577, 693-873, 1021-1109, 1113-1249, 1850-1920) ------------------------
# __call__ draws from np.random in the reference's call order, moves / filters boxes and labels, updates img_shape and appends the
# image work to r['_geo'] as (kind, a[, fill]) steps (include/dsl_hip.h, dsl_geo_step); GpuBatchPipeline renders them with
# dsl_image_geo.  Pinned to the reference's own classes (tests/golden/geo_transforms.json).
_LABEL_OF = {'gt_bboxes': 'gt_labels', 'gt_bboxes_ignore': 'gt_labels_ignore'}


def _u8(values):
    """The bytes numpy stores when it assigns these values into a uint8 image (123.675 -> 123)."""
    return tuple(int(v) for v in np.asarray(values, np.float64).astype(np.uint8).reshape(-1)[:3])


@PIPELINES.register_module()
class RandomShift:
    def __init__(self, shift_ratio=0.5, max_shift_px=32, filter_thr_px=1):
        assert 0 <= shift_ratio <= 1
        assert max_shift_px >= 0
        self.shift_ratio, self.max_shift_px, self.filter_thr_px = shift_ratio, max_shift_px, int(filter_thr_px)

    def __call__(self, r):
        if not np.random.random() < self.shift_ratio:
            return r
        h, w = r['img_shape'][:2]
        dx = np.random.randint(-self.max_shift_px, self.max_shift_px)        # numpy's randint: the upper bound is exclusive
        dy = np.random.randint(-self.max_shift_px, self.max_shift_px)
        for key in r.get('bbox_fields', []):
            b = r[key].copy()
            b[..., 0::2] += dx
            b[..., 1::2] += dy
            b[..., 0::2] = np.clip(b[..., 0::2], 0, w)
            b[..., 1::2] = np.clip(b[..., 1::2], 0, h)
            valid = ((b[..., 2] - b[..., 0]) > self.filter_thr_px) & ((b[..., 3] - b[..., 1]) > self.filter_thr_px)
            if key == 'gt_bboxes' and not valid.any():
                return r           # no gt box survives: the image is not shifted either (fields visited before keep their shift)
            r[key] = b[valid]
            if _LABEL_OF.get(key) in r:
                r[_LABEL_OF[key]] = r[_LABEL_OF[key]][valid]
        if abs(int(dx)) >= w or abs(int(dy)) >= h:
            raise ValueError(f'RandomShift: drawn shift {(int(dx), int(dy))} is not smaller than the image {(h, w)}')
        r.setdefault('_geo', []).append((L.GEO_SHIFT, (int(dx), int(dy))))
        return r


@PIPELINES.register_module()
class RandomCrop:
    def __init__(self, crop_size, crop_type='absolute', allow_negative_crop=False, bbox_clip_border=True):
        if crop_type not in ('relative_range', 'relative', 'absolute', 'absolute_range'):
            raise ValueError(f'Invalid crop_type {crop_type}.')
        if crop_type in ('absolute', 'absolute_range'):
            assert crop_size[0] > 0 and crop_size[1] > 0
            assert isinstance(crop_size[0], int) and isinstance(crop_size[1], int)
        else:
            assert 0 < crop_size[0] <= 1 and 0 < crop_size[1] <= 1
        self.crop_size, self.crop_type = crop_size, crop_type
        self.allow_negative_crop, self.bbox_clip_border = allow_negative_crop, bbox_clip_border

    def _get_crop_size(self, h, w):
        cs = self.crop_size
        if self.crop_type == 'absolute':
            return min(cs[0], h), min(cs[1], w)
        if self.crop_type == 'absolute_range':
            assert cs[0] <= cs[1]
            crop_h = np.random.randint(min(h, cs[0]), min(h, cs[1]) + 1)
            crop_w = np.random.randint(min(w, cs[0]), min(w, cs[1]) + 1)
            return crop_h, crop_w
        if self.crop_type == 'relative':
            return int(h * cs[0] + 0.5), int(w * cs[1] + 0.5)
        cs = np.asarray(cs, dtype=np.float32)                   # relative_range
        rh, rw = cs + np.random.rand(2) * (1 - cs)
        return int(h * rh + 0.5), int(w * rw + 0.5)

    def __call__(self, r):
        h, w = r['img_shape'][:2]
        ch, cw = self._get_crop_size(h, w)
        assert ch > 0 and cw > 0
        off_h = int(np.random.randint(0, max(h - ch, 0) + 1))
        off_w = int(np.random.randint(0, max(w - cw, 0) + 1))
        new_h, new_w = min(off_h + int(ch), h) - off_h, min(off_w + int(cw), w) - off_w      # what the slice yields
        off = np.array([off_w, off_h, off_w, off_h], dtype=np.float32)
        for key in r.get('bbox_fields', []):
            b = r[key] - off
            if self.bbox_clip_border:
                b[:, 0::2] = np.clip(b[:, 0::2], 0, new_w)
                b[:, 1::2] = np.clip(b[:, 1::2], 0, new_h)
            valid = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
            if key == 'gt_bboxes' and not valid.any() and not self.allow_negative_crop:
                return None        # a crop without gt area: the caller draws another sample
            r[key] = b[valid, :]
            if _LABEL_OF.get(key) in r:
                r[_LABEL_OF[key]] = r[_LABEL_OF[key]][valid]
        r['img_shape'] = (new_h, new_w, 3)
        if (new_h, new_w) != (h, w):
            r.setdefault('_geo', []).append((L.GEO_CROP, (off_w, off_h, new_w, new_h)))
        return r


@PIPELINES.register_module()
class Expand:
    def __init__(self, mean=(0, 0, 0), to_rgb=True, ratio_range=(1, 4), seg_ignore_label=None, prob=0.5):
        self.to_rgb, self.ratio_range = to_rgb, ratio_range
        self.mean = mean[::-1] if to_rgb else mean              # the image is BGR
        self.min_ratio, self.max_ratio = ratio_range
        self.seg_ignore_label, self.prob = seg_ignore_label, prob

    def __call__(self, r):
        if np.random.uniform(0, 1) > self.prob:
            return r
        h, w = r['img_shape'][:2]
        ratio = np.random.uniform(self.min_ratio, self.max_ratio)
        big_h, big_w = int(h * ratio), int(w * ratio)
        left = int(np.random.uniform(0, w * ratio - w))
        top = int(np.random.uniform(0, h * ratio - h))
        for key in r.get('bbox_fields', []):
            r[key] = r[key] + np.tile((left, top), 2).astype(r[key].dtype)
        r['img_shape'] = (big_h, big_w, 3)
        if (big_h, big_w) != (h, w):
            r.setdefault('_geo', []).append((L.GEO_EXPAND, (left, top, big_w, big_h), _u8(self.mean)))
        return r


def _patch_overlaps(patch, boxes, eps=1e-6):
    """IoU of one patch with every box in float32, the union floored at eps (mmdet/core/evaluation/bbox_overlaps.py)."""
    p, b = patch.astype(np.float32), boxes.astype(np.float32).reshape(-1, 4)
    if b.shape[0] == 0:
        return np.zeros((0,), np.float32)
    area_p = (p[2] - p[0]) * (p[3] - p[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = np.maximum(np.minimum(p[2], b[:, 2]) - np.maximum(p[0], b[:, 0]), 0) * \
        np.maximum(np.minimum(p[3], b[:, 3]) - np.maximum(p[1], b[:, 1]), 0)
    union = np.maximum(area_p + area_b - inter, eps)
    return (inter / union).astype(np.float32)


def _centre_in_patch(boxes, patch):
    c = (boxes[:, :2] + boxes[:, 2:]) / 2
    return (c[:, 0] > patch[0]) * (c[:, 1] > patch[1]) * (c[:, 0] < patch[2]) * (c[:, 1] < patch[3])


@PIPELINES.register_module()
class MinIoURandomCrop:
    def __init__(self, min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.3, bbox_clip_border=True):
        self.min_ious = min_ious
        self.sample_mode = (1, *min_ious, 0)           # 1: return the image as it is
        self.min_crop_size, self.bbox_clip_border = min_crop_size, bbox_clip_border

    def __call__(self, r):
        assert 'bbox_fields' in r
        boxes = np.concatenate([r[key] for key in r['bbox_fields']], 0)
        h, w = r['img_shape'][:2]
        while True:
            mode = np.random.choice(self.sample_mode)
            self.mode = mode
            if mode == 1:
                return r
            for _ in range(50):
                new_w = np.random.uniform(self.min_crop_size * w, w)
                new_h = np.random.uniform(self.min_crop_size * h, h)
                if new_h / new_w < 0.5 or new_h / new_w > 2:
                    continue
                left = np.random.uniform(low=w - new_w, high=1.0)       # the reference's one-argument uniform(w - new_w)
                top = np.random.uniform(low=h - new_h, high=1.0)
                patch = np.array((int(left), int(top), int(left + new_w), int(top + new_h)))
                if patch[2] == patch[0] or patch[3] == patch[1]:
                    continue
                overlaps = _patch_overlaps(patch, boxes)
                if len(overlaps) > 0 and overlaps.min() < mode:
                    continue
                if len(overlaps) > 0:
                    if not _centre_in_patch(boxes, patch).any():
                        continue
                    for key in r.get('bbox_fields', []):
                        b = r[key].copy()
                        mask = _centre_in_patch(b, patch)
                        b = b[mask]
                        if self.bbox_clip_border:
                            b[:, 2:] = b[:, 2:].clip(max=patch[2:])
                            b[:, :2] = b[:, :2].clip(min=patch[:2])
                        b -= np.tile(patch[:2], 2)
                        r[key] = b
                        if _LABEL_OF.get(key) in r:
                            r[_LABEL_OF[key]] = r[_LABEL_OF[key]][mask]
                x0, y0 = int(patch[0]), int(patch[1])
                x1, y1 = min(int(patch[2]), w), min(int(patch[3]), h)
                r['img_shape'] = (y1 - y0, x1 - x0, 3)
                if (y1 - y0, x1 - x0) != (h, w):
                    r.setdefault('_geo', []).append((L.GEO_CROP, (x0, y0, x1 - x0, y1 - y0)))
                return r


@PIPELINES.register_module()
class CutOut:
    def __init__(self, n_holes, cutout_shape=None, cutout_ratio=None, fill_in=(0, 0, 0)):
        assert (cutout_shape is None) ^ (cutout_ratio is None), 'Either cutout_shape or cutout_ratio should be specified.'
        assert isinstance(cutout_shape, (list, tuple)) or isinstance(cutout_ratio, (list, tuple))
        if isinstance(n_holes, tuple):
            assert len(n_holes) == 2 and 0 <= n_holes[0] < n_holes[1]
        else:
            n_holes = (n_holes, n_holes)
        self.n_holes, self.fill_in = n_holes, fill_in
        self.with_ratio = cutout_ratio is not None
        self.candidates = cutout_ratio if self.with_ratio else cutout_shape
        if not isinstance(self.candidates, list):
            self.candidates = [self.candidates]

    def __call__(self, r):
        h, w = r['img_shape'][:2]
        steps = r.setdefault('_geo', [])
        for _ in range(np.random.randint(self.n_holes[0], self.n_holes[1] + 1)):
            x1 = np.random.randint(0, w)
            y1 = np.random.randint(0, h)
            index = np.random.randint(0, len(self.candidates))
            if not self.with_ratio:
                cut_w, cut_h = self.candidates[index]
            else:
                cut_w, cut_h = int(self.candidates[index][0] * w), int(self.candidates[index][1] * h)
            x2, y2 = np.clip(x1 + cut_w, 0, w), np.clip(y1 + cut_h, 0, h)
            if x2 > x1 and y2 > y1:
                steps.append((L.GEO_CUTOUT, (int(x1), int(y1), int(x2), int(y2)), _u8(self.fill_in)))
        return r


GEO_TRANSFORMS = (RandomShift, RandomCrop, Expand, MinIoURandomCrop, CutOut)


class SampleRejected(Exception):
    """A transform returned None for sample `index` (RandomCrop without gt area) and no `resample` was given."""

    def __init__(self, index):
        super().__init__(f'sample {index} was rejected by its pipeline and there is no resample callback')
        self.index = index


def _affine_forward(kind, value, w, h):
    """Forward matrix (input pixel -> output pixel) of one child of the reference's imgaug AFFINE_TRANSFORM[_WEAK]
    (semi_aug.py:36-88) about the image centre (w / 2 - 0.5, h / 2 - 0.5); rotation / shear in degrees, positive rotation
    clockwise in image coordinates.  imgaug is not available to this build: the convention follows its documentation, UNPINNED."""
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    T = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    M = np.eye(3)
    if kind == 'translate_x':
        M = T(value * w, 0)
    elif kind == 'translate_y':
        M = T(0, value * h)
    elif kind == 'rotate':
        a = np.deg2rad(value)
        M = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    elif kind == 'shear':
        M = np.array([[1, -np.tan(np.deg2rad(value)), 0], [0, 1, 0], [0, 0, 1]])
    return T(cx, cy) @ M @ T(-cx, -cy)


def _draw_affine(rng, weak):
    """iaa.OneOf of the four Affine children with their parameter ranges (semi_aug.py:36-88), interpolation order from [0, 1]."""
    kind = ('translate_x', 'translate_y', 'rotate', 'shear')[rng.randint(4)]
    if kind.startswith('translate'):
        lim = 0.05 if weak else 0.1
    else:
        lim = 10.0 if weak else 30.0           # DEGREE = 30 (:35); the in-box transform uses 10
    return kind, float(rng.uniform(-lim, lim)), int(rng.randint(2))


@PIPELINES.register_module()
class RandomAugmentBBox_Fast:
    """mmdet/datasets/pipelines/semi_aug.py:344-531.  Built: aug_type 'affine' (the DSL config's, RLA_*.py:93) and 'default'.
    __call__ draws the parameters and moves the boxes on the host; the image work is recorded as passes (`r['_aug']`) that
    GpuBatchPipeline renders with dsl_image_aug.  An image WITHOUT boxes takes the reference's colour branch (:494-497,
    RandAug policy of one op at probability 1, autoaug_fast.py): Color / Contrast / Brightness / Sharpness with the factor
    0.18 level + 0.1 (`_enhancer_impl`, :392-399), Solarize with threshold 256 - int(25.6 level) (:371-372), Posterize keeping
    4 - int(0.4 level) bits (:244-247), AutoContrast and Equalize (:219-224) - all nine ops are rendered, Pillow's arithmetic bit for
    bit (tests/golden/ubaug_pil.npz, randaug_pil.npz)."""
    COLOR_OPS = ('Identity', 'AutoContrast', 'Equalize', 'Solarize', 'Color', 'Contrast', 'Brightness', 'Sharpness', 'Posterize')

    def __init__(self, aug_type='strong', magnitude=10, weighted_inbox_selection=False):
        if aug_type not in ('affine', 'default'):
            raise NotImplementedError(f"RandomAugmentBBox_Fast(aug_type={aug_type!r}): 'affine' (configs/fcos_semi) and 'default' are built")
        self.aug_type, self.magnitude, self.weighted = aug_type, magnitude, weighted_inbox_selection
        self.skipped_ops = 0            # ops drawn but not rendered: none since round 6 (kept for the replay test's assertion)
        self.rng = np.random

    def __call__(self, r):
        h, w = r['img_shape'][:2]
        passes = r.setdefault('_aug', [])
        boxes = r['gt_bboxes']
        if boxes.shape[0] == 0:
            op = self.COLOR_OPS[self.rng.randint(len(self.COLOR_OPS))]
            level = self.rng.randint(1, self.magnitude)
            f = float(level) * 1.8 / 10 + 0.1
            if op in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
                kind = dict(Color=L.AUG_SATURATION, Contrast=L.AUG_CONTRAST, Brightness=L.AUG_BRIGHTNESS, Sharpness=L.AUG_SHARPNESS)[op]
                passes.append(dict(kind=kind, f=f, op=op))
            elif op == 'Solarize':
                passes.append(dict(kind=L.AUG_SOLARIZE, f=float(256 - int(level * 256 / 10)), op=op))
            elif op == 'Posterize':
                passes.append(dict(kind=L.AUG_POSTERIZE, f=float(4 - int(level * 4 / 10)), op=op))
            elif op in ('AutoContrast', 'Equalize'):
                passes.append(dict(kind=L.AUG_AUTOCONTRAST if op == 'AutoContrast' else L.AUG_EQUALIZE, op=op))
            return r
        if self.aug_type == 'default':
            return r
        # array_to_bb (:150-155): imgaug's BoundingBox orders its corners (x1 <= x2, y1 <= y2) on construction
        boxes = np.stack([np.minimum(boxes[:, 0], boxes[:, 2]), np.minimum(boxes[:, 1], boxes[:, 3]),
                          np.maximum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 1], boxes[:, 3])], 1)
        if self.rng.randint(2) == 0:           # bbox_affine_transform (:431-452): one box, the weak transform inside it
            n = boxes.shape[0]
            if self.weighted:
                area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
                k = int(self.rng.choice(n, p=area / area.sum()))
            else:
                k = int(self.rng.randint(n))
            x0, y0, x1, y1 = (int(v) for v in boxes[k])
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)     # (a box sticking out is clamped: the reference's
                                                                                # negative slice index would wrap around)
            if x1 > x0 and y1 > y0:
                kind, val, order = _draw_affine(self.rng, weak=True)
                passes.append(dict(kind=L.AUG_AFFINE, M=_affine_forward(kind, val, x1 - x0, y1 - y0), order=order, roi=(x0, y0, x1, y1)))
        else:                                   # affine_transform (:454-461): the whole image and its boxes
            kind, val, order = _draw_affine(self.rng, weak=False)
            M = _affine_forward(kind, val, w, h)
            passes.append(dict(kind=L.AUG_AFFINE, M=M, order=order, roi=(0, 0, w, h)))
            b = boxes.astype(np.float64)
            out = np.zeros_like(b)
            for i, (bx1, by1, bx2, by2) in enumerate(b):       # imgaug: the four corners move, the box is their hull
                c = np.array([[bx1, by1, 1], [bx2, by1, 1], [bx2, by2, 1], [bx1, by2, 1]], np.float64) @ M.T
                out[i] = [c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()]
            boxes = out
        boxes = boxes.astype(np.float64)
        boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w)             # :519-527
        boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h)
        keep = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) > 0
        r['gt_bboxes'] = boxes[keep].astype(np.float32)
        r['gt_labels'] = r['gt_labels'][keep]
        return r


@PIPELINES.register_module()
class UBAug:
    """mmdet/datasets/pipelines/transforms.py:2098-2140 (Unbiased Teacher's strong augmentation): RandomApply(ColorJitter(0.4, 0.4,
    0.4, 0.1), 0.8), RandomGrayscale(0.2), RandomApply(GaussianBlur(0.1 .. 2.0), 0.5), three RandomErasing.  The parameters are
    drawn here the way torchvision draws them (ColorJitter: a random order of the four adjustments, factors U(0.6, 1.4) and hue
    U(-0.1, 0.1); RandomErasing.get_params: ten attempts per rectangle); the image passes are Pillow's arithmetic, pinned by
    tests/golden/ubaug_pil.npz.  The reference hands mmcv's BGR array to ToPILImage as if it were RGB: the passes treat the
    stored channel order as RGB in the same way."""

    def __init__(self):
        self.rng = np.random

    @staticmethod
    def _erase_rect(rng, h, w, scale, ratio):
        area = h * w
        for _ in range(10):
            ea = area * rng.uniform(scale[0], scale[1])
            ar = np.exp(rng.uniform(np.log(ratio[0]), np.log(ratio[1])))
            eh, ew = int(round(np.sqrt(ea * ar))), int(round(np.sqrt(ea / ar)))
            if eh < h and ew < w:
                i, j = int(rng.randint(0, h - eh + 1)), int(rng.randint(0, w - ew + 1))
                return (j, i, j + ew, i + eh)
        return None

    def __call__(self, r):
        h, w = r['img_shape'][:2]
        passes, rng = r.setdefault('_aug', []), self.rng
        if rng.rand() < 0.8:
            fac = {L.AUG_BRIGHTNESS: rng.uniform(0.6, 1.4), L.AUG_CONTRAST: rng.uniform(0.6, 1.4), L.AUG_SATURATION: rng.uniform(0.6, 1.4),
                   L.AUG_HUE: rng.uniform(-0.1, 0.1)}
            kinds = [L.AUG_BRIGHTNESS, L.AUG_CONTRAST, L.AUG_SATURATION, L.AUG_HUE]
            for i in rng.permutation(4):
                f = float(fac[kinds[i]])
                passes.append(dict(kind=kinds[i], f=float(int(f * 255)) if kinds[i] == L.AUG_HUE else f))
        if rng.rand() < 0.2:
            passes.append(dict(kind=L.AUG_GRAY))
        if rng.rand() < 0.5:
            sigma = float(rng.uniform(0.1, 2.0))
            fr = blur_box_radius(sigma)
            if fr != 0:
                passes += [dict(kind=L.AUG_BLUR_H, f=fr)] * 3 + [dict(kind=L.AUG_BLUR_V, f=fr)] * 3
        rects = []
        for p_, scale, ratio in ((0.7, (0.05, 0.2), (0.3, 3.3)), (0.5, (0.02, 0.2), (0.1, 6)), (0.3, (0.02, 0.2), (0.05, 8))):
            if rng.rand() < p_:
                rc = self._erase_rect(rng, h, w, scale, ratio)
                if rc is not None:
                    rects.append(rc)
        if rects:
            passes.append(dict(kind=L.AUG_ERASE, rects=rects, seed=int(rng.randint(0, 2 ** 31 - 1))))
        return r


def blur_box_radius(radius, passes=3):
    """Pillow BoxBlur.c `_gaussian_blur_radius` (float arithmetic as in the C source): the fractional box radius of
    ImageFilter.GaussianBlur(radius)."""
    radius = np.float32(radius)
    sigma2 = np.float32(radius * radius / np.float32(passes))
    big_l = np.float32(np.sqrt(12.0 * np.float64(sigma2) + 1.0))
    l_ = np.float32(np.floor((np.float64(big_l) - 1.0) / 2.0))
    a = np.float32((2 * l_ + 1) * (l_ * (l_ + 1) - 3 * sigma2))
    a = np.float32(a / np.float32(6 * (sigma2 - (l_ + 1) * (l_ + 1))))
    return float(np.float32(l_ + a))


META_KEYS = ('filename', 'ori_filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'scale_idx', 'flip',
             'flip_direction', 'img_norm_cfg', 'PS', 'PS_place', 'PS_mode')
_SKIP = ('LoadImageFromFile', 'LoadAnnotations', 'DefaultFormatBundle', 'Collect', 'ImageToTensor')


class GpuBatchPipeline:
    """pipeline: the config's list of transform dicts (train_pipeline / unlabel_train_pipeline).  __call__(samples) with samples =
    list of dict(img = uint8 [H, W, 3] BGR tensor / array, gt_bboxes [G, 4] fp32, gt_labels [G] int64, gt_bboxes_ignore [K, 4],
    filename) returns the batch dict the detector's train_step takes: img [N, 3, Hc, Wc] fp32 on the device, img_metas and the
    per-image box lists."""

    def __init__(self, pipeline, device='cuda'):
        self.device = device
        self.transforms = []
        for cfg in pipeline:
            t = cfg['type']
            if t in _SKIP:
                continue
            self.transforms.append(PIPELINES.build(cfg))
        norm = [t for t in self.transforms if isinstance(t, Normalize)]
        assert len(norm) == 1, 'the pipeline needs exactly one Normalize'
        self.norm = norm[0]
        self._geo_split = self._place_geo()

    def _place_geo(self):
        """Where the geometric transforms render.  In front of Resize their steps run from the uploads into per-sample images that
        become dsl_image_prep's sources; after Resize / PatchShuffle / RandomFlip and in front of the augmentations and Normalize
        they run between two uint8 canvases.  Returns the index of the first transform behind the front group (None: the pipeline
        lists no geometric transform and renders as it always did); any other position is refused here."""
        if not any(isinstance(t, GEO_TRANSFORMS) for t in self.transforms):
            return None
        stage, last_geo = 0, None      # 0 start, 1 after Resize, 2 after PatchShuffle / RandomFlip, 3 after a geometric transform
        names = {4: 'the augmentation passes', 5: 'Normalize'}      # behind those, 4 / 5 after the augmentations / Normalize
        split = next(i for i, t in enumerate(self.transforms) if not isinstance(t, GEO_TRANSFORMS))      # (Normalize is there)
        for i, t in enumerate(self.transforms):
            name = type(t).__name__
            if isinstance(t, Resize):
                if any(isinstance(u, Resize) for u in self.transforms[:i]):
                    raise NotImplementedError(f'{name} at position {i}: a second Resize in a pipeline with geometric transforms is not rendered')
                if stage != 0:
                    raise NotImplementedError(f'{name} at position {i}: with geometric transforms Resize comes before PatchShuffle / RandomFlip '
                                              'and the augmentations')
                stage = 1
            elif isinstance(t, (PatchShuffle, RandomFlip)):
                if stage == 3:
                    raise NotImplementedError(f'{last_geo[1]} at position {last_geo[0]}: a geometric transform between Resize and {name} '
                                              f'(position {i}) is not rendered; put it before Resize or after RandomFlip')
                if stage > 3:
                    raise NotImplementedError(f'{name} at position {i}: after {names[stage]} is not rendered')
                stage = 2
            elif isinstance(t, GEO_TRANSFORMS):
                if stage >= 4:
                    raise NotImplementedError(f'{name} at position {i}: a geometric transform after {names[stage]} is not rendered; put it '
                                              'before Resize, or after RandomFlip and before the augmentations and Normalize')
                if stage == 0 and i > split:
                    raise NotImplementedError(f'{name} at position {i}: a geometric transform before Resize goes in front of every '
                                              f'other transform ({type(self.transforms[split]).__name__} at position {split} precedes it)')
                if stage >= 1:
                    stage, last_geo = 3, (i, name)
            elif isinstance(t, (RandomAugmentBBox_Fast, UBAug)):
                stage = max(stage, 4)
            elif isinstance(t, Normalize):
                stage = 5
        return split

    def draw(self, s, h, w):
        """Host side of one sample of size h x w: every transform draws its parameters and updates boxes / meta; no image work.
        None when a transform rejects the sample (RandomCrop without gt area)."""
        r = dict(filename=s.get('filename'), ori_filename=s.get('filename'), ori_shape=(h, w, 3), img_shape=(h, w, 3),
                 gt_bboxes=np.asarray(s.get('gt_bboxes', np.zeros((0, 4))), np.float32).reshape(-1, 4),
                 gt_labels=np.asarray(s.get('gt_labels', np.zeros((0,))), np.int64).reshape(-1),
                 gt_bboxes_ignore=np.asarray(s.get('gt_bboxes_ignore', np.zeros((0, 4))), np.float32).reshape(-1, 4),
                 bbox_fields=['gt_bboxes_ignore', 'gt_bboxes'], scale_factor=np.ones(4, np.float32))
        for k in ('scale', 'flip', 'flip_direction'):          # forced parameters (tests; the test pipeline's MultiScaleFlipAug)
            if k in s:
                r[k] = s[k]
        split = self._geo_split
        for i, t in enumerate(self.transforms):
            if split is not None:
                if i == split:                      # the steps drawn in front of Resize render from the upload
                    r['_geo_pre'], r['_geo'] = r.pop('_geo', []), []
                elif i > split and isinstance(t, GEO_TRANSFORMS):
                    r.setdefault('_prep_shape', r['img_shape'])      # what dsl_image_prep renders: the size in front of the first step
            r = t(r)
            if r is None:
                return None
        r.setdefault('_prep_shape', r['img_shape'])
        r.setdefault('pad_shape', r['img_shape'])
        r.setdefault('flip', False)
        r.setdefault('flip_direction', None)
        return r

    @staticmethod
    def meta(r, hc, wc):
        m = {k: r.get(k) for k in META_KEYS}
        m['batch_input_shape'] = (hc, wc)
        return m

    def _render_geo(self, jobs):
        """dsl_image_geo over jobs = dicts(src, src_h, src_w, src_ld, steps, dst, dst_h, dst_w, dst_ld) (device addresses): one launch,
        or, where a list is longer than GEO_MAX_STEPS, successive launches that ping-pong two buffers holding the images in between.
        Returns the tensors that must stay alive until the launches have run."""
        M = L.GEO_MAX_STEPS
        chunks = [max(1, (len(j['steps']) + M - 1) // M) for j in jobs]
        offs, total = {}, 0
        for q, j in enumerate(jobs):
            if chunks[q] > 1:
                sizes = [L.geo_out_size(j['steps'][:M * (c + 1)], j['src_h'], j['src_w']) for c in range(chunks[q] - 1)]
                j['_mid'] = sizes
                offs[q], total = total, total + max(h * w for h, w in sizes) * 3
        tmp = [torch.empty(total, dtype=torch.uint8, device=self.device) for _ in range(2)] if total else []
        keep = list(tmp)
        for k in range(max(chunks)):
            live = [q for q in range(len(jobs)) if chunks[q] > k]
            its = (L.GeoItem * len(live))()
            for it, q in zip(its, live):
                j = jobs[q]
                if k == 0:
                    src = (j['src'], j['src_h'], j['src_w'], j['src_ld'])
                else:
                    mh, mw = j['_mid'][k - 1]
                    src = (tmp[(k - 1) % 2].data_ptr() + offs[q], mh, mw, mw)
                if k == chunks[q] - 1:
                    dst = (j['dst'], j['dst_h'], j['dst_w'], j['dst_ld'])
                else:
                    mh, mw = j['_mid'][k]
                    dst = (tmp[k % 2].data_ptr() + offs[q], mh, mw, mw)
                L.geo_fill_item(it, j['steps'][M * k:M * (k + 1)], *src, *dst)
            tab = torch.frombuffer(bytearray(bytes(its)), dtype=torch.uint8).to(self.device)
            keep.append(tab)
            L.check(L.lib.dsl_image_geo(C.cast(its, C.c_void_p), L.ptr(tab), len(live), max(it.dst_h for it in its),
                                        max(it.dst_w for it in its), L.stream_ptr()), 'dsl_image_geo')
        return keep

    def _prep_table(self, results, srcs, shape_key):
        """The dsl_image_prep_item table: srcs = (address, h, w) per sample, new_h x new_w = r[shape_key]."""
        items = (L.ImagePrepItem * len(results))()
        inv = (1.0 / self.norm.std.astype(np.float64)).astype(np.float32)
        for i, (r, src) in enumerate(zip(results, srcs)):
            it = items[i]
            it.src, it.src_h, it.src_w = src
            it.new_h, it.new_w = r[shape_key][0], r[shape_key][1]
            it.flip, it.to_rgb = (FLIP_BITS[r['flip_direction'] or 'horizontal'] if r['flip'] else 0), int(bool(self.norm.to_rgb))
            it.ps_mode, it.ps_crop = r.get('_ps', (0, 0))
            for c in range(3):
                it.mean[c], it.inv_std[c] = float(self.norm.mean[c]), float(inv[c])
        return torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(self.device)

    def draw_batch(self, samples, resample=None):
        """Host side of a batch: (uint8 image tensors, drawn results).  resample(i): a replacement for sample i when a transform
        rejects it (the reference's dataset loop draws another index the same way, datasets/custom.py:193-198); without it a
        rejection raises SampleRejected."""
        imgs, results = [], []
        for i, s in enumerate(samples):
            while True:
                img = s['img']
                img = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
                assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
                r = self.draw(s, *img.shape[:2])
                if r is not None:
                    break
                if resample is None:
                    raise SampleRejected(i)
                s = resample(i)
            imgs.append(img)
            results.append(r)
        return imgs, results

    def __call__(self, samples, resample=None):
        n = len(samples)
        imgs, results = self.draw_batch(samples, resample)
        srcs = [img.to(self.device, non_blocking=True).contiguous() for img in imgs]
        hc, wc = max(r['pad_shape'][0] for r in results), max(r['pad_shape'][1] for r in results)       # merge/pad
        keep = []
        prep_src = [(src.data_ptr(), src.shape[0], src.shape[1]) for src in srcs]
        pre = [i for i, r in enumerate(results) if r.get('_geo_pre')]
        if pre:
            # the steps in front of Resize: one launch from the uploads into one allocation of per-sample images, which become
            # dsl_image_prep's sources (a sample without steps keeps pointing at its upload)
            sizes = {i: L.geo_out_size(results[i]['_geo_pre'], *srcs[i].shape[:2]) for i in pre}
            buf = torch.empty(sum(h * w for h, w in sizes.values()) * 3, dtype=torch.uint8, device=self.device)
            jobs, off = [], 0
            for i in pre:
                h, w = sizes[i]
                jobs.append(dict(src=srcs[i].data_ptr(), src_h=srcs[i].shape[0], src_w=srcs[i].shape[1], src_ld=srcs[i].shape[1],
                                 steps=results[i]['_geo_pre'], dst=buf.data_ptr() + off, dst_h=h, dst_w=w, dst_ld=w))
                prep_src[i] = (buf.data_ptr() + off, h, w)
                off += h * w * 3
            keep += [buf] + self._render_geo(jobs)
        post = any(r.get('_geo') for r in results) and self._geo_split is not None
        tab = self._prep_table(results, prep_src, '_prep_shape' if post else 'img_shape')
        out = torch.empty(n, 3, hc, wc, dtype=torch.float32, device=self.device)
        n_pass = max(len(r.get('_aug', ())) for r in results)
        if n_pass == 0 and not post:
            L.check(L.lib.dsl_image_prep(L.ptr(tab), n, L.ptr(out), hc, wc, L.stream_ptr()), 'dsl_image_prep')
        else:
            # the unlabeled stream (RandomAugmentBBox_Fast, UBAug): Resize / PatchShuffle / Flip into uint8 canvases, one launch per
            # augmentation pass over the batch (an image with fewer passes is copied), then Normalize / Pad
            a = torch.empty(n, hc, wc, 3, dtype=torch.uint8, device=self.device)
            keep.append(a)
            tab_n = tab
            if post:
                # the steps behind Resize / PatchShuffle / RandomFlip: those render into a canvas sized by the largest resized image,
                # dsl_image_geo moves that into the final canvas; the later stages see the final img_shape
                h1, w1 = max(r['_prep_shape'][0] for r in results), max(r['_prep_shape'][1] for r in results)
                a1 = torch.empty(n, h1, w1, 3, dtype=torch.uint8, device=self.device)
                L.check(L.lib.dsl_image_prep_u8(L.ptr(tab), n, L.ptr(a1), h1, w1, L.stream_ptr()), 'dsl_image_prep_u8')
                jobs = [dict(src=a1.data_ptr() + i * h1 * w1 * 3, src_h=r['_prep_shape'][0], src_w=r['_prep_shape'][1], src_ld=w1,
                             steps=r.get('_geo', []), dst=a.data_ptr() + i * hc * wc * 3, dst_h=hc, dst_w=wc, dst_ld=wc)
                        for i, r in enumerate(results)]
                tab_n = self._prep_table(results, prep_src, 'img_shape')
                keep += [a1, tab_n] + self._render_geo(jobs)
            else:
                L.check(L.lib.dsl_image_prep_u8(L.ptr(tab), n, L.ptr(a), hc, wc, L.stream_ptr()), 'dsl_image_prep_u8')
            if n_pass:
                a = self._render_aug(results, n_pass, a, hc, wc, keep)
            L.check(L.lib.dsl_image_normalize(L.ptr(a), L.ptr(tab_n), n, L.ptr(out), hc, wc, L.stream_ptr()), 'dsl_image_normalize')
        self._keep = (srcs + keep, tab)            # alive until the launch has run (stream order)
        self.last_passes = [list(r.get('_aug', ())) for r in results]      # what was rendered (tests replay it on the oracle)
        self.last_geo = [(list(r.get('_geo_pre', ())), list(r.get('_geo', ()))) for r in results]      # (front of Resize, behind it)
        metas = [self.meta(r, hc, wc) for r in results]
        return dict(img=out, img_metas=metas, gt_bboxes=[torch.from_numpy(r['gt_bboxes']) for r in results],
                    gt_labels=[torch.from_numpy(r['gt_labels']) for r in results],
                    gt_bboxes_ignore=[torch.from_numpy(r['gt_bboxes_ignore']) for r in results])

    def _render_aug(self, results, n_pass, a, hc, wc, keep):
        """One dsl_image_aug launch per pass from canvas a into a second one and back; returns the canvas holding the result."""
        n = len(results)
        b = torch.empty_like(a)
        sums = torch.empty(int(L.lib.dsl_image_aug_scratch_bytes(n)) // 8, dtype=torch.int64, device=self.device)
        # every pass's item table in ONE host -> device copy
        its = (L.AugItem * (n * n_pass))()
        need_mean = [0] * n_pass
        for k in range(n_pass):
            for i, r in enumerate(results):
                it, ps = its[k * n + i], r.get('_aug', ())
                it.h, it.w = r['img_shape'][0], r['img_shape'][1]
                if k >= len(ps):
                    continue
                ps_k = ps[k]
                it.kind = ps_k['kind']
                need_mean[k] |= int(it.kind == L.AUG_CONTRAST) | 2 * int(it.kind in (L.AUG_AUTOCONTRAST, L.AUG_EQUALIZE))
                it.f[0] = float(ps_k.get('f', 0.0))
                if it.kind == L.AUG_AFFINE:
                    x0, y0, x1, y1 = ps_k['roi']
                    Mi = np.linalg.inv(ps_k['M'])
                    for q in range(6):
                        it.m[q] = float(Mi[q // 3, q % 3])
                    it.roi[0], it.roi[1], it.roi[2], it.roi[3] = x0, y0, x1, y1
                    it.order, it.cval = int(ps_k['order']), 125
                if it.kind == L.AUG_ERASE:
                    it.seed = ps_k['seed']
                    for q, rc in enumerate(ps_k['rects'][:3]):
                        for e in range(4):
                            it.rect[q][e] = int(rc[e])
        at = torch.frombuffer(bytearray(bytes(its)), dtype=torch.uint8).to(self.device)
        keep += [b, sums, at]
        isz = C.sizeof(L.AugItem)
        for k in range(n_pass):
            L.check(L.lib.dsl_image_aug(at.data_ptr() + k * n * isz, n, L.ptr(a), L.ptr(b), hc, wc, L.ptr(sums), need_mean[k],
                                        L.stream_ptr()), 'dsl_image_aug')
            a, b = b, a
        return a


@PIPELINES.register_module()
class MultiScaleFlipAug:
    """test_time_aug.py:10-120: one view per (scale, flip) of ONE image - scales outer, flip_args = [(False, None)] + [(True, d)
    for d in flip_direction] inner.  `views(h, w)` is the host side alone (the metas, in that order); __call__(sample) renders
    them and returns the reference's dict of lists, batched for forward_test: img = [view][1, 3, Hc, Wc], img_metas = [view][1]."""

    def __init__(self, transforms, img_scale=None, scale_factor=None, flip=False, flip_direction='horizontal', device='cuda'):
        assert img_scale is not None and scale_factor is None, 'the configs give img_scale'
        many = isinstance(img_scale, (list, tuple)) and len(img_scale) > 0 and isinstance(img_scale[0], (list, tuple))
        self.img_scale = [tuple(s) for s in (img_scale if many else [img_scale])]      # a config loader may hand lists over
        assert all(len(s) == 2 for s in self.img_scale), img_scale
        self.flip = flip
        self.flip_direction = list(flip_direction) if isinstance(flip_direction, (list, tuple)) else [flip_direction]
        assert all(d in FLIP_BITS for d in self.flip_direction), self.flip_direction
        if not self.flip and self.flip_direction != ['horizontal']:          # test_time_aug.py:76-82
            warnings.warn('flip_direction has no effect when flip is set to False')
        if self.flip and not any(t['type'] == 'RandomFlip' for t in transforms):
            warnings.warn('flip has no effect when RandomFlip is not in transforms')
        self.pipeline = GpuBatchPipeline(transforms, device=device)

    def _forced(self, sample):
        flip_args = [(False, None)] + ([(True, d) for d in self.flip_direction] if self.flip else [])
        return [dict(sample, scale=scale, flip=flip, flip_direction=d) for scale in self.img_scale for flip, d in flip_args]

    def views(self, h, w, filename=None):
        out = []
        for s in self._forced(dict(filename=filename)):
            r = self.pipeline.draw(s, h, w)
            out.append(self.pipeline.meta(r, *r['pad_shape'][:2]))
        return out

    def __call__(self, sample):
        img = sample['img']
        img = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
        sample = dict(sample, img=img.to(self.pipeline.device).contiguous())      # ONE upload: every view renders from the same device copy
        data = [self.pipeline([s]) for s in self._forced(sample)]
        return dict(img=[d['img'] for d in data], img_metas=[d['img_metas'] for d in data])

"""Teacher / test-time sweep: network forward + on-GPU post-processing (dsl_fcos_detect).

Mirrors SingleStageDetector.simple_test (mmdet/models/detectors/single_stage.py:86-107) ->
FCOSHead.get_bboxes (dense_heads/fcos_head.py:340-548) -> multiclass_nms (core/post_processing/
bbox_nms.py:7-94) -> bbox2result (core/bbox/transforms.py:99-116) of the reference; the detections stay
on the GPU (`detect_device`) for the pseudo-label refresh, and `simple_test` converts them to the
reference's per-class numpy lists.

Test-time augmentation (`aug_test`) mirrors SingleStageDetector.aug_test (single_stage.py:109-135) ->
BBoxTestMixin.aug_test_bboxes / merge_aug_bboxes (dense_heads/dense_test_mixins.py:38-108, 173-200): every view's candidates
are mapped back to the original image on the device (dsl_fcos_detect_collect) into one pool, and one sort + NMS runs over the
pool (dsl_fcos_detect_finish); nothing but the final detections crosses to the host."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .params import HeadOptions, class_layout


class DetectPlan:
    def __init__(self, n, sizes, strides, device, num_classes=80, nms_pre=1000, max_per_img=100, score_thr=0.05,
                 iou_thr=0.5, ld_cls=80, nms_method=0, soft_sigma=0.0, soft_min_score=0.0, head=None):
        """head: params.HeadOptions (None = the default head).  Its kind's record (params.HEAD_KINDS) names the struct around the
        dsl_det_desc `desc` (`_ext` keeps it alive), whether the head's dsl_atss_desc (`atss`) is attached, and the flags that reach
        the kernels: DSL_HEAD_EXP_DECODE (norm_on_bbox=False), DSL_HEAD_ATSS (anchor-delta decode), DSL_HEAD_PAA, or DSL_HEAD_GFL alone
        with rows of 4 (reg_max + 1) floats."""
        head = head or HeadOptions()
        kind = head.kind
        self._ext = d = getattr(L, kind.det_desc[0])()
        for member in kind.det_desc[1:]:
            holder, d = d, getattr(d, member)
        self.atss = head.atss_desc() if kind.det_mask & L.HEAD_ATSS else None
        if self.atss is not None:
            holder.atss = C.addressof(self.atss)
        for field, option in kind.det_fields:
            setattr(self._ext, field, getattr(head, option))
        d.nms_method, d.soft_sigma, d.soft_min_score = nms_method, soft_sigma, soft_min_score      # L.NMS_*; all zero: the hard NMS
        d.nlvl, d.n = len(sizes), n
        d.h, d.w = L.seg5([s[0] for s in sizes]), L.seg5([s[1] for s in sizes])
        d.stride = L.seg5(strides)
        d.num_classes, d.nms_pre, d.max_per_img = num_classes, nms_pre, max_per_img
        d.score_thr, d.iou_thr = score_thr, iou_thr
        d.ld_cls, d.ld_rc = ld_cls, head.reg_layout()[1]
        d.head_flags = head.flags() & kind.det_mask
        # centerness_on_reg=False: the centerness logit is this column of the logits' rows (FcosLossPlan.ctr_col)
        self.ctr_col = None if head.centerness_on_reg else class_layout(num_classes)[1]
        self.dets = torch.zeros(n, max_per_img, 5, device=device)
        self.labels = torch.zeros(n, max_per_img, dtype=torch.int64, device=device)
        self.count = torch.zeros(n, dtype=torch.int32, device=device)
        self.img_shapes = torch.zeros(n, 2, device=device)
        self.scale_factors = torch.ones(n, 4, device=device)
        need = L.lib.dsl_detect_workspace_bytes(C.byref(d))
        self.ws = torch.empty(need, dtype=torch.uint8, device=device)
        d.dets, d.det_labels, d.det_count = L.ptr(self.dets), L.ptr(self.labels), L.ptr(self.count)
        d.img_shapes, d.scale_factors = L.ptr(self.img_shapes), L.ptr(self.scale_factors)
        d.workspace, d.workspace_bytes = L.ptr(self.ws), need
        self.desc, self.n = d, n
        self._keep = []

    def bind(self, cls_logits, regctr, scales):
        self.desc.cls_logits, self.desc.regctr, self.desc.scales = L.ptr(cls_logits), L.ptr(regctr), L.ptr(scales)
        if self.ctr_col is not None:
            self.desc.ctr, self.desc.ld_ctr = self.desc.cls_logits + 4 * self.ctr_col, self.desc.ld_cls
        self._keep = [cls_logits, regctr, scales]

    def set_meta(self, img_shapes, scale_factors, rescale):
        self.img_shapes.copy_(torch.tensor([[float(s[0]), float(s[1])] for s in img_shapes]), non_blocking=True)
        if rescale:
            sf = []
            for s in scale_factors:
                a = np.asarray(s, dtype=np.float32).reshape(-1)
                sf.append(np.repeat(a, 4) if a.size == 1 else a[:4])
            self.scale_factors.copy_(torch.from_numpy(np.stack(sf)), non_blocking=True)
            self.desc.scale_factors = L.ptr(self.scale_factors)
        else:
            self.desc.scale_factors = L.ptr(None)

    def run(self):
        L.check(L.lib.dsl_fcos_detect(C.byref(self.desc), L.stream_ptr()), 'dsl_fcos_detect')


FLIP_CODES = {None: 0, 'horizontal': 1, 'vertical': 2, 'diagonal': 3}      # DSL_FLIP_* (bit 0: x, bit 1: y)


class AugMerge:
    """The candidate pool of one original image over `nviews` views, and the merged detections ([1, max_per_img, 5] etc.).
    `collect(view, dp, ...)` takes a view's bound DetectPlan (n == 1; its geometry may differ from the other views'),
    `finish(rescale)` runs the score threshold, sort, class-offset NMS (or Soft-NMS, `nms_method`) and max_per_img cut over the pool; count[0] = -1 says that a
    view was missing from the pool (finish consumes the views' records: every image collects all of its views again)."""

    def __init__(self, nviews, nlvl, device, num_classes=80, nms_pre=1000, max_per_img=100, score_thr=0.05, iou_thr=0.5,
                 nms_method=0, soft_sigma=0.0, soft_min_score=0.0):
        if nviews > L.MAX_AUG:
            raise ValueError(f'test-time augmentation: {nviews} views, at most {L.MAX_AUG} (DSL_MAX_AUG) are merged')
        d = L.DetDesc()
        d.nms_method, d.soft_sigma, d.soft_min_score = nms_method, soft_sigma, soft_min_score
        d.nlvl, d.n = nlvl, 1
        d.num_classes, d.nms_pre, d.max_per_img = num_classes, nms_pre, max_per_img
        d.score_thr, d.iou_thr = score_thr, iou_thr
        self.dets = torch.zeros(1, max_per_img, 5, device=device)
        self.labels = torch.zeros(1, max_per_img, dtype=torch.int64, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        d.dets, d.det_labels, d.det_count = L.ptr(self.dets), L.ptr(self.labels), L.ptr(self.count)
        self.bytes = int(L.lib.dsl_detect_aug_workspace_bytes(C.byref(d), nviews))
        if self.bytes == 0:
            raise RuntimeError(f'dsl_detect_aug_workspace_bytes: {L.lib.dsl_last_error().decode()}')
        self.pool = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.desc, self.nviews = d, nviews

    def collect(self, view, dp, img_shape, scale_factor, flip=False, flip_direction=None):
        if dp.n != 1:
            raise ValueError(f'test-time augmentation takes one image per view (aug_test_bboxes: "only one image in the batch"), got {dp.n}')
        dp.set_meta([img_shape], [scale_factor], True)          # the map-back always divides by the view's scale factor
        code = FLIP_CODES[flip_direction or 'horizontal'] if flip else 0
        L.check(L.lib.dsl_fcos_detect_collect(C.byref(dp.desc), C.byref(self.desc), view, self.nviews, code, L.ptr(self.pool), self.bytes,
                                              L.stream_ptr()), 'dsl_fcos_detect_collect')

    def finish(self, rescale):
        L.check(L.lib.dsl_fcos_detect_finish(C.byref(self.desc), self.nviews, int(bool(rescale)), L.ptr(self.pool), self.bytes,
                                             L.stream_ptr()), 'dsl_fcos_detect_finish')
        return self.dets, self.labels, self.count


SOFT_METHODS = {'linear': L.NMS_LINEAR, 'gaussian': L.NMS_GAUSSIAN, 'naive': L.NMS_NAIVE}      # mmcv.ops.soft_nms's `method`


def _test_cfg(det):
    """test_cfg -> the keyword arguments of DetectPlan / AugMerge.  nms.type 'nms' (or absent): the hard NMS, iou_threshold 0.5;
    'soft_nms': mmcv.ops.soft_nms's keys and defaults (iou_threshold 0.3, sigma 0.5, min_score 1e-3, method 'linear')."""
    cfg = det.test_cfg or {}
    nms = cfg.get('nms', {})
    kind = nms.get('type', 'nms')
    if kind not in ('nms', 'soft_nms'):
        raise NotImplementedError(f"test_cfg.nms.type={kind!r}: the detection post-processing builds 'nms' and 'soft_nms'")
    soft = kind == 'soft_nms'
    out = dict(nms_pre=cfg.get('nms_pre', 1000), max_per_img=cfg.get('max_per_img', 100), score_thr=cfg.get('score_thr', 0.05),
               iou_thr=nms.get('iou_threshold', nms.get('iou_thr', 0.3 if soft else 0.5)), nms_method=L.NMS_HARD, soft_sigma=0.0,
               soft_min_score=0.0)
    if soft:
        method = nms.get('method', 'linear')
        if method not in SOFT_METHODS:
            raise ValueError(f'test_cfg.nms.method={method!r}: soft_nms has {sorted(SOFT_METHODS)}')
        out.update(nms_method=SOFT_METHODS[method], soft_sigma=float(nms.get('sigma', 0.5)), soft_min_score=float(nms.get('min_score', 1e-3)))
    return out


def _detplan(det, plan, store, N):
    dp = getattr(plan, 'detplan', None)
    if dp is None:
        dp = DetectPlan(N, plan.level_sizes, det.bbox_head.strides, store.device, num_classes=store.num_classes,
                        ld_cls=store.logit_ld, head=store.head, **_test_cfg(det))
        dp.bind(plan.bufs['cls_logits'], plan.bufs['regctr'], store.scales_ptr())
        plan.detplan = dp
    return dp


def detect_device(det, img, img_metas, rescale=False, store=None, single_stream=False):
    """Forward + post-processing; returns (dets [N,100,5], labels [N,100], count [N]) on the GPU."""
    eng = det._get_engine()
    store = store or det.store
    N, _, H, W = img.shape
    plan = eng.plan(store, N, H, W, training=False, single_stream=single_stream)
    plan.bind_image(img)
    plan.fwd.run()
    dp = _detplan(det, plan, store, N)
    dp.set_meta([m['img_shape'] for m in img_metas], [m.get('scale_factor', 1.0) for m in img_metas], rescale)
    dp.run()
    return dp.dets, dp.labels, dp.count


def bbox2result(bboxes, labels, num_classes):
    """core/bbox/transforms.py:99-116."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    return [bboxes[labels == i, :] for i in range(num_classes)]


def simple_test(det, img, img_metas, rescale=False, store=None):
    dets, labels, count = detect_device(det, img, img_metas, rescale, store)
    dets, labels, count = dets.cpu().numpy(), labels.cpu().numpy(), count.cpu().numpy()
    return [bbox2result(dets[i, :count[i]], labels[i, :count[i]], det.bbox_head.num_classes) for i in range(len(count))]


def aug_test_device(det, imgs, img_metas, rescale=False, store=None):
    """Per view: forward + collect into the image's pool; then one finish.  Returns (dets [1,100,5], labels [1,100], count [1])
    on the GPU, in the original image's coordinates when `rescale`, else in the first view's (dense_test_mixins.py:99-104)."""
    eng = det._get_engine()
    store = store or det.store
    nviews = len(imgs)
    cfg = _test_cfg(det)
    pools = det._aug_merges.setdefault(store, {})          # weakly keyed by the store object (an id() could be reused once it is freed)
    key = (nviews, tuple(sorted(cfg.items())))
    mg = pools.get(key)
    if mg is None:
        mg = pools[key] = AugMerge(nviews, len(det.bbox_head.strides), store.device, num_classes=store.num_classes, **cfg)
    for v, (img, metas) in enumerate(zip(imgs, img_metas)):
        N, _, H, W = img.shape
        if N != 1 or len(metas) != 1:
            raise ValueError(f'test-time augmentation takes one image per view (aug_test_bboxes: "only one image in the batch"), got {N}')
        plan = eng.plan(store, N, H, W, training=False)
        plan.bind_image(img)
        plan.fwd.run()
        m = metas[0]
        mg.collect(v, _detplan(det, plan, store, N), m['img_shape'], m.get('scale_factor', 1.0), m.get('flip', False),
                   m.get('flip_direction'))
    return mg.finish(rescale)


def aug_test(det, imgs, img_metas, rescale=False, store=None):
    """SingleStageDetector.aug_test: a one-element list of per-class arrays."""
    dets, labels, count = aug_test_device(det, imgs, img_metas, rescale, store)
    dets, labels, k = dets.cpu().numpy(), labels.cpu().numpy(), int(count.cpu()[0])
    if k < 0:
        raise RuntimeError('dsl_fcos_detect_finish: a view of the pool was not collected for this image, or with another nlvl / nms_pre / '
                           'num_classes than the pool\'s (det_count = -1)')
    return [bbox2result(dets[0, :k], labels[0, :k], det.bbox_head.num_classes)]

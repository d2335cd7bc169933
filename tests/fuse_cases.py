"""Inputs of the pseudo_fuse_kernel edge tests (tests/test_detect_edges_gpu.py; tests/test_detect_edges_cpu.py checks what each one
hits with dsl_amd.pseudo.fuse_host).  dets [k, 5] float32 (x1, y1, x2, y2, score), labels [k] int64."""
import numpy as np

C = 6
PARSE = float(np.float32(0.3))
NMS_THR = float(np.float32(0.1))
f32 = np.float32


def _apart(k):
    """k boxes that do not touch each other."""
    x = 40.0 * np.arange(k, dtype=np.float32)
    return np.stack([x + 1.5, np.full(k, 2.5, f32), x + 31.25, np.full(k, 30.75, f32)], 1)


def _dets(boxes, scores):
    return np.concatenate([np.asarray(boxes, f32), np.asarray(scores, f32)[:, None]], 1)


def rounding_ties():
    """Rows 0 and 1 (one class): 0.4000001 < 0.4000004, both 0.4 after rounding to 6 decimals - row 0 stays in front."""
    return _dets(_apart(4), [0.4000001, 0.4000004, 0.5, 0.4000004]), np.array([2, 2, 2, 4], np.int64)


def threshold_rules():
    """Row 0: score == parse_thr (kept); row 1: one ulp below (parsed out); row 2: one ulp above fp32(0.1), which rounds to
    nms_thr itself and is dropped by the strict score_threshold of the second NMS."""
    s = [f32(PARSE), np.nextafter(f32(PARSE), f32(0)), np.nextafter(f32(NMS_THR), f32(1))]
    return _dets(_apart(3), s), np.array([1, 1, 1], np.int64)


def truncation():
    """int() truncates toward zero: rows 0 and 1 become [0,0,16,16] and [0,0,16,8], IoU exactly 0.5 = iou_thr (both kept);
    row 2 becomes [-3,-2,10,7], not [-4,-3,10,7]."""
    b = [[0.9, 0.2, 16.7, 16.99], [-0.5, 0.3, 16.2, 8.9], [-3.7, -2.2, 10.5, 7.9]]
    return _dets(b, [0.9, 0.8, 0.7]), np.zeros(3, np.int64)


def label_range():
    return _dets(_apart(4), [0.9, 0.8, 0.7, 0.6]), np.array([-1, C, 0, C - 1], np.int64)


def random_dets(seed, k):
    """k detections with labels in -1 .. C, overlapping boxes of a 200 x 200 image, scores in 0.02 .. 0.98."""
    r = np.random.RandomState(seed)
    xy = r.uniform(-5, 150, (k, 2)).astype(f32)
    wh = r.uniform(4, 60, (k, 2)).astype(f32)
    return _dets(np.concatenate([xy, xy + wh], 1), r.uniform(0.02, 0.98, k)), r.randint(-1, C + 1, k).astype(np.int64)


def random_old(seed, k):
    """k stored labels: boxes and scores as a label file holds them (whole coordinates, 6-decimal scores; some at or below
    nms_thr, some labels out of range)."""
    d, l = random_dets(seed, k)
    return dict(rects=np.trunc(d[:, :4]).astype(f32), tags=l, scores=np.round(d[:, 4].astype(np.float64), 6).astype(f32))

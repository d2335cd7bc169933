"""fp32 model of the Soft-NMS pass of detect.hip (dsl_det_desc.nms_method != 0) and the synthetic inputs of
tests/test_soft_nms_cpu.py / tests/test_soft_nms_gpu.py (no reference files are read here).

The rule is mmcv's batched_nms with nms=dict(type='soft_nms'), as the reference's mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127 states
it, per image and class over the candidates detect_ref / aug_ref hand the hard NMS (score threshold, nms_pre, the best CAND_CAP):

  repeat   pick the remaining candidate of the class with the highest CURRENT score - equal scores: the lowest candidate number,
           the order detect_ref documents for the hard NMS -, emit it with that score, multiply every other remaining score of the
           class by w(IoU(pick, other)), drop the candidates whose score is now < min_score
  then     the emitted detections of all classes by rescored score, descending (equal scores: ascending candidate number), the
           first max_per_img

  linear   w = 1 - iou if iou > iou_thr else 1      gaussian   w = exp(-iou * iou / sigma)      naive   w = 0 if iou > iou_thr else 1

Operation order is the kernel's: IoU = inter / (sa + sb - inter) on the class-offset boxes box + label * (max + 1) with the pick as
`a` (iou_gt's expression, so that 'naive' decides exactly as the hard NMS), w in fp32, score * w.  0 / 0 of two zero-area boxes is
no overlap.  `bound=False` runs every class to its end instead of stopping it after max_per_img picks: the two must agree."""
import numpy as np
import torch

import aug_ref as A
import detect_ref as R

METHODS = {'linear': 1, 'gaussian': 2, 'naive': 3}              # DSL_NMS_*
F = np.float32


def valid_pairs(boxes, scores, cens, score_thr, cap=R.CAND_CAP):
    """aug_ref.finish's candidate stage: boxes [K, 4], labels [K], final scores [K] of the valid pairs in candidate order."""
    row, lab = torch.nonzero(scores > score_thr, as_tuple=True)
    final = (scores * cens[:, None])[row, lab]
    if len(row) > cap:
        keep = final.sort(descending=True, stable=True)[1][:cap].sort()[0]
        row, lab, final = row[keep], lab[keep], final[keep]
    return boxes[row].numpy().astype(F), lab.numpy(), final.numpy().astype(F)


def weight(method, iou, iou_thr, sigma):
    if method == 'gaussian':
        with np.errstate(invalid='ignore'):
            return np.where(iou > 0, np.exp(-(iou * iou) / F(sigma)), F(1)).astype(F)
    with np.errstate(invalid='ignore'):
        over = iou > F(iou_thr)
    return np.where(over, F(1) - iou if method == 'linear' else F(0), F(1)).astype(F)


def soft_nms(b, lab, final, iou_thr, max_per_img, method, sigma=0.5, min_score=1e-3, bound=True):
    """Returns dets [k, 5], labels [k] and a record: per pick the relative gap between the two highest current scores of its class
    ('pick_gaps'), the exp arguments of the gaussian decays ('exp_args'), the emitted scores in output order before the cut
    ('emitted') and the largest number of decays an emitted candidate went through ('n_decays')."""
    rec = dict(pick_gaps=[], exp_args=[], emitted=None, n_decays=0)
    if len(final) == 0:
        rec['emitted'] = np.zeros(0, F)
        return torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), rec
    ob = (b + (lab.astype(F) * (b.max() + F(1)))[:, None]).astype(F)
    area = ((ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1])).astype(F)
    cur = final.copy()
    emitted = []
    for c in np.unique(lab):
        idx = np.nonzero(lab == c)[0]                            # ascending candidate number
        live = np.ones(len(idx), bool)
        decays = np.zeros(len(idx), int)
        picks = 0
        while live.any() and not (bound and picks == max_per_img):
            s = np.where(live, cur[idx], F(-1))
            m = int(np.argmax(s))                                # the first of equal scores
            top = np.sort(s[live])[::-1]
            if len(top) > 1:
                rec['pick_gaps'].append(float((top[0] - top[1]) / top[0]) if top[0] > 0 else 0.0)
            i = idx[m]
            emitted.append(i)
            rec['n_decays'] = max(rec['n_decays'], int(decays[m]))
            live[m] = False
            picks += 1
            o = idx[live]
            wh = np.maximum(np.minimum(ob[i, 2:], ob[o, 2:]) - np.maximum(ob[i, :2], ob[o, :2]), F(0))
            inter = wh[:, 0] * wh[:, 1]
            with np.errstate(invalid='ignore', divide='ignore'):
                iou = (inter / (area[i] + area[o] - inter)).astype(F)
            if method == 'gaussian':
                rec['exp_args'].append((-(iou * iou) / F(sigma))[iou > 0])
            w = weight(method, iou, iou_thr, sigma)
            cur[o] = cur[o] * w
            decays[live] += w != 1
            live[live] = ~(cur[o] < F(min_score))
    e = np.array(sorted(emitted), dtype=np.int64)
    e = e[np.argsort(-cur[e].astype(np.float64), kind='stable')]
    rec['emitted'] = cur[e]
    e = e[:max_per_img]
    dets = np.concatenate([b[e], cur[e, None]], 1)
    return torch.from_numpy(dets), torch.from_numpy(lab[e]), rec


def detect(case, method, sigma=0.5, min_score=1e-3, bound=True, max_per_img=None):
    """Per image (dets, labels, record) of a detect_ref.Case."""
    return [soft_nms(*valid_pairs(*R.candidates(case, i), case.score_thr), case.iou_thr, max_per_img or case.max_per_img, method, sigma,
                     min_score, bound) for i in range(case.n)]


def aug(views, metas, nms_pre, score_thr, iou_thr, max_per_img, method, sigma=0.5, min_score=1e-3):
    """aug_ref.aug_test_bboxes with the Soft-NMS over the pooled candidates of the views (rescale=True)."""
    parts = [A.collect(*v, m['img_shape'], m['scale_factor'], m['flip_direction'] if m['flip'] else None, nms_pre, False)
             for v, m in zip(views, metas)]
    return soft_nms(*valid_pairs(*[torch.cat([p[k] for p in parts]) for k in range(3)], score_thr), iou_thr, max_per_img, method, sigma,
                    min_score)


# ---- tolerances -------------------------------------------------------------------------------------------------------------------
ULP_PER_DECAY = 2.0 ** -22                                       # "a few fp32 ulp per decay": IoU's five roundings reach w, then one product
# Largest relative error of this model's fp32 exp against the fp64 exp of the same fp32 argument over the gaussian decays of every
# input below: measured 1.73e-7 (test_soft_nms_cpu.py::test_exp_error_is_the_recorded_one measures it again and holds it to this)
EXP_ERR = 1.8e-7


def score_rtol(n_decays, method):
    per = ULP_PER_DECAY + (4 * EXP_ERR if method == 'gaussian' else 0.0)
    return n_decays * per


def exp_error(args):
    """max |fp32 exp - fp64 exp| / fp64 exp over fp32 arguments."""
    a = np.concatenate(args) if len(args) else np.zeros(0, F)
    if a.size == 0:
        return 0.0
    want = np.exp(a.astype(np.float64))
    return float(np.max(np.abs(np.exp(a).astype(np.float64) - want) / want))


# ---- synthetic inputs -------------------------------------------------------------------------------------------------------------
LEVELS = {1: [(4, 6)], 2: [(4, 6), (2, 3)]}                     # strides 8, 16 on a 32 x 48 image: 24 / 30 locations
SHAPE = (32, 48)
LONG = [(8, 12), (2, 3)]                                        # 64 x 96 at stride 8, (2 x 3 at stride 16 covers its top left): 102 locations
# (levels, C) -> the first seed whose inputs have the margin property test_soft_nms_cpu.py::test_competing_scores_are_far_apart asserts
SEEDS = {(1, 3): 2, (1, 80): 1, (2, 3): 1, (2, 80): 1, ('long', 3): 299, ('long', 80): 1125}
AUG_SEED = 3
AUG_CLUSTER = 14 + 11                                           # the pooled cluster of aug_views


def _locations(sizes):
    out = []
    for l, (h, w) in enumerate(sizes):
        s = A.STRIDES[l]
        out += [(l, y * w + x, x * s + s // 2, y * s + s // 2) for y in range(h) for x in range(w)]
    return out


def make_inputs(sizes, shape, C, n, seed, cluster=None, single=True):
    """Per image: one class holds a cluster - every location (or the first `cluster`) predicts a box that covers almost the whole
    image, corners jittered by up to an eighth of the image in steps of 1/8 pixel (exact in fp32 through decode and clip), pairwise
    IoU 0.55 - 1 -, one class holds exactly one candidate, with C > 3 one more class a pair (both at locations of the cluster, with
    their boxes), every other class nothing (logit -50).  Class numbers move with the image.  Scores and centerness are seeded."""
    g = torch.Generator().manual_seed(seed)
    H, W = shape
    cls = [torch.full((n, C, h, w), -50.0) for h, w in sizes]
    raw = [torch.full((n, 4, h, w), 0.25) for h, w in sizes]
    ctr = [torch.zeros(n, 1, h, w) for h, w in sizes]
    locs = _locations(sizes)
    for i in range(n):
        c_cluster, c_single, c_pair = (1 + 16 * i) % C, (0 + 3 * i) % C, (2 + 37 * i) % C
        if C == 3:
            c_cluster, c_single = (1 + i) % 3, (0 + i) % 3       # class (2 + i) % 3 stays empty
            c_pair = None
        members = locs if cluster is None else locs[:cluster]
        for l, p, px, py in members:
            s = A.STRIDES[l]
            j = torch.randint(0, 8 * min(H, W) // 8 + 1, (4,), generator=g).float() / 8.0
            x1, y1, x2, y2 = min(float(j[0]), px), min(float(j[1]), py), max(W - float(j[2]), px), max(H - float(j[3]), py)
            R.flat(raw[l], i)[:, p] = torch.tensor([px - x1, py - y1, x2 - px, y2 - py]) / s
            R.flat(cls[l], i)[c_cluster, p] = float(torch.rand(1, generator=g) * 4.0 - 1.0)      # sigmoid: 0.27 .. 0.95
            R.flat(ctr[l], i)[0, p] = float(torch.rand(1, generator=g) * 3.0)
        if single:
            l, p, px, py = locs[(7 + 5 * i) % len(locs)]
            R.flat(cls[l], i)[c_single, p] = float(torch.rand(1, generator=g) * 2.0)
        if c_pair is not None:
            for l, p, px, py in (locs[0], locs[23]):
                R.flat(cls[l], i)[c_pair, p] = float(torch.rand(1, generator=g) * 2.0)
    return cls, raw, ctr


def case(levels, C, max_per_img, iou_thr=0.3, seed=None):
    """n = 2 on LEVELS[levels] ('long': LONG, a cluster of 70 of its 102 locations - more than a wave)."""
    sizes, shape, cluster = (LONG, (64, 96), 70) if levels == 'long' else (LEVELS[levels], SHAPE, None)
    cls, raw, ctr = make_inputs(sizes, shape, C, 2, SEEDS[levels, C] if seed is None else seed, cluster)
    return R.Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=max_per_img, score_thr=0.05, iou_thr=iou_thr, img_shapes=[shape] * 2)


def cluster_size(levels):
    return 70 if levels == 'long' else sum(h * w for h, w in LEVELS[levels])


LONG_MIN_SCORE = 1e-30                                           # keeps a whole cluster in the running: the longest chain of decays


def exact_case(kind):
    """Inputs whose sigmoids are exact on every device (logit 0 -> 0.5f, 50 -> 1.0f), for the legs without a decay in the output.
    'empty': no valid pair.  'drop': class 1 at all 24 locations with the cluster's near-identical boxes, one of them at score 1,
    the others at 0.5 - every other candidate decays below min_score = 0.45 at the first pick and the class emits one box."""
    sizes = LEVELS[1]
    cls, raw, ctr = make_inputs(sizes, SHAPE, 3, 2, 5, single=False)
    for c, t in zip(cls, ctr):
        t[:] = 50.0
        c[:] = torch.where(c > -50.0, torch.zeros(()), c)
        if kind == 'empty':
            c[:] = -50.0
    if kind == 'drop':
        for i in range(2):
            R.flat(cls[0], i)[(1 + i) % 3, 9 + i] = 50.0
    return R.Case(cls, raw, ctr, 3, nms_pre=1000, max_per_img=100, score_thr=0.05, iou_thr=0.3, img_shapes=[SHAPE] * 2)


def aug_views(seed=AUG_SEED):
    """Two views of a 64 x 96 image: itself, and its half-size horizontal flip; two levels each."""
    v0 = make_inputs([(8, 12), (4, 6)], (64, 96), 3, 1, seed, cluster=14)
    v1 = make_inputs([(4, 6), (2, 3)], (32, 48), 3, 1, seed + 1, cluster=11)
    metas = [dict(img_shape=(64, 96, 3), scale_factor=np.ones(4, F), flip=False, flip_direction=None),
             dict(img_shape=(32, 48, 3), scale_factor=np.full(4, 0.5, F), flip=True, flip_direction='horizontal')]
    return [v0, v1], metas


def min_gap(rec):
    """The smallest relative gap between two scores that compete: for a pick, or for adjacent places of the pooled output."""
    e = rec['emitted'].astype(np.float64)
    gaps = list(rec['pick_gaps']) + list((e[:-1] - e[1:]) / e[:-1])
    return min(gaps) if gaps else 1.0

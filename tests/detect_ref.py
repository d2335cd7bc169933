"""fp32 model of dsl_fcos_detect with the tie rules detect.hip documents stated explicitly, and the structured inputs of
tests/test_detect_edges_cpu.py / tests/test_detect_edges_gpu.py (no reference files are read here).

The model is aug_ref.collect (one view, no flip) + aug_ref.finish per image, in the kernel's operation order wherever a result is a
decision: decode, clip, division by the 4-element scale factor, class offset label * (max + 1), IoU = inter / (sa + sb - inter),
strict comparisons.  Where the reference leaves a choice among equal values to torch.topk / sort, the rules are the kernel's:

  per-level top-k   stable descending sort of the keys, the first nms_pre, back in index order (zero keys included)
  candidates        (level, index-ordered slot, class) order
  the cap           the first CAND_CAP of a stable descending sort of the final scores, back in candidate order
  the NMS order     stable descending sort of the final score

test_detect_edges_cpu.py pins the model to oracle.fcos_oracle.get_bboxes on tie-free inputs and proves, from the model alone, that
every structured input below has the property it was built for.

Inputs are built so that equality on the device does not depend on expf: tied scores come from bit-identical logits, distinct
scores are >= 2e-5 apart, and boxes are exact - raw distances are dyadic fractions (0.25, 2, k / 8 on level 0, 0.5 / stride) with
scales == 1, so that raw * stride is a whole or half pixel count (the 1-pixel boxes) and decode and clip are exact in fp32."""
import numpy as np
import torch

import aug_ref as A

CAND_CAP = 16384                                               # detect.hip
NMS_THREADS = 1024
SIZES = [(24, 32), (12, 16), (6, 8), (3, 4), (2, 2)]           # 768 + 192 + 48 + 12 + 4 = 1 024 locations
STRIDES = A.STRIDES
SHAPE = (192, 256)
PS = [h * w for h, w in SIZES]
SEG = 256                                                      # ordered_compact's wave segment at P = 768 (16 waves, 64 * 4 granules)
KEY_LOGITS = (2.0, 1.0, 0.0, -1.0)                             # the four centerness logits of the tied inputs


class Case:
    def __init__(self, cls, raw, ctr, C, nms_pre, max_per_img=100, score_thr=0.05, iou_thr=0.5, img_shapes=None, scale_factors=None,
                 rescale=False):
        self.cls, self.raw, self.ctr, self.C = cls, raw, ctr, C
        self.n = cls[0].shape[0]
        self.nms_pre, self.max_per_img, self.score_thr, self.iou_thr = nms_pre, max_per_img, score_thr, iou_thr
        self.img_shapes = img_shapes or [SHAPE] * self.n
        self.scale_factors = scale_factors or [1.0] * self.n
        self.rescale = rescale

    def image(self, i):
        """The n == 1 case of image i (a view of the collect / finish tests)."""
        return Case([x[i:i + 1] for x in self.cls], [x[i:i + 1] for x in self.raw], [x[i:i + 1] for x in self.ctr], self.C, self.nms_pre,
                    self.max_per_img, self.score_thr, self.iou_thr, [self.img_shapes[i]], [self.scale_factors[i]], self.rescale)

    def permuted(self, order):
        idx = torch.tensor(order)
        return Case([x[idx] for x in self.cls], [x[idx] for x in self.raw], [x[idx] for x in self.ctr], self.C, self.nms_pre,
                    self.max_per_img, self.score_thr, self.iou_thr, [self.img_shapes[i] for i in order],
                    [self.scale_factors[i] for i in order], self.rescale)


def sf4(s):
    a = np.asarray(s, np.float32).reshape(-1)
    return np.repeat(a, 4) if a.size == 1 else a[:4]


def select(keys, k):
    """Indices of the top k keys of one level, in index order: ties (zero keys too) go to the lowest indices."""
    if not 0 < k < len(keys):
        return torch.arange(len(keys))
    return keys.sort(descending=True, stable=True)[1][:k].sort()[0]


def level_keys(case, img, lvl):
    sc = case.cls[lvl][img].reshape(case.C, -1).t().sigmoid()
    return (sc * case.ctr[lvl][img].reshape(-1).sigmoid()[:, None]).max(1)[0]


def candidates(case, img):
    """Boxes [R, 4], scores [R, C], centerness [R] of image `img` after the per-level top-k, rows in (level, slot) order."""
    v = case.image(img)
    sf = sf4(case.scale_factors[img]) if case.rescale else np.ones(4, np.float32)
    return A.collect(v.cls, v.raw, v.ctr, case.img_shapes[img], sf, None, case.nms_pre, False)


def detect(case, cap=CAND_CAP, max_per_img=None, cap_keeps='lowest'):
    """Per image: dets [k, 5], labels [k], number of valid pairs.  cap_keeps='highest': the wrong cut, for the tests of the inputs."""
    return [A.finish(*candidates(case, i), score_thr=case.score_thr, iou_thr=case.iou_thr,
                     max_per_img=max_per_img or case.max_per_img, cap=cap, cap_keeps=cap_keeps) for i in range(case.n)]


def final_scores(case, img):
    """Final scores of the valid pairs of image `img`, in candidate order."""
    _, s, c = candidates(case, img)
    row, lab = torch.nonzero(s > case.score_thr, as_tuple=True)
    return (s * c[:, None])[row, lab]


def iou_fp32(a, b):
    """iou_gt's expression on two boxes (fp32 tensors of 4)."""
    w = (torch.min(a[2], b[2]) - torch.max(a[0], b[0])).clamp(min=0)
    h = (torch.min(a[3], b[3]) - torch.max(a[1], b[1])).clamp(min=0)
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


# ---- structured inputs ------------------------------------------------------------------------------------------------------------
def blank(n, C, cls=-50.0, ctr=50.0, raw=0.25):
    """No valid pair (sigmoid(-50) = 2e-22), centerness sigmoid(50) == 1.0f, boxes of half a stride: no two of a level overlap, and
    boxes of different levels have IoU <= 0.25."""
    return ([torch.full((n, C, h, w), cls) for h, w in SIZES], [torch.full((n, 4, h, w), raw) for h, w in SIZES],
            [torch.full((n, 1, h, w), ctr) for h, w in SIZES])


def flat(t, img):
    """[n, K, h, w] -> the [K, P] view of image img."""
    return t[img].reshape(t.shape[1], -1)


def groups(seed):
    """Per level: one of four key groups per location (0: highest key), seeded."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 4, (P,), generator=g) for P in PS]


def fill_tied(cls, ctr, img, C, seed, cls_logit=3.0):
    """Every location: class loc % C at `cls_logit`, centerness logit KEY_LOGITS[group]: keys and final scores take four values,
    and which locations a level's top-k picks shows in the output as (class, box)."""
    grp = groups(seed)
    for l, P in enumerate(PS):
        loc = torch.arange(P)
        flat(cls[l], img)[loc % C, loc] = cls_logit
        flat(ctr[l], img)[0] = torch.tensor(KEY_LOGITS)[grp[l]]
    return grp


def tie_cut(keys, k):
    """The k-th key's tie group of one level: (members per wave segment, need = how many of them belong to the top k)."""
    kth = keys.sort(descending=True)[0][k - 1]
    tie = keys == kth
    need = k - int((keys > kth).sum())
    return [int(tie[s:s + SEG].sum()) for s in range(0, len(keys), SEG)], need


def topk_ties(which, seed=11):
    """Level 0 (768 locations = three wave segments) selects nms_pre < 768 keys out of four distinct values; the k-th key's group is
    the second highest, cut in its first / second / third segment.  'both_select': nms_pre = 110, levels 0 and 1 both select and
    cut inside a tie group, levels 2 - 4 take everything."""
    C = 5
    cls, raw, ctr = blank(1, C)
    grp = fill_tied(cls, ctr, 0, C, seed)
    g0 = grp[0]
    top = int((g0 == 0).sum())
    t = [int((g0[s:s + SEG] == 1).sum()) for s in range(0, 768, SEG)]
    k = {'within_first': top + t[0] // 2, 'beyond_first': top + t[0] + t[1] // 2, 'third': top + t[0] + t[1] + t[2] // 2,
         'both_select': 110}[which]
    return Case(cls, raw, ctr, C, nms_pre=k, max_per_img=NMS_THREADS)


def all_equal():
    """The untrained head: one logit everywhere.  Levels 0 and 1 keep their lowest 100 indices."""
    C = 3
    cls, raw, ctr = blank(1, C, cls=-2.0, ctr=0.0)
    return Case(cls, raw, ctr, C, nms_pre=100, max_per_img=NMS_THREADS)


FEW_POS = (torch.arange(40) * 19 + 3) % 768                     # level 0's locations with a positive key


def few_positive(which, max_per_img):
    """nms_pre = 100.  Level 0: 40 positive keys, 728 keys exactly 0 (centerness logit -200); level 1: 192 zero keys; levels 2 - 4 are
    taken whole.  'one': of the zero-key locations only level 0's location 5 has a class above score_thr - a valid pair of final
    score 0; 'all': every zero-key location has one."""
    C = 4
    cls, raw, ctr = blank(1, C, ctr=0.0)
    for l, P in enumerate(PS):
        loc = torch.arange(P)
        if l < 2:
            flat(ctr[l], 0)[0] = -200.0
            if which == 'all':
                flat(cls[l], 0)[loc % C, loc] = 3.0
        else:
            flat(cls[l], 0)[loc % C, loc] = 3.0
    flat(ctr[0], 0)[0, FEW_POS] = torch.tensor(KEY_LOGITS)[torch.arange(40) % 4]
    flat(cls[0], 0)[FEW_POS % C, FEW_POS] = 3.0
    flat(cls[0], 0)[2, 5] = 3.0
    return Case(cls, raw, ctr, C, nms_pre=100, max_per_img=max_per_img)


def logit(p):
    return torch.log(p / (1 - p)).float()


TIE_P = 0.2                                                     # the tied final score
HEAD_LOCS = [24 + 25 * j for j in range(40)]                    # 2 - 3 per 64-location wave segment of det_compact_kernel


def tied_layout(n_ties, sig_locs, head_base):
    """One image, C = 20, every location selected, centerness 1.0f: 40 distinct 'head' scores head_base + 1e-3 j > TIE_P (one pair
    at each of HEAD_LOCS, boxes of half a stride) and n_ties pairs that share the score TIE_P, handed out in (location, class) order:
    2 classes at a 'signature' location (sig_locs; box of half a stride, so each such pair has a (class, box) of its own and nothing
    suppresses it), 20 classes at every other location, whose box is the whole image - same-class duplicates, of which the NMS keeps
    the first one per class.  Returns the inputs and, per tie in candidate order, whether it is a signature pair."""
    C = 20
    cls, raw, ctr = blank(1, C)
    lg = torch.full((sum(PS), C), -50.0)
    rw = torch.full((sum(PS), 4), 0.25)
    tie = float(logit(torch.tensor(TIE_P, dtype=torch.float64)))
    is_sig, left = [], n_ties
    for i in range(sum(PS)):
        if i in HEAD_LOCS:
            j = HEAD_LOCS.index(i)
            lg[i, i % C] = logit(torch.tensor(head_base + 1e-3 * j, dtype=torch.float64))
            continue
        sig = i in sig_locs
        classes = sorted([i % C, (i + 7) % C]) if sig else list(range(C))
        if not sig:
            rw[i] = 64.0                                          # 64 strides >= 512 pixels: clipped to the image on every side
        for c in classes[:left]:
            lg[i, c] = tie
            is_sig.append(sig)
        left -= min(left, len(classes))
    assert left == 0
    o = 0
    for l, P in enumerate(PS):
        flat(cls[l], 0)[:] = lg[o:o + P].t()
        flat(raw[l], 0)[:] = rw[o:o + P].t()
        o += P
    return (cls, raw, ctr), is_sig


def survivors_inside(is_sig, n_above, n_above_surviving):
    """What the NMS keeps of the best CAND_CAP pairs: the surviving heads, one whole-image box per class, and every signature pair
    among the ties that the cap keeps (the lowest candidate numbers)."""
    return n_above_surviving + 20 + sum(is_sig[:CAND_CAP - n_above])


TIED_SIG = [0, 6, 12, 18, 30] + list(range(560, 1024, 8))


def at_cap(delta, which, max_per_img=100):
    """C = 20, every location selected: exactly CAND_CAP + delta valid pairs.
    'distinct': the first 819 locations' 20 classes and 4 + delta classes of the next (819 * 20 + 4 = 16 384); scores
    0.3 + 2e-5 * rank, ranks shuffled over the pairs, centerness 1.0f.
    'zeros': the same, but only 25 locations (500 pairs) keep centerness 1, every other location's centerness sigmoid is 0: fewer
    positive scores than CAND_CAP, and the valid zero scores are the tie group that fills the cap.
    'tied' (max_per_img is set here): tied_layout - 40 heads above one tie group of CAND_CAP + delta - 40 pairs that straddles rank
    CAND_CAP when delta > 0.  The signature pairs sit at five early locations and at every 8th location from 560 on, on both sides
    of the cut; max_per_img is one less than the survivors inside the cap, so that the output holds the heads, 20 whole-image boxes
    and every signature pair in front of the cut but the last: a cut that keeps other members of the group than the lowest candidate
    numbers changes dets and labels."""
    C = 20
    nv = CAND_CAP + delta
    if which == 'tied':
        (cls, raw, ctr), is_sig = tied_layout(nv - 40, TIED_SIG, 0.6)
        return Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=survivors_inside(is_sig, 40, 40) - 1)
    cls, raw, ctr = blank(1, C)
    rank = torch.randperm(nv, generator=torch.Generator().manual_seed(5)).double()
    lg = logit(0.3 + 2e-5 * rank)
    full = torch.cat([flat(c, 0).t() for c in cls])              # [1024, C] copy, rows in (level, location) order
    full.view(-1)[:nv] = lg
    o = 0
    for l, P in enumerate(PS):
        flat(cls[l], 0)[:] = full[o:o + P].t()
        if which == 'zeros':
            loc = torch.arange(P)
            flat(ctr[l], 0)[0, (o + loc) % 33 != 0] = -200.0     # 25 of the first 820 locations keep centerness 1
        o += P
    return Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=max_per_img)


def score_ties():
    """Two final scores over 2 048 candidates of 8 classes, boxes of 4 strides: a level's same-class neighbours one row apart
    overlap with IoU 0.6 and are suppressed, and many more than max_per_img = 100 survive."""
    C = 8
    cls, raw, ctr = blank(1, C, ctr=0.0, raw=2.0)
    for l, P in enumerate(PS):
        loc = torch.arange(P)
        lg = torch.where((loc // 5) % 2 == 0, 2.0, 1.0)
        flat(cls[l], 0)[loc % 4, loc] = lg
        flat(cls[l], 0)[4 + loc % 3, loc] = lg
    return Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=100)


def put_box(cls, raw, x, y, ltrb, c, lg):
    """Level 0, image 0: location (x, y) -> box centre (8x + 4, 8y + 4) -/+ ltrb pixels, class c at logit lg."""
    loc = y * SIZES[0][1] + x
    flat(raw[0], 0)[:, loc] = torch.tensor(ltrb, dtype=torch.float32) / 8.0
    flat(cls[0], 0)[c, loc] = lg


THR_BOXES = dict(A=(2, 2), B=(3, 2), C=(10, 2), D=(11, 2), E=(18, 2), F=(19, 2), H0=(2, 10), H1=(6, 10))


def thresholds(score_thr):
    """Level 0, integer boxes, centerness 1.0f; all coordinates and the class offset label * (max + 1) = label * 161 are whole numbers
    far below 2^24, so the offset boxes and their IoU are exact in fp32 whatever the class:
      A [16,16,32,32] / B [16,16,32,24], class 7: IoU 128 / 256 == 0.5 == iou_thr - both kept (strict >)
      C [80,16,96,32] / D [80,16,96,25], class 7: IoU 144 / 256 - D suppressed
      E [144,16,160,32] class 7 / F [144,16,160,25] class 3: the same pair in two classes - both kept
      H0, H1: logit 0, score exactly 0.5f: invalid at score_thr = 0.5, valid just below."""
    C = 10
    cls, raw, ctr = blank(1, C)
    big, half, more = (4, 4, 12, 12), (12, 4, 4, 4), (12, 4, 4, 5)
    put_box(cls, raw, *THR_BOXES['A'], big, 7, 3.0)
    put_box(cls, raw, *THR_BOXES['B'], half, 7, 2.0)
    put_box(cls, raw, *THR_BOXES['C'], big, 7, 3.5)
    put_box(cls, raw, *THR_BOXES['D'], more, 7, 2.5)
    put_box(cls, raw, *THR_BOXES['E'], big, 7, 4.0)
    put_box(cls, raw, *THR_BOXES['F'], more, 3, 1.5)
    put_box(cls, raw, *THR_BOXES['H0'], (2, 2, 2, 2), 1, 0.0)
    put_box(cls, raw, *THR_BOXES['H1'], (2, 2, 2, 2), 1, 0.0)
    return Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=100, score_thr=score_thr, iou_thr=0.5)


BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))


def degenerate():
    """img_shape 100 x 130 on the 192 x 256 map: locations beyond it clip to zero width and / or height, same-class boxes of a row
    become identical zero-area boxes and their IoU is 0 / 0."""
    C = 3
    cls, raw, ctr = blank(1, C, ctr=0.0)
    fill_tied(cls, ctr, 0, C, 23)
    return Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=NMS_THREADS, img_shapes=[(100, 130)])


BATCH_SHAPES = [(192, 256), (150, 200), (100, 130)]
BATCH_SF = [[1.25, 1.2, 1.25, 1.2], [0.8, 0.75, 0.8, 0.75], [1.5, 1.6, 1.5, 1.6]]


def batch(rescale):
    """n = 3: image 0 without a valid pair, image 1 with exactly one (level 2), image 2 full (the tied pattern; level 0 selects)."""
    C = 5
    cls, raw, ctr = blank(3, C)
    flat(cls[2], 1)[4, 9] = 1.0
    flat(ctr[2], 1)[0, 9] = 0.5
    fill_tied(cls, ctr, 2, C, 31)
    return Case(cls, raw, ctr, C, nms_pre=300, max_per_img=100, img_shapes=BATCH_SHAPES, scale_factors=BATCH_SF, rescale=rescale)


def many_survivors(C, max_per_img):
    """1-pixel boxes around 1 024 distinct centres, two classes per location, four tied scores: 2 048 candidates that all survive.
    C == 1 has one pair per location and so exactly 1 024 survivors - more are not possible on 1 024 locations with one class, as
    two pairs of a location share their box: there max_per_img = 1 024 is met exactly, not exceeded."""
    cls, raw, ctr = blank(1, C, ctr=0.0)
    grp = groups(41)
    for l, P in enumerate(PS):
        raw[l][:] = 0.5 / STRIDES[l]
        loc = torch.arange(P)
        lg = torch.tensor(KEY_LOGITS)[grp[l]]
        flat(cls[l], 0)[loc % C, loc] = lg
        flat(cls[l], 0)[(loc + max(C // 2, 1)) % C, loc] = lg
    return Case(cls, raw, ctr, C, nms_pre=1000, max_per_img=max_per_img)


AUG_SIG1 = list(range(40, 400, 8))


def aug_tie_at_cap():
    """Two views of 20 480 pairs each, both tied_layout: view 0 with CAND_CAP - 3 000 ties and heads from 0.6, view 1 with 6 000 ties
    and heads from 0.7 at the same (location, class) boxes, which suppress view 0's.  CAND_CAP + 3 080 pairs are valid; the cut
    lies inside view 1's ties, between its signature pairs (every 8th location from 40 to 400), and max_per_img is one less than
    the survivors inside the cap."""
    (c0, r0, t0), sig0 = tied_layout(CAND_CAP - 3000, TIED_SIG, 0.6)
    (c1, r1, t1), sig1 = tied_layout(6000, AUG_SIG1, 0.7)
    m = survivors_inside(sig0 + sig1, 80, 40) - 1
    return [Case(c0, r0, t0, 20, nms_pre=1000, max_per_img=m), Case(c1, r1, t1, 20, nms_pre=1000, max_per_img=m)]


def aug_empty():
    return [Case(*blank(1, 20), 20, nms_pre=1000), Case(*blank(1, 20), 20, nms_pre=1000)]


def aug_ref(views, cap=CAND_CAP, max_per_img=None, cap_keeps='lowest'):
    v = views[0]
    metas = [dict(img_shape=SHAPE + (3,), scale_factor=np.ones(4, np.float32), flip=False, flip_direction=None) for _ in views]
    return A.aug_test_bboxes([(x.cls, x.raw, x.ctr) for x in views], metas, v.nms_pre, False, rescale=True, cap=cap,
                             score_thr=v.score_thr, iou_thr=v.iou_thr, max_per_img=max_per_img or v.max_per_img, cap_keeps=cap_keeps)

"""tests/detect_ref.py without a GPU: the model agrees exactly with oracle.fcos_oracle.get_bboxes where no two keys or scores are
equal, and every structured input of tests/test_detect_edges_gpu.py has the property it was built for.  Only the model is used
here, never the kernel."""
import numpy as np
import pytest
import torch

import aug_ref as A
import detect_ref as R
from dsl_amd.pseudo import fuse_host

CAP = R.CAND_CAP


@pytest.mark.parametrize('C,sf,rescale', [(80, [[1.25, 1.2, 1.25, 1.2], [0.8, 0.75, 0.8, 0.75]], True), (3, [1.5, 0.5], True),
                                          (3, [1.5, 0.5], False)])
def test_model_equals_the_oracle_without_ties(C, sf, rescale):
    """n = 2, per-image img_shape, a 4-vector and a scalar scale factor; level 0 goes through the top-k."""
    from oracle import fcos_oracle as O
    g = torch.Generator().manual_seed(100 + C)
    sizes = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]
    views = [A.view_inputs(g, C, sizes, False) for _ in range(2)]
    cls, raw, ctr = ([torch.cat([v[k][l] for v in views]) for l in range(5)] for k in range(3))
    shapes = [(96, 128), (80, 100)]
    case = R.Case(cls, raw, ctr, C, nms_pre=50, img_shapes=shapes, scale_factors=sf, rescale=rescale)
    for i in range(2):
        keys = R.level_keys(case, i, 0)
        assert len(keys.unique()) == len(keys)
        assert len(R.final_scores(case, i).unique()) == len(R.final_scores(case, i))
    px = [torch.relu(r) * s for r, s in zip(raw, R.STRIDES)]
    sfs = [R.sf4(s).tolist() for s in sf]
    batched = O.get_bboxes(cls, px, ctr, torch.tensor(shapes, dtype=torch.float32), sfs, nms_pre=50, rescale=rescale)
    for i, (b, l, nvalid) in enumerate(R.detect(case)):
        # the oracle on image i alone: bit for bit.  (In the batched call the image's logits sit at other offsets of the tensor, and
        # torch's vectorised CPU sigmoid rounds the last bit of a few elements differently between its vector body and its scalar
        # tail: there the scores may differ by one ulp, everything else is still equal.)
        rb, rl = O.get_bboxes([x[i:i + 1] for x in cls], [x[i:i + 1] for x in px], [x[i:i + 1] for x in ctr],
                              torch.tensor(shapes[i:i + 1], dtype=torch.float32), sfs[i:i + 1], nms_pre=50, rescale=rescale)[0]
        assert 20 <= len(rb) and nvalid < CAP
        assert torch.equal(b, rb) and torch.equal(l, rl)
        bb, bl = batched[i]
        assert torch.equal(l, bl) and torch.equal(b[:, :4], bb[:, :4]) and torch.allclose(b[:, 4], bb[:, 4], rtol=2e-7, atol=0)


def test_the_inputs_saturate_as_intended():
    t = torch.tensor([50.0, -200.0, 0.0]).sigmoid()
    assert t[0] == 1.0 and t[1] == 0.0 and t[2] == 0.5
    assert float(torch.tensor(-50.0).sigmoid()) > 0        # an invalid pair, not a zero key


@pytest.mark.parametrize('which', ['within_first', 'beyond_first', 'third'])
def test_topk_tie_group_is_cut_inside_and_spans_segments(which):
    case = R.topk_ties(which)
    keys = R.level_keys(case, 0, 0)
    assert len(keys) == 3 * R.SEG and case.nms_pre < len(keys) and len(keys.unique()) == 4
    per_seg, need = R.tie_cut(keys, case.nms_pre)
    assert sum(1 for t in per_seg if t > 0) >= 2
    assert 0 < need < sum(per_seg)                                    # cut strictly inside the group
    if which == 'within_first':
        assert need < per_seg[0]
    elif which == 'beyond_first':
        assert per_seg[0] < need < per_seg[0] + per_seg[1]
    else:
        assert per_seg[0] + per_seg[1] < need
    # a wrong choice among the ties changes the output: every selected location shows as a (class, box) of its own, and sure takes
    # lie behind the first tie that is left out, so that one tie too many shifts their slots
    sel = R.select(keys, case.nms_pre)
    kth = keys.sort(descending=True)[0][case.nms_pre - 1]
    left_out = torch.nonzero(keys == kth).squeeze(1)[need]
    assert int((keys[left_out:] > kth).sum()) > 0
    b, l, nvalid = R.detect(case)[0]
    assert nvalid == case.nms_pre + sum(R.PS[1:]) == len(b) <= case.max_per_img
    lvl0 = {(int(c), tuple(x.tolist())) for c, x in zip(l, b[:, :4]) if x[2] - x[0] == 4}
    assert lvl0 == {(int(i) % 5, (8.0 * (int(i) % 32) + 2, 8.0 * (int(i) // 32) + 2, 8.0 * (int(i) % 32) + 6, 8.0 * (int(i) // 32) + 6)) for i in sel}


def test_both_select_mixes_selecting_and_whole_levels():
    case = R.topk_ties('both_select')
    assert [P > case.nms_pre for P in R.PS] == [True, True, False, False, False]
    for lvl in (0, 1):
        per_seg, need = R.tie_cut(R.level_keys(case, 0, lvl), case.nms_pre)
        assert 0 < need < sum(per_seg)
    assert R.detect(case)[0][2] == 2 * case.nms_pre + sum(R.PS[2:])


def test_all_equal_keeps_the_lowest_indices():
    case = R.all_equal()
    for lvl in (0, 1):
        keys = R.level_keys(case, 0, lvl)
        assert len(keys.unique()) == 1
        assert torch.equal(R.select(keys, case.nms_pre), torch.arange(case.nms_pre))
    b, l, nvalid = R.detect(case)[0]
    assert nvalid == 3 * (200 + sum(R.PS[2:])) == len(b)


@pytest.mark.parametrize('which,max_per_img,zeros_out', [('one', 20, 0), ('one', 1024, 1), ('all', 1024, 161)])
def test_few_positive_keys(which, max_per_img, zeros_out):
    case = R.few_positive(which, max_per_img)
    k0, k1 = R.level_keys(case, 0, 0), R.level_keys(case, 0, 1)
    assert int((k0 > 0).sum()) == 40 < case.nms_pre < len(k0) and int((k0 == 0).sum()) == 728 and int((k1 == 0).sum()) == 192
    sel = R.select(k0, case.nms_pre)
    zero_idx = torch.nonzero(k0 == 0).squeeze(1)
    assert set(sel.tolist()) == set(R.FEW_POS.tolist()) | set(zero_idx[:60].tolist())
    assert 5 in sel.tolist() and float(k0[5]) == 0.0                  # the zero-key location with a class above score_thr
    fs = R.final_scores(case, 0)
    assert int((fs == 0).sum()) == (1 if which == 'one' else 161)          # 'all': 60 + 100 zero-key locations, two classes at location 5
    b, l, nvalid = R.detect(case)[0]
    survivors = len(R.detect(case, max_per_img=4096)[0][0])
    assert (survivors > max_per_img) == (max_per_img == 20)
    assert len(b) == min(survivors, max_per_img)
    assert int((b[:, 4] == 0).sum()) == zeros_out                     # the score-0 boxes come out when there is room for them
    if zeros_out:
        assert bool((b[-zeros_out:, 4] == 0).all())


@pytest.mark.parametrize('which,max_per_img', [('distinct', 100), ('zeros', 1024)])
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_valid_counts_at_the_path_switch(delta, which, max_per_img):
    case = R.at_cap(delta, which, max_per_img)
    fs = R.final_scores(case, 0)
    assert len(fs) == CAP + delta
    srt = fs.sort(descending=True)[0]
    if which == 'distinct':
        assert bool((R.candidates(case, 0)[2][:820] == 1.0).all())
        assert float((srt[:-1] - srt[1:]).min()) > 1e-5
    else:
        assert int((fs > 0).sum()) == 500 < CAP and float(srt[500]) == 0.0
    b, l, nvalid = R.detect(case, cap=CAP)[0]
    assert nvalid == CAP + delta
    inside = len(R.detect(case, cap=CAP, max_per_img=4096)[0][0])      # survivors inside the cap: the documented deviation does not apply
    assert inside > max_per_img and len(b) == max_per_img
    if which == 'zeros':
        assert int((b[:, 4] > 0).sum()) == 500 and int((b[:, 4] == 0).sum()) == 524


COMPACT_SEG = 1280                                                    # det_compact_kernel's wave segment at 20 480 pairs


def tie_cut_of_the_cap(fs):
    """Of final scores in candidate order: (is a member of the tie group, need = members inside the best CAND_CAP)."""
    kth = fs.sort(descending=True)[0][CAP - 1]
    return fs == kth, CAP - int((fs > kth).sum())


@pytest.mark.parametrize('delta', [-1, 0, 1, 2000])
def test_tied_at_the_cap_shows_the_cut_in_the_output(delta):
    case = R.at_cap(delta, 'tied')
    _, scores, cens = R.candidates(case, 0)
    assert bool((cens == 1.0).all())
    valid = (scores > case.score_thr).reshape(-1)                     # pair index = candidate order
    fs = R.final_scores(case, 0)
    assert len(fs) == CAP + delta and len(fs.unique()) == 41 and int((fs == fs.min()).sum()) == CAP + delta - 40
    srt = fs.sort(descending=True)[0]
    assert float((srt[:39] - srt[1:40]).min()) > 5e-4 and srt[39] > srt[40] + 0.3
    inside = len(R.detect(case, max_per_img=4096)[0][0])
    assert inside == case.max_per_img + 1 > 100                       # more survive inside the cap than are asked for
    b, l, nvalid = R.detect(case)[0]
    assert nvalid == CAP + delta and len(b) == case.max_per_img
    small = (b[:, 2] - b[:, 0] == 4) & (b[:, 4] == fs.min())          # signature pairs of level 0 in the output
    if delta > 0:
        tie, need = tie_cut_of_the_cap(fs)
        assert srt[CAP - 1] == srt[CAP] and 0 < need < int(tie.sum())    # the group straddles rank CAND_CAP, cut strictly inside
        pair = torch.nonzero(valid).squeeze(1)[tie]                   # pair indices of the group's members
        cut = int(pair[need])                                         # the first member that is left out
        # heads lie behind the cut (a tie too many moves or drops them), and the output holds signature pairs right up to the cut
        head_pair = torch.nonzero(valid).squeeze(1)[~tie]
        assert int((head_pair > cut).sum()) >= 2
        last_sig_x = float(b[small][-1, 0])
        assert last_sig_x > 0
        wrong = R.detect(case, cap_keeps='highest')[0]
        assert not (torch.equal(wrong[0], b) and torch.equal(wrong[1], l))      # another cut changes dets and labels
    if delta == 2000:
        segs = lambda p: {int(x) // COMPACT_SEG for x in p}
        assert len(segs(pair[:need])) >= 2 and len(segs(pair[need:])) >= 2      # members on both sides of the cut in several wave segments
        # signature pairs on both sides, the ones in front in the output
        loc_cut = cut // 20
        assert any(i < loc_cut for i in R.TIED_SIG[5:]) and any(loc_cut < i < 1000 and valid[i * 20:(i + 1) * 20].any() for i in R.TIED_SIG[5:])
        assert int(small.sum()) >= 30


def test_score_ties_reach_the_nms():
    case = R.score_ties()
    fs = R.final_scores(case, 0)
    assert len(fs) == 2048 and len(fs.unique()) == 2
    full = R.detect(case, max_per_img=4096)[0]
    assert case.max_per_img < len(full[0]) < 2048                      # some are suppressed, many more than max_per_img survive
    b, l, _ = R.detect(case)[0]
    assert len(l.unique()) >= 7 and len(b[:, 4].unique()) == 1         # the first 100 all carry the higher score, in many classes


def test_thresholds_sit_exactly_on_the_bounds():
    case = R.thresholds(0.5)
    boxes, scores, cens = R.candidates(case, 0)
    w = R.SIZES[0][1]
    row = {k: y * w + x for k, (x, y) in R.THR_BOXES.items()}
    assert bool((cens == 1.0).all())
    assert float(scores[row['H0'], 1]) == 0.5 == float(scores[row['H1'], 1]) and R.BELOW_HALF < 0.5
    offs = boxes[(scores > 0.05).any(1)].max() + 1.0
    assert float(offs) == 161.0
    ob = lambda k, c: boxes[row[k]] + torch.tensor(float(c)) * offs
    assert boxes[row['A']].tolist() == [16, 16, 32, 32] and boxes[row['B']].tolist() == [16, 16, 32, 24]
    assert float(R.iou_fp32(ob('A', 7), ob('B', 7))) == 0.5 == case.iou_thr          # exactly the threshold, offset included
    assert float(R.iou_fp32(ob('C', 7), ob('D', 7))) == 0.5625
    assert float(R.iou_fp32(ob('E', 7), ob('F', 3))) == 0.0 and float(R.iou_fp32(boxes[row['E']], boxes[row['F']])) == 0.5625
    b, l, nvalid = R.detect(case)[0]
    assert nvalid == 6 and l.tolist() == [7, 7, 7, 7, 3]               # E, C, A, B, F by score; D is gone
    assert b[:, :4].tolist() == [boxes[row[k]].tolist() for k in 'ECABF']
    b2, l2, nvalid2 = R.detect(R.thresholds(R.BELOW_HALF))[0]
    assert nvalid2 == 8 and l2.tolist() == [7, 7, 7, 7, 3, 1, 1] and b2[5:, 4].tolist() == [0.5, 0.5]


def test_degenerate_boxes_have_undefined_iou():
    case = R.degenerate()
    b, l, nvalid = R.detect(case)[0]
    assert nvalid == 1024 == len(b)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert int((area == 0).sum()) > 300
    # identical zero-area boxes of one class: 0 / 0
    i = next(i for i in range(len(b)) if area[i] == 0 and any(torch.equal(b[j, :4], b[i, :4]) and l[j] == l[i] for j in range(i)))
    j = next(j for j in range(i) if torch.equal(b[j, :4], b[i, :4]) and l[j] == l[i])
    assert torch.isnan(R.iou_fp32(b[i, :4], b[j, :4]))


@pytest.mark.parametrize('rescale', [True, False])
def test_batch_has_an_empty_a_single_and_a_full_image(rescale):
    case = R.batch(rescale)
    assert len(set(case.img_shapes)) == 3 and all(len(set(s)) > 1 for s in case.scale_factors)
    out = R.detect(case)
    assert [o[2] for o in out] == [0, 1, 300 + sum(R.PS[1:])]
    assert [len(o[0]) for o in out] == [0, 1, case.max_per_img]
    per_seg, need = R.tie_cut(R.level_keys(case, 2, 0), case.nms_pre)
    assert 0 < need < sum(per_seg)
    other = R.detect(R.batch(not rescale))
    assert not torch.equal(out[2][0][:, :4], other[2][0][:, :4])          # the scale factor is applied only when asked for


@pytest.mark.parametrize('C', [1, 3, 80])
def test_many_survivors(C):
    case = R.many_survivors(C, 1024)
    b, l, nvalid = R.detect(case, max_per_img=4096)[0]
    # nothing is suppressed.  C == 1: one pair per location, so 1 024 survivors is all that 1 024 locations can give - there
    # max_per_img = 1 024 is met exactly; C = 3 and 80 exceed it
    assert nvalid == len(b) == (1024 if C == 1 else 2048)
    assert len(b[:, 4].unique()) == 4
    assert bool((b[:, 2] - b[:, 0] <= 1).all() and (b[:, 3] - b[:, 1] <= 1).all())
    assert len(R.detect(R.many_survivors(C, 1))[0][0]) == 1


def test_aug_pools():
    views = R.aug_tie_at_cap()
    b, l, nvalid = R.aug_ref(views)
    assert nvalid == CAP + 3080 and len(b) == views[0].max_per_img
    fs = torch.cat([R.final_scores(v, 0) for v in views])
    tie, need = tie_cut_of_the_cap(fs)
    n0 = len(R.final_scores(views[0], 0))
    assert 0 < need < int(tie.sum()) and int(tie[:n0].sum()) < need           # the cut lies inside view 1's ties
    assert len(R.aug_ref(views, max_per_img=4096)[0]) == views[0].max_per_img + 1 > 100
    assert bool((b[:40, 4] > 0.699).all()) and int((b[:, 4] > 0.5).sum()) == 40      # view 1's heads lead and suppress view 0's twins
    wrong = R.aug_ref(views, cap_keeps='highest')
    assert not (torch.equal(wrong[0], b) and torch.equal(wrong[1], l))
    b, l, nvalid = R.aug_ref(R.aug_empty())
    assert nvalid == 0 and len(b) == 0


# ---- pseudo_fuse_kernel's inputs: what each is meant to hit, by dsl_amd.pseudo.fuse_host ------------------------------------------
def test_fuse_inputs():
    import fuse_cases as F
    f32 = np.float32
    # rounding ties: unequal before, equal after; the earlier detection first
    d, l = F.rounding_ties()
    assert d[0, 4] < d[1, 4] and round(float(d[0, 4]), 6) == round(float(d[1, 4]), 6)
    out = fuse_host(d, l, F.PARSE, 0.5, F.NMS_THR, F.C)
    assert out['tags'].tolist() == [2, 2, 2, 4] and out['rects'][1:3].tolist() == np.trunc(d[:2, :4]).tolist()      # behind row 2's 0.5
    # thresholds
    d, l = F.threshold_rules()
    assert d[0, 4] == f32(F.PARSE) and d[1, 4] < f32(F.PARSE) and d[2, 4] > f32(F.NMS_THR) and f32(round(float(d[2, 4]), 6)) == f32(F.NMS_THR)
    out = fuse_host(d, l, F.PARSE, 0.5, F.NMS_THR, F.C)
    assert out['rects'].tolist() == [np.trunc(d[0, :4]).tolist()]
    out = fuse_host(d, l, 0.05, 0.5, F.NMS_THR, F.C)
    assert len(out['rects']) == 2                                        # the rounded score == nms_thr stays out even when parsed
    # truncation
    d, l = F.truncation()
    assert (d[:, :4] < 0).any() and (d[:, :4] != np.trunc(d[:, :4])).any()
    t = torch.from_numpy(np.trunc(d[:, :4]))
    assert float(R.iou_fp32(t[0], t[1])) == 0.5 and float(R.iou_fp32(torch.from_numpy(d[0, :4]), torch.from_numpy(d[1, :4]))) != 0.5
    assert len(fuse_host(d, l, F.PARSE, 0.5, F.NMS_THR, F.C)['rects']) == 3
    # labels
    d, l = F.label_range()
    assert set(l.tolist()) >= {-1, F.C, 0, F.C - 1}
    assert sorted(fuse_host(d, l, F.PARSE, 0.5, F.NMS_THR, F.C)['tags'].tolist()) == [0, F.C - 1]

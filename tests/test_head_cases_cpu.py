"""The generated head cases (tests/head_cases.py) are what tests/test_head_cases_gpu.py needs: every mixture fit's decisions lie at
least 1e-9 from their thresholds - the device adds its float64 sums in butterfly order, numpy in sequence; over at most 80 terms
below 1e4 that differs by about 1e-12 -, the cases reach the code paths they exist for, and the models evaluate them in seconds."""
import time

import numpy as np
import pytest
import torch

import atss_ref as AR
import head_cases as HC
import paa_ref as PR


@pytest.fixture(scope='module')
def refs():
    t = time.time()
    out = {k: HC.ref(k) for k in HC.ASSIGN_CASES}
    out['MIX'] = HC.mix()
    out['seconds'] = time.time() - t
    return out


def box_of(c, image, box):
    return sum(len(g) for g in c['gts'][:image]) + box


def test_the_models_evaluate_every_case_in_seconds(refs):
    print('all cases, both assignments, candidate losses and reassignments:', refs['seconds'], 's')
    assert refs['seconds'] < 30.0
    for k in HC.ASSIGN_CASES:
        c = HC.case(k)
        assert c['M'] == c['B'] * sum(h * w for h, w in c['sizes']) and tuple(c['cls'].shape) == (c['M'], c['C'])
    assert HC.case('G70')['M'] == 5118 and len(HC.case('G2L')['sizes']) == 2 and HC.case('R')['C'] == 80


@pytest.mark.parametrize('name', ['G70', 'G64', 'G2L', 'GT', 'MIX'])
def test_boxes_lie_on_the_half_pixel_grid(name):
    c = HC.mix() if name == 'MIX' else HC.case(name)
    for g in c['gts']:
        assert bool((g * 2 == (g * 2).round()).all()) and (len(g) == 0 or (float(g.min()) >= 0 and float(g.max()) <= 512))
    r = torch.cat(HC.case('R')['gts'])
    assert not bool((r * 2 == (r * 2).round()).all())


@pytest.mark.parametrize('name', HC.ASSIGN_CASES + ('MIX',))
def test_margins_of_every_mixture_fit(refs, name):
    re = refs[name]['re']
    rows = [(k, b['flag'], b['n_iter'], len(b['index'])) + HC.box_margins(b) for k, b in enumerate(re['boxes'])]
    for r in rows:
        print(name, 'box %d flag %d iterations %d samples %d margin %.3e gap %.3e' % r)
    assert HC.thin_margins(re) == []
    for b in re['boxes']:          # var_margin is reported wherever a fit ran
        assert b['flag'] == 1 or b['var_margin'] >= HC.MARGIN


def test_sample_counts_flags_and_ties_are_present(refs):
    m = refs['MIX']
    boxes = m['re']['boxes']
    counts = [len(b['index']) for b in boxes]
    assert counts == HC.MIX_COUNTS and {80, 70, 65, 64, 63, 2, 1, 0} <= set(counts)
    assert [len(g) for g in m['gts']] == [4, 0, 5, 5]                       # an image without boxes between two that have some
    flags = [b['flag'] for b in boxes]
    laws = [b[2] for b in HC.MIX_BOXES]
    assert flags[laws.index('bad')] == 2 and boxes[laws.index('bad')]['n_iter'] == 1
    nat = boxes[laws.index('flag2')]
    assert nat['flag'] == 2 and nat['n_iter'] > 1 and len(nat['index']) == 23
    assert all(f == 1 for f, n in zip(flags, counts) if n < 2) and all(f != 1 for f, n in zip(flags, counts) if n >= 2)
    assert sum(m['re']['npos']) > 0 and any(b['flag'] == 0 and b['n_iter'] >= 10 for b in boxes)
    # a level with more candidates than topk (the cut) and one with fewer (the break), in one box
    cand = m['cand_gt'].numpy()
    assert max(HC.MIX_BOXES[0][1]) > 16 > min(HC.MIX_BOXES[1][1]) > 0 and int((cand >= 0).sum()) > sum(counts)
    # bit-equal losses: at the arg-max (gap exactly 0) and across the top-k cut of a level
    ties = [k for k, b in enumerate(boxes) if b['flag'] == 0 and b['gap'] == 0.0 and HC.gap_is_a_tie(b)]
    assert ties and all(laws[k] == 'tie' for k in ties)
    ms = PR.mstarts(m['sizes'], m['B'])
    cut = 0
    for k in [i for i, law in enumerate(laws) if law == 'tie']:
        img, g = HC.MIX_BOXES[k][0], k - box_of(m, HC.MIX_BOXES[k][0], 0)
        for l, (h, w) in enumerate(m['sizes']):
            lo = int(ms[l]) + img * h * w
            x = np.sort(m['pos_loss'].numpy()[lo:lo + h * w][cand[lo:lo + h * w] == g])
            cut += len(x) > 16 and x[15] == x[16]
    assert cut > 0


def test_g70_and_g64_reach_the_second_sample(refs):
    """The big box of image 0: 70 samples with anchor_scale 4 (16 / 16 / 16 / 16 / 6 of 169 / 101 / 45 / 19 / 6 candidates), exactly
    64 with anchor_scale 8 and none on the last level; the ATSS assignment of G70 selects 70 candidates per box."""
    c = HC.case('G70')
    cand, ms = refs['G70']['paa']['cand_gt'].numpy(), PR.mstarts(c['sizes'], c['B'])
    per = [int((cand[int(ms[l]):int(ms[l]) + h * w] == 0).sum()) for l, (h, w) in enumerate(c['sizes'])]
    assert per == [169, 101, 45, 19, 6]
    assert len(refs['G70']['re']['boxes'][0]['index']) == 70 and refs['G70']['re']['boxes'][0]['flag'] == 0
    b = refs['G64']['re']['boxes'][0]
    lvl = np.searchsorted(ms, b['index'], side='right') - 1
    assert len(b['index']) == 64 and [int((lvl == l).sum()) for l in range(5)] == [16, 16, 16, 16, 0]
    cands = AR.assign_image(c['sizes'], c['gts'][0], c['gls'][0], c['pads'][0], c['topk'], c['anchor_scale'], c['C'])[4]
    assert [len(x) for x in cands] == [70]
    assert [len(g) for g in c['gts']] == [1, 0, 3] and min(refs['G70']['atss']['npos'][0], refs['G70']['atss']['npos'][2]) > 0
    assert sum(refs['G70']['re']['npos']) > 0 and (c['M'] + 255) // 256 == 20


def test_gt_reaches_the_corner_rules(refs):
    c = HC.case('GT')
    a, p = refs['GT']['atss'], refs['GT']['paa']
    assert [len(g) for g in c['gts']] == [5, 0, 1, 7] and c['C'] == 18
    P = sum(h * w for h, w in c['sizes'])
    split = [h * w for h, w in c['sizes']]

    def image(t, i):          # level-major -> the locations of image i in level order
        o, out = 0, []
        for n in split:
            out.append(t[o + i * n:o + (i + 1) * n])
            o += c['B'] * n
        return torch.cat(out)
    # the duplicate pair (boxes 0 and 2 of image 0): ATSS gives every shared anchor to the lower, PAA's arg-max too, its low-quality
    # pass (the anchors at the pair's maximum IoU) to the higher
    assert torch.equal(c['gts'][0][0], c['gts'][0][2]) and int(c['gls'][0][0]) != int(c['gls'][0][2])
    ai, pc = image(a['assign_idx'], 0), image(p['cand_gt'], 0)
    assert int((ai == 0).sum()) > 0 and int((ai == 2).sum()) == 0
    assert int((pc == 0).sum()) > 0 and int((pc == 2).sum()) > 0
    anchors = torch.cat(AR.level_anchors(c['sizes'], c['anchor_scale']))
    iou = AR.iou_matrix(anchors, c['gts'][0])
    assert bool((iou[pc == 2, 2] == iou[:, 2].max()).all()) and bool((iou[pc == 0, 0] < iou[:, 0].max()).all())
    # the zero-area box (box 2 of image 3): best IoU 0, and with min_pos_iou = 0 it holds every valid anchor of zero IoU that no
    # later box takes; ATSS gives it nothing.  The box beyond the pad shape (box 4): no ATSS positive either
    z = c['gts'][3][2]
    assert float((z[2] - z[0]) * (z[3] - z[1])) == 0.0
    pc3, ai3 = image(p['cand_gt'], 3), image(a['assign_idx'], 3)
    assert int((pc3 == 2).sum()) > 100 and int((ai3 == 2).sum()) == 0 and int((ai3 == 4).sum()) == 0
    b = c['gts'][3][4]
    assert float(b[0]) >= c['pads'][3][1] and float(b[1]) >= c['pads'][3][0]
    assert int((image(a['cls_weight'], 3) == 0).sum()) > 0 and len(pc3) == P
    # the box centred on (24, 32): on level 1 its nine candidates end inside a quartet of equidistant anchors
    g = c['gts'][0][4]
    cx, cy = float(g[0] + g[2]) / 2, float(g[1] + g[3]) / 2
    assert (cx, cy) == (24.0, 32.0)
    ctr = AR.level_anchors(c['sizes'], c['anchor_scale'])[1]
    d = (((ctr[:, 0] + ctr[:, 2]) / 2 - cx).pow(2) + ((ctr[:, 1] + ctr[:, 3]) / 2 - cy).pow(2)).sqrt().sort()[0]
    assert float(d[8]) == float(d[9]) and int((d == d[8]).sum()) == 4 and c['topk'] == 9
    d0 = (((anchors[:320, 0] + anchors[:320, 2]) / 2 - cx).pow(2) + ((anchors[:320, 1] + anchors[:320, 3]) / 2 - cy).pow(2)).sqrt().sort()[0]
    assert float(d0[0]) == 0.0 and float(d0[1]) == float(d0[4]) == 8.0


def test_pads_and_levels_off_the_fixture_geometry():
    for k in ('G70', 'G2L', 'GT', 'R'):
        c = HC.case(k)
        off = [p for p in c['pads'] if any(v % s for v in p for s in c['strides'][:2])]
        assert off and len(set(c['pads'])) == (len(c['pads']) if k != 'G70' else 2), k
    assert HC.case('G2L')['strides'] == (8, 16) and HC.case('G2L')['B'] == 1
    inv = AR.valid_masks(HC.case('G2L')['sizes'], HC.case('G2L')['pads'][0], (8, 16))
    assert all(bool(m.all()) for m in inv)          # ceil(90 / 8) = 12, ceil(141 / 8) = 18: every anchor valid, by the rounding up alone

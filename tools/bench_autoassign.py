"""Times the AutoAssign head on the shape bench.py uses (2 x 800 x 1344, 80 classes, COCO-shaped synthetic boxes):
  dsl_aa_assign beside dsl_fcos_assign and dsl_aa_loss beside dsl_fcos_loss (the default FCOS head) on the same head outputs -
  device events around CALLS launches after WARM, ROUNDS windows per launch, the two heads' windows alternating - and
  one AutoAssign step (forward_train + backward, no optimizer) beside one FCOS step, alternating as well.
Every figure is the median of its windows with their (min, max).  Prints one JSON line.
Usage: python tools/bench_autoassign.py [--steps 20] [--warmup 5] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, H, W, C = 2, 800, 1344, 80
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
CALLS, WARM = 200, 20


def boxes(rng):
    """COCO-shaped: about 7 boxes per image on average, up to 40; sides log-uniform from 12 px to most of the canvas."""
    out = []
    for k in (7, 40):
        w, h = np.exp(rng.uniform(np.log(12), np.log(700), k)), np.exp(rng.uniform(np.log(12), np.log(600), k))
        w, h = np.minimum(w, W - 1), np.minimum(h, H - 1)
        x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
        out.append(torch.from_numpy(np.stack([x, y, x + w, y + h], 1).astype('float32')))
    return out, [torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')) for b in out]


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternating(fns, calls, warm, rounds):
    """{name: [ms per call of each window]}: per round one window of every function, in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, calls))
    return out


def summary(ms, scale=1.0, digits=1):
    return dict(median=round(statistics.median(ms) * scale, digits), min=round(min(ms) * scale, digits), max=round(max(ms) * scale, digits))


def loss_plans(gtb, gtl):
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    g = torch.Generator().manual_seed(0)
    plans = {}
    for kind, head in (('fcos', HeadOptions()), ('autoassign', HeadOptions(head_kind='autoassign', bbox_weight=5.0))):
        p = FcosLossPlan(N, SIZES, 'cuda', num_classes=C, head=head, max_gt=256)
        p.set_targets(gtb, gtl)
        p.assign()
        if not plans:
            cls = (torch.randn(p.M, p.LD_CLS, generator=g) * 1.5 - 2.5).cuda()
            raw = (torch.randn(p.M, p.LD_RC, generator=g) * 1.5).cuda()
            scales = torch.ones(5).cuda()
        p.bind_outputs(cls, raw, scales)
        plans[kind] = p
    return plans


def step_fn(model, batch):
    def run():
        losses = model.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'])
        sum(losses.values()).backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from test_autoassign_cpu import aa_model_cfg
    from util import fcos_model_cfg
    rng = np.random.RandomState(0)
    gtb, gtl = boxes(rng)
    plans = loss_plans(gtb, gtl)
    torch.cuda.synchronize()
    out = dict(shape=[N, H, W], boxes=[len(b) for b in gtb], locations=plans['autoassign'].M,
               positives=dict(fcos=int(plans['fcos'].stats[0])), prior_sum=round(float(plans['autoassign'].stats[1]), 1))
    t = alternating({k: p.assign for k, p in plans.items()}, CALLS, WARM, a.rounds)
    out['assign_us'] = {k: summary(v, 1e3) for k, v in t.items()}
    t = alternating({k: p.loss for k, p in plans.items()}, CALLS, WARM, a.rounds)
    out['loss_us'] = {k: summary(v, 1e3) for k, v in t.items()}
    img = (torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(1)) * 40).cuda()
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * N
    batch = dict(img=img, img_metas=metas, gt_bboxes=gtb, gt_labels=gtl)
    models = {k: build_detector(cfg).cuda() for k, cfg in (('fcos', fcos_model_cfg()), ('autoassign', aa_model_cfg()))}
    t = alternating({k: step_fn(m, batch) for k, m in models.items()}, a.steps, a.warmup, a.rounds)
    out['step_ms'] = {k: summary(v, 1.0, 3) for k, v in t.items()}
    out['img_s'] = {k: round(N / statistics.median(v) * 1e3, 1) for k, v in t.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()

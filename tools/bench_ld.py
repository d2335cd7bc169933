"""Times Localization Distillation on the shape bench.py uses (2 x 800 x 1344, 80 classes, reg_max 16, 50 boxes per image):
  dsl_ld_loss beside dsl_gfl_loss on the same head outputs (device events around CALLS launches after WARM, three windows), and
  one LD step (teacher inference forward + student forward_train + backward, no optimizer) beside one GFL step.
Prints one JSON line.  Usage: python tools/bench_ld.py [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, H, W, C, REG_MAX, BOXES = 2, 800, 1344, 80, 16, 50
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
CALLS, WARM = 200, 20


def boxes(rng):
    out = []
    for _ in range(N):
        w, h = rng.uniform(24, 400, BOXES), rng.uniform(24, 400, BOXES)
        x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
        out.append(torch.from_numpy(np.stack([x, y, x + w, y + h], 1).astype('float32')))
    return out, [torch.from_numpy(rng.randint(0, C, BOXES).astype('int64')) for _ in range(N)]


def timed(fn, calls, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def loss_plans(gtb, gtl):
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    g = torch.Generator().manual_seed(0)
    plans = {}
    for kind in ('gfl', 'ld'):
        head = HeadOptions(head_kind='gfl', reg_max=REG_MAX, bbox_weight=2.0, ld_weight=0.25 if kind == 'ld' else None)
        p = FcosLossPlan(N, SIZES, 'cuda', num_classes=C, head=head, max_gt=256)
        p.set_targets(gtb, gtl, None, [(H, W)] * N)
        p.assign()
        if not plans:
            cls = (torch.randn(p.M, p.LD_CLS, generator=g) * 1.5 - 2.5).cuda()
            raw = (torch.randn(p.M, p.LD_RC, generator=g) * 2.0).cuda()
            soft = (torch.randn(p.M, p.LD_RC, generator=g) * 2.0).cuda()
            scales = torch.ones(5).cuda()
        p.bind_outputs(cls, raw, scales)
        p.quality()
        if kind == 'ld':
            p.bind_soft(soft, p.LD_RC, scales)
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
    a = ap.parse_args()
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from test_gfl_cpu import gfl_model_cfg
    from test_ld_cpu import ld_model_cfg
    rng = np.random.RandomState(0)
    gtb, gtl = boxes(rng)
    plans = loss_plans(gtb, gtl)
    out = dict(shape=[N, H, W], positives=int((plans['gfl'].labels < C).sum()))
    for k, p in plans.items():
        out[f'{k}_loss_us'] = [round(1e3 * t, 1) for t in timed(p.loss, CALLS, WARM)]
    img = (torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(1)) * 40).cuda()
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * N
    batch = dict(img=img, img_metas=metas, gt_bboxes=gtb, gt_labels=gtl)
    for k, cfg in (('gfl', gfl_model_cfg()), ('ld', ld_model_cfg())):
        model = build_detector(cfg).cuda()
        ms = timed(step_fn(model, batch), a.steps, a.warmup)
        out[f'{k}_step_ms'] = [round(t, 3) for t in ms]
        out[f'{k}_img_s'] = [round(N / t * 1e3, 1) for t in ms]
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Times PAA on the shape bench.py uses (2 x 800 x 1344, 80 classes, 40 boxes per image):
  DSL_OP_PAA_REFINE (dsl_paa_pos_loss + dsl_paa_reassign) and its two halves, dsl_paa_assign beside dsl_atss_assign and dsl_paa_loss
  beside the ATSS loss on the same head outputs (device events around CALLS launches after WARM, three windows), and
  one PAA step (forward_train + backward, no optimizer) beside one ATSS step.
Prints one JSON line.  Usage: python tools/bench_paa.py [--steps 20] [--warmup 5]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, H, W, C, BOXES = 2, 800, 1344, 80, 40
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
    for kind in ('atss', 'paa'):
        head = HeadOptions(assigner='atss', bbox_weight=2.0) if kind == 'atss' else HeadOptions(head_kind='paa', bbox_weight=1.3, ctr_weight=0.5)
        p = FcosLossPlan(N, SIZES, 'cuda', num_classes=C, head=head, max_gt=256)
        p.set_targets(gtb, gtl, None, [(H, W)] * N)
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
    a = ap.parse_args()
    from dsl_amd import _lib as L
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from test_atss_cpu import atss_model_cfg
    from test_paa_cpu import paa_model_cfg
    rng = np.random.RandomState(0)
    gtb, gtl = boxes(rng)
    plans = loss_plans(gtb, gtl)
    paa = plans['paa']

    def entry(name):
        return lambda: L.check(getattr(L.lib, name)(ctypes.byref(paa.paa), L.stream_ptr()), name)

    def us(fn):
        return [round(1e3 * t, 1) for t in timed(fn, CALLS, WARM)]
    paa.refine()
    torch.cuda.synchronize()
    out = dict(shape=[N, H, W], boxes_per_image=BOXES, candidates=int((paa.cand_gt >= 0).sum()), positives=int(paa.stats[0]),
               em_iterations_max=int(paa.gmm_iters.max()), em_flags=[int((paa.gmm_flags == f).sum()) for f in (1, 2)])
    out['atss_assign_us'], out['paa_assign_us'] = us(plans['atss'].assign), us(paa.assign)
    paa.assign()
    out['paa_pos_loss_us'], out['paa_reassign_us'] = us(entry('dsl_paa_pos_loss')), us(entry('dsl_paa_reassign'))
    out['paa_refine_us'] = us(paa.refine)
    out['atss_loss_us'], out['paa_loss_us'] = us(plans['atss'].loss), us(paa.loss)
    img = (torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(1)) * 40).cuda()
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * N
    batch = dict(img=img, img_metas=metas, gt_bboxes=gtb, gt_labels=gtl)
    for k, cfg in (('atss', atss_model_cfg()), ('paa', paa_model_cfg())):
        model = build_detector(cfg).cuda()
        ms = timed(step_fn(model, batch), a.steps, a.warmup)
        out[f'{k}_step_ms'] = [round(t, 3) for t in ms]
        out[f'{k}_img_s'] = [round(N / t * 1e3, 1) for t in ms]
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()

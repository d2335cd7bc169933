"""Step time of a C-class head against the 80-class one at the benchmark's shape (2 x 3 x 800 x 1344, supervised step + FlatSGD),
in one process, alternating A / B windows so that clock and thermal drift fall on both alike.

    python tools/ab_num_classes.py [C=20] [rounds=6] [steps=20]

Prints one JSON line: per-round ms / step of both, medians, and the B / A ratio."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from dsl_amd import detectors  # noqa: E402,F401  (registers the model classes)
from dsl_amd.data import mark_ready  # noqa: E402
from dsl_amd.optim import FlatSGD  # noqa: E402
from dsl_amd.registry import build_detector  # noqa: E402


def make(C, batch):
    cfg = bench.model_cfg()
    cfg['bbox_head']['num_classes'] = C
    model = build_detector(cfg)
    model.init_weights()
    model = model.cuda()
    opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))
    b = dict(batch, gt_labels=[l % C for l in batch['gt_labels']])
    ev = torch.cuda.Event()
    ev.record()

    def step():
        mark_ready(b['img'], event=ev)
        out = model.train_step(b, opt)
        out['loss'].backward()
        opt.step()
        return out
    return step


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n * 1e3
    assert all(torch.isfinite(v).all() for v in out['log_vars'].values())
    return dt


def main():
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    import warnings
    warnings.simplefilter('ignore')
    batch = bench.synth_batch(0, 2)
    a, b = make(80, batch), make(C, batch)
    window(a, 5)
    window(b, 5)
    ra, rb = [], []
    for r in range(rounds):
        first, second = ((a, ra), (b, rb)) if r % 2 == 0 else ((b, rb), (a, ra))
        for fn, acc in (first, second):
            acc.append(round(window(fn, steps), 3))
    ma, mb = statistics.median(ra), statistics.median(rb)
    print(json.dumps(dict(classes_a=80, classes_b=C, steps_per_window=steps, ms_a=ra, ms_b=rb, median_ms_a=ma, median_ms_b=mb,
                          ratio_b_over_a=round(mb / ma, 4))))


if __name__ == '__main__':
    main()

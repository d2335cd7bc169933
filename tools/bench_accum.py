"""Gradient accumulation: what it costs on the device.

  python tools/bench_accum.py kernel [--reps 50]     dsl_grad_accumulate in each mode over n_train of the full model, against
                                                      dsl_sgd_step over the same n IN THE SAME RUN (the yardstick: it moves 23
                                                      bytes per element, SET moves 8, ADD / FOLD 12); device events, one line each
  python tools/bench_accum.py step [--k 4] [--steps 40] [--rounds 3]
                                                      img/s of the full-size step (2 x 800 x 1344) in windows of k micro-steps
                                                      against plain steps, alternating, one model each in one process

Needs the GPU; prints JSON lines."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model():
    import bench
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.optim import FlatSGD
    from dsl_amd.registry import build_detector
    model = build_detector(bench.model_cfg()).cuda()
    opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))
    return model, opt


def kernel(args):
    from dsl_amd import _lib as L
    model, _ = _model()
    st = model.store
    n = st.n_train
    g = torch.randn(n, device='cuda') * 1e-3
    acc, mom = torch.zeros_like(g), torch.zeros_like(g)
    p = st.train.clone()
    p16 = torch.empty(n, dtype=torch.bfloat16, device='cuda')
    sp = L.stream_ptr()

    def acc_call(mode):
        return lambda: L.check(L.lib.dsl_grad_accumulate(L.ptr(acc), L.ptr(g), n, mode, sp), 'dsl_grad_accumulate')

    def sgd():
        L.check(L.lib.dsl_sgd_step(L.ptr(p), L.ptr(g), L.ptr(mom), L.ptr(p16), L.ptr(st.group), n, 0.0, 0.9, 1e-4, 2.0, 0.0, None, 0.0, 0, sp),
                'dsl_sgd_step')

    # bytes per element: what each kernel has to move (fp32 reads + writes, the bias flag, the bf16 copy)
    cases = [('dsl_sgd_step', sgd, 4 * 3 + 1 + 4 * 2 + 2), ('set', acc_call(L.ACC_SET), 8), ('add', acc_call(L.ACC_ADD), 12),
             ('fold', acc_call(L.ACC_FOLD), 12)]
    res = {name: [] for name, _, _ in cases}
    for rnd in range(args.rounds + 1):          # alternating; round 0 warms up
        for name, fn, _ in cases:
            if name == 'fold':
                g.mul_(0.0)          # (FOLD writes g: keep its values from growing over the repetitions)
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[name].append(e0.elapsed_time(e1) / args.reps)
    for name, _, bpe in cases:
        ms = sorted(res[name])
        med = ms[len(ms) // 2]
        print(json.dumps(dict(kernel=name, n=n, ms=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                              bytes_per_element=bpe, gb_per_s=round(n * bpe / med / 1e6, 1))), flush=True)


def step(args):
    import bench
    from dsl_amd.data import mark_ready
    batch = bench.synth_batch(0, 2)
    ready = torch.cuda.Event()
    ready.record()
    runs = {}
    for name, k in (('plain', 1), (f'k{args.k}', args.k)):
        model, opt = _model()
        model.loss_scale = 1.0 / k

        def one(i, model=model, opt=opt, k=k):
            closing = (i + 1) % k == 0
            if k > 1:
                opt.set_closing(closing)
            mark_ready(batch['img'], event=ready)
            out = model.train_step(batch, opt)
            out['loss'].backward()
            opt.step() if closing else opt.accumulate()
            return out
        for i in range(2 * max(k, 4)):
            one(i)
        torch.cuda.synchronize()
        runs[name] = one
    res = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, one in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                o = one(i)
                if (i + 1) % 10 == 0:
                    _ = {kk: float(v) for kk, v in o['log_vars'].items()}
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[name].append(round(2 * args.steps / dt, 2))
    print(json.dumps(dict(what='img/s per round, alternating', steps=args.steps, **res)), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernel', 'step'])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--k', type=int, default=4)
    ap.add_argument('--steps', type=int, default=40)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_accum.py measures on the GPU'
    assert a.steps % a.k == 0, '--steps must be a multiple of --k (whole windows)'
    {'kernel': kernel, 'step': step}[a.what](a)

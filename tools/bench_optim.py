"""The optimizer kernels over the default model's whole parameter buffer: what each costs on the device.

  python tools/bench_optim.py [--reps 25] [--rounds 5]

Times dsl_sgd_step (the yardstick, twice: `sgd_step` and `sgd_step_again` give the spread of a kernel repeated against itself in the
same alternation), dsl_optim_step(kind=SGD) on the legacy two-group table, with Nesterov momentum, and the Adam kinds, over n_train
elements.  Device events around `reps` launches, the variants alternated round by round in one process, round 0 a warm-up; at
least 100 timed launches per variant (reps x rounds).  Achieved bytes/s from the algorithmic bytes per element: SGD 23 (p, g, m
read; p, m written; 2 B bf16 copy; 1 B group id), the Adam kinds 31 (v read and written on top).  The learning rate is 0 (and
AdamW's decay with it), so that the buffers keep their values over the repetitions.

Needs the GPU; prints JSON lines."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(args):
    import bench
    from dsl_amd import _lib as L
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    model = build_detector(bench.model_cfg()).cuda()
    st = model.store
    n = st.n_train
    g = torch.randn(n, device='cuda') * 1e-3
    p = st.train.clone()
    m, v = torch.zeros_like(g), torch.zeros_like(g)
    p16 = torch.empty(n, dtype=torch.bfloat16, device='cuda')
    sp = L.stream_ptr()

    def sgd_step():
        L.check(L.lib.dsl_sgd_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(p16), L.ptr(st.group), n, 0.0, 0.9, 1e-4, 2.0, 0.0, None, 0.0, 0, sp),
                'dsl_sgd_step')

    def optim(kind, nesterov=False):
        d = L.OptimDesc()
        d.kind, d.n_groups = kind, 2
        d.lr[0], d.lr[1], d.wd[0], d.wd[1] = 0.0, 0.0, 1e-4, 0.0          # the legacy table: weights, conv biases (store.group)
        d.momentum, d.nesterov, d.first_step = 0.9, int(nesterov), 0
        d.beta1, d.beta2, d.eps, d.step_scale, d.rsqrt_bc2 = 0.9, 0.999, 1e-8, 1.0, 1.0
        vp = L.ptr(v) if kind != L.OPT_SGD else None
        return lambda: L.check(L.lib.dsl_optim_step(C.byref(d), L.ptr(p), L.ptr(g), L.ptr(m), vp, L.ptr(p16), L.ptr(st.group), n, None, sp),
                               'dsl_optim_step')

    cases = [('sgd_step', sgd_step, 23), ('optim_sgd', optim(L.OPT_SGD), 23), ('optim_nesterov', optim(L.OPT_SGD, True), 23),
             ('optim_adam', optim(L.OPT_ADAM), 31), ('optim_adamw', optim(L.OPT_ADAMW), 31), ('sgd_step_again', sgd_step, 23)]
    res = {name: [] for name, _, _ in cases}
    for rnd in range(args.rounds + 1):          # alternating; round 0 warms up
        for name, fn, _ in cases:
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
        print(json.dumps(dict(kernel=name, n=n, launches=args.reps * args.rounds, ms=round(med, 4), ms_min=round(ms[0], 4),
                              ms_max=round(ms[-1], 4), bytes_per_element=bpe, gb_per_s=round(n * bpe / med / 1e6, 1))), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    assert a.reps * a.rounds >= 100, 'at least 100 timed launches per variant (--reps x --rounds)'
    assert torch.cuda.is_available(), 'bench_optim.py measures on the GPU'
    main(a)

"""Gradient accumulation on the GPU: dsl_grad_accumulate against torch, FlatSGD.accumulate() / the fold in front of the closing
step() against a window summed by hand, the hook, two ranks, the runner, device memory.

Every comparison is a comparison of BITS (torch.equal on integer views): the backward pass is deterministic and the accumulator is
a fixed-order fp32 sum, one rounding per element and micro-step - exactly what `acc += g` does in torch."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import fcos_model_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 192
OPT = dict(lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def make_batch(seed, n=4, first=0):
    """n images 3 x 128 x 192 (bf16-representable), three boxes each; `seed` picks the batch, `first` the images of a 4-image
    batch a rank sees."""
    from oracle import fcos_oracle as O
    g = torch.Generator().manual_seed(1000 + seed)
    img = (torch.randn(4, 3, H, W, generator=g) * 30).bfloat16().float()
    rng = np.random.RandomState(50 + seed)
    gtb = [torch.from_numpy(O.synth_boxes(rng, 3, H=H, W=W, lo=8, hi=100)) for _ in range(4)]
    gtl = [torch.from_numpy(rng.randint(0, 80, len(b)).astype('int64')) for b in gtb]
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * 4
    sl = slice(first, first + n)
    return dict(img=img[sl].cuda(), img_metas=metas[sl], gt_bboxes=gtb[sl], gt_labels=gtl[sl])


def build(rla=False):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from oracle import fcos_oracle as O
    from oracle import rla_oracle as RO
    cfg = fcos_model_cfg()
    if rla:
        cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
    model = build_detector(cfg)
    model.load_state_dict((RO if rla else O).synth_state_dict(0))
    return model.cuda()


def _state(model, opt):
    torch.cuda.synchronize()
    return [t.clone() for t in (model.store.train, opt.momentum_buf, model.store.train16)]


def _assert_state_equal(a, b, where):
    for what, x, y in zip(('train', 'momentum', 'train16'), a, b):
        assert _same(x, y), f'{where}: {what} differs on {int((_bits(x) != _bits(y)).sum())} elements'


# ---- 4. the kernel -------------------------------------------------------------------------------------------------------------
GUARD = 64
SENTINEL = -12345.0


def _special_values(n, seed):
    """Four micro-step gradients of n floats: normal values of mixed magnitude (sums that round), +-0, denormals, +-inf, NaN."""
    g = torch.Generator().manual_seed(seed)
    vs = []
    for j in range(4):
        v = torch.randn(n, generator=g) * (10.0 ** torch.randint(-6, 7, (n,), generator=g).float())
        vs.append(v)
    tiny = torch.tensor([1e-45, -1e-45, 5e-39, -5e-39, 1.1754942e-38, 0.0, -0.0, 1e-40], dtype=torch.float32)
    big = torch.tensor([float('inf'), -float('inf'), float('nan'), 3.0e38, -3.0e38, 1.0, 1.0 + 2 ** -23, 2 ** -24], dtype=torch.float32)
    pool = torch.cat([tiny, big])
    for j, v in enumerate(vs):
        m = min(n, 4 * len(pool))
        idx = torch.randint(0, len(pool), (m,), generator=g)
        v[:m] = pool[idx]
        if n >= 8:          # the same slots across the micro-steps: -0 + -0, -0 + 0, denormals that cancel, inf - inf, overflow, ties, NaN
            v[:8] = torch.tensor([[-0.0, -0.0, 0.0, float('inf'), 3.0e38, 1.0, 5e-39, float('nan')],
                                  [-0.0, 0.0, 0.0, -float('inf'), 3.0e38, 2 ** -24, -5e-39, 1.0],
                                  [-0.0, -0.0, 0.0, 1.0, 1.0, 2 ** -24, 1e-40, 1.0],
                                  [-0.0, -0.0, 0.0, 1.0, 1.0, 2 ** -24, 1e-40, 1.0]][j])
            v[2:3].view(torch.int32)[0] = [1, 1, 2, -2 ** 31 + 4][j]          # 1 + 1 + 2 - 4 units of the smallest denormal
    return vs


@pytest.mark.parametrize('n', [4, 1020, 4100, 2 ** 20 + 8, 2 ** 21 + 12])          # (the last: past 2048 blocks, the grid-stride loop's second trip)
@pytest.mark.parametrize('j', [0, 3])
def test_kernel_set_add_add_fold_vs_torch(n, j):
    """SET, ADD, ADD, FOLD on slices that start 4 j floats into a larger allocation (as bucket slices do), against `acc = g0;
    acc += g1; acc += g2; g3 = acc + g3` in torch fp32 - on the device (all bits, NaN included) and on the host (every element
    whose result is not NaN: +-0, denormals kept, +-inf) - and 64 sentinel floats on both sides of both buffers stay untouched."""
    from dsl_amd import _lib as L
    vs = _special_values(n, 7 * n + j)
    off = GUARD + 4 * j
    total = off + n + GUARD
    acc_buf = torch.full((total,), SENTINEL, device='cuda')
    g_buf = torch.full((total,), SENTINEL, device='cuda')
    acc, g = acc_buf[off:off + n], g_buf[off:off + n]
    assert acc.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    dev = [v.cuda() for v in vs]
    sp = L.stream_ptr()
    ref_dev = ref_cpu = None
    for step, mode in enumerate((L.ACC_SET, L.ACC_ADD, L.ACC_ADD, L.ACC_FOLD)):
        g.copy_(dev[step])
        L.check(L.lib.dsl_grad_accumulate(L.ptr(acc), L.ptr(g), n, mode, sp), 'dsl_grad_accumulate')
        if step == 0:
            ref_dev, ref_cpu = dev[0].clone(), vs[0].clone()
        elif mode == L.ACC_ADD:
            ref_dev += dev[step]
            ref_cpu += vs[step]
        torch.cuda.synchronize()
        if mode != L.ACC_FOLD:
            assert _same(acc, ref_dev), f'step {step}: acc differs from torch on the device on {int((_bits(acc) != _bits(ref_dev)).sum())} elements'
            assert _same(g, dev[step]), f'step {step}: g was written'
    # FOLD: g holds the window's sum, acc is left as it was
    want_dev, want_cpu = ref_dev + dev[3], ref_cpu + vs[3]
    assert _same(g, want_dev), f'fold differs from torch on the device on {int((_bits(g) != _bits(want_dev)).sum())} elements'
    assert _same(acc, ref_dev), 'FOLD wrote acc'
    ok = ~torch.isnan(want_cpu)
    got = g.cpu()
    assert torch.equal(torch.isnan(got), ~ok)
    assert torch.equal(_bits(got)[ok], _bits(want_cpu)[ok]), 'fold differs from torch on the host (denormals / signed zeros?)'
    if n >= 8:
        assert int(_bits(got)[2]) == 0 and int(_bits(got)[0]) == -2 ** 31          # denormals cancel to +0; -0 four times stays -0
        assert int(_bits(acc.cpu())[2]) == 4                                        # ... through a denormal partial sum
        assert int(_bits(got)[6]) == 2 * int(_bits(torch.tensor([1e-40]))[0]) > 0   # a denormal result (its bits are linear in the value)
        assert int(_bits(got)[1]) == 0 and bool(torch.isnan(got[3])) and float(got[4]) == float('inf') and float(got[5]) == 1.0
    for name, buf in (('acc', acc_buf), ('g', g_buf)):
        assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all()), f'{name}: guard band written'


# ---- 5. a window equals its manual sum -----------------------------------------------------------------------------------------
LEGS = ['plain', 'clip', 'rla', 'defer_head', 'proxy']
K = 3


def _make(leg, max_norm=None):
    from dsl_amd.optim import FlatSGD
    model = build(rla=leg == 'rla')
    kw = dict(OPT)
    if leg == 'clip':
        kw['grad_clip'] = dict(max_norm=max_norm, norm_type=2)
    opt = FlatSGD(model, defer_head_update=leg == 'defer_head', **kw)
    if leg == 'proxy':
        model.comm_proxy = dict(carrier='lib', wgs=32, passes=2)
    assert model.store.defer_head == (leg == 'defer_head')
    model.loss_scale = 1.0 / K
    return model, opt


def _manual_window(model, opt, batches):
    """Existing code only: K passes at loss_scale 1 / K, the gradients cloned and summed in order in torch, one step() on the sum.
    Returns the sum."""
    clones = []
    for b in batches:
        out = model.train_step(b, opt)
        out['loss'].backward()
        model.wait_grads()
        torch.cuda.synchronize()
        clones.append(model.store.grad.clone())
    total = clones[0].clone()
    for c in clones[1:]:
        total += c
    model.store.grad.copy_(total)
    torch.cuda.synchronize()
    opt.step()
    return total


def _accumulated_window(model, opt, batches, leg):
    n_buckets = None
    for j, b in enumerate(batches):
        closing = j == len(batches) - 1
        opt.set_closing(closing)
        out = model.train_step(b, opt)
        out['loss'].backward()
        if leg == 'proxy':
            if not closing:
                assert model.exchange.pending == [] and model.exchange.todo == [] and model.exchange.partials_valid is False
            else:
                n_buckets = len(model.exchange.buckets)
                assert len(model.exchange.pending) + len(model.exchange.todo) == n_buckets == 4
        assert opt.acc_count == j
        if closing:
            opt.step()
        else:
            opt.accumulate()
    assert opt.acc_count == 0
    if leg == 'proxy':          # every bucket was folded on the communication stream, in front of its stand-in collective
        assert len(model.exchange.folded) == n_buckets and model.exchange.pending == [] and model.exchange.todo == []


@pytest.mark.parametrize('leg', LEGS)
def test_window_equals_its_manual_sum(leg):
    """accumulate, accumulate, step against three gradients summed by hand and stepped once - parameters, momentum and the bf16
    copy bit for bit, over two windows (the second: first_step off, SET after FOLD)."""
    windows = [[make_batch(3 * w + j) for j in range(K)] for w in range(2)]
    max_norm = None
    b_model, b_opt = _make(leg, max_norm=1.0)
    ref = []
    for w, batches in enumerate(windows):
        total = _manual_window(b_model, b_opt, batches) if not (leg == 'clip' and w == 0) else None
        if total is None:
            # the clipping leg: max_norm = half the first window's norm (rounded to 3 digits), so that clipping binds
            clones = []
            for b in batches:
                out = b_model.train_step(b, b_opt)
                out['loss'].backward()
                b_model.wait_grads()
                torch.cuda.synchronize()
                clones.append(b_model.store.grad.clone())
            total = clones[0].clone()
            for c in clones[1:]:
                total += c
            max_norm = float(f'{float(total.double().norm()) / 2:.3g}')
            b_opt.max_norm = max_norm
            b_model.store.grad.copy_(total)
            torch.cuda.synchronize()
            b_opt.step()
        if leg == 'clip':
            norm = float(total.double().norm())
            print(f'window {w}: accumulated gradient norm {norm:.6g}, max_norm {max_norm}')
            assert np.isfinite(norm) and max_norm < norm, (max_norm, norm)
        ref.append(_state(b_model, b_opt))
    assert b_opt.steps == 2
    del b_model, b_opt
    a_model, a_opt = _make(leg, max_norm=max_norm)
    for w, batches in enumerate(windows):
        _accumulated_window(a_model, a_opt, batches, leg)
        _assert_state_equal(_state(a_model, a_opt), ref[w], f'{leg} window {w}')
    assert a_opt.steps == 2
    # the window is no part of the optimizer's state, and loading a state empties it
    sd = a_opt.state_dict()
    assert set(sd) == {'momentum', 'steps', 'param_groups', 'regions'}
    a_opt.set_closing(False)
    out = a_model.train_step(windows[0][0], a_opt)
    out['loss'].backward()
    a_opt.accumulate()
    assert a_opt.acc_count == 1
    a_opt.load_state_dict(sd)
    assert a_opt.acc_count == 0 and a_model.exchange.fold_acc is None
    torch.cuda.synchronize()


def test_step_and_accumulate_refuse_a_mismatched_backward_pass():
    """Under the data-parallel schedule a window is exchanged once, by its closing pass: accumulate() behind a pass that queued its
    exchange, and step() behind a pass that was told not to, raise instead of training on a wrong gradient."""
    model, opt = _make('proxy')
    b = make_batch(0)
    out = model.train_step(b, opt)          # closing by default: the exchange is queued
    out['loss'].backward()
    with pytest.raises(RuntimeError, match='set_closing'):
        opt.accumulate()
    opt.step()
    opt.set_closing(False)
    out = model.train_step(b, opt)
    out['loss'].backward()
    with pytest.raises(RuntimeError, match='set_closing'):
        opt.step()
    opt.accumulate()
    torch.cuda.synchronize()


# ---- 6. k = 1 through the new hook = the plain hook ----------------------------------------------------------------------------
def test_cumulative_hook_with_one_iteration_windows_is_the_plain_hook():
    from dsl_amd.optim import FlatSGD
    from dsl_amd.runner import SemiEpochBasedRunner
    batches = [make_batch(j) for j in range(3)]
    finals = []
    for cfg in (dict(type='OptimizerHook', grad_clip=None), dict(type='GradientCumulativeOptimizerHook', cumulative_iters=1, grad_clip=None)):
        model = build()
        opt = FlatSGD(model, **OPT)
        runner = SemiEpochBasedRunner(model, optimizer=opt, max_epochs=1)
        runner.register_training_hooks(None, optimizer_config=cfg)
        runner.run([batches])
        assert runner.iter == 3 and opt.steps == 3 and opt.acc_count == 0 and opt._acc is None and model.loss_scale == 1.0
        finals.append(_state(model, opt))
        del model, opt, runner
    _assert_state_equal(finals[0], finals[1], 'k = 1')


# ---- 7. two ranks --------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, port, clip):
    """One rank of test 7 (run as a process of its own, see _two_ranks)."""
    import torch.distributed as dist
    from dsl_amd import _lib as L
    from dsl_amd.optim import FlatSGD
    from dsl_amd.parallel import HipDistributedDataParallel
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=2)
    errs = []
    k = 2
    batches = [make_batch(j, n=2, first=2 * rank) for j in range(k)]          # rank-different halves of two 4-image batches
    clip_cfg = dict(max_norm=1.0, norm_type=2) if clip else None

    def gather(t):
        lst = [torch.empty_like(t) for _ in range(2)]
        dist.all_gather(lst, t)
        return lst

    # each rank's accumulator, by hand: the late exchange leaves the LOCAL gradient in store.grad behind backward()
    r_model = build()
    HipDistributedDataParallel(r_model, comm='torch', grad_dtype='fp32')
    r_opt = FlatSGD(r_model, **OPT)
    r_model.loss_scale = 1.0 / k
    acc = None
    for b in batches:
        out = r_model.train_step(b, r_opt)
        out['loss'].backward()
        assert r_model.late_exchange and len(r_model.exchange.todo) == 4 and not r_model.exchange.pending
        torch.cuda.synchronize()
        acc = r_model.store.grad.clone() if acc is None else acc.add_(r_model.store.grad)
    r_model.wait_grads()
    torch.cuda.synchronize()
    accs = gather(acc)
    if _same(accs[0], accs[1]):
        errs.append('the ranks accumulated the same gradient: the batches do not differ')
    total = accs[0] + accs[1]          # (two addends: the order does not matter)
    del r_model, r_opt

    # the window under test
    model = build()
    HipDistributedDataParallel(model, comm='torch', grad_dtype='fp32')
    opt = FlatSGD(model, grad_clip=clip_cfg, **OPT)
    model.loss_scale = 1.0 / k
    if clip:
        model.clip_partials = torch.zeros(8 * L.SUMSQ_PARTS, device='cuda')      # the norm in pieces from the first step on
    for j, b in enumerate(batches):
        closing = j == k - 1
        opt.set_closing(closing)
        out = model.train_step(b, opt)
        out['loss'].backward()
        if not closing:
            if model.exchange.pending or model.exchange.todo or model.exchange.partials_valid:
                errs.append('a non-closing micro-step queued a gradient collective')
            opt.accumulate()
            continue
        if clip and not (model.exchange.partials_valid and len(model.exchange.pending) == 4):
            errs.append(f'clipping: not the norm in pieces ({model.exchange.partials_valid}, {len(model.exchange.pending)} queued)')
        if not clip and not (model.late_exchange and len(model.exchange.todo) == 4):
            errs.append(f'no clipping: not the late exchange ({model.late_exchange}, {len(model.exchange.todo)} left)')
        opt.step()
    torch.cuda.synchronize()
    if len(model.exchange.folded) != 4:
        errs.append(f'{len(model.exchange.folded)} of 4 buckets folded in front of their exchange')
    if not _same(model.store.grad, total):
        errs.append(f'store.grad != acc_rank0 + acc_rank1 on {int((_bits(model.store.grad) != _bits(total)).sum())} elements')
    got = _state(model, opt)
    for what, t in zip(('train', 'momentum', 'train16'), got):
        a, b_ = gather(_bits(t).to(torch.int32))
        if not torch.equal(a, b_):
            errs.append(f'{what} differs between the ranks on {int((a != b_).sum())} words')
    infos = model.exchange.buckets

    # host reference: one process, one update with the summed accumulators
    h_model = build()
    h_opt = FlatSGD(h_model, grad_clip=clip_cfg, **OPT)
    out = h_model.train_step(make_batch(0, n=2), h_opt)          # (builds the packs and the bucket list; its gradient is replaced)
    out['loss'].backward()
    torch.cuda.synchronize()
    h_model.store.grad.copy_(total)
    if clip:
        h_model.clip_partials = torch.zeros(8 * L.SUMSQ_PARTS, device='cuda')
        for n_, info in enumerate(infos):          # the pieces in the order the buckets are exchanged in
            lo, hi = info['bucket']
            L.check(L.lib.dsl_sumsq_partial(L.ptr(h_model.store.grad[lo:hi]), hi - lo,
                                            C.c_void_p(h_model.clip_partials.data_ptr() + n_ * L.SUMSQ_PARTS * 4), L.stream_ptr()), 'dsl_sumsq_partial')
        h_model.exchange.partials_valid, h_model.exchange.n_partials = True, len(infos) * L.SUMSQ_PARTS
    torch.cuda.synchronize()
    h_opt.step()
    want = _state(h_model, h_opt)
    for what, x, y in zip(('train', 'momentum', 'train16'), got, want):
        if not _same(x, y):
            errs.append(f'{what} differs from the host reference on {int((_bits(x) != _bits(y)).sum())} elements')
    if clip:
        norm = float(total.double().norm())
        print(f'rank {rank}: accumulated norm {norm:.6g}, gnorm_sq {float(opt.gnorm_sq):.6g} / reference {float(h_opt.gnorm_sq):.6g}')
        if float(opt.gnorm_sq) != float(h_opt.gnorm_sq):
            errs.append('the clipping norm differs from the reference')
    dist.destroy_process_group()
    print('RESULT rank', rank, '; '.join(errs) if errs else 'ok', flush=True)
    return 0 if not errs else 1


def _two_ranks(clip, out_dir, limit=240):
    """Two processes, each under its own `timeout`; the parent stops at the first non-zero exit."""
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests'), os.environ.get('PYTHONPATH', '')]))
    logs = [os.path.join(str(out_dir), f'rank{r}.log') for r in range(2)]
    procs = [subprocess.Popen(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), str(r), str(port), str(int(clip))],
                              stdout=open(logs[r], 'w'), stderr=subprocess.STDOUT, env=env, cwd=ROOT) for r in range(2)]
    rcs = [None, None]
    try:
        while any(rc is None for rc in rcs) and all(rc in (None, 0) for rc in rcs):
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    try:
                        rcs[i] = p.wait(0.1)
                    except subprocess.TimeoutExpired:
                        pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    outs = [open(f).read() for f in logs]
    for r in range(2):
        assert rcs[r] == 0 and f'RESULT rank {r} ok' in outs[r], f'rank {r} exit {rcs[r]}:\n{outs[r][-4000:]}\n--- other rank:\n{outs[1 - r][-2000:]}'


@pytest.mark.parametrize('clip', [False, True])
def test_two_ranks_exchange_the_accumulated_window_once(clip, tmp_path):
    """Two ranks (gloo collectives, both on one GPU, fp32 gradients), k = 2, rank-different batches: without clipping (late
    exchange) and with it (the norm in pieces).  Non-closing micro-steps queue no collective; after the window both ranks hold
    the same bits, store.grad holds acc_rank0 + acc_rank1 (each rank's accumulator summed by hand from its local gradients), and
    weights / momentum / bf16 copy are those of one process updated once with that sum."""
    _two_ranks(clip, tmp_path)


# ---- 8. the runner -------------------------------------------------------------------------------------------------------------
def test_train_detector_accumulates_through_the_config_key(tmp_path):
    import json
    from dsl_amd.apis import train_detector
    from dsl_amd.data import SyntheticSemiLoader
    from dsl_amd.pseudo import PseudoLabelBank
    from dsl_amd.registry import Config
    model = build()
    model.loss_scale = 0.5
    cfg = Config(dict(
        model=fcos_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.)),
        optimizer_config=dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2, grad_clip=dict(max_norm=35, norm_type=2)),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[50, 80]),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]), custom_hooks=[dict(type='NumClassCheckHook')],
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=str(tmp_path)))
    bank = PseudoLabelBank(num_classes=80, thres='adathres.json')
    loader = SyntheticSemiLoader(bank, n_labeled=3, n_unlabeled=3, iters_per_epoch=5, H=H, W=W, W_img=190, img_std=30.0)
    runner = train_detector(model, [loader], cfg, distributed=False, validate=False)
    torch.cuda.synchronize()
    opt = runner.optimizer
    assert runner.iter == 5 and opt.steps == 3 and opt.acc_count == 0          # windows of 2, 2 and the last iteration alone
    assert opt.max_norm == 35.0
    assert runner._det(runner.model).loss_scale == 0.5                          # what the hook found
    recs = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'train.log.json'))]
    assert len(recs) == 5
    for r in recs:
        assert all(np.isfinite(v) for k_, v in r.items() if k_.startswith('loss')) and r['loss'] > 0, r
    assert bool(torch.isfinite(model.store.train).all())


# ---- 9. memory -----------------------------------------------------------------------------------------------------------------
def _used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free, total - free - torch.cuda.memory_reserved()


def test_device_memory_is_constant_after_the_first_window():
    """The accumulator comes from torch's allocator once; the library allocates nothing: hipMemGetInfo after the first window =
    after three more."""
    model, opt = _make('plain')
    batches = [make_batch(j) for j in range(K)]
    _accumulated_window(model, opt, batches, 'plain')
    acc_ptr = opt._acc.data_ptr()
    used0, foreign0 = _used_bytes()
    alloc0 = torch.cuda.memory_allocated()
    for _ in range(3):
        _accumulated_window(model, opt, batches, 'plain')
    used1, foreign1 = _used_bytes()
    print('device memory in use', used0, '->', used1, '; not held by torch', foreign0, '->', foreign1)
    assert opt._acc.data_ptr() == acc_ptr and opt._acc.shape == model.store.grad.shape and opt._acc.dtype == torch.float32
    assert used1 == used0 and foreign1 - foreign0 <= 0, (used0, used1, foreign0, foreign1)
    assert torch.cuda.memory_allocated() == alloc0


if __name__ == '__main__':          # one rank of test 7
    sys.exit(_rank_main(int(sys.argv[1]), int(sys.argv[2]), bool(int(sys.argv[3]))))

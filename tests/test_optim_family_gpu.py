"""The optimizer family on the training step: AdamW, Adam and Nesterov SGD with norm_decay_mult = 0 and a custom_keys entry, through
FlatSGD._walk's schedules (per bucket, late exchange, deferred head update, RLA_ResNet), gradient clipping, accumulation, resume
and the runner's hooks - the small model of test_bucket_update_gpu.py.

Per step the weights, both moments and train16 are held against the float64 update (tests/optim_ref.py) under the rounding bound
derived in test_optim_kernel_gpu.py's docstring (twice the first-order bound, the moments' bounds carried into the weight's), with
each element's learning rate and decay derived from its parameter's NAME.  The buffers around an update are copied to the host, as
test_bucket_update_gpu.py's snapshots are (a synchronous copy: a device-side clone queued on the caller's stream would race with
the per-bucket updates, which are ordered behind their gradients' events and not behind the caller's stream), and the float64
update runs as torch float64 on the GPU, chunk by chunk: 32 M elements per step and buffer."""
import copy
import math

import pytest
import torch

import optim_ref as R
from test_bucket_update_gpu import LR_SCALE, _bits, _no_host_sync, _set_lr, build, make_batch

pytestmark = pytest.mark.gpu
PW = dict(norm_decay_mult=0., custom_keys={'backbone': dict(lr_mult=0.1)})
CFGS = dict(AdamW=dict(type='AdamW', lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, paramwise_cfg=PW),
            Adam=dict(type='Adam', lr=1e-4, weight_decay=1e-4, paramwise_cfg=PW),
            Nesterov=dict(type='SGD', lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4, paramwise_cfg=PW))
CHUNK = 1 << 22


def _opt(model, kind, **kw):
    from dsl_amd.optim import build_optimizer
    cfg = dict(copy.deepcopy(CFGS[kind]), **kw)
    return build_optimizer(model, cfg, grad_clip=cfg.pop('grad_clip', None))


def _state(opt):
    return [opt.momentum_buf] + ([opt.exp_avg_sq] if opt.kind != 'SGD' else [])


class FamilyRef:
    """Per element of the flat buffer: covered by a named parameter or not, and its (lr_mult, decay_mult) from the NAME
    (optim_ref.mults).  Also checks opt.group_ids against the names."""

    def __init__(self, model, opt):
        st = model.store
        n = st.n_train
        self.n, self.opt = n, opt
        self.covered = torch.zeros(n, dtype=torch.bool)
        lm, dm = torch.ones(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
        pairs = set()
        for k, p in model.named_parameters():
            if not p.requires_grad:
                continue
            assert p.untyped_storage().data_ptr() == st.train.untyped_storage().data_ptr(), k
            geo = (tuple(p.shape), tuple(p.stride()), p.storage_offset())
            a, b = R.mults(k, PW)
            pairs.add((a, b))
            lm.as_strided(*geo).fill_(a)
            dm.as_strided(*geo).fill_(b)
            self.covered.as_strided(*geo).fill_(True)
            ids = opt.group_ids.as_strided(*geo)
            assert bool((ids == ids.reshape(-1)[0]).all()) and opt.group_table[int(ids.reshape(-1)[0])] == (a, b), f'group id of {k}'
        assert pairs == {(1.0, 1.0), (0.1, 1.0), (1.0, 0.0)} == set(opt.group_table)
        assert not bool(opt.group_ids[~self.covered].any()), 'padding is not group 0'
        assert int(self.covered.sum()) > 0.9 * n
        self.lm, self.dm, self.cov = lm.cuda(), dm.cuda(), self.covered.cuda()

    def check(self, step_index, before, g, after, t16, clip=None):
        """before / after: [p, m(, v)] HOST copies around the update, g the fp32 gradient it read (host); the float64 math runs
        on the device, chunk by chunk.  Returns a list of failures and updates self.worst (largest |err| / bound per buffer)."""
        opt, errs = self.opt, []
        adam = opt.kind != 'SGD'
        lr0 = float(opt.param_groups[0]['lr'])          # (group 0 is (1, 1): its lr is the base rate the hooks set)
        lrs = {pair: R.f32(gr['lr']) for pair, gr in zip(opt.group_table, opt.param_groups)}
        assert lrs[(1.0, 1.0)] == R.f32(lr0)
        wds = {pair: R.f32(opt.weight_decay * pair[1]) for pair in opt.group_table}
        if adam:
            kind, hp = R.KINDS[opt.kind], R.adam_hp(opt.beta1, opt.beta2, opt.eps, step_index + 1)
        else:
            kind, hp = R.SGD, R.sgd_hp(opt.momentum, opt.nesterov, step_index == 0)
        self.worst = getattr(self, 'worst', {})
        for lo in range(0, self.n, CHUNK):
            sl = slice(lo, min(self.n, lo + CHUNK))
            lr_e, wd_e = torch.zeros_like(self.lm[sl]), torch.zeros_like(self.lm[sl])
            for pair in opt.group_table:
                sel = (self.lm[sl] == pair[0]) & (self.dm[sl] == pair[1])
                lr_e[sel], wd_e[sel] = lrs[pair], wds[pair]
            b4, aft = [t[sl].cuda() for t in before], [t[sl].cuda() for t in after]
            ref = R.update(kind, hp, b4[0].double(), g[sl].cuda().double(), b4[1].double(), b4[2].double() if adam else None, lr_e, wd_e, clip)
            cov = self.cov[sl]
            for name, got in zip(('p', 'm', 'v') if adam else ('p', 'm'), aft):
                err = (got.double() - ref[name].x).abs()
                bad = cov & ~(err <= 2 * ref[name].e)
                if bool(bad.any()):
                    i = int(bad.nonzero()[0])
                    errs.append(f'{name} beyond twice the bound on {int(bad.sum())} elements, first {lo + i}: err {float(err[i]):.3e} '
                                f'bound {float(ref[name].e[i]):.3e}')
                self.worst[name] = max(self.worst.get(name, 0.0), float((err / ref[name].e)[cov].max()))
            for name, a, b in zip('pmv', b4, aft):
                if bool((~cov & (_bits(a) != _bits(b))).any()):
                    errs.append(f'padding elements of {name} changed')
        if not torch.equal(_bits(t16), _bits(after[0].bfloat16())):
            errs.append('train16 != bf16(train)')
        if int((self.covered & (after[0] != before[0])).sum()) < 0.5 * int(self.covered.sum()):
            errs.append('fewer than half of the parameters changed: the update did not run')
        return errs


def _padding_rows_zero(model, opt, errs):
    st = model.store
    o, n, shape = st.train_regions['head.cls_w']
    rows = slice(o + 80 * shape[1] * shape[2] * shape[3], o + n)
    ob, nb, _ = st.train_regions['head.cls_b']
    for what, buf in [('train', st.train), ('train16', st.train16)] + list(zip(('exp_avg', 'exp_avg_sq'), _state(opt))):
        for sl in (rows, slice(ob + 80, ob + nb)):
            if bool((buf[sl] != 0).any()):
                errs.append(f'padding rows of the class predictor are not 0 in {what}')


def _snap(model, opt, first=False):
    """[p, m(, v)] on the host (the moments do not exist in front of the first step: zeros)."""
    p = model.store.train.cpu()
    return [p] + ([torch.zeros_like(p) for _ in opt.STATE] if first else [t.cpu() for t in _state(opt)])


def _model(leg):
    model = build(rla=leg == 'rla')
    if leg == 'proxy_late':
        model.comm_proxy = dict(carrier='lib', wgs=32, passes=2)
    return model


def _finals(model, opt):
    torch.cuda.synchronize()
    return [t.clone() for t in [model.store.train, model.store.train16] + _state(opt)]


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), f'{what}: buffer {i} differs on {int((_bits(x) != _bits(y)).sum())} elements'


@pytest.mark.parametrize('leg', ['plain', 'proxy_late', 'defer_head', 'rla'])
@pytest.mark.parametrize('kind', ['AdamW', 'Adam', 'Nesterov'])
def test_family_update_vs_float64_restatement(kind, leg):
    """Three unclipped steps with the lr changed once.  After each: weights, moments and train16 against the float64 update, group
    ids against the names, the class predictor's padding rows still zero.  Then the same steps with no synchronisation: the same
    bits."""
    batch = make_batch(0)
    finals = []
    for capture in (True, False):
        model = _model(leg)
        opt = _opt(model, kind, defer_head_update=leg == 'defer_head')
        assert opt.max_norm is None and not opt.legacy and model.store.defer_head == (leg == 'defer_head')
        if not capture:
            _no_host_sync(model)
        ref = None
        for s in range(len(LR_SCALE)):
            _set_lr(opt, s)
            out = model.train_step(batch, opt)
            out['loss'].backward()
            if leg == 'proxy_late':
                assert model.late_exchange and len(model.exchange.todo) == 4
            if not capture:
                opt.step()
                continue
            torch.cuda.synchronize()
            before, g = _snap(model, opt, s == 0), model.store.grad.cpu()
            opt.step()
            torch.cuda.synchronize()
            after = _snap(model, opt)
            if ref is None:
                ref = FamilyRef(model, opt)
            errs = ref.check(s, before, g, after, model.store.train16.cpu())
            _padding_rows_zero(model, opt, errs)
            assert not errs, f'{kind} {leg} step {s}: ' + '; '.join(errs)
        if capture:
            print(f'{kind} {leg}: worst |err| / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ref.worst.items()))
            assert getattr(opt, '_side1' if leg == 'defer_head' else '_opt_stream', None) is not None          # the per-bucket path
        finals.append(_finals(model, opt))
        del model, opt
    _same_bits(finals[0], finals[1], f'{kind} {leg}: the unsynchronized run')


def _three_steps(kind, prepare=None, **kw):
    model = _model('plain')
    opt = _opt(model, kind, **kw)
    _no_host_sync(model)
    batch = make_batch(0)
    for s in range(len(LR_SCALE)):
        _set_lr(opt, s)
        out = model.train_step(batch, opt)
        out['loss'].backward()
        if prepare:
            prepare(model, opt, s)
        opt.step()
    return model, opt


@pytest.mark.parametrize('kind', ['AdamW', 'Adam', 'Nesterov'])
def test_flat_path_with_a_clip_of_one_equals_the_per_bucket_path(kind):
    """max_norm = 1e30 takes the whole-buffer path behind the gradient norm and multiplies every gradient by exactly 1: the bits
    of the per-bucket path."""
    a, oa = _three_steps(kind)
    b, ob = _three_steps(kind, grad_clip=dict(max_norm=1e30, norm_type=2))
    assert oa._opt_stream is not None and ob._opt_stream is None and ob.max_norm == 1e30
    _same_bits(_finals(a, oa), _finals(b, ob), f'{kind}: flat path')


@pytest.mark.parametrize('kind', ['AdamW', 'Adam', 'Nesterov'])
def test_clipping_below_one(kind):
    """A max_norm of half the first gradient's norm: the squared norm the kernel read is the float64 one to the summation's
    rounding (at most 600 fp32 additions deep for these 32 M elements: about 130 float4 per thread, then the block and fold
    trees), and the update is the restatement's with oracle.fcos_oracle.clip_coef's definition of the coefficient,
    min(max_norm / (norm + 1e-6), 1), evaluated in fp32 as the kernel does."""
    model = _model('plain')
    batch = make_batch(0)
    out = model.train_step(batch, _opt(model, kind))
    out['loss'].backward()
    torch.cuda.synchronize()
    norm0 = float(model.store.grad.double().pow(2).sum().sqrt())
    del model
    model = _model('plain')
    opt = _opt(model, kind, grad_clip=dict(max_norm=0.5 * norm0, norm_type=2))
    ref = None
    for s in range(2):
        _set_lr(opt, s)
        out = model.train_step(batch, opt)
        out['loss'].backward()
        torch.cuda.synchronize()
        before, g = _snap(model, opt, s == 0), model.store.grad.cpu()
        opt.step()
        torch.cuda.synchronize()
        after = _snap(model, opt)
        exact = float(g.double().pow(2).sum())
        got = float(opt.gnorm_sq)
        assert abs(got - exact) <= 600 * R.U * exact, (got, exact)
        clip = R.clip_coef(got, opt.max_norm)
        assert float(clip.x) < 1.0 and (s > 0 or abs(float(clip.x) - 0.5) < 1e-3), float(clip.x)
        ref = ref or FamilyRef(model, opt)
        errs = ref.check(s, before, g, after, model.store.train16.cpu(), clip=clip)
        assert not errs, f'{kind} clipped step {s}: ' + '; '.join(errs)
    assert opt._opt_stream is None          # the whole-buffer path


@pytest.mark.parametrize('kind', ['AdamW', 'Nesterov'])
def test_accumulate_then_step_equals_a_step_on_the_sum(kind):
    """accumulate() on one batch, step() on another: the bits of a twin whose store.grad was overwritten with the fp32 sum of the
    two gradients before a plain step()."""
    b0, b1 = make_batch(0), make_batch(0, flip=True)
    grads = []
    model = _model('plain')
    opt = _opt(model, kind)
    _no_host_sync(model)
    for b in (b0, b1):
        opt.set_closing(b is b1)
        out = model.train_step(b, opt)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads.append(model.store.grad.clone())
        if b is b0:
            opt.accumulate()
    opt.step()
    want = _finals(model, opt)
    del model, opt
    twin = _model('plain')
    topt = _opt(twin, kind)
    _no_host_sync(twin)
    out = twin.train_step(b1, topt)
    out['loss'].backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(twin.store.grad), _bits(grads[1]))
    twin.store.grad.copy_(grads[0] + grads[1])
    torch.cuda.synchronize()
    topt.step()
    _same_bits(want, _finals(twin, topt), f'{kind}: accumulate + step')


@pytest.mark.parametrize('kind', ['AdamW', 'Nesterov'])
def test_resume_after_two_steps_equals_three_steps(kind):
    from dsl_amd.optim import FlatSGD
    a, oa = _three_steps(kind)
    want = _finals(a, oa)
    stop = {}

    def snap(model, opt, s):
        if s == 2:
            model.store.wait_pending()
            torch.cuda.synchronize()
            stop.update(weights={k: v.clone() for k, v in model.state_dict().items()}, opt=copy.deepcopy(opt.state_dict()))
            assert stop['opt']['kind'] == opt.kind and stop['opt']['steps'] == 2
    _three_steps(kind, prepare=snap)
    model = _model('plain')
    model.load_state_dict(stop['weights'])
    opt = _opt(model, kind)
    sd = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in stop['opt'].items()}          # (a checkpoint loads to the CPU)
    opt.load_state_dict(sd)
    _no_host_sync(model)
    _set_lr(opt, 2)
    out = model.train_step(make_batch(0), opt)
    out['loss'].backward()
    opt.step()
    assert opt.steps == 3
    _same_bits(want, _finals(model, opt), f'{kind}: resume')
    if kind == 'AdamW':
        plain = FlatSGD(model, lr=0.01, momentum=0.9)
        with pytest.raises(RuntimeError, match="'AdamW'.*'SGD'"):
            plain.load_state_dict(sd)


def test_runner_adamw_with_cosine_annealing_and_exp_warmup(tmp_path):
    """train_detector's hook registration with AdamW and policy='CosineAnnealing' by iteration behind an exponential warm-up, six
    iterations: every group's lr at every iteration is the closed form, and the weights are those of a manual loop that sets these
    rates and calls step()."""
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config
    from util import fcos_model_cfg
    n_it, wu, ratio = 6, 4, 0.1
    batch = make_batch(0)
    ocfg = dict(type='AdamW', lr=1e-4, weight_decay=0.05, paramwise_cfg=PW)

    def rate(base, it):
        target = base * 0.01
        lr = target + 0.5 * (base - target) * (1 + math.cos(math.pi * (it / n_it)))
        return lr * ratio ** (1 - it / wu) if it < wu else lr

    a = build()
    oa = _opt(a, 'AdamW', **{k: v for k, v in ocfg.items() if k != 'type'})
    for it in range(n_it):
        for g in oa.param_groups:
            g['lr'] = rate(g['initial_lr'], it)
        out = a.train_step(batch, oa)
        out['loss'].backward()
        oa.step()

    class Loader:
        def __len__(self):
            return n_it

        def __iter__(self):
            return iter([batch] * n_it)

    seen = []

    class Spy:
        def __getattr__(self, name):
            return lambda runner: None

        def after_train_iter(self, r):
            seen.append([g['lr'] for g in r.optimizer.param_groups])

    b = build()
    cfg = Config(dict(
        model=fcos_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2), optimizer=ocfg, optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='CosineAnnealing', by_epoch=False, min_lr_ratio=0.01, warmup='exp', warmup_iters=wu, warmup_ratio=ratio),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=2, hooks=[dict(type='TextLoggerHook')]), custom_hooks=[dict(type='NumClassCheckHook')],
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=str(tmp_path)))
    import dsl_amd.runner as RN
    orig = RN.SemiEpochBasedRunner.register_training_hooks

    def with_spy(self, *args, **kw):
        orig(self, *args, **kw)
        self.register_hook(Spy(), priority='LOW')
    RN.SemiEpochBasedRunner.register_training_hooks = with_spy
    try:
        runner = train_detector(b, [Loader()], cfg, distributed=False, validate=False)
    finally:
        RN.SemiEpochBasedRunner.register_training_hooks = orig
    assert runner.iter == n_it and len(seen) == n_it
    assert any(type(h).__name__ == 'CosineAnnealingLrUpdaterHook' for h in runner._hooks)
    opt = runner.optimizer
    assert type(opt).__name__ == 'FlatAdamW' and len(opt.param_groups) == 3
    for it, lrs in enumerate(seen):
        for g, lr in zip(opt.param_groups, lrs):
            assert lr == pytest.approx(rate(g['initial_lr'], it), rel=1e-12, abs=0), (it, g['name'])
            assert lr == rate(g['initial_lr'], it)          # (the same expression: the manual loop ran these very rates)
    det = runner._det(runner.model)
    _same_bits(_finals(a, oa), _finals(det, opt), 'runner vs manual loop')

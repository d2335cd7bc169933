"""The optimizer family without a GPU: the float64 restatement (tests/optim_ref.py) against torch.optim, the parameter-group rules,
the learning-rate policies against closed forms, dsl_optim_desc's ctypes mirror, the refusals, and build_optimizer through group
construction on a CPU-resident store."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

import optim_ref as R
from optim_ref import REFUSALS, refused_call
from util import fcos_model_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PW = dict(norm_decay_mult=0., custom_keys={'backbone': dict(lr_mult=0.1)})


def build(rla=False):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    cfg = fcos_model_cfg()
    if rla:
        cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
    return build_detector(cfg)


@pytest.fixture(scope='module')
def models():
    return dict(default=build(), rla=build(rla=True))


# ---- 1. the restatement against torch.optim ---------------------------------------------------------------------------------------
def _grads(gen, n):
    """Magnitudes 1e-6 .. 1e3, both signs, every seventh element exactly zero."""
    g = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 9 - 6)
    g = g * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g[::7] = 0.0
    return g


@pytest.mark.parametrize('kind', ['Adam', 'AdamW', 'Nesterov'])
def test_restatement_matches_torch_optim_in_float64(kind):
    """Five steps in float64, two parameter tensors with their own (lr, wd), the lr changed after the second step.  The weights
    agree to 1e-12 relative; the Nesterov leg cancels near zero weights and gets an absolute floor of 1e-15 beside it."""
    gen = torch.Generator().manual_seed(11)
    n = 4096
    ps = [torch.randn(n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64) * 1e-2]
    rates = [(1e-3, 1e-2), (2.5e-4, 0.0)]
    tp = [p.clone().requires_grad_(True) for p in ps]
    groups = [dict(params=[q], lr=lr, weight_decay=wd) for q, (lr, wd) in zip(tp, rates)]
    if kind == 'Nesterov':
        opt = torch.optim.SGD(groups, lr=1.0, momentum=0.9, nesterov=True, foreach=False)
    else:
        opt = getattr(torch.optim, kind)(groups, lr=1.0, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    mine = [dict(p=p.clone(), m=torch.zeros_like(p), v=torch.zeros_like(p)) for p in ps]
    worst = 0.0
    for t in range(1, 6):
        scale = 1.0 if t <= 2 else 0.3
        gs = [_grads(gen, n) for _ in ps]
        for grp, q, g, (lr, _) in zip(opt.param_groups, tp, gs, rates):
            grp['lr'] = lr * scale
            q.grad = g.clone()
        opt.step()
        for s, g, (lr, wd), q in zip(mine, gs, rates, tp):
            if kind == 'Nesterov':
                out = R.update(R.SGD, R.sgd_hp(0.9, True, t == 1, fp32=False), s['p'], g, s['m'], None, lr * scale, wd)
            else:
                out = R.update(R.KINDS[kind], R.adam_hp(0.9, 0.999, 1e-8, t, fp32=False), s['p'], g, s['m'], s['v'], lr * scale, wd)
                s['v'] = out['v'].x
            s['p'], s['m'] = out['p'].x, out['m'].x
            err = (s['p'] - q.detach()).abs()
            floor = 1e-15 if kind == 'Nesterov' else 0.0
            worst = max(worst, float((err / q.detach().abs().clamp(min=1e-300)).max()))
            assert bool((err <= 1e-12 * q.detach().abs() + floor).all()), (kind, t, float(err.max()))
    print(f'{kind}: worst relative difference of the weights over five steps {worst:.2e}')


# ---- 2. parameter groups --------------------------------------------------------------------------------------------------------
def _trainable(model):
    return [k for k, p in model.named_parameters() if p.requires_grad]


@pytest.mark.parametrize('which', ['default', 'rla'])
def test_bias_keys_only_equal_the_oracles_rule(models, which):
    from dsl_amd.optim import param_group_mults
    from oracle.fcos_oracle import param_group_rule
    pw = dict(bias_lr_mult=2., bias_decay_mult=0.)
    names = _trainable(models[which])
    assert len(names) > 100
    for k in names:
        want = param_group_rule(k, 1.0, 1.0, 2.0, 0.0)
        assert R.mults(k, pw) == want, k
        assert param_group_mults(k, pw) == want, k


@pytest.mark.parametrize('which', ['default', 'rla'])
def test_norm_decay_mult_reaches_exactly_the_norm_parameters(models, which):
    from dsl_amd.optim import build_groups
    model = models[which]
    table, ids, by_name = build_groups(model, dict(norm_decay_mult=0.))
    assert table == [(1.0, 1.0), (1.0, 0.0)]
    hit = sorted(k for k, g in by_name.items() if g == 1)
    want = sorted(k for k in _trainable(model) if '.gn.' in k or '.bn' in k or 'downsample.1' in k or '.stage_bns.' in k)
    assert hit == want and len(hit) >= 16
    if which == 'rla':
        assert any('.gn.' not in k for k in hit), 'no trained BatchNorm among the norm parameters of RLA_ResNet'
    else:
        assert all('.gn.' in k for k in hit)
    for k in hit:
        assert R.mults(k, dict(norm_decay_mult=0.)) == (1.0, 0.0)


def test_custom_keys_precedence():
    from dsl_amd.optim import param_group_mults
    pw = dict(bias_lr_mult=2., bias_decay_mult=0., norm_decay_mult=0.,
              custom_keys={'bbox_head': dict(lr_mult=0.5), 'bbox_head.cls_convs': dict(lr_mult=0.25, decay_mult=3.0), 'neck': dict(decay_mult=0.5)})
    for f in (param_group_mults, R.mults):
        assert f('bbox_head.cls_convs.0.conv.weight', pw) == (0.25, 3.0)          # the longer key wins
        assert f('bbox_head.reg_convs.0.conv.weight', pw) == (0.5, 1.0)
        assert f('bbox_head.cls_convs.1.gn.weight', pw) == (0.25, 3.0)            # ... and switches the norm rule off
        assert f('bbox_head.conv_cls.bias', pw) == (0.5, 1.0)                     # ... and the bias rule
        assert f('neck.fpn_convs.0.conv.bias', pw) == (1.0, 0.5)
        assert f('backbone.layer2.0.conv1.weight', pw) == (1.0, 1.0)
        assert f('neck.lateral_convs.0.conv.bias', dict(bias_lr_mult=2., bias_decay_mult=0.)) == (2.0, 0.0)
    # same length: alphabetical order decides
    pw2 = dict(custom_keys={'conv_b': dict(lr_mult=3.0), 'conv_a': dict(lr_mult=2.0)})
    assert param_group_mults('x.conv_a.conv_b.weight', pw2) == R.mults('x.conv_a.conv_b.weight', pw2) == (2.0, 1.0)
    with pytest.raises(NotImplementedError, match='no_such_key'):
        param_group_mults('a.weight', dict(no_such_key=1.0))
    # accepted, nothing to apply to
    assert param_group_mults('a.weight', dict(dwconv_decay_mult=0.1, dcn_offset_lr_mult=0.1)) == (1.0, 1.0)


def test_more_than_16_pairs_is_refused(models):
    from dsl_amd.optim import FlatSGD, build_groups
    model = models['default']
    names = [k for k in _trainable(model) if k.endswith('.weight')][:17]
    ck = {k: dict(lr_mult=0.01 * (i + 1)) for i, k in enumerate(names)}
    with pytest.raises(NotImplementedError, match='18 distinct'):
        build_groups(model, dict(custom_keys=ck))
    with pytest.raises(NotImplementedError, match='18 distinct'):
        FlatSGD(model, lr=0.01, momentum=0.9, paramwise_cfg=dict(custom_keys=ck))
    ck.pop(names[-1])
    ck.pop(names[-2])
    table, _, _ = build_groups(model, dict(custom_keys=ck))          # 15 + the base pair
    assert len(table) == 16


def _check_groups(model, opt, pw):
    """group_ids against the names: every element of every trainable parameter carries the id of its (lr_mult, decay_mult) pair,
    every element no parameter covers (tile padding, the predictors' padding rows) is group 0."""
    ids = opt.group_ids
    assert ids.dtype == torch.uint8 and ids.device.type == 'cpu' and ids.numel() == model.store.n_train
    covered = torch.zeros(ids.numel(), dtype=torch.bool)
    seen = set()
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        view = ids.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset())
        pair = R.mults(k, pw)
        assert opt.group_table[opt.group_of[k]] == pair, k
        assert bool((view == opt.group_of[k]).all()), k
        covered.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset()).fill_(True)
        seen.add(pair)
    assert opt.group_table[0] == (1.0, 1.0) and set(opt.group_table) == seen | {(1.0, 1.0)}
    assert int((~covered).sum()) > 0 and not bool(ids[~covered].any()), 'padding is not group 0'
    o, n, shape = model.store.train_regions['head.cls_w']
    assert not bool(ids[o + 80 * shape[1] * shape[2] * shape[3]:o + n].any())          # padding rows of the class predictor
    for g, (lm, dm) in zip(opt.param_groups, opt.group_table):
        assert (g['lr_mult'], g['decay_mult']) == (lm, dm) and g['initial_lr'] == g['lr'] and 'name' in g


@pytest.mark.parametrize('cfg', [
    dict(type='Adam', lr=1e-4, weight_decay=1e-4), dict(type='AdamW', lr=1e-4, betas=(0.9, 0.99), weight_decay=0.05),
    dict(type='SGD', lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)], ids=['Adam', 'AdamW', 'Nesterov'])
@pytest.mark.parametrize('which', ['default', 'rla'])
def test_build_optimizer_through_group_construction(models, which, cfg):
    from dsl_amd.optim import FlatAdam, FlatSGD, build_optimizer
    model = models[which]
    opt = build_optimizer(model, dict(cfg, paramwise_cfg=PW))
    assert isinstance(opt, FlatSGD) and not opt.legacy and opt.kind == ('SGD' if cfg['type'] == 'SGD' else cfg['type'])
    assert isinstance(opt, FlatAdam) == (cfg['type'] != 'SGD')
    assert opt.group_table == [(1.0, 1.0), (0.1, 1.0), (1.0, 0.0)]
    assert [g['lr'] for g in opt.param_groups] == [cfg['lr'], cfg['lr'] * 0.1, cfg['lr']]
    _check_groups(model, opt, PW)
    d = opt._desc()
    assert d.n_groups == 3 and d.kind == dict(SGD=0, Adam=1, AdamW=2)[cfg['type']]
    assert [d.wd[k] for k in range(3)] == [R.f32(cfg['weight_decay']), R.f32(cfg['weight_decay']), 0.0]
    if cfg['type'] != 'SGD':
        b1, b2 = cfg.get('betas', (0.9, 0.999))
        assert d.step_scale == R.f32(1 / (1 - b1)) and d.rsqrt_bc2 == R.f32(1 / math.sqrt(1 - b2))
        opt.steps = 99999
        d = opt._desc()
        assert d.step_scale == 1.0 and abs(d.rsqrt_bc2 - 1.0) < 1e-6
    else:
        assert d.nesterov == 1 and d.first_step == 1


def test_plain_sgd_keeps_the_legacy_path_and_its_groups(models):
    from dsl_amd.optim import FlatSGD
    model = models['default']
    for pw in (None, dict(bias_lr_mult=2., bias_decay_mult=0.)):
        opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=pw)
        assert opt.legacy and opt.group_ids is None and [g['name'] for g in opt.param_groups] == ['weights', 'conv_bias']
        assert set(opt.state_dict()) == {'momentum', 'steps', 'param_groups', 'regions'}
    opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., norm_decay_mult=0.))
    assert not opt.legacy and opt.group_table == [(1.0, 1.0), (2.0, 1.0), (1.0, 0.0)]


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(models):
    from dsl_amd.optim import FlatAdam, FlatAdamW, FlatSGD, build_optimizer
    from dsl_amd.runner import SemiEpochBasedRunner, build_lr_hook
    model = models['default']
    with pytest.raises(NotImplementedError, match='amsgrad'):
        build_optimizer(model, dict(type='AdamW', lr=1e-4, amsgrad=True))
    with pytest.raises(NotImplementedError, match='dampening'):
        build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, dampening=0.1))
    with pytest.raises(NotImplementedError, match='OneCycle.*step.*CosineAnnealing.*poly.*exp.*fixed'):
        build_lr_hook(dict(policy='OneCycle', max_lr=0.1))
    with pytest.raises(NotImplementedError, match="warm-up 'cubic'"):
        build_lr_hook(dict(policy='step', step=[8], warmup='cubic', warmup_iters=5))
    r = SemiEpochBasedRunner(type('M', (), {'train_step': None})(), max_epochs=1)
    with pytest.raises(NotImplementedError, match='momentum_config'):
        r.register_training_hooks(None, momentum_config=dict(policy='cyclic'))
    # a state of another kind
    adamw, adam = FlatAdamW(model, lr=1e-4), FlatAdam(model, lr=1e-4)
    sgd, nest = FlatSGD(model, lr=0.01, momentum=0.9), FlatSGD(model, lr=0.01, momentum=0.9, nesterov=True)
    assert adamw.state_dict()['kind'] == 'AdamW' and nest.state_dict()['kind'] == 'SGD' and 'exp_avg_sq' in adam.state_dict()
    with pytest.raises(RuntimeError, match="'AdamW'.*'SGD'"):
        sgd.load_state_dict(adamw.state_dict())
    with pytest.raises(RuntimeError, match="'SGD'.*'Adam'"):
        adam.load_state_dict(sgd.state_dict())
    with pytest.raises(RuntimeError, match="'Adam'.*'AdamW'"):
        adamw.load_state_dict(adam.state_dict())
    with pytest.raises(RuntimeError, match='parameter groups'):
        sgd.load_state_dict(nest.state_dict())          # same kind, but a group table the bias flag cannot hold
    other = FlatAdamW(model, lr=1e-4, paramwise_cfg=PW)
    with pytest.raises(RuntimeError, match='parameter groups'):
        adamw.load_state_dict(other.state_dict())


def test_adam_state_round_trip_remaps_both_moments(models):
    """exp_avg_sq travels through state_dict / load_state_dict / _adopt_loaded_state region by region, as the momentum does."""
    from dsl_amd.optim import FlatAdamW
    model = models['default']
    st = model.store
    a = FlatAdamW(model, lr=1e-4, paramwise_cfg=PW)
    a.momentum_buf = torch.arange(st.n_train, dtype=torch.float32) % 1013
    a.exp_avg_sq = torch.arange(st.n_train, dtype=torch.float32) % 911
    a.steps = 7
    a.param_groups[1]['lr'] = 3e-6
    sd = a.state_dict()
    assert sd['momentum'] is a.exp_avg and sd['exp_avg_sq'] is a.exp_avg_sq and sd['groups'] == a.group_table
    # another layout: every region shifted
    regs, m2, v2, off = {}, [], [], 0
    for i, (k, (o, n, _)) in enumerate(sorted(st.train_regions.items(), key=lambda kv: kv[1][0])):
        pad = 8 * (i % 3)
        m2 += [a.momentum_buf[o:o + n], torch.full((pad,), -7.0)]
        v2 += [a.exp_avg_sq[o:o + n], torch.full((pad,), -7.0)]
        regs[k] = (off, n)
        off += n + pad
    b = FlatAdamW(model, lr=1e-4, paramwise_cfg=PW)
    b.load_state_dict(dict(sd, momentum=torch.cat(m2), exp_avg_sq=torch.cat(v2), regions=regs))
    b._adopt_loaded_state()
    assert b.steps == 7 and b.param_groups[1]['lr'] == 3e-6
    for k, (o, n, _) in st.train_regions.items():
        assert torch.equal(b.momentum_buf[o:o + n], a.momentum_buf[o:o + n]) and torch.equal(b.exp_avg_sq[o:o + n], a.exp_avg_sq[o:o + n]), k
    assert -7.0 not in b.exp_avg_sq and -7.0 not in b.momentum_buf


# ---- 4. learning-rate policies ----------------------------------------------------------------------------------------------------
class FakeRunner:
    def __init__(self, max_epochs=12, per_epoch=50):
        self.epoch = self.iter = 0
        self.max_epochs, self.max_iters = max_epochs, max_epochs * per_epoch
        self.data_loader = [None] * per_epoch
        self.optimizer = type('O', (), {})()
        self.optimizer.param_groups = [dict(lr=0.0, initial_lr=0.01), dict(lr=0.0, initial_lr=0.002), dict(lr=0.0, initial_lr=3e-5)]

    def at(self, it):
        self.iter, self.epoch = it, it // len(self.data_loader)
        return self


def _closed(policy, cfg, base, prog):
    """The regular rate in float64; prog = (progress, max progress) in the policy's unit."""
    at, end = prog
    if policy == 'step':
        return base * cfg.get('gamma', 0.1) ** sum(1 for s in cfg['step'] if at >= s)
    if policy == 'CosineAnnealing':
        target = base * cfg['min_lr_ratio'] if 'min_lr_ratio' in cfg else cfg['min_lr']
        return target + 0.5 * (base - target) * (1 + math.cos(math.pi * at / end))
    if policy == 'poly':
        return (base - cfg.get('min_lr', 0.0)) * (1 - at / end) ** cfg.get('power', 1.0) + cfg.get('min_lr', 0.0)
    if policy == 'exp':
        return base * cfg['gamma'] ** at
    return base


POLICIES = [('step', dict(step=[3, 7])), ('step', dict(step=[120, 400], gamma=0.5)), ('CosineAnnealing', dict(min_lr_ratio=0.01)),
            ('CosineAnnealing', dict(min_lr=1e-6)), ('poly', dict(power=0.9, min_lr=1e-5)), ('poly', dict()), ('exp', dict(gamma=0.97)),
            ('fixed', dict())]
WARMUPS = [dict(), dict(warmup='linear', warmup_iters=120, warmup_ratio=1.0 / 3), dict(warmup='constant', warmup_iters=120, warmup_ratio=0.25),
           dict(warmup='exp', warmup_iters=120, warmup_ratio=0.001), dict(warmup='exp', warmup_iters=2, warmup_ratio=0.1, warmup_by_epoch=True)]


@pytest.mark.parametrize('by_epoch', [True, False])
@pytest.mark.parametrize('policy, cfg', POLICIES, ids=[f'{p}{i}' for i, (p, _) in enumerate(POLICIES)])
def test_lr_policies_against_closed_forms(policy, cfg, by_epoch):
    """Every policy with every warm-up, progress by epoch and by iteration, at iterations around each hand-over (the last warm-up
    iteration, the first regular one), each milestone and the end: every group's rate equals the closed form to 1e-12 relative."""
    from dsl_amd.runner import LR_POLICIES, build_lr_hook
    for wu in WARMUPS:          # (step milestones given in the other unit are reached early or never: checked all the same)
        hook = build_lr_hook(dict(policy=policy, by_epoch=by_epoch, **cfg, **wu))
        assert type(hook) is LR_POLICIES[policy]
        r = FakeRunner()
        n_wu = wu.get('warmup_iters', 0) * (50 if wu.get('warmup_by_epoch') else 1)
        its = sorted({0, 1, 49, 50, 51, 99, 100, 101, 119, 120, 121, 149, 150, 151, 349, 350, 351, 399, 400, 401, 599})
        for it in its:
            hook.before_train_iter(r.at(it))
            prog = (r.epoch, r.max_epochs) if by_epoch else (r.iter, r.max_iters)
            for g in r.optimizer.param_groups:
                want = _closed(policy, cfg, g['initial_lr'], prog)
                if wu and it < n_wu:
                    ratio, kind = wu['warmup_ratio'], wu['warmup']
                    want *= (ratio if kind == 'constant' else 1 - (1 - it / n_wu) * (1 - ratio) if kind == 'linear'
                             else ratio ** (1 - it / n_wu))
                assert g['lr'] == pytest.approx(want, rel=1e-12, abs=0), (policy, wu, it, g)
        if wu:          # the hand-over: iteration n_wu - 1 is still warmed up, iteration n_wu is at the regular rate exactly
            hook.before_train_iter(r.at(n_wu - 1))
            warmed = [g['lr'] for g in r.optimizer.param_groups]
            hook.before_train_iter(r.at(n_wu))
            prog = (r.epoch, r.max_epochs) if by_epoch else (r.iter, r.max_iters)
            for g, w in zip(r.optimizer.param_groups, warmed):
                assert g['lr'] == pytest.approx(_closed(policy, cfg, g['initial_lr'], prog), rel=1e-12, abs=0)
                assert w != g['lr'] or wu['warmup_ratio'] == 1.0


def test_step_policy_values_are_the_ones_it_always_gave():
    """The DSL configs' settings (step by epoch, linear warm-up over 500 iterations from 1/3; 'constant' of the supervised FCOS
    config): bit-equal to the expression StepLrUpdaterHook has always evaluated, initial_lr * (gamma^k * warm-up factor)."""
    from dsl_amd.runner import build_lr_hook
    for wu in ('linear', 'constant', None):
        hook = build_lr_hook(dict(policy='step', warmup=wu, warmup_iters=500, warmup_ratio=1.0 / 3, step=[20, 26]) if wu else
                             dict(policy='step', step=[20, 26]))
        r = FakeRunner(max_epochs=30, per_epoch=40)
        for it in list(range(0, 520, 7)) + [499, 500, 501, 799, 800, 801, 1039, 1040, 1041, 1199]:
            hook.before_train_iter(r.at(it))
            f = 0.1 ** sum(1 for s in (20, 26) if r.epoch >= s)
            if wu == 'linear' and it < 500:
                k = (1 - it / 500) * (1 - 1.0 / 3)
                f = f * (1 - k)
            elif wu == 'constant' and it < 500:
                f = f * (1.0 / 3)
            assert [g['lr'] for g in r.optimizer.param_groups] == [g['initial_lr'] * f for g in r.optimizer.param_groups], (wu, it)
            assert hook._factor(r) == f


# ---- 5. ABI ---------------------------------------------------------------------------------------------------------------------
def test_optim_desc_mirror_matches_the_header(tmp_path):
    from dsl_amd import _lib as L
    src = tmp_path / 'sizes.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsl_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d %d\\n", sizeof(dsl_optim_desc), offsetof(dsl_optim_desc, max_norm), offsetof(dsl_optim_desc, wd),\n'
                   '         DSL_OPT_SGD, DSL_OPT_ADAM, DSL_OPT_ADAMW, DSL_OPT_MAX_GROUPS);\n  return 0;\n}\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    size, last, wd, k0, k1, k2, ng = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert ctypes.sizeof(L.OptimDesc) == size and L.OptimDesc.max_norm.offset == last and L.OptimDesc.wd.offset == wd
    assert L.OptimDesc._fields_[-1][0] == 'max_norm'
    assert (L.OPT_SGD, L.OPT_ADAM, L.OPT_ADAMW, L.OPT_MAX_GROUPS) == (k0, k1, k2, ng) == (0, 1, 2, 16)
    assert 'dsl_optim_step' not in L.MISSING and len(L.lib.dsl_optim_step.argtypes) == 10


@pytest.mark.parametrize('case, word', REFUSALS, ids=[f'{i}-{w.decode().replace(" ", "_")}' for i, (_, w) in enumerate(REFUSALS)])
def test_dsl_optim_step_validates_before_it_launches(case, word):
    rc, err = refused_call(case)
    assert rc != 0 and b'dsl_optim_step' in err and word in err, (rc, err)

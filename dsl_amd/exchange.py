"""The data-parallel gradient exchange of one detector: which gradient bucket is all-reduced when and on which stream, what is still
in flight, and who folds an accumulation window into it.  The detector owns one GradExchange (FCOS.exchange) and
drives it from its backward pass (begin / segment_done / finish); the optimizer asks it for late buckets, pending work, the folded
buckets and the clipping norm's partial sums; HipDistributedDataParallel sets the carrier."""
import ctypes as C

import torch
import torch.distributed as dist

from . import _lib as L
from .parallel import StreamWork

# What a backward pass does with its gradient buckets (GradExchange.mode):
NONE = 'none'          # nothing to exchange: one process (no proxy), or every collective switched off
BANKED = 'banked'      # a non-closing micro-step of an accumulation window: no collective, pending / todo stay empty, no norm partials
LATE = 'late'          # the buckets are noted; the optimizer asks for each exchange right in front of that bucket's update
EAGER = 'eager'        # each bucket's exchange is queued as soon as its backward segment is
# Late exchange (round 6; set by an optimizer that updates bucket by bucket without a global norm, FlatSGD._sync_defer): the
# collectives are queued BEHIND the whole backward pass, in the order the next forward pass needs the parameters (layer2's
# bucket first, head + FPN last), and nothing waits for them at the end of the step - the per-bucket updates record named
# events SLOT_UPD + k, the next step's forward list waits for them stage by stage (engine.Plan._fwd_resnet).  Queued
# bucket by bucket behind each segment ("eager") the traffic shared the tail of the backward pass with the weight
# gradients, the next step's frozen prefix and the step boundary: the one-GPU proxy priced that at 10 % of the step
# whatever queue carried it, the late exchange on the weight-gradient queue at 5.7 % (profiles/r06_comm_queue_sweep.txt).


def exchange_mode(world_size, comm_off, proxy, on_gpu, closing, late_wanted, clip_partials, backbone, defer):
    """The mode of the next backward pass, from the settings alone (no device, no process group).  proxy: FCOS.comm_proxy (it
    counts on ONE process with the gradients on the GPU); clip_partials: GradExchange.clip_partials or None; defer: Plan.defer."""
    if not ((world_size > 1 and not comm_off) or (proxy and world_size == 1 and on_gpu)):
        return NONE
    if not closing:
        return BANKED
    if on_gpu and late_wanted and clip_partials is None and backbone != 'rla' and not defer:
        return LATE
    return EAGER


class GradExchange:
    def __init__(self, store):
        self.store = store
        # ---- settings (HipDistributedDataParallel, bench.py and the optimizer set them; the detector forwards its public names)
        self.group = None             # torch.distributed process group (None: the default one)
        self.world_size = 1
        self.rccl = None              # parallel.RcclComm: the exchanges go through the C-ABI's communicator instead of torch.distributed
        self.grad_bf16 = False        # gradient buckets cross xGMI as bf16 copies (half the bytes); master gradient, norm, update stay fp32
        self.comm_off = False         # DSL_COMM=none / bench.py's attribution probe: every collective skipped (timing only - WRONG gradients)
        # Communication proxy (one-GPU measurement of what the collectives cost the DEVICE; bench.py extra.comm_proxy):
        # dict(carrier='lib' | 'torch', wgs=32, passes=2).  The step then runs its data-parallel schedule - bucket events, communication
        # stream, per-bucket optimizer steps behind each bucket's "all-reduce" - with dsl_comm_proxy (value-preserving passes over the
        # bucket on `wgs` workgroups) in place of RCCL; carrier 'lib' = the library's placed communication stream (what comm='rccl'
        # uses), 'torch' = a stream from torch's pool, as ProcessGroupNCCL runs its kernels on one of its own
        self.comm_proxy = None
        self.comm_trace = None        # set to [] (bench.py --gpus N): per step, per gradient bucket, timed events of its all-reduce
        self.late_wanted = False      # an optimizer that updates bucket by bucket without a global norm asks for LATE (FlatSGD._sync_defer)
        # Gradient accumulation (FlatSGD.accumulate / set_closing, GradientCumulativeOptimizerHook).  closing False: the next
        # backward pass is a window's non-closing micro-step - it queues NO gradient collective (each rank banks its local gradient,
        # the window's sum is exchanged once).  fold_acc: the optimizer's bank while a window is open - the closing pass's
        # exchange(info) folds it into the bucket (DSL_ACC_FOLD) in front of the collective and lists the bucket in `folded`
        self.closing = True
        self.clip_partials = None     # [buckets * SUMSQ_PARTS] floats: FlatSGD with grad_clip asks for the norm in pieces, per bucket
        # ---- state of the last backward pass
        self.mode = NONE
        self.buckets = []             # its segments' infos that complete a bucket (range, event slot), in completion order
        self.pending = []             # one waitable per exchange queued and not yet waited for
        self.todo = []                # LATE: the buckets not yet handed out, in the order the next forward pass needs the parameters
        self.folded = set()           # (lo, hi) of the buckets whose exchange folded the accumulation window into them
        self.fold_acc = None
        self.partials_valid = False   # clip_partials[:n_partials] holds the norm of every bucket of this pass
        self.n_partials = 0
        self._n_exchanged = 0
        self._proxy = None            # comm_proxy where it counts for this pass
        # ---- resources, each made on first need
        self._comm_stream = None
        self._pool_stream = None
        self._g16 = None

    def comm_stream(self):
        """The library's placed communication stream (one per device and process)."""
        if self._comm_stream is None:
            from .detectors import role_stream
            self._comm_stream = role_stream('comm', self.store.device)
        return self._comm_stream

    def _carrier_stream(self):
        """The stream this pass's exchanges are queued on: the communication stream, or for the proxy's carrier 'torch' one of torch's pool."""
        if self._proxy is not None and self._proxy.get('carrier', 'lib') == 'torch':
            if self._pool_stream is None:
                self._pool_stream = torch.cuda.Stream()
            return self._pool_stream
        return self.comm_stream()

    # ---- the backward pass ------------------------------------------------------------------------------------------------------
    def begin(self, plan):
        """Top of a backward pass: settles the mode, forgets the last pass, makes the streams this one needs."""
        st = self.store
        on_gpu = st.grad.is_cuda
        self._proxy = self.comm_proxy if (self.comm_proxy and self.world_size == 1 and on_gpu) else None
        self.mode = exchange_mode(self.world_size, self.comm_off, self.comm_proxy, on_gpu, self.closing, self.late_wanted,
                                  self.clip_partials, st.backbone, getattr(plan, 'defer', False))
        self.buckets = [info for _, info in plan.bwd_segments if info['bucket'] is not None]
        self.pending, self.todo, self.folded = [], [], set()
        self.partials_valid, self._n_exchanged = False, 0
        if self.mode in (LATE, EAGER) and on_gpu:
            self.comm_stream()          # (the library's streams first: a pool stream for the proxy's 'torch' carrier is drawn after them)
            self._carrier_stream()

    def segment_done(self, info):
        """Behind a backward segment's list.  (bucket None: the deferred head update - its bucket completes with a later list)"""
        if info['bucket'] is None:
            return
        if self.mode == EAGER:
            self.exchange(info)
        elif self.mode == LATE:
            self.todo.append(info)

    def finish(self):
        """End of a backward pass."""
        # late: nothing is queued here - the optimizer asks for each bucket's exchange right in front of that bucket's update
        # (next_late), so that on ONE hardware queue the order is exchange, update, exchange, update ... in the order the next
        # forward pass needs the parameters; queued all at once the first update sat behind every exchange (measured: 13 - 18 %)
        self.todo.reverse()
        self.n_partials = self._n_exchanged * L.SUMSQ_PARTS
        self.partials_valid = bool(self.mode in (LATE, EAGER) and self.store.grad.is_cuda and self.clip_partials is not None
                                   and 0 < self.n_partials <= self.clip_partials.numel())

    def exchange(self, info):
        """Queues the exchange of one bucket of the last backward pass and lists its waitable in `pending`."""
        lo, hi = info['bucket']
        acc, st, proxy = self.fold_acc, self.store, self._proxy
        if not st.grad.is_cuda:            # host tensors (the gloo unit test of the bucket order): nothing to order against
            if acc is not None:
                raise NotImplementedError('dsl_amd: gradient accumulation runs on the GPU only (dsl_grad_accumulate)')
            self.pending.append(dist.all_reduce(st.grad[lo:hi], group=self.group, async_op=True))
            return
        cs = self._carrier_stream()
        csp = C.c_void_p(cs.cuda_stream)
        L.check(min(L.lib.dsl_stream_wait_slot(info['slot'], csp), 0), 'dsl_stream_wait_slot')
        if info['main']:
            cs.wait_stream(torch.cuda.current_stream())
        g = st.grad[lo:hi]
        if acc is not None:
            # the closing micro-step of an accumulation window: the bucket becomes the window's sum (bank + this pass) on the
            # communication stream, behind the bucket's weight gradients and in front of everything that reads it from here on
            L.check(L.lib.dsl_grad_accumulate(C.c_void_p(acc.data_ptr() + lo * 4), L.ptr(g), hi - lo, L.ACC_FOLD, csp), 'dsl_grad_accumulate')
            self.folded.add((int(lo), int(hi)))
        if proxy is not None:
            # the bucket's stand-in collective (no peer: the values stay): same stream, same event, same optimizer hand-over
            L.check(L.lib.dsl_comm_proxy(L.ptr(g), (hi - lo) // 4 * 4, int(proxy.get('wgs', 32)), int(proxy.get('passes', 2)), csp),
                    'dsl_comm_proxy')
            self.pending.append(StreamWork(cs))
            self._n_exchanged += 1
            return
        with torch.cuda.stream(cs):
            if self.comm_trace:
                es = torch.cuda.Event(enable_timing=True)
                es.record()            # the bucket's named event has fired and the previous bucket's traffic is queued
                self.comm_trace[-1]['buckets'].append(dict(mb=(hi - lo) * (2 if self.grad_bf16 else 4) / 1e6, start=es, done=None))
            work = None
            if self.grad_bf16:
                # the bucket crosses xGMI as a bf16 copy (RCCL's own ring then adds in bf16 per hop; the fp32 master gradient
                # gets the result back): cast -> all-reduce -> cast back, all on the communication stream
                if self._g16 is None or self._g16.device != g.device:
                    self._g16 = torch.empty(st.grad.numel(), dtype=torch.bfloat16, device=g.device)
                g16 = self._g16[lo:hi]
                L.check(L.lib.dsl_cast_bf16(L.ptr(g), L.ptr(g16), hi - lo, csp), 'dsl_cast_bf16')
                if self.rccl is not None:
                    L.check(L.lib.dsl_allreduce_bucket_bf16(self.rccl.comm, L.ptr(g16), hi - lo, csp), 'dsl_allreduce_bucket_bf16')
                elif dist.get_backend(self.group) == 'gloo':
                    # (the CPU-side test carrier has no bf16 sum: the bf16-rounded values are added in fp32 and rounded back)
                    t32 = g16.float()
                    dist.all_reduce(t32, group=self.group, async_op=True).wait()
                    g16.copy_(t32)
                else:
                    dist.all_reduce(g16, group=self.group, async_op=True).wait()      # (orders cs behind the collective)
                L.check(L.lib.dsl_cast_f32(L.ptr(g16), L.ptr(g), hi - lo, csp), 'dsl_cast_f32')
            elif self.rccl is not None:
                self.rccl.all_reduce(g, cs)
            else:
                work = dist.all_reduce(g, group=self.group, async_op=True)
            if self.clip_partials is not None:
                # the clipping norm of the REDUCED bucket, as soon as it has arrived: only the fold + the update stay behind the
                # last bucket (FlatSGD.step)
                if work is not None:
                    work.wait()
                    work = None
                L.check(L.lib.dsl_sumsq_partial(L.ptr(g), hi - lo, C.c_void_p(self.clip_partials.data_ptr() + self._n_exchanged * L.SUMSQ_PARTS * 4),
                                                csp), 'dsl_sumsq_partial')
            self.pending.append(work if work is not None else StreamWork(cs))
        self._n_exchanged += 1

    # ---- after the pass: the optimizer, gradient readers -------------------------------------------------------------------------
    def next_late(self):
        """Late exchange: queues the next bucket's collective (order: layer2, layer3, layer4, head + FPN) and returns (info, work), or
        None when every bucket of the last backward pass has been handed out."""
        if not self.todo:
            return None
        info = self.todo.pop(0)
        n = len(self.pending)
        self.exchange(info)
        return info, self.pending[n]

    def wait(self):
        """Every exchange of the last backward pass is queued and the caller's stream ordered behind it: store.grad holds the sums."""
        while self.next_late() is not None:      # (a late exchange nobody asked for bucket by bucket: an optimizer with a global norm)
            pass
        for w in self.pending:
            w.wait()
        self.pending = []

    def clear_pending(self):
        """The optimizer's walk has ordered each bucket's update behind that bucket's exchange: nothing is left to wait for."""
        self.pending = []

    def open_window(self, acc):
        """Gradient accumulation: `acc` is the open window's bank; the closing pass's exchanges fold it into their buckets."""
        self.fold_acc = acc

    def close_window(self):
        self.fold_acc = None

    def want_norm_partials(self):
        """Data parallel + clipping: from the next backward pass on, the norm arrives in pieces - one partial sum per bucket,
        computed on the communication stream behind that bucket's all-reduce - and only their fold precedes the update."""
        if self.world_size > 1 and self.store.grad.is_cuda and self.clip_partials is None:
            self.clip_partials = torch.zeros(8 * L.SUMSQ_PARTS, device=self.store.device)

    def take_norm_partials(self):
        """(partial sums, how many of them) of the last backward pass's reduced buckets, once; None when that pass left none."""
        if not self.partials_valid:
            return None
        self.partials_valid = False
        return self.clip_partials, int(self.n_partials)

    # ---- the small collectives ---------------------------------------------------------------------------------------------------
    def all_reduce_async(self, t, after_current=False):
        """Sum `t` over the ranks beside the caller's stream; returns an object whose wait() orders the current stream behind it.
        after_current: the collective must see everything queued on the current stream so far (torch's process group
        orders its own stream that way by itself)."""
        if self.rccl is None or not t.is_cuda:
            return dist.all_reduce(t, group=self.group, async_op=True)
        cs = self.comm_stream()
        if after_current:
            cs.wait_stream(torch.cuda.current_stream())
        t.record_stream(cs)
        self.rccl.all_reduce(t, cs)
        return StreamWork(cs)

    def all_reduce_log(self, vec):
        """The step's log vector summed over the ranks, in place, on the caller's stream."""
        if self.rccl is not None and vec.is_cuda:
            self.rccl.all_reduce(vec)
        else:
            dist.all_reduce(vec, group=self.group)

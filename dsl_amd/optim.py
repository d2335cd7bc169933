"""Fused SGD over the flat parameter buffer (dsl_sgd_step): momentum, weight decay, the reference's
paramwise rules (bias_lr_mult / bias_decay_mult), gradient-norm clipping and the bf16 re-pack in one
pass.  Replaces torch.optim.SGD + mmcv OptimizerHook's clip_grad_norm_
(mmdet/apis/train.py:111,157-166; configs/fcos_semi/*.py `optimizer`, `optimizer_config`).

The optimizer family (dsl_optim_step): Nesterov SGD, Adam and AdamW, and mmcv's full paramwise_cfg as a table of up to 16
(lr_mult, decay_mult) groups (param_group_mults / build_groups below).  Plain momentum SGD with at most the two bias keys keeps
launching dsl_sgd_step with store.group, unchanged."""
import bisect
import ctypes as C
import math
import os

import torch

from . import _lib as L
from .exchange import BANKED, EAGER, LATE
from .registry import OPTIMIZERS


from .tuning import skip_items

PARAMWISE_KEYS = ('custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult', 'dcn_offset_lr_mult')
LEGACY_KEYS = ('bias_lr_mult', 'bias_decay_mult')          # what dsl_sgd_step's one-bit flag expresses


def is_norm_param(name):
    """mmcv decides by module type (_BatchNorm, _InstanceNorm, GroupNorm, LayerNorm); here by the state-dict name: the towers'
    GroupNorms (`.gn.`), BatchNorms (`.bnN`, `downsample.1`) and RLA_ResNet's per-block `stage_bns`."""
    return ('.gn.' in name) or ('.bn' in name) or ('downsample.1' in name) or ('.stage_bns.' in name)


def param_group_mults(name, paramwise_cfg=None):
    """(lr_mult, decay_mult) of the parameter with state-dict name `name`: mmcv 1.3.x DefaultOptimizerConstructor.add_params,
    restated FROM MEMORY (mmcv is not a dependency):
      1. custom_keys first: the keys sorted alphabetically, then by length descending (stable); the first key that is a substring
         of the name wins, its lr_mult / decay_mult (default 1) apply and NO other rule does.
      2. otherwise lr_mult = bias_lr_mult for a leaf `bias` outside norm layers (and outside DCN modules: none are built);
      3. otherwise decay_mult = norm_decay_mult for any parameter of a norm layer; else dwconv_decay_mult for a depth-wise
         convolution (none are built); else bias_decay_mult for a leaf `bias`; else 1.
    dwconv_decay_mult and dcn_offset_lr_mult are accepted and have no parameter to apply to."""
    pw = paramwise_cfg or {}
    unknown = [k for k in pw if k not in PARAMWISE_KEYS]
    if unknown:
        raise NotImplementedError(f'dsl_amd: paramwise_cfg keys {unknown} are not built ({", ".join(PARAMWISE_KEYS)})')
    custom = pw.get('custom_keys') or {}
    for key in sorted(sorted(custom), key=len, reverse=True):
        if key in name:
            return float(custom[key].get('lr_mult', 1.0)), float(custom[key].get('decay_mult', 1.0))
    leaf = name.rsplit('.', 1)[-1]
    norm = is_norm_param(name)
    lm = dm = 1.0
    if leaf == 'bias' and not norm:
        lm = float(pw.get('bias_lr_mult', 1.0))
    if norm:
        dm = float(pw.get('norm_decay_mult', 1.0))
    elif leaf == 'bias':
        dm = float(pw.get('bias_decay_mult', 1.0))
    return lm, dm


def build_groups(model, paramwise_cfg=None):
    """The group table and the per-element group ids of a detector's flat parameter buffer: one group per distinct
    (lr_mult, decay_mult) pair over model.named_parameters() (trainable ones), group 0 always (1, 1).  Every parameter is a view
    into store.train and has to lie inside one region of store.train_regions; what no parameter covers (tile padding, the
    predictors' padding rows) is group 0.  Returns ([(lr_mult, decay_mult)], uint8 CPU tensor [n_train], {name: group})."""
    st = model.store
    regs = sorted((int(o), int(n), k) for k, (o, n, _) in st.train_regions.items())
    starts = [r[0] for r in regs]
    table, by_name, todo = [(1.0, 1.0)], {}, []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        lo = int(p.storage_offset())
        hi = lo + sum((int(d) - 1) * int(s) for d, s in zip(p.shape, p.stride()))
        r = regs[max(bisect.bisect_right(starts, lo) - 1, 0)]
        if not (r[0] <= lo and hi < r[0] + r[1]):
            raise RuntimeError(f'parameter {name} [{lo}, {hi}] is not inside one region of the flat parameter buffer (nearest: {r[2]})')
        pair = param_group_mults(name, paramwise_cfg)
        if pair not in table:
            table.append(pair)
        by_name[name] = table.index(pair)
        todo.append((p, by_name[name]))
    if len(table) > L.OPT_MAX_GROUPS:
        raise NotImplementedError(f'dsl_amd: paramwise_cfg yields {len(table)} distinct (lr_mult, decay_mult) pairs; '
                                  f'dsl_optim_step has {L.OPT_MAX_GROUPS} groups')
    ids = torch.zeros(st.n_train, dtype=torch.uint8)
    for p, k in todo:
        if k:
            ids.as_strided(tuple(p.shape), tuple(p.stride()), int(p.storage_offset())).fill_(k)
    return table, ids, by_name


_PACK_SIDE = True                          # data-gradient weight packs off the caller's stream (measured: tools/experiments_r2.txt (exp_r2l))


@OPTIMIZERS.register_module(name='SGD')
class FlatSGD:
    def __init__(self, model, lr=0.01, momentum=0.9, weight_decay=0.0, paramwise_cfg=None, grad_clip=None,
                 defer_head_update=False, late_exchange=True, nesterov=False, dampening=0, **kw):
        if dampening != 0:
            raise NotImplementedError(f'dsl_amd: SGD dampening={dampening!r} is not built (0 only)')
        self.nesterov = bool(nesterov)
        if self.nesterov and float(momentum) == 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')          # (torch.optim.SGD's wording)
        self.momentum = float(momentum)
        self._setup(model, lr, weight_decay, paramwise_cfg, grad_clip, defer_head_update, late_exchange,
                    legacy=not self.nesterov and all(k in LEGACY_KEYS for k in (paramwise_cfg or {})))

    kind = 'SGD'          # saved with the state (family path); a state of another kind is refused
    STATE = ('momentum_buf',)          # the flat state buffers, laid out like store.train (state_dict key: _STATE_KEYS)
    _STATE_KEYS = dict(momentum_buf='momentum', exp_avg_sq='exp_avg_sq')

    def _setup(self, model, lr, weight_decay, paramwise_cfg, grad_clip, defer_head_update, late_exchange, legacy):
        self.model = model
        self.store = model.store
        self.exchange = model.exchange          # the detector's gradient exchange (data parallel, accumulation windows)
        pw = dict(paramwise_cfg or {})
        self.paramwise_cfg = pw
        self.bias_lr_mult = float(pw.get('bias_lr_mult', 1.0))
        self.bias_decay_mult = float(pw.get('bias_decay_mult', 1.0))
        self.weight_decay = float(weight_decay)
        self.max_norm = None
        if grad_clip:
            assert grad_clip.get('norm_type', 2) == 2
            self.max_norm = float(grad_clip['max_norm'])
        self.legacy = bool(legacy)          # plain momentum SGD, bias keys only: dsl_sgd_step on store.group, as ever
        if self.legacy:
            # two groups so that LR schedulers written against torch optimizers keep working
            self.param_groups = [dict(lr=lr, initial_lr=lr, name='weights'),
                                 dict(lr=lr * self.bias_lr_mult, initial_lr=lr * self.bias_lr_mult, name='conv_bias')]
            self.group_table = self.group_ids = self.group_of = None
        else:
            # one group per distinct (lr_mult, decay_mult) pair (build_groups); the ids belong to this optimizer, store.group stays
            self.group_table, self.group_ids, self.group_of = build_groups(model, pw)
            self.param_groups = [dict(lr=lr * lm, initial_lr=lr * lm, lr_mult=lm, decay_mult=dm, name=f'lr_mult={lm:g},decay_mult={dm:g}')
                                 for lm, dm in self.group_table]
        self._group_dev = None
        self.momentum_buf = None
        self.gnorm_sq = None
        self.steps = 0
        self._loaded_regions = None          # load_state_dict: name -> (offset, size) of the restored momentum, until step() adopts it
        self._side1 = self._opt_stream = None          # the walk's streams, made at first need
        self._sumsq_ws = None
        self._acc = None          # gradient accumulation (accumulate()): the open window's running sum, laid out like store.grad
        self.acc_count = 0        # micro-steps banked in the open window
        self.late_exchange = bool(late_exchange)      # data parallel without clipping: collectives behind the backward pass (see _sync_defer)
        self.defer_head_update = bool(defer_head_update)      # opt-in (measured slower on one GPU, LAB_NOTES: deferred head update)
        self._sync_defer()

    def _sync_defer(self):
        """Deferred head update (engine.Plan.defer): possible when the update is element-wise per bucket - no gradient
        clipping (a global norm needs every gradient first), per-bucket steps on, packs on the side stream.  The flag lives on
        the parameter store because it shapes the op lists; opt-in (constructor argument defer_head_update)."""
        want = (self.max_norm is None and _PACK_SIDE and self.defer_head_update
                and self.store.backbone != 'rla')
        # Late exchange (data parallel): with an element-wise per-bucket update nothing at the end of a step has to
        # wait for the collectives - the detector queues them behind the backward pass and the next forward pass waits stage by stage
        self.exchange.late_wanted = bool(self.max_norm is None and _PACK_SIDE and self.late_exchange and self.store.backbone != 'rla')
        if bool(getattr(self.store, 'defer_head', False)) != want:
            self.store.wait_pending() if self.store.train.is_cuda else None
            self.store.defer_head = want        # plans are keyed by it (Engine.plan): lists built the other way are not reused

    def zero_grad(self, set_to_none=False):
        # every gradient element is overwritten by the backward kernels; nothing to clear
        return

    def _adopt_loaded_state(self):
        """A momentum tensor restored by load_state_dict (CPU tensor, possibly laid out by another build) -> a buffer laid out like this
        model's parameter buffer.  Called by step(); separate so that it can be checked without a device."""
        # state restored from a checkpoint (CPU tensor, possibly laid out by another build): move it into a buffer laid out like
        # the parameter buffer, REGION BY REGION (name -> offset, size, saved with the state), and keep the step count (resume
        # must not re-zero momentum).  A prefix copy is only right when the two layouts differ by trailing padding; a state
        # without a region table whose size is off by more than that is refused instead of being attached to the wrong parameters.
        for attr in self.STATE:          # (the Adam kinds: the second moment the same way)
            setattr(self, attr, self._remap(getattr(self, attr)))
        self._loaded_regions = None

    def _remap(self, loaded):
        st = self.store
        src = loaded.reshape(-1)
        buf = torch.zeros_like(st.train)
        regs = self._loaded_regions
        cur = {k: (int(v[0]), int(v[1])) for k, v in st.train_regions.items()}
        if regs:
            regs = {k: (int(v[0]), int(v[1])) for k, v in regs.items()}
            missing = [k for k in cur if k not in regs]
            if missing:
                raise RuntimeError(f'optimizer state: no momentum for {len(missing)} parameter regions of this model (first: {missing[:3]})')
            for k, (o, n) in cur.items():
                so, sn = regs[k]
                m = min(n, sn)          # (a region's tail is tile padding: zeros in both)
                buf.view(-1)[o:o + m].copy_(src[so:so + m].to(device=st.device, dtype=buf.dtype))
        else:
            if abs(buf.numel() - src.numel()) > 4096:
                raise RuntimeError(f'optimizer state: momentum has {src.numel()} elements, the parameter buffer {buf.numel()}, and the '
                                   'state carries no region table to remap it by (saved by an older build with another layout?)')
            n = min(buf.numel(), src.numel())
            buf.view(-1)[:n].copy_(src[:n].to(device=st.device, dtype=buf.dtype))
        return buf

    def step(self):
        st = self.store
        fresh = False
        if self.momentum_buf is None:
            # (zeros, queued on the CALLER's stream: the per-bucket path below runs on other streams that are not ordered behind the
            # caller's - `fresh` makes them wait for this fill.  Round 4: without that wait the fill could land AFTER the first
            # bucket's update had written its momentum - that bucket then started its second step from zero momentum; which buckets,
            # if any, depended on how far the GPU lagged behind the host: found as a flaky bit-exactness test once the optimizer's
            # stream was shared between model instances)
            for attr in self.STATE:
                setattr(self, attr, torch.zeros_like(st.train))
            self.steps = 0
            fresh = True
        elif (self.momentum_buf.device != st.device or self.momentum_buf.shape != st.train.shape
              or self._loaded_regions is not None):
            self._adopt_loaded_state()
            fresh = True          # (copied into place on the caller's stream just now: the same ordering as for the zero fill)
        if not self.legacy and (self._group_dev is None or self._group_dev.device != st.device):
            self._group_dev = self.group_ids.to(st.device)
            fresh = True          # (uploaded on the caller's stream: the same ordering again)
        if self.gnorm_sq is None or self.gnorm_sq.device != st.device:
            self.gnorm_sq = torch.zeros(1, device=st.device)
        if self.exchange.mode == BANKED:
            raise RuntimeError('FlatSGD.step(): the last backward pass was declared non-closing (set_closing(False)) and queued no '
                               'gradient exchange: call set_closing(True) in front of the train_step whose step() closes the window')
        self._walk(True, fresh)
        self.steps += 1
        if self.acc_count:
            self.acc_count = 0
            self.exchange.close_window()
        self.set_closing(True)

    def set_closing(self, closing):
        """Gradient accumulation under data parallel: says whether the NEXT backward pass closes its window, i.e. is followed by
        step() (True, the default) or by accumulate() (False: that pass queues no gradient collective - the window's sum is exchanged
        once, by the closing pass).  Call it in front of train_step (the eager backward pass is queued in there);
        GradientCumulativeOptimizerHook does so in before_train_iter.  step() sets it back to True."""
        self.exchange.closing = bool(closing)

    def accumulate(self):
        """Banks the gradient of the backward pass that has just run instead of applying it: step() with the update kernel swapped
        for dsl_grad_accumulate - the same buckets on the same streams behind the same events (_walk), so the next backward pass
        cannot overwrite a bucket this call still reads.  The next step() folds the bank into store.grad (DSL_ACC_FOLD) in front
        of whatever reads each bucket first.  The bank is one fp32 tensor like store.grad, made at the first call."""
        st, ex = self.store, self.exchange
        if not st.grad.is_cuda:
            raise RuntimeError('FlatSGD.accumulate() runs on the GPU only (dsl_grad_accumulate; no host fallback)')
        if ex.mode in (LATE, EAGER) or ex.pending or ex.todo:
            raise RuntimeError('FlatSGD.accumulate(): the last backward pass queued its gradient exchange - a window is exchanged once, '
                               'by its closing pass: call set_closing(False) in front of the train_step of a micro-step that accumulates')
        fresh = False
        if self._acc is None or self._acc.device != st.device or self._acc.shape != st.grad.shape:
            # (from torch's allocator on the CALLER's stream, written on the walk's streams: they wait, as for the momentum's fill)
            self._acc = torch.empty_like(st.grad)
            self.acc_count = 0
            fresh = True
        self._walk(False, fresh)
        self.acc_count += 1
        ex.open_window(self._acc)          # (the exchange folds it into each bucket in front of that bucket's exchange)

    def _acc_launch(self, lo, hi, mode, tp):
        L.check(L.lib.dsl_grad_accumulate(C.c_void_p(self._acc.data_ptr() + lo * 4), C.c_void_p(self.store.grad.data_ptr() + lo * 4),
                                          hi - lo, mode, tp), 'dsl_grad_accumulate')

    def _desc(self):
        """dsl_optim_desc of the step about to run: the groups' current rates (the LR hooks write param_groups[k]['lr']), weight
        decay per group, and this kind's scalars."""
        d = L.OptimDesc()
        d.kind, d.n_groups = L.OPT_SGD, len(self.param_groups)
        for k, g in enumerate(self.param_groups):
            d.lr[k] = float(g['lr'])
            d.wd[k] = self.weight_decay * float(g['decay_mult'])
        d.momentum, d.nesterov, d.first_step = self.momentum, int(self.nesterov), int(self.steps == 0)
        d.max_norm = self.max_norm or 0.0
        return d

    def _update(self, lo, hi, gptr, stream_ptr):
        """The update of elements [lo, hi) of the flat buffers on the stream `stream_ptr`; gptr: the squared gradient norm on the
        device (clipping), or None.  _walk's one way to the kernels, per bucket and flat."""
        st = self.store
        at = lambda t, size: C.c_void_p(t.data_ptr() + lo * size)          # noqa: E731
        if self.legacy:
            lr = float(self.param_groups[0]['lr'])
            blr = float(self.param_groups[1]['lr']) / lr if lr != 0 else self.bias_lr_mult
            L.check(L.lib.dsl_sgd_step(at(st.train, 4), at(st.grad, 4), at(self.momentum_buf, 4), at(st.train16, 2), at(st.group, 1),
                                       hi - lo, lr, self.momentum, self.weight_decay, blr, self.bias_decay_mult, L.ptr(gptr),
                                       self.max_norm or 0.0, int(self.steps == 0), stream_ptr), 'dsl_sgd_step')
            return
        v = getattr(self, 'exp_avg_sq', None)
        L.check(L.lib.dsl_optim_step(C.byref(self._desc()), at(st.train, 4), at(st.grad, 4), at(self.momentum_buf, 4),
                                     at(v, 4) if v is not None else None, at(st.train16, 2), at(self._group_dev, 1), hi - lo,
                                     L.ptr(gptr), stream_ptr), 'dsl_optim_step')

    def _walk(self, update, fresh):
        """The schedule shared by step() (update=True) and accumulate() (False): which stream touches which gradient bucket behind
        which events.  accumulate() swaps dsl_sgd_step for dsl_grad_accumulate and leaves the data-gradient packs alone (the
        weights did not move: SLOT_PACKS still stands for packs of the current weights); every wait and record is the same.
        step() with banked micro-steps (acc_count > 0) folds the bank into each bucket first, unless that bucket's exchange did
        (the exchange lists those in `folded`)."""
        st, ex = self.store, self.exchange
        window = update and self.acc_count > 0
        acc_mode = L.ACC_ADD if self.acc_count else L.ACC_SET
        sp = L.stream_ptr()
        self._sync_defer()          # (OptimizerHook may set max_norm after construction)
        infos = ex.buckets          # completion order; a deferred bucket comes last
        if self.max_norm is None and infos and st.grad.is_cuda and all(i['bucket'][0] % 4 == 0 for i in infos):
            # No gradient clipping (the supervised config): the update is element-wise, so each gradient bucket - head + FPN,
            # layer4, layer3, layer2, in the order the backward pass completes them - is updated on the optimizer's own stream
            # as soon as its weight gradients (data parallel: its all-reduce) are done, beside the rest of the backward pass,
            # instead of one pass over all 32 M parameters behind the last weight gradient.  Same arithmetic, same bits.
            cur = torch.cuda.current_stream()
            deferred = any(i.get('deferred') for i in infos)
            if deferred:
                # Deferred head update: the buckets the next forward pass needs first are updated on the CALLER's stream (idle once
                # the data-gradient chain is through), the deferred bucket on the weight-gradient stream itself, in order behind the
                # towers' group.  A stream of the optimizer's own would do logically, but streams share four hardware queues: it
                # landed on the weight-gradient stream's queue, and the three early updates - hence the whole next forward pass -
                # then sat behind the deferred 0.5 ms group (measured: 401 instead of 430 img/s, profiles/r04_defer_first.txt).
                if self._side1 is None:
                    h = C.c_void_p()
                    L.check(L.lib.dsl_side_stream(1, C.byref(h)), 'dsl_side_stream')
                    self._side1 = torch.cuda.ExternalStream(h.value)
                os_ = None
            else:
                if self._opt_stream is None:
                    from .detectors import role_stream          # one optimizer stream per device and process (hardware queues)
                    self._opt_stream = role_stream('optimizer', st.device)
                os_ = self._opt_stream
            pend = list(ex.pending)
            # late exchange: the backward pass queued no collective - each is asked for here, in front of its bucket's update
            late = bool(ex.todo) and not deferred and not pend
            seq = list(enumerate(infos[::-1] if late else infos))
            if fresh:
                for s_ in ([self._side1] if deferred else [os_]):
                    s_.wait_stream(cur)          # the momentum buffer's zero fill (see above)
            for k, info in seq:
                lo, hi = info['bucket']
                tgt = (self._side1 if info.get('deferred') else cur) if deferred else os_
                tp = C.c_void_p(tgt.cuda_stream)
                if late:
                    got = ex.next_late()
                    assert got is not None and got[0] is info, 'late exchange: bucket order'
                    pend.append(got[1])
                if pend:
                    with torch.cuda.stream(tgt):
                        pend[k].wait()
                        tr = ex.comm_trace
                        if tr and k < len(tr[-1]['buckets']):
                            ed = torch.cuda.Event(enable_timing=True)
                            ed.record()
                            tr[-1]['buckets'][k]['done'] = ed
                elif not (deferred and info.get('deferred')):          # (the deferred bucket's stream IS the one its gradients ran on)
                    never = L.lib.dsl_stream_wait_slot(int(info['slot']), tp)
                    # (data parallel with the exchanges already waited for on the caller's stream - FCOS.wait_grads: the update must
                    #  follow them, not only its weight gradients)
                    if (info['main'] or never != 0 or ex.world_size > 1) and tgt is not cur:
                        tgt.wait_stream(cur)
                if 'sgd' in skip_items():          # step-level ablation (tools/step_ablation.sh): timing only
                    continue
                if not update:
                    self._acc_launch(lo, hi, acc_mode, tp)
                    continue
                # (ex.folded is read bucket by bucket: the late exchanges run, and fold, inside this walk)
                if window and (int(lo), int(hi)) not in ex.folded:          # (no exchange in front of this bucket's update: the fold goes here)
                    self._acc_launch(lo, hi, L.ACC_FOLD, tp)
                self._update(lo, hi, None, tp)
                if late:          # "gradient bucket <slot> is updated": what the next forward pass waits for in front of that stage
                    L.check(L.lib.dsl_stream_record_slot(L.SLOT_UPD + int(info['slot']), tp), 'dsl_stream_record_slot')
            ex.clear_pending()
            if deferred:
                s1p = C.c_void_p(self._side1.cuda_stream)
                L.check(L.lib.dsl_stream_record_slot(L.SLOT_HEADW, s1p), 'dsl_stream_record_slot')
                st._pending_ev = torch.cuda.Event()
                st._pending_ev.record(self._side1)
                # the data-gradient packs read every bucket: behind the caller's stream (its three updates) AND the deferred one,
                # i.e. forked from the caller's stream onto the weight-gradient stream, in order behind the deferred update
                if update:
                    st.repack_dgrad(sp, side=True)
            elif late:
                # nothing on the caller's stream waits: the next forward pass waits per stage (SLOT_UPD), every other reader of the
                # parameters calls ParamStore.wait_pending; the data-gradient packs follow the last update on the optimizer's stream
                # (= side stream 1, where repack_dgrad(side=True) queues them) and mark SLOT_PACKS for the next backward pass
                st._pending_ev = torch.cuda.Event()
                st._pending_ev.record(os_)
                st.repack_dgrad(sp, side=True)
            else:
                cur.wait_stream(os_)
                if update:
                    st.repack_dgrad(sp, side=_PACK_SIDE)
            return
        ex.wait()
        for i in infos:
            if i.get('deferred'):        # a list built for the deferred head update left its last weight gradients unjoined
                L.lib.dsl_stream_wait_slot(int(i['slot']), sp)
        if not update:
            self._acc_launch(0, st.n_train, acc_mode, sp)
            return
        if window:
            # the buckets whose exchange folded them (data parallel) are done; the rest - one GPU: everything - in front of the norm
            done = ex.folded
            rest = [(0, st.n_train)] if not done else [i['bucket'] for i in infos if (int(i['bucket'][0]), int(i['bucket'][1])) not in done]
            for lo, hi in rest:
                self._acc_launch(lo, hi, L.ACC_FOLD, sp)
        gptr = None
        if self.max_norm is not None:
            ex.want_norm_partials()          # (data parallel: from the next backward pass on the norm arrives in pieces, per bucket)
            parts = ex.take_norm_partials()
            if parts is not None:
                L.check(L.lib.dsl_sumsq_fold(L.ptr(parts[0]), parts[1], L.ptr(self.gnorm_sq), sp), 'dsl_sumsq_fold')
            else:
                if self._sumsq_ws is None or self._sumsq_ws.device != st.device:
                    self._sumsq_ws = torch.zeros(1024, device=st.device)
                L.check(L.lib.dsl_sumsq_det(L.ptr(st.grad), st.n_train, L.ptr(self.gnorm_sq), L.ptr(self._sumsq_ws), sp), 'dsl_sumsq_det')
            gptr = self.gnorm_sq
        self._update(0, st.n_train, gptr, sp)
        st.repack_dgrad(sp, side=_PACK_SIDE)

    def state_dict(self):
        # regions: where every named parameter lives in the flat momentum buffer - what load_state_dict / step remap by.
        # (late exchange / deferred head update: the last step's updates may still be writing the momentum on another stream)
        self.store.wait_pending()
        sd = dict(momentum=self.momentum_buf, steps=self.steps, param_groups=self.param_groups,
                  regions={k: (int(v[0]), int(v[1])) for k, v in self.store.train_regions.items()})
        if not self.legacy:          # (the legacy path's state keeps its four keys: checkpoints of every earlier build)
            sd.update(kind=self.kind, groups=[tuple(g) for g in self.group_table])
            for attr in self.STATE[1:]:
                sd[self._STATE_KEYS[attr]] = getattr(self, attr)
        return sd

    def load_state_dict(self, sd):
        """Restores momentum, the step count (first-step rule of torch.optim.SGD: buf = grad) and the groups' learning
        rates.  The momentum tensor may live on the CPU (runner.resume loads with map_location='cpu'); step() moves it.
        A state of another kind (no `kind`: plain SGD) or with another group table is refused: its moments mean something else."""
        theirs = sd.get('kind', 'SGD')
        if theirs != self.kind:
            raise RuntimeError(f'optimizer state: saved by kind {theirs!r}, this optimizer is of kind {self.kind!r}')
        groups = [tuple(float(x) for x in g) for g in sd['groups']] if sd.get('groups') else None
        if groups != (None if self.legacy else [tuple(g) for g in self.group_table]):
            raise RuntimeError(f'optimizer state: its parameter groups (lr_mult, decay_mult) {groups or "of plain SGD (bias flag)"} are not '
                               f'this optimizer\'s {self.group_table or "of plain SGD (bias flag)"}: nesterov / paramwise_cfg differ')
        self.store.wait_pending()          # (the buffer replaced here may still be written by the last step's updates)
        for attr in self.STATE:
            m = sd.get(self._STATE_KEYS[attr])
            setattr(self, attr, m.detach().clone() if isinstance(m, torch.Tensor) else None)
        if any(getattr(self, attr) is None for attr in self.STATE):          # (saved before the first step)
            for attr in self.STATE:
                setattr(self, attr, None)
        self.steps = int(sd['steps']) if self.momentum_buf is not None else 0
        self.param_groups = [dict(g) for g in sd['param_groups']]
        self._loaded_regions = dict(sd['regions']) if sd.get('regions') else None
        if self._loaded_regions is None and self.momentum_buf is not None:
            self._loaded_regions = {}          # (falsy, but makes step() run the size check once)
        self.gnorm_sq = None
        self._sumsq_ws = None
        self.acc_count = 0          # (the accumulation window is not part of the state: a resume starts a fresh one)
        self.exchange.close_window()


@OPTIMIZERS.register_module(name='Adam')
class FlatAdam(FlatSGD):
    """torch.optim.Adam (and AdamW: FlatAdamW) over the flat parameter buffer, dsl_optim_step's Adam kinds.  The first moment is
    `momentum_buf` (exp_avg), so every reader of FlatSGD's state keeps working; the second, `exp_avg_sq`, lies beside it, laid out
    like store.train and zero-filled with it on the caller's stream.  The bias corrections of step t = steps + 1 are computed
    here in double (there is no device step counter).  The schedule - buckets, streams, late exchange, deferred head update,
    accumulation, clipping - is FlatSGD._walk's, unchanged."""
    kind = 'Adam'
    STATE = ('momentum_buf', 'exp_avg_sq')

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, paramwise_cfg=None, grad_clip=None,
                 defer_head_update=False, late_exchange=True, amsgrad=False, **kw):
        if amsgrad:
            raise NotImplementedError('dsl_amd: amsgrad=True is not built (Adam / AdamW without the running maximum)')
        self.beta1, self.beta2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        if not (0.0 <= self.beta1 < 1.0 and 0.0 <= self.beta2 < 1.0 and self.eps >= 0.0):
            raise ValueError(f'invalid betas {betas!r} / eps {eps!r}')
        self.momentum, self.nesterov = 0.0, False
        self.exp_avg_sq = None
        self._setup(model, lr, weight_decay, paramwise_cfg, grad_clip, defer_head_update, late_exchange, legacy=False)

    exp_avg = property(lambda self: self.momentum_buf)

    def _desc(self):
        d = super()._desc()
        d.kind = L.OPT_ADAMW if self.kind == 'AdamW' else L.OPT_ADAM
        t = self.steps + 1
        d.beta1, d.beta2, d.eps = self.beta1, self.beta2, self.eps
        d.step_scale = 1.0 / (1.0 - self.beta1 ** t)
        d.rsqrt_bc2 = 1.0 / math.sqrt(1.0 - self.beta2 ** t)
        return d


@OPTIMIZERS.register_module(name='AdamW')
class FlatAdamW(FlatAdam):
    """torch.optim.AdamW: the decay leaves the gradient and multiplies the weight (p *= 1 - lr wd) in front of Adam's update."""
    kind = 'AdamW'

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)


def build_optimizer(model, cfg, grad_clip=None):
    cfg = dict(cfg)
    t = cfg.pop('type')
    cls = OPTIMIZERS.get(t)
    if cls is None:
        raise KeyError(f'optimizer {t} is not available on the HIP path')
    m = model.module if hasattr(model, 'module') else model
    return cls(m, grad_clip=grad_clip, **cfg)

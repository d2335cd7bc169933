"""The per-bucket SGD update and the late gradient exchange against host math.

Without gradient clipping FlatSGD.step updates the gradient buckets (head + FPN, layer4, layer3, layer2) one at a time on the
optimizer's stream, and with more than one rank it queues each bucket's all-reduce right in front of that bucket's update (late
exchange, FlatSGD(late_exchange=True)).  Here the weights, the momentum and the bf16 copies that path leaves behind are compared
with a float64 update computed on the host from the captured fp32 gradient, weights and momentum, with learning rate and weight
decay derived from the parameter NAMES (oracle.fcos_oracle.param_group_rule); the two-rank tests sum the ranks' local gradients on
the host and compare what the collectives delivered bit for bit."""
import os
import queue
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from util import fcos_model_cfg

pytestmark = pytest.mark.gpu
H, W = 128, 192
OPT = dict(lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))
LR_SCALE = (1 / 3, 1 / 3, 1.0)          # per step: a warm-up hook's factor on every group's initial lr (changes once)
CHUNK = 1 << 22


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def make_batch(rank, C=80, flip=False):
    """test_ddp_gpu.make_batch with labels below C: two images per rank of a fixed 4-image batch.  flip: the same images
    mirrored left-right (boxes unchanged), a batch with other gradients."""
    from oracle import fcos_oracle as O
    g = torch.Generator().manual_seed(77)
    img = (torch.randn(4, 3, H, W, generator=g) * 30).bfloat16().float()
    if flip:
        img = img.flip(-1).contiguous()
    rng = np.random.RandomState(9)
    gtb = [torch.from_numpy(O.synth_boxes(rng, 3, H=H, W=W, lo=8, hi=100)) for _ in range(4)]
    gtl = [torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')) for b in gtb]
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * 4
    sl = slice(2 * rank, 2 * rank + 2)
    return dict(img=img[sl].cuda(), img_metas=metas[sl], gt_bboxes=gtb[sl], gt_labels=gtl[sl])


def build(C=80, rla=False):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from oracle import fcos_oracle as O
    from oracle import rla_oracle as RO
    cfg = fcos_model_cfg(num_classes=C)
    if rla:
        cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
    model = build_detector(cfg)
    model.load_state_dict((RO if rla else O).synth_state_dict(0, num_classes=C))
    return model.cuda()


def _set_lr(opt, step):
    for g in opt.param_groups:
        g['lr'] = g['initial_lr'] * LR_SCALE[step]


def _no_host_sync(model):
    """The autograd bridges read their incoming gradient back on a detector's first backward calls (detectors._check_grad_now):
    spend that budget so that an unsynchronized run really has no host synchronization in it."""
    model.__dict__['_grad_checks_left'] = dict(total=0, train_step=0)


def _f32(x):
    return float(np.float32(x))


def _ulp32(x):
    """ulp of float32 at magnitude x (float64 tensor, x >= 0); the smallest subnormal at 0."""
    _, e = torch.frexp(x)
    u = torch.pow(2.0, (e.to(torch.float64) - 24).clamp(min=-149))
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -149), u)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


class HostRef:
    """Per element of the flat parameter buffer: which named parameter owns it and the multipliers of its learning rate and
    weight decay, derived from the parameter's name as oracle.sgd_step does (not read from store.group)."""

    def __init__(self, model, opt):
        from oracle.fcos_oracle import param_group_rule
        st = model.store
        n = st.n_train
        self.n, self.opt = n, opt
        idx = torch.arange(n, dtype=torch.int64)
        self.owner = torch.full((n,), -1, dtype=torch.int64)
        self.lm = torch.ones(n, dtype=torch.float64)
        self.dm = torch.ones(n, dtype=torch.float64)
        self.names = []
        mom = st.named_views(opt.momentum_buf) if opt.momentum_buf is not None else None
        blm, bdm = opt.bias_lr_mult, opt.bias_decay_mult
        for k, p in model.named_parameters():
            if not p.requires_grad:
                continue
            # state-dict names whose tensors are views into store.train, the gradients the same views into store.grad
            assert p.untyped_storage().data_ptr() == st.train.untyped_storage().data_ptr(), k
            gr = p.grad
            assert gr is not None and gr.untyped_storage().data_ptr() == st.grad.untyped_storage().data_ptr(), k
            assert (gr.shape, gr.stride(), gr.storage_offset()) == (p.shape, p.stride(), p.storage_offset()), k
            if mom is not None:
                mv = mom[k]
                assert (mv.shape, mv.stride(), mv.storage_offset()) == (p.shape, p.stride(), p.storage_offset()), k
            e = idx.as_strided(p.shape, p.stride(), p.storage_offset()).reshape(-1)
            assert bool((self.owner[e] == -1).all()), f'{k} overlaps {self.names[int(self.owner[e].max())]}'
            self.owner[e] = len(self.names)
            self.names.append(k)
            lm, dm = param_group_rule(k, 1.0, 1.0, blm, bdm)
            self.lm[e], self.dm[e] = lm, dm
        self.covered = self.owner >= 0
        assert len(self.names) > 100 and int(self.covered.sum()) > 0.9 * n
        # store.group (the kernel's bias flag) agrees with the names: set exactly on the elements of parameters the rule treats as
        # biases (the padding behind a region is nobody's: not checked here, it must simply stay as it is - see check())
        is_bias = (self.lm != 1.0) | (self.dm != 1.0)
        flag = st.group.cpu() != 0
        bad = self.covered & (flag != is_bias)
        assert not bool(bad.any()), f'store.group disagrees with the names on {int(bad.sum())} elements, first: ' \
            f'{sorted({self.names[int(o)] for o in self.owner[bad][:1000]})[:5]}'

    def _who(self, mask, lo):
        at = torch.nonzero(mask).flatten()[:3] + lo
        return [(int(i), self.names[int(self.owner[i])] if int(self.owner[i]) >= 0 else 'padding') for i in at]

    def check(self, lr, first, p0, g, m0, p1, m1, t16):
        """Host tensors: p0, g, m0 (None on the first step) the fp32 buffers in front of the update, p1, m1, t16 behind it.
        Per covered element, in float64 with the kernel's formula (optim.hip sgd_kernel) and its fp32 arguments:
            d = g + wd_e p,   m = d (first step) or mom m + d,   p -= lr_e m
        |m_hip - m_ref| <= 2 ulp32 of the largest term of m (|g|, |wd_e p|, |d|, |mom m0|, |m|), |p_hip - p_ref| <= 2 ulp32 of
        max(|p_ref|, |lr_e m_ref|) plus the momentum's own deviation carried through lr_e (hipcc may contract to FMA: bit equality
        with the host is not required).  Elements no named parameter covers keep their bits.  train16 = bf16(train) bit for bit.
        Returns a list of failures."""
        errs = []
        lr32, wd32, mom32 = _f32(lr), _f32(self.opt.weight_decay), _f32(self.opt.momentum)
        changed = 0
        for lo in range(0, self.n, CHUNK):
            sl = slice(lo, min(self.n, lo + CHUNK))
            cov = self.covered[sl]
            P0, G = p0[sl].double(), g[sl].double()
            M0 = torch.zeros_like(P0) if first else m0[sl].double()
            lr_e, wd_e = lr32 * self.lm[sl], wd32 * self.dm[sl]
            wp = wd_e * P0
            d = G + wp
            m = d if first else mom32 * M0 + d
            p = P0 - lr_e * m
            em = (m1[sl].double() - m).abs()
            sm = torch.stack([G.abs(), wp.abs(), d.abs(), (mom32 * M0).abs(), m.abs()]).amax(0)
            bad = cov & (em > 2 * _ulp32(sm))
            if bad.any():
                errs.append(f'momentum off the float64 update on {int(bad.sum())} elements, first {self._who(bad, lo)}, '
                            f'max |err| / ulp {float((em / _ulp32(sm))[bad].max()):.1f}')
            ep = (p1[sl].double() - p).abs()
            tol = 2 * _ulp32(torch.maximum(p.abs(), (lr_e * m).abs())) + lr_e * em
            bad = cov & (ep > tol)
            if bad.any():
                errs.append(f'weights off the float64 update on {int(bad.sum())} elements, first {self._who(bad, lo)}, '
                            f'max |err| / ulp {float((ep / _ulp32(p.abs()))[bad].max()):.1f}')
            unc = ~cov
            m0b = torch.zeros_like(p0[sl]) if first else m0[sl]
            bad = unc & ((_bits(p1[sl]) != _bits(p0[sl])) | (_bits(m1[sl]) != _bits(m0b)))
            if bad.any():
                errs.append(f'{int(bad.sum())} padding elements of the flat buffer changed, first {self._who(bad, lo)}')
            changed += int((cov & (p1[sl] != p0[sl])).sum())
        if not torch.equal(_bits(t16), _bits(p1.bfloat16())):
            errs.append(f'train16 != bf16(train) on {int((_bits(t16) != _bits(p1.bfloat16())).sum())} elements')
        if changed < 0.5 * int(self.covered.sum()):
            errs.append(f'only {changed} of {int(self.covered.sum())} parameters changed: the update did not run')
        return errs


def _snapshot(model, opt):
    st = model.store
    m = opt.momentum_buf.cpu().clone() if opt.momentum_buf is not None else None
    return st.train.cpu().clone(), st.grad.cpu().clone(), m, st.train16.cpu().clone()


# ---- 1. one process: the per-bucket update of every schedule against the float64 host update --------------------------------------
LEGS = ['plain', 'proxy_late', 'defer_head', 'rla', 'c20']


def _single(leg):
    from dsl_amd.optim import FlatSGD
    C = 20 if leg == 'c20' else 80
    model = build(C=C, rla=leg == 'rla')
    opt = FlatSGD(model, defer_head_update=leg == 'defer_head', **OPT)
    if leg == 'proxy_late':
        # the data-parallel schedule on one GPU: the late path with the value-preserving stand-in for each bucket's all-reduce
        model.comm_proxy = dict(carrier='lib', wgs=32, passes=2)
    assert opt.max_norm is None
    assert model.store.defer_head == (leg == 'defer_head')
    return model, opt, C


def _check_padding_rows(model, opt, C, errs, step):
    st = model.store
    o, n, shape = st.train_regions['head.cls_w']
    rows = slice(o + C * shape[1] * shape[2] * shape[3], o + n)
    ob, nb, _ = st.train_regions['head.cls_b']
    for what, buf in (('train', st.train), ('momentum', opt.momentum_buf), ('train16', st.train16)):
        for sl in (rows, slice(ob + C, ob + nb)):
            if bool((buf[sl] != 0).any()):
                errs.append(f'step {step}: padding rows of the classification predictor are not 0 in {what}')


@pytest.mark.parametrize('leg', LEGS)
def test_bucket_update_vs_host_reference(leg):
    """Three unclipped steps (lr changed once, as a warm-up hook does: the bias-lr ratio path of step()): after each, with the
    gradients captured behind backward() + synchronize, weights / momentum / train16 against the float64 host update and the
    data-gradient packs against a fresh repack on the caller's stream.  Then the same three steps with no synchronization
    anywhere - where a missing stream edge shows - must end with the same bits."""
    from dsl_amd import _lib as L
    batch = None
    finals = []
    for capture in (True, False):
        model, opt, C = _single(leg)
        if batch is None:
            batch = make_batch(0, C)
        if not capture:
            _no_host_sync(model)
        ref = None
        for s in range(len(LR_SCALE)):
            _set_lr(opt, s)
            out = model.train_step(batch, opt)
            out['loss'].backward()
            if leg == 'proxy_late':
                assert model.late_exchange and len(model.exchange.todo) == 4, (model.late_exchange, len(model.exchange.todo))
            if not capture:
                opt.step()
                continue
            torch.cuda.synchronize()
            p0, g, m0, _ = _snapshot(model, opt)
            opt.step()
            torch.cuda.synchronize()
            p1, _, m1, t16 = _snapshot(model, opt)
            if ref is None:
                ref = HostRef(model, opt)
            errs = ref.check(opt.param_groups[0]['lr'], s == 0, p0, g, m0, p1, m1, t16)
            if leg == 'c20':
                _check_padding_rows(model, opt, C, errs, s)
            # the data-gradient packs were built from the updated weights: a repack now gives the same bits
            st = model.store
            packs = st.wT16.clone()
            st.repack_dgrad(L.stream_ptr(), side=False)
            torch.cuda.synchronize()
            if not torch.equal(_bits(packs), _bits(st.wT16)):
                errs.append(f'wT16 differs from a fresh repack_dgrad on {int((_bits(packs) != _bits(st.wT16)).sum())} elements')
            assert not errs, f'{leg} step {s}: ' + '; '.join(errs)
        # the per-bucket path was taken (the whole-buffer path sets neither stream)
        assert getattr(opt, '_side1' if leg == 'defer_head' else '_opt_stream', None) is not None
        torch.cuda.synchronize()
        finals.append(tuple(t.cpu().clone() for t in (model.store.train, opt.momentum_buf, model.store.train16)))
        del model, opt
    for what, a, b in zip(('train', 'momentum', 'train16'), finals[0], finals[1]):
        assert torch.equal(_bits(a), _bits(b)), f'{leg}: {what} of the unsynchronized run differs on {int((_bits(a) != _bits(b)).sum())} elements'


def test_optimizer_state_dict_waits_for_late_updates():
    """FlatSGD.state_dict() right behind step() on the late path (one GPU, proxy exchange): the updates may still run on the
    optimizer's stream, so state_dict() waits for them - a copy of the momentum taken on the caller's stream right away equals
    the momentum read after a synchronize.  (The caller's stream is drained in front of the last step, so that the copy would
    start at once, while that step's exchanges and updates still run.)"""
    model, opt, C = _single('proxy_late')
    batch = make_batch(0, C)
    _no_host_sync(model)
    for s in range(2):
        out = model.train_step(batch, opt)
        out['loss'].backward()
        if s == 1:
            torch.cuda.current_stream().synchronize()
        opt.step()
    sd = opt.state_dict()
    snap = sd['momentum'].clone()
    torch.cuda.synchronize()
    assert sd['momentum'] is opt.momentum_buf
    assert torch.equal(_bits(snap), _bits(opt.momentum_buf))


# ---- 2. two ranks (one GPU each, or both on one GPU with gloo): the late exchange with real collectives ----------------------------
def _ddp(late, comm, grad_dtype):
    from dsl_amd.optim import FlatSGD
    from dsl_amd.parallel import HipDistributedDataParallel
    model = build()
    ddp = HipDistributedDataParallel(model, comm=comm, grad_dtype=grad_dtype)
    opt = FlatSGD(model, **OPT) if late else FlatSGD(model, late_exchange=False, **OPT)
    _no_host_sync(model)
    return model, ddp, opt


def _gather(t):
    lst = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(lst, t)
    return lst


def _ranks_agree(tensors, errs, where):
    for what, t in tensors:
        a, b = _gather(_bits(t).view(torch.int32))
        if not torch.equal(a, b):
            errs.append(f'{where}: {what} differs between the ranks on {int((a != b).sum())} words')


def _schedules(rank, comm, grad_dtype):
    """Three steps each: late exchange checked against the host (rank 0), the eager schedule, and the late one with a gradient
    reader (wait_grads) between backward and step."""
    errs = []
    batch = make_batch(rank)
    finals = {}
    for name in ('late', 'eager', 'late_wait_grads'):
        late = name != 'eager'
        model, ddp, opt = _ddp(late, comm, grad_dtype)
        st = model.store
        ref, losses = None, []
        for s in range(len(LR_SCALE)):
            _set_lr(opt, s)
            out = ddp.train_step(batch, opt)
            out['loss'].backward()
            todo, pend = len(model.exchange.todo), len(model.exchange.pending)
            if late and not (model.late_exchange and todo == 4 and pend == 0):
                errs.append(f'{name} step {s}: not the late path (late_exchange {model.late_exchange}, {todo} buckets left, {pend} queued)')
            if not late and (model.late_exchange or todo or pend != 4):
                errs.append(f'{name} step {s}: not the eager path (late_exchange {model.late_exchange}, {todo} left, {pend} queued)')
            if name == 'late':
                # nothing has been exchanged yet: what store.grad holds now is this rank's local gradient
                torch.cuda.synchronize()
                p0, local, m0, _ = _snapshot(model, opt)
                locs = _gather(local)
            if name == 'late_wait_grads':
                model.wait_grads()
            opt.step()
            torch.cuda.synchronize()
            p1, g, m1, t16 = _snapshot(model, opt)
            losses.append({k: float(v) for k, v in out['log_vars'].items()})
            _ranks_agree((('train', p1), ('momentum', m1), ('train16', t16)), errs, f'{name} step {s}')
            if name == 'late':
                if grad_dtype == 'bf16':          # the gloo carrier: bf16 copies added in fp32, rounded back (detectors.exchange)
                    want = (locs[0].bfloat16().float() + locs[1].bfloat16().float()).bfloat16().float()
                else:
                    want = locs[0] + locs[1]
                if not torch.equal(_bits(g), _bits(want)):
                    errs.append(f'late step {s}: store.grad != the sum of the local gradients on {int((_bits(g) != _bits(want)).sum())} elements')
                if rank == 0:
                    if ref is None:
                        ref = HostRef(model, opt)
                    errs += [f'late step {s}: {e}' for e in ref.check(opt.param_groups[0]['lr'], s == 0, p0, want, m0, p1, m1, t16)]
        finals[name] = (p1, m1, t16, losses)
        del model, ddp, opt, st
    for other in ('eager', 'late_wait_grads'):
        for i, what in enumerate(('train', 'momentum', 'train16')):
            a, b = finals['late'][i], finals[other][i]
            if not torch.equal(_bits(a), _bits(b)):
                errs.append(f'{what} after 3 steps: late != {other} on {int((_bits(a) != _bits(b)).sum())} elements')
        if finals['late'][3] != finals[other][3]:
            errs.append(f'logged losses: late {finals["late"][3]} != {other} {finals[other][3]}')
    return errs


def _second_backward(rank, comm):
    """backward(A) -> backward(B) -> step() ends with the bits of backward(B) -> step(), in both schedules."""
    errs = []
    batch, batch_a = make_batch(rank), make_batch(rank, flip=True)
    for late in (True, False):
        res = []
        for twice in (False, True):
            model, ddp, opt = _ddp(late, comm, 'fp32')
            if twice:
                out = ddp.train_step(batch_a, opt)
                out['loss'].backward()
            out = ddp.train_step(batch, opt)
            out['loss'].backward()
            opt.step()
            torch.cuda.synchronize()
            p1, g, m1, t16 = _snapshot(model, opt)
            res.append((p1, g, m1, t16, float(out['log_vars']['loss'])))
            _ranks_agree((('train', p1), ('grad', g)), errs, f'late={late} twice={twice}')
            del model, ddp, opt
        for i, what in enumerate(('train', 'grad', 'momentum', 'train16')):
            a, b = res[0][i], res[1][i]
            if not torch.equal(_bits(a), _bits(b)):
                errs.append(f'late={late}: {what} after backward(A), backward(B), step differs from backward(B), step '
                            f'on {int((_bits(a) != _bits(b)).sum())} elements')
        if res[0][4] != res[1][4]:
            errs.append(f'late={late}: loss {res[1][4]} != {res[0][4]}')
    return errs


def _rank_worker(rank, world, port, q, mode, grad_dtype, comm, one_gpu_per_rank):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(rank if one_gpu_per_rank else 0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        errs = _schedules(rank, comm, grad_dtype) if mode == 'schedules' else _second_backward(rank, comm)
        dist.destroy_process_group()
        q.put((rank, '; '.join(errs) if errs else 'ok'))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def _two_ranks(mode, grad_dtype='fp32', comm='torch', one_gpu_per_rank=False, timeout=600):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, mode, grad_dtype, comm, one_gpu_per_rank)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            try:
                # (once a rank has failed the other may wait in a collective forever: do not wait long for it)
                r = q.get(timeout=timeout if all(v == 'ok' for v in res.values()) else 30)
            except queue.Empty:
                break
            res[r[0]] = r[1]
    finally:
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
    assert len(res) == 2 and all(v == 'ok' for v in res.values()), \
        '\n'.join(f'rank {r}: {res.get(r, "no result")}' for r in range(2))


@pytest.mark.parametrize('grad_dtype', ['fp32', 'bf16'])
def test_late_exchange_two_ranks_vs_host_reference(grad_dtype):
    """HipDistributedDataParallel + FlatSGD with the defaults (late exchange) on two ranks sharing the GPU, gloo collectives.  Per
    step: the local gradients (nothing is exchanged behind backward()) summed on the host equal what store.grad holds after step()
    bit for bit (bf16: the bf16 copies added in fp32 and rounded back, as the gloo carrier does), the weights match the float64
    update of that sum, and train / momentum / train16 are identical on the ranks.  After three steps the eager schedule
    (late_exchange=False) and a late run with wait_grads() between backward and step (a gradient reader) end with the same bits
    and the same logged losses."""
    _two_ranks('schedules', grad_dtype=grad_dtype)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL needs one GPU per rank: this box has fewer than 2')
def test_late_exchange_two_ranks_vs_host_reference_rccl():
    """The same with the exchanges carried by the C-ABI's rcclComm_t (comm='rccl'), one GPU per rank."""
    _two_ranks('schedules', comm='rccl', one_gpu_per_rank=True)


def test_second_backward_before_step_two_ranks():
    """A second training pass before step() first finishes the previous pass's exchanges (late: queues them; eager: waits for
    them), so that no collective is dropped or still writing store.grad when the new pass writes it - the loss kernel writes the
    scale gradients there, the weight gradients the rest: backward(A) -> backward(B) -> step() gives the bits of backward(B) ->
    step() in both schedules."""
    _two_ranks('second_backward')

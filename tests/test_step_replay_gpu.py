"""Every launch of the shipped full-size step against float64 math (tests/op_ref.py), one launch at a time.

OpList.run is replaced by a replay that hands the library one op at a time (a one-element dsl_op array through dsl_run_ops, the device
drained around it) and skips the ordering ops (FORK, JOIN, RECORD, WAIT, PROF).  Before each checked launch its real inputs are read
from device memory and its outputs recomputed in float64 from the descriptor; after it every output element must be within
|got - ref| <= 2^-8 |ref| (bf16 only) + beta S, and no other byte of the outputs' allocations may have changed.  Because each launch
gets the inputs the previous launches really produced, bf16 noise cannot build up along the step: the bars are one launch's rounding,
at the tiles, split factors, weight-gradient tables and schedules that ship.  Per leg also: the weight packs each launch reads equal
the current fp32 weights, every gradient element was written by a checked launch, the normal concurrent run gives the replay's bits,
and negative controls on the captured operands are flagged.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

import op_ref as R
from util import fcos_model_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy

# Kinds that run unchecked here, each covered elsewhere.
EXEMPT = {
    R.OP_RLA: 'test_rla_gpu.py',
    R.OP_PACK_DGRAD: 'the pack-integrity check of this file',
}
ORDERING = {R.OP_FORK, R.OP_JOIN, R.OP_RECORD, R.OP_WAIT, R.OP_PROF}


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def build_model(rla=False, fp8=False, **head):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    cfg = fcos_model_cfg(**head)
    if rla:
        from oracle import rla_oracle as RO
        cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
        sd = RO.synth_state_dict(0)
    else:
        from oracle import fcos_oracle as O
        sd = O.synth_state_dict(0, num_classes=head.get('num_classes', 80))
    if fp8:
        cfg['fp8'] = dict(layers='towers')
    model = build_detector(cfg)
    model.load_state_dict(sd)
    return model.cuda()


class Replay:
    """The per-launch checker of one leg: statistics per kind, gradient coverage, pack checks, negative controls."""

    def __init__(self, model, opt=None):
        self.model, self.opt = model, opt
        self.stats = {}             # kind name -> [launches, worst ratio]
        self.failures = []
        self.controls = {}          # control name -> [flagged?, ...]
        self.covered = None
        self.pack_checks = 0
        self.per_out = {}           # LOSS output -> worst ratio (losses, g_scales, g_cls, g_rc, logvec)
        self.skipped = []           # controls that could not apply to this step's operands (printed)
        self.active = False

    def roots(self):
        from dsl_amd import ops
        eng = self.model._get_engine()
        return {'engine': eng, 'plans': list(eng.plans.values()), 'store': self.model.store, 'opt': self.opt,
                'pixtabs': ops._pixtabs, 'model': self.model}

    # -- (b) the weight packs a launch reads ------------------------------------------------------------------------------
    def check_weights(self, mem, d, name):
        st = self.model.store
        a16 = mem.find(st.train16.data_ptr(), 0, 'train16')[0]
        ptr = int(d.wgt or 0)
        if not ptr or d.flags & R.CONV_FP8:
            return
        K = d.kh * d.kw * d.cs
        if a16.start <= ptr < a16.start + a16.nbytes:
            off = (ptr - st.train16.data_ptr()) // 2
            got = st.train16[off:off + d.cd * K]
            want = st.train[off:off + d.cd * K].bfloat16()
            if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
                self.failures.append((name, 'train16 != bf16(train) in the weights it reads'))
            self.pack_checks += 1
            return
        if st.wT16 is not None and st.wT16.data_ptr() <= ptr < st.wT16.data_ptr() + st.wT16.numel() * 2:
            lay, _ = st.wT_layout()
            off = (ptr - st.wT16.data_ptr()) // 2
            # the rows it reads (cd input channels x kh kw cs): a whole pack, or a row range of one (an input-channel slice)
            hit = [(k, o) for k, (o, n) in lay.items() if o <= off and off + d.cd * K <= o + n]
            if not hit:
                self.failures.append((name, f'wgt reads wT16 [{off}, {off + d.cd * K}): not inside one pack'))
                return
            k, o = hit[0]
            got, want = st.wT16[off:off + d.cd * K], rebuild_pack(st, k)[off - o:off - o + d.cd * K]
            if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
                self.failures.append((name, f'dgrad pack {k} != the pack of the current fp32 weights '
                                            f'({int((got != want).sum())} elements differ)'))
            self.pack_checks += 1

    # -- one launch ---------------------------------------------------------------------------------------------------------
    def launch(self, mem, idx, op, stream, multis):
        from dsl_amd import _lib as L
        one = (L.Op * 1)()
        C.memmove(C.addressof(one[0]), C.addressof(op), C.sizeof(L.Op))

        def go():
            # drained on both sides: an op with i[6] > 0 runs on a side stream of the library, which does not wait for the reference's
            # reads queued on torch's stream (an in-place addend would be read after the launch has overwritten it)
            torch.cuda.synchronize()
            L.check(L.lib.dsl_run_ops(one, 1, stream), 'dsl_run_ops(replay)')
            torch.cuda.synchronize()

        kind = op.kind
        if kind not in R.CHECKED:
            if kind not in EXEMPT:
                self.failures.append((f'op {idx}', f'kind {R.KIND_NAMES.get(kind, kind)} is neither checked nor exempt'))
            go()
            return
        nm = f'{R.KIND_NAMES[kind]}#{idx}'
        if kind == R.OP_CONV:
            d = C.cast(op.desc, C.POINTER(L.ConvDesc)).contents
            self.check_weights(mem, d, nm)
            if d.mode == 1:
                nm += '(mode1)'
            if d.flags & R.CONV_FP8:
                nm += '(fp8)'
        lr = R.op_ref(mem, op, multis, nm)
        res = R.run_checked(mem, lr, go)
        key = R.KIND_NAMES[kind] + ('.mode1' if '(mode1)' in nm else '') + ('.fp8' if '(fp8)' in nm else '')
        if kind == R.OP_FP8_PREP and lr.extra.get('cold'):
            self.stats.setdefault('FP8_PREP.cold', [0, 0.0])[0] += 1          # scale 1: nothing recorded yet
        if kind == R.OP_LOSS:
            d = C.cast(op.desc, C.POINTER(L.FcosDesc)).contents
            key += f'.C{d.num_classes}' + ('.sisoft' if d.soft_weight != 0 and d.n % 2 == 1 and d.n >= 3 else '')
            for oname, ratio, _, _ in res:
                k_ = oname.split('.')[-1]
                self.per_out[k_] = max(self.per_out.get(k_, 0.0), ratio)
        s = self.stats.setdefault(key, [0, 0.0])
        s[0] += 1
        for oname, ratio, nbad, worst in res:
            s[1] = max(s[1], ratio)
            if nbad:
                self.failures.append((oname, f'{nbad} elements over the bar, worst |err|/bound {ratio:.3g} at flat index {worst}',
                                      _describe(op, lr, oname, worst, mem)))
        self.cover(mem, lr)
        self.negative_controls(mem, op, lr, nm, multis)

    def cover(self, mem, lr):
        st = self.model.store
        g0 = st.grad.data_ptr()
        for o in lr.outs:
            if o.dtype == torch.float32 and g0 <= o.ptr < g0 + st.n_train * 4:
                self.covered[(o.ptr - g0) // 4 + o.idx.reshape(-1)] = True

    # -- (e) negative controls on the captured operands: references only, never a modified launch -----------------------------
    def negative_controls(self, mem, op, lr, nm, multis):
        from dsl_amd import _lib as L
        kind = op.kind
        if kind == R.OP_WGRAD_MULTI:
            m = multis[op.p[0]]
            descs = [m.descs[g] for g in range(len(m.descs))]
            big = max(range(len(descs)), key=lambda g: _wgrad_work(descs[g]))
            self._control(mem, lr, descs, big, dict(drop_img=1), f'WGRAD_MULTI image 1 dropped ({nm}[{big}])', work=_wgrad_work(descs[big]))
        elif kind == R.OP_WGRAD_GROUP and op.i[0] == 8:          # the towers' group (4 + 4 tower layers)
            arr = C.cast(op.desc, C.POINTER(L.WgradDesc))
            descs = [arr[g] for g in range(op.i[0])]
            self._control(mem, lr, descs, 0, dict(drop_img=1), 'tower WGRAD_GROUP image 1 dropped')
            d = descs[0]
            mid = d.gh[0] * d.gw[0] // 2 // 32 * 32
            self._control(mem, lr, descs, 0, dict(drop_stage=(mid, 32)), 'tower WGRAD_GROUP one 32-pixel stage dropped')
        elif kind == R.OP_LOSS:
            d = C.cast(op.desc, C.POINTER(L.FcosDesc)).contents
            if d.soft_weight != 0 and d.n % 2 == 1 and d.n >= 3:
                self._ref_control(mem, lr, R.loss_ref(mem, d, 'control', partner_level=0), 0, 'LOSS sisoft partner from level lvl')
            bad = R.loss_ref(mem, d, 'control', relu_mask=False)
            if torch.equal(bad.outs[1].ref, lr.outs[1].ref):
                # no positive has raw x scale <= 0 in this step: the control cannot tell (test_fcos_loss_gpu.py forces one and flags it)
                self.skipped.append('LOSS ReLU mask dropped from g_rc (no positive with raw x scale <= 0)')
            else:
                self._ref_control(mem, lr, bad, 1, 'LOSS ReLU mask dropped from g_rc')
        elif kind == R.OP_ASSIGN:
            d = C.cast(op.desc, C.POINTER(L.FcosDesc)).contents
            self._ref_control(mem, lr, R.assign_ref(mem, d, 'control', radius=1.0), 0, 'ASSIGN radius 1.0')
        elif kind == R.OP_QUANT_FP8_DELAYED:
            bad = R.quant_fp8_delayed_ref(mem, op.p[0], op.p[1], op.p[2], op.p[3], op.l[0], op.i[0], op.i[1], op.i[2], 'control',
                                          scale_mul=2.0)
            self._ref_control(mem, lr, bad, 0, 'QUANT_FP8_DELAYED scale doubled')
        elif kind == R.OP_CONV and '(mode1)' in nm and 'dgrad border tap' not in self.controls:
            d = C.cast(op.desc, C.POINTER(L.ConvDesc)).contents
            if d.kh == 3 and d.pad == 1:
                bad = R.conv_ref(mem, d, nm, drop=lambda s, t, g: (t == 0) & (g['y'] == 0))
                o, ob = lr.outs[0], bad.outs[0]
                self.controls['dgrad border tap'] = [R.compare(o.got(mem), ob.ref, o.bound())[1] > 0]

    def _ref_control(self, mem, lr, bad, k, name):
        """Output k of the launch against a perturbed reference `bad` of the same captured operands, under the launch's own bar."""
        o = lr.outs[k]
        self.controls[name] = self.controls.get(name, []) + [R.compare(o.got(mem), bad.outs[k].ref, o.bound())[1] > 0]

    def _control(self, mem, lr, descs, k, drop, name, work=0):
        bad = R.wgrad_ref(mem, descs, 'control', drop={k: drop})
        dw_ptr = int(descs[k].dw)
        good = [o for o in lr.outs if o.ptr == dw_ptr and o.name.endswith('.dw')][0]
        ob = [o for o in bad.outs if o.ptr == dw_ptr and o.name.endswith('.dw')][0]
        flagged = R.compare(good.got(mem), ob.ref, good.bound())[1] > 0
        prev = self.controls.get(name)
        if name.startswith('WGRAD_MULTI'):            # keep the largest member seen over all multi launches
            key = 'WGRAD_MULTI image 1 dropped (largest member)'
            if key not in self.controls or work > self.controls[key][1]:
                self.controls[key] = [flagged, work, name]
            return
        self.controls[name] = (prev or []) + [flagged]

    # -- the replayed OpList.run ---------------------------------------------------------------------------------------------
    def install(self, monkeypatch):
        from dsl_amd import _lib as L
        from dsl_amd import engine, ops
        orig = engine.OpList.run
        rp = self

        def run(self_):
            if not rp.active:
                return orig(self_)
            if not self_.items:
                return
            if self_.arr is None:
                self_.arr = (L.Op * len(self_.items))(*self_.items)
            multis = {m.host.data_ptr(): m for m in self_.keep if isinstance(m, ops.WgradMulti)}
            stream = L.stream_ptr()
            torch.cuda.synchronize()
            mem = R.Memory(rp.roots())          # (no allocation is made or freed while a list runs)
            for k in range(len(self_.arr)):
                op = self_.arr[k]
                if op.kind in ORDERING:
                    continue
                rp.launch(mem, k, op, stream, multis)

        monkeypatch.setattr(engine.OpList, 'run', run)

    def begin(self):
        torch.cuda.synchronize()
        self.covered = torch.zeros(self.model.store.n_train, dtype=torch.bool, device='cuda')
        self.active = True

    def end(self):
        torch.cuda.synchronize()
        self.active = False


def _describe(op, lr, oname, worst, mem):
    """The descriptor fields and the worst element of a failed output (for the report)."""
    from dsl_amd import _lib as L
    txt = ''
    if op.kind == R.OP_CONV:
        d = C.cast(op.desc, C.POINTER(L.ConvDesc)).contents
        txt = ' '.join(f'{f}={list(getattr(d, f))[:d.nseg] if f in ("gh", "gw", "sh", "sw", "dh", "dw", "ah", "aw") else getattr(d, f)}'
                       for f, _ in d._fields_ if f not in ('src', 'wgt', 'dst', 'scale', 'bias', 'addend', 'mask', 'workspace',
                                                           'gn_ws', 'gn_x', 'gn_gamma', 'gn_beta', 'gn_stats'))
        txt += f' addend={bool(d.addend)} mask={bool(d.mask)} gn_ws={bool(d.gn_ws)} gn_x={bool(d.gn_x)}'
    o = [o for o in lr.outs if o.name == oname]
    if o:
        o = o[0]
        got = o.got(mem).reshape(-1)
        txt += f' | worst: got {float(got[worst]):.6g} ref {float(o.ref.reshape(-1)[worst]):.6g} S {float(o.S.reshape(-1)[worst]):.6g}'
        if o.idx.dim() == 2:
            txt += f' row {worst // o.idx.shape[1]} col {worst % o.idx.shape[1]} of {tuple(o.idx.shape)}'
    return txt


def _wgrad_work(d):
    return sum(d.n * d.gh[s] * d.gw[s] for s in range(d.nseg)) * d.cd * d.cs * d.kh * d.kw


def rebuild_pack(st, name):
    """The dgrad pack `name` from the current fp32 weights (params.ParamStore.repack_dgrad, csrc/optim.hip pack_dgrad_batched_kernel):
    out[ci][t][co] = bf16(w[co][t][ci] * scale[co]) - one fp32 product, one round to nearest even - zero for co >= cout, taps selected
    for RLA's parity-class packs.  No tap flip: the mode-1 gather reads tap (r, s) at ((y + pad - r) / stride, ...)."""
    from dsl_amd.ops import s2_class
    if name == 'head.cls':
        w, co, cop, cin, sc = st.tview('head.cls_w'), st.num_classes, st.cls_pad, 256, None
    elif name == 'head.regctr':
        w, co, cop, cin, sc = st.tview('head.regctr_w'), 5, 64, 256, None
    else:
        s = st.convs[name.split('#')[0]]
        w, co, cop, cin = st.tview(s.name + '.weight'), s.cout, s.cout_pad, s.cin_store
        sc = st.bn_scale[st.bn_off[s.bn]:st.bn_off[s.bn] + s.cout] if s.bn else None
    w = w.reshape(w.shape[0], -1, cin)[:co].float()
    if sc is not None:
        w = w * sc.view(-1, 1, 1)
    if '#s2' in name:
        _, _, taps = s2_class(int(name[-2]), int(name[-1]))
        w = torch.stack([w[:, t] if t >= 0 else torch.zeros_like(w[:, 0]) for t in taps], 1)
    out = torch.zeros(cin, w.shape[1], cop, dtype=torch.bfloat16, device=w.device)
    out[:, :, :co] = w.permute(2, 1, 0).bfloat16()
    return out.reshape(-1)


def check_bn_fold(st):
    """bn_scale / bn_bias against gamma / sqrt(var + eps), beta - mean * scale in float64 (fp32 arithmetic: within 2^-21 relative)."""
    bad = []
    for name, off in st.bn_off.items():
        if name in dict(getattr(st, 'bn_train_off', {})):
            o, c = st.bn_train_off[name]
            g, b = st.tview('bn_train.weight')[o:o + c], st.tview('bn_train.bias')[o:o + c]
            m, v = st.fview('bn_train.running_mean')[o:o + c], st.fview('bn_train.running_var')[o:o + c]
        else:
            g, b = st.fview(name + '.weight'), st.fview(name + '.bias')
            m, v = st.fview(name + '.running_mean'), st.fview(name + '.running_var')
            c = g.numel()
        sc = g.double() / torch.sqrt(v.double() + 1e-5)
        bi = b.double() - m.double() * sc
        got_s, got_b = st.bn_scale[off:off + c].double(), st.bn_bias[off:off + c].double()
        if not torch.allclose(got_s, sc, rtol=2 ** -21, atol=0) or not torch.allclose(got_b, bi, rtol=2 ** -21, atol=2 ** -21 * float(
                (m.double() * sc).abs().max())):
            bad.append(name)
    return bad


# ------------------------------------------------------------------------------------------------------------------------------
# the legs
def _sup_batch():
    return _bench().synth_batch(0, 2)


def _dsl_batch(num_classes=80):
    from oracle import fcos_oracle as O
    bench = _bench()
    b = bench.synth_batch(0, 2)
    b['gt_labels'] = [l % num_classes for l in b['gt_labels']]
    rng = np.random.RandomState(77)
    ig0 = [torch.zeros(0, 4), T(bench.synth_boxes(rng, 3))]
    img, gtb, gtl, ig = O.append_half_scale(b['img'].cpu(), b['gt_bboxes'], b['gt_labels'], ig0)
    metas = [dict(img_shape=(800, 1333, 3), pad_shape=(800, 1344, 3), scale_factor=1.0)] * 3
    return img.cuda(), metas, gtb, gtl, ig


def _fwd_bwd(model, img, metas, gtb, gtl, ig=None):
    losses = model.forward_train(img, metas, gtb, gtl, ig)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return torch.stack([v.detach().float().reshape(()) for v in losses.values()]).cpu()


LEGS = ['sup', 'dsl_n3', 'defer_sgd', 'rla_dsl_n3', 'fp8_704x1088', 'inference', 'dsl_n3_c3']


def _leg(name, replay_on, monkeypatch):
    """Runs leg `name` with the replay on or off; returns (model, replay, results for the concurrent-vs-serial comparison)."""
    from dsl_amd import tuning
    tuning.tune('side')
    if name in ('dsl_n3', 'rla_dsl_n3', 'dsl_n3_c3'):
        monkeypatch.setitem(tuning._values, 'tower_slots', '128')
    head = dict(loss_weight=3.0, soft_weight=1.0, soft_warm_up=0) if 'dsl' in name else {}
    if name == 'dsl_n3_c3':                 # the tail loss instantiation (C % 4 != 0) with sisoft, and the cd = 3 predictor
        head['num_classes'] = 3
    model = build_model(rla=name.startswith('rla'), fp8=name.startswith('fp8'), **head)
    if 'dsl' in name:
        model.bbox_head.cur_iter = 1
    opt = None
    if name == 'defer_sgd':
        from dsl_amd.optim import FlatSGD
        opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.),
                      defer_head_update=True)
    rp = Replay(model, opt)
    if replay_on:
        rp.install(monkeypatch)
    out = {}
    if name in ('sup', 'dsl_n3', 'rla_dsl_n3', 'fp8_704x1088', 'dsl_n3_c3'):
        if name == 'sup':
            b = _sup_batch()
            args = (b['img'], b['img_metas'], b['gt_bboxes'], b['gt_labels'], None)
        elif name == 'fp8_704x1088':
            bench = _bench()
            b = bench.synth_batch(0, 2, H=704, W=1088)
            args = (b['img'], b['img_metas'], b['gt_bboxes'], b['gt_labels'], None)
        else:
            args = _dsl_batch(3 if name == 'dsl_n3_c3' else 80)
        rp.begin()
        out['losses'] = _fwd_bwd(model, *args)
        rp.end()
        out['grad'] = model.store.grad[:model.store.n_train].clone()
    elif name == 'defer_sgd':
        b = _sup_batch()
        b2 = dict(b, img=(b['img'] * 0.9).bfloat16().float())
        o1 = model.train_step(b, opt)
        o1['loss'].backward()
        opt.step()
        rp.begin()
        o2 = model.train_step(b2, opt)
        o2['loss'].backward()
        opt.step()
        rp.end()
        torch.cuda.synchronize()
        out['losses'] = o2['loss'].detach().float().reshape(1).cpu()
        out['grad'] = model.store.grad[:model.store.n_train].clone()
        out['train'] = model.store.train.clone()
        out['mom'] = opt.momentum_buf.clone()
    else:                                                   # inference plan, as sweep.simple_test runs it
        from dsl_amd import sweep
        b = _sup_batch()
        model.eval()
        rp.begin()
        dets, labels, count = sweep.detect_device(model, b['img'], b['img_metas'])
        rp.end()
        out['dets'], out['count'] = dets.clone(), count.clone()
    return model, rp, out


@pytest.mark.parametrize('leg', LEGS)
def test_every_launch_of_the_full_size_step_vs_fp64(monkeypatch, leg):
    t0 = time.time()
    # (d) the normal concurrent run of the same step from the same state and batch
    model, _, conc = _leg(leg, False, monkeypatch)
    del model
    torch.cuda.synchronize()
    model, rp, ser = _leg(leg, True, monkeypatch)
    wall = time.time() - t0
    print(f'\n[{leg}] wall {wall:.1f} s, pack checks {rp.pack_checks}')
    for k in sorted(rp.stats):
        print(f'  {k:18s} launches {rp.stats[k][0]:4d}  worst |err|/bound {rp.stats[k][1]:.3f}')
    for k, v in sorted(rp.per_out.items()):
        print(f'  LOSS.{k:13s} worst |err|/bound {v:.3f}')
    for k, v in rp.controls.items():
        print(f'  control {k}: flagged {v[0] if k.startswith("WGRAD_MULTI") else v}')
    for k in sorted(set(rp.skipped)):
        print(f'  control {k}: skipped')
    # (a) every checked launch within its bar (and nothing unchecked slipped in)
    assert not rp.failures, rp.failures[:10]
    assert rp.stats, 'no launch was checked'
    for k in ('CONV', 'GN_FWD'):
        assert rp.stats.get(k, [0])[0] > 0, (k, rp.stats)
    if leg != 'inference':
        for k in ('CONV.mode1', 'GN_BWD', 'WGRAD_MULTI', 'SUM2X2'):
            assert rp.stats.get(k, [0])[0] > 0, (k, sorted(rp.stats))
        for k in ('ASSIGN', 'LOSS'):
            assert sum(v[0] for n, v in rp.stats.items() if n.split('.')[0] == k) > 0, (k, sorted(rp.stats))
    if leg == 'dsl_n3_c3':
        assert rp.stats.get('LOSS.C3.sisoft', [0])[0] > 0, sorted(rp.stats)
    if leg == 'dsl_n3':
        assert rp.stats.get('LOSS.C80.sisoft', [0])[0] > 0, sorted(rp.stats)
    if leg == 'fp8_704x1088':
        assert rp.stats.get('CONV.fp8', [0])[0] > 0, sorted(rp.stats)
        # the kinds the engine emits (its delayed scaling: one weight / scale preparation per step, the FPN outputs' quantiser)
        for k in ('FP8_PREP', 'FP8_PREP.cold', 'QUANT_FP8_DELAYED'):
            assert rp.stats.get(k, [0])[0] > 0, (k, sorted(rp.stats))
    # (b) packs and casts: checked at every consumer above; the BatchNorm fold
    assert rp.pack_checks > 0
    assert not check_bn_fold(model.store), check_bn_fold(model.store)
    # (c) gradient coverage
    st = model.store
    if leg != 'inference':
        unc = ~rp.covered
        exempt = torch.zeros_like(unc)
        for rname, (off, n, shape) in st.train_regions.items():
            if rname.startswith('bn_train.'):                                   # written by OP_RLA (exempt above)
                exempt[off:off + n] = True
            elif rname == 'head.scales':                                          # 5 levels in a region of 8: never written
                assert not bool(st.grad[off + 5:off + n].any()), rname
                exempt[off + 5:off + n] = True
            elif rname in ('head.cls_w', 'head.cls_b', 'head.regctr_w', 'head.regctr_b'):       # predictor padding rows: never written
                used = (st.num_classes if 'cls' in rname else 5) * (n // shape[0])
                pad = slice(off + used, off + n)
                assert not bool(st.grad[pad].any()), rname
                exempt[pad] = True
        left = (unc & ~exempt).nonzero().view(-1)
        if left.numel():
            names = sorted({r for r, (o, n, _) in st.train_regions.items() for i in left[:2000].tolist() if o <= i < o + n})
            raise AssertionError(f'{left.numel()} gradient elements written by no checked launch: {names[:10]}')
    # (d) concurrent == serialized replay, bit for bit
    for k in conc:
        assert torch.equal(conc[k].cpu(), ser[k].cpu()), (leg, k)
    # (e) negative controls flagged
    if leg != 'inference':
        assert rp.controls, 'no negative control ran'
        for k, v in rp.controls.items():
            assert (v[0] if k.startswith('WGRAD_MULTI') else all(v)), (k, v)
        if leg == 'sup':
            assert 'tower WGRAD_GROUP image 1 dropped' in rp.controls and 'dgrad border tap' in rp.controls
        assert 'ASSIGN radius 1.0' in rp.controls
        if 'dsl' in leg:
            assert 'LOSS sisoft partner from level lvl' in rp.controls
        if leg == 'fp8_704x1088':
            assert 'QUANT_FP8_DELAYED scale doubled' in rp.controls

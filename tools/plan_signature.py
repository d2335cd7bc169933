"""Op-list signature of the step plans: one line per op of every list a plan runs, in execution order, with every field of the
descriptor the op points to.  Two commits whose outputs agree build the same lists - same ops, order, streams, descriptors - so a
refactor of dsl_amd/engine.py / engine_rla.py is checked by running this file on both and diffing:

    python tools/plan_signature.py --out sig.txt            (needs the GPU: a plan allocates its buffers; seconds per leg)

Pointers are printed as A<k>+<offset>(<allocation bytes>): k numbers the distinct allocations in order of first appearance in the
leg's walk (tests/op_ref.Memory maps a pointer to its allocation), H = a non-null pointer into no tensor (host structures).
For eight legs three optimizer steps on the tests/golden/net_tiny.npz batch follow, and the sha256 of the trained weights.
Nothing is launched beyond what building a model and a plan launches (and those steps).
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from dsl_amd import _lib as L  # noqa: E402
from dsl_amd import detectors, ops, params, tuning  # noqa: E402,F401
from dsl_amd.optim import FlatSGD  # noqa: E402
from dsl_amd.registry import build_detector  # noqa: E402
import op_ref as R  # noqa: E402
from util import fcos_model_cfg  # noqa: E402


def tracked_l1(plan):
    """The descriptors a plan re-points at layer1's output buffer of the step, as [(descriptor, field, byte offset)].  The one
    place that knows how Plan stores them: its registry list, or the dict `_pp` of the builds before the registry."""
    reg = getattr(plan, '_l1_tracked', None)
    if reg is not None:
        return list(reg)
    pp = getattr(plan, '_pp', None) or {}
    out = [(pp['c3'], 'dst', 0)] if 'c3' in pp else []
    for key in ('c1', 'ds'):
        out += [(d, 'x' if isinstance(d, L.BneckDesc) else 'src', off) for d, off in pp.get(key, [])]
    return out + [(pp[key], 'x', 0) for key in ('wg_c1', 'wg_ds') if key in pp]


KINDS = {getattr(L, n): n[3:] for n in dir(L) if n.startswith('OP_')}
RLA_KINDS = {getattr(L, n): n[4:] for n in dir(L) if n.startswith('RLA_') and isinstance(getattr(L, n), int)}
DESC_OF = {L.OP_CONV: L.ConvDesc, L.OP_WGRAD: L.WgradDesc, L.OP_GN_FWD: L.GnDesc, L.OP_GN_BWD: L.GnDesc, L.OP_BNECK: L.BneckDesc,
           L.OP_RLA: L.RlaDesc, L.OP_GFL_QUALITY: L.GflDesc, L.OP_PAA_REFINE: L.PaaDesc}


class Names:
    """Pointer -> 'A<k>+<offset>(<bytes>)'."""

    def __init__(self, roots):
        self.mem, self.k = R.Memory(roots), {}

    def __call__(self, ptr):
        ptr = int(ptr or 0)
        if not ptr:
            return '0'
        try:
            a, off = self.mem.find(ptr, 0, '')
        except R.PointerError:
            return 'H'
        return f'A{self.k.setdefault(a.start, len(self.k))}+{off}({a.nbytes})'

    def maybe(self, v):
        """An int64 op argument that may carry a pointer (the stem's BatchNorm vectors)."""
        s = self(v) if v > (1 << 32) else 'H'
        return str(v) if s == 'H' else s

    def struct(self, tab_ptr, ctype, n):
        """n items of a device-side table."""
        raw = self.mem.typed(tab_ptr, torch.uint8, n * C.sizeof(ctype), ctype.__name__).cpu().numpy().tobytes()
        return [ctype.from_buffer_copy(raw, k * C.sizeof(ctype)) for k in range(n)]


def val(names, ctype, v):
    if ctype is C.c_void_p:
        return names(v)
    if issubclass(ctype, C.Array):
        return '[' + ','.join(val(names, ctype._type_, x) for x in v) + ']'
    if issubclass(ctype, C.Structure):
        return '{' + fields(names, v) + '}'
    return repr(v)


def fields(names, s):
    return ' '.join(f'{n}={val(names, t, getattr(s, n))}' for n, t in s._fields_ if not n.startswith('pad_'))


def head_desc(op):
    """An ASSIGN / LOSS op points at a dsl_fcos_desc or at the head's wider descriptor that starts with one."""
    f = C.cast(op.desc, C.POINTER(L.FcosDesc)).contents.head_flags
    if hasattr(params, 'HEAD_KINDS'):          # the kind whose flags are all set and the most: its record names the outer struct
        kind = max((k for k in params.HEAD_KINDS.values() if f & k.flags == k.flags), key=lambda k: bin(k.flags).count('1'))
        t = getattr(L, kind.loss_desc[0])
    else:          # a tree from before the head-kind table
        t = L.PaaDesc if f & L.HEAD_PAA else L.LdDesc if f & L.HEAD_LD else L.GflDesc if f & L.HEAD_GFL else L.FcosDesc
    return C.cast(op.desc, C.POINTER(t)).contents


def walk(plan):
    """[(list name, OpList)] in execution order."""
    lists = [('prefix', plan.prefix), ('fwd_rest', plan.fwd_rest)] if getattr(plan, 'prefix', None) is not None else [('fwd', plan.fwd)]
    if plan.training:
        lists += [('assign_ops', plan.assign_ops), ('quality_ops', plan.quality_ops), ('loss_ops', plan.loss_ops)]
        lists += [(f'bwd[{k}] ' + ' '.join(f'{a}={v}' for a, v in sorted(info.items())), ol) for k, (ol, info) in enumerate(plan.bwd_segments)]
    return [(n, ol) for n, ol in lists if ol is not None]


def members(op, ol):
    """[(descriptor, label)] an op reaches: its own descriptor, the members of a group array or of a multi table."""
    if op.kind == L.OP_WGRAD_GROUP:
        arr = C.cast(op.desc, C.POINTER(L.WgradDesc))
        return [(arr[g], f'member {g}') for g in range(op.i[0])]
    if op.kind == L.OP_WGRAD_MULTI:
        m = [k for k in ol.keep if isinstance(k, ops.WgradMulti) and k.host.data_ptr() == op.p[0]][0]
        sub = [s for s, c in enumerate(m.counts) for _ in range(c)]
        return [(m.descs[g], f'member {g} sub {sub[g]}') for g in range(len(m.descs))]
    if op.kind in (L.OP_ASSIGN, L.OP_LOSS):
        return [(head_desc(op), 'desc')]
    if op.kind in DESC_OF and op.desc:
        return [(C.cast(op.desc, C.POINTER(DESC_OF[op.kind])).contents, 'desc')]
    return []


def tables(names, op, d):
    """The item tables an op's arguments point at."""
    if op.kind == L.OP_FP8_PREP:
        return names.struct(op.p[0], L.Fp8PrepItem, op.i[0])
    if op.kind == L.OP_RLA and d.kind == L.RLA_REC_SUM:
        return names.struct(d.p[0], L.RecSumItem, d.i[0])
    if op.kind == L.OP_RLA and d.kind == L.RLA_BN_POST:
        return names.struct(d.p[0], L.BnPostItem, d.i[0])
    return []


def signature(plan, roots, out):
    names = Names(roots)
    where = {}
    for lname, ol in walk(plan):
        out(f'== {lname}: {len(ol.items)} ops')
        for k, op in enumerate(ol.items):
            kind = KINDS.get(op.kind, str(op.kind))
            ms = members(op, ol)
            if op.kind == L.OP_RLA:
                kind += '.' + RLA_KINDS.get(ms[0][0].kind, '?')
            out(f'{k} {kind} i={list(op.i)} p=[{",".join(names(p) for p in op.p)}] l=[{",".join(names.maybe(v) for v in op.l)}]')
            for g, (d, label) in enumerate(ms):
                where[C.addressof(d)] = (lname.split(' ')[0], k, g)
                out(f'    {label}: {fields(names, d)}')
                for t, it in enumerate(tables(names, op, d)):
                    out(f'      item {t}: {fields(names, it)}')
            if op.kind == L.OP_FP8_PREP:
                for t, it in enumerate(tables(names, op, None)):
                    out(f'      item {t}: {fields(names, it)}')
    out('== descriptors that follow layer1\'s output buffer')
    for line in sorted(f'{where.get(C.addressof(d), "not in any list")} {field} +{off}' for d, field, off in tracked_l1(plan)):
        out('    ' + line)


# ---- legs ------------------------------------------------------------------------------------------------------------------------
def resnet_cfg():
    return fcos_model_cfg()


def rla_cfg():
    cfg = fcos_model_cfg()
    cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
    return cfg


def fp8_cfg():
    return dict(fcos_model_cfg(), fp8=dict(layers='towers'))


def norelu_cfg():
    cfg = fcos_model_cfg()
    cfg['neck']['relu_before_extra_convs'] = False
    return cfg


def atss_cfg():
    from test_atss_cpu import atss_model_cfg
    return atss_model_cfg()


def plain_cfg():
    from test_head_options_cpu import PLAIN_HEAD
    return fcos_model_cfg(**PLAIN_HEAD)


def ld_cfg():
    from test_ld_cpu import ld_model_cfg
    return ld_model_cfg()


def gfl_cfg():
    from test_gfl_cpu import gfl_model_cfg
    return gfl_model_cfg()


def paa_cfg():
    from test_paa_cpu import paa_model_cfg
    return paa_model_cfg()


def autoassign_cfg():
    from test_autoassign_cpu import aa_model_cfg
    return aa_model_cfg()


TINY = (64, 96)         # tests/golden/net_tiny.npz
ODD = (160, 224)        # test_train_step_vs_oracle_other_batch_sizes_and_shapes: levels 20x28, 10x14, 5x7, 3x4, 2x2
# (name, config, N, (H, W), tuning knobs, options: defer / eval / single_stream / steps = also train three steps)
LEGS = [
    ('resnet N=1', resnet_cfg, 1, TINY, {}, {}),
    ('resnet N=2', resnet_cfg, 2, TINY, {}, dict(steps=True)),
    ('resnet N=3', resnet_cfg, 3, TINY, {}, {}),
    ('resnet N=3 odd levels', resnet_cfg, 3, ODD, {}, {}),
    ('resnet side=0', resnet_cfg, 2, TINY, dict(side='0'), dict(steps=True)),
    ('resnet img_split= img_split_bwd=', resnet_cfg, 2, TINY, dict(img_split='', img_split_bwd=''), {}),
    ('resnet img_split_bwd=234', resnet_cfg, 2, TINY, dict(img_split_bwd='234'), {}),
    ('resnet img_split_bwd=234 N=3 odd levels', resnet_cfg, 3, ODD, dict(img_split_bwd='234'), {}),
    ('resnet bneck_fwd=', resnet_cfg, 2, TINY, dict(bneck_fwd=''), {}),
    ('resnet bneck_fwd= N=3 odd levels', resnet_cfg, 3, ODD, dict(bneck_fwd=''), {}),
    ('resnet bneck_fwd=23', resnet_cfg, 2, TINY, dict(bneck_fwd='23'), {}),
    ('resnet pipe_prefix=0', resnet_cfg, 2, TINY, dict(pipe_prefix='0'), {}),
    ('resnet defer_head_update', resnet_cfg, 2, TINY, {}, dict(defer=True, steps=True)),
    ('resnet fp8 towers', fp8_cfg, 2, TINY, {}, {}),
    ('resnet relu_before_extra_convs=False', norelu_cfg, 2, TINY, {}, {}),
    ('resnet plain head', plain_cfg, 2, TINY, {}, {}),
    ('resnet ATSS head', atss_cfg, 2, TINY, {}, dict(steps=True)),
    ('resnet GFL head', gfl_cfg, 2, TINY, {}, dict(steps=True)),
    ('resnet LD head', ld_cfg, 2, TINY, {}, {}),          # (signature only: its step needs the teacher's sweep, tests/test_ld_gpu.py)
    ('resnet PAA head', paa_cfg, 2, TINY, {}, dict(steps=True)),
    ('resnet eval', resnet_cfg, 2, TINY, {}, dict(eval=True)),
    ('resnet eval single_stream', resnet_cfg, 2, TINY, {}, dict(eval=True, single_stream=True)),
    ('rla N=3', rla_cfg, 3, TINY, {}, dict(steps=True, tile=2)),
    ('rla N=3 odd levels', rla_cfg, 3, ODD, {}, {}),
    ('rla side=0', rla_cfg, 3, TINY, dict(side='0'), {}),
    ('rla rla_split=', rla_cfg, 3, TINY, dict(rla_split=''), {}),
    ('rla rla_split_bwd=123', rla_cfg, 3, TINY, dict(rla_split_bwd='123'), {}),
    ('rla rla_tail=0', rla_cfg, 3, TINY, dict(rla_tail='0'), {}),
    ('resnet AutoAssign head', autoassign_cfg, 2, TINY, {}, dict(steps=True)),          # (last: the legs above keep their text)
]


def build_model(cfg_fn, defer=False):
    from oracle import fcos_oracle as O
    from oracle import rla_oracle as RO
    cfg = cfg_fn()
    torch.manual_seed(3)
    model = build_detector(cfg)
    if model.store.head.is_default():          # (the other heads keep their seeded initialisation, as their tests do)
        model.load_state_dict((RO if cfg['backbone']['type'] == 'RLA_ResNet' else O).synth_state_dict(0))
    model = model.cuda()
    opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.),
                  defer_head_update=defer)
    return model, opt


def trained_hash(cfg_fn, defer, tile=1):
    """sha256 of the trainable parameters after three steps on the fixture batch (tile=2: its images repeated 2 x 2 to 128 x 192, the
    smallest size the RLA step is tested at elsewhere; the boxes stay where they are)."""
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_tiny.npz'))
    B = int(d['B'])
    img = torch.from_numpy(d['img']).repeat(1, 1, tile, tile).cuda()
    gtb, gtl = [torch.from_numpy(d[f'gt{i}']) for i in range(B)], [torch.from_numpy(d[f'gl{i}']) for i in range(B)]
    metas = [dict(img_shape=tuple(img.shape[2:]) + (3,), pad_shape=tuple(img.shape[2:]) + (3,), scale_factor=1.0)] * B
    model, opt = build_model(cfg_fn, defer)
    for _ in range(3):
        res = model.train_step(dict(img=img, img_metas=metas, gt_bboxes=gtb, gt_labels=gtl), opt)
        res['loss'].backward()
        opt.step()
    model.store.wait_pending()
    torch.cuda.synchronize()
    return hashlib.sha256(model.store.train.cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='-', help='output file (default: standard output)')
    ap.add_argument('--legs', default='', help='only the legs whose name contains this text')
    ap.add_argument('--no-steps', action='store_true', help='signatures only, no training steps')
    args = ap.parse_args()
    fh = sys.stdout if args.out == '-' else open(args.out, 'w')
    out = lambda s: print(s, file=fh, flush=True)
    tuning.tune('side')         # (DSL_TUNE parsed before the overrides below)
    for name, cfg_fn, N, (H, W), knobs, opt_ in LEGS:
        if args.legs not in name:
            continue
        saved = dict(tuning._values)
        for k, v in knobs.items():
            tuning.set_tune(k, v)
        try:
            out(f'#### {name}: N={N} H={H} W={W} ' + ' '.join(f'{k}={v!r}' for k, v in sorted(knobs.items())))
            model, opt = build_model(cfg_fn, opt_.get('defer', False))
            eng = model._get_engine()
            plan = eng.plan(model.store, N, H, W, training=not opt_.get('eval', False), single_stream=opt_.get('single_stream', False))
            torch.cuda.synchronize()
            signature(plan, {'engine': eng, 'plan': plan, 'store': model.store, 'opt': opt, 'pixtabs': ops._pixtabs, 'model': model}, out)
            del plan, eng, model, opt
            if opt_.get('steps') and not args.no_steps:
                out(f'trained weights sha256 {trained_hash(cfg_fn, opt_.get("defer", False), opt_.get("tile", 1))}')
            torch.cuda.empty_cache()
        finally:
            tuning._values.clear()
            tuning._values.update(saved)
        print('done:', name, file=sys.stderr, flush=True)


if __name__ == '__main__':
    main()

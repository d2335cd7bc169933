"""LD without a GPU: tests/ld_ref.py against what the reference's own LDHead computed (tests/golden/ld_*.npz, written by
tests/golden/make_ld_golden.py), the configuration surface of LDHead / KnowledgeDistillationKLDivLoss /
KnowledgeDistillationSingleStageDetector, the isolation of the teacher, and the ctypes mirror of dsl_ld_desc."""
import ctypes
import os
import subprocess

import pytest
import torch

import atss_ref as AR
import ld_ref as LR
from test_gfl_cpu import gfl_model_cfg, load_case as gfl_load_case, loss_kw, ref_assign

T = torch.from_numpy
CASES = 'abcd'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_case(d):
    c = gfl_load_case(d)
    c.update(soft=[T(d[f'soft{l}']) for l in range(5)], soft_scales=T(d['soft_scales']), T=float(d['T']), ld_weight=float(d['ld_weight']))
    return c


def ld_kw(c):
    return dict(loss_kw(c), T=c['T'], ld_weight=c['ld_weight'])


def ld_head_cfg(**kw):
    """bbox_head of configs/ld/ld_r18_gflv1_r101_fpn_coco_1x.py."""
    head = dict(type='LDHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1, strides=[8, 16, 32, 64, 128]),
                loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0),
                loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25),
                loss_ld=dict(type='KnowledgeDistillationKLDivLoss', loss_weight=0.25, T=10), reg_max=16,
                loss_bbox=dict(type='GIoULoss', loss_weight=2.0))
    head.update(kw)
    return head


def ld_model_cfg(teacher=None, head=None, **kw):
    """The distillation detector of configs/ld on the caffe ResNet-50 of configs/fcos, with a GFL R50-caffe teacher given as a dict."""
    cfg = gfl_model_cfg()
    cfg['type'] = 'KnowledgeDistillationSingleStageDetector'
    cfg['bbox_head'] = ld_head_cfg(**(head or {}))
    cfg['teacher_config'] = dict(model=gfl_model_cfg()) if teacher is None else teacher
    cfg.update(kw)
    return cfg


def build(cfg=None):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(cfg or ld_model_cfg())


# ---- the model against the reference's outputs -----------------------------------------------------------------------------------
def test_fixture_covers_the_cases(golden):
    d = {c: golden(f'ld_{c}.npz') for c in CASES}
    assert all(int(d[c]['B']) == 2 and [tuple(s) for s in d[c]['sizes']] == AR.SIZES for c in CASES)
    a = d['a']
    assert (int(a['num_classes']), int(a['reg_max']), float(a['T']), float(a['ld_weight'])) == (80, 16, 10.0, 0.25) and a['reg0'].shape[1] == 68
    assert bool((T(a['soft_scales']) != T(a['scales'])).all())
    assert all(int(d[c]['num_classes']) == 3 for c in 'bcd')
    assert len(d['b']['gt1']) == 0 and min(int(v) for v in d['b']['npos']) == 0 and max(int(v) for v in d['b']['npos']) > 0
    assert (int(d['c']['reg_max']), float(d['c']['T'])) == (15, 1.0) and d['c']['reg0'].shape[1] == 64 and d['c']['soft0'].shape[1] == 64
    assert (int(d['d']['reg_max']), float(d['d']['T']), float(d['d']['ld_weight'])) == (3, 2.5, 1.0)
    for c in CASES:          # teacher logits on the 1 / 8 grid, shaped as the student's
        for l in range(5):
            s = T(d[c][f'soft{l}'])
            assert s.shape == d[c][f'reg{l}'].shape and torch.equal(s * 8, (s * 8).round())


@pytest.mark.parametrize('case', CASES)
def test_redraw_conditions_hold_for_the_stored_case(golden, case):
    """Conditions (5) - (7) of make_gfl_golden.py, re-asserted from the stored arrays: no target distance within 1e-4 of an integer, no
    predicted edge equal to a target edge, no tie for a positive's best class."""
    d = golden(f'ld_{case}.npz')
    c = load_case(d)
    dist, dec, tgt, pos = T(d['dfl_targets']), T(d['decoded']), T(d['tgt']), T(d['pos']).long()
    assert len(pos) > 0
    assert not bool(((dist - dist.round()).abs() < 1e-4).any())
    assert not bool((dec == tgt).any())
    top2 = AR.levels_to_flat(c['cls'])[pos].sigmoid().topk(2, 1)[0]
    assert not bool((top2[:, 0] == top2[:, 1]).any())


@pytest.mark.parametrize('case', CASES)
def test_ref_losses_equal_reference(golden, case):
    d = golden(f'ld_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    assert torch.equal(a['labels'], T(d['labels']).long()) and a['npos'] == [int(v) for v in d['npos']]
    cls, raw, soft = (AR.levels_to_flat(c[k]).double() for k in ('cls', 'reg', 'soft'))
    out = LR.loss(cls, raw, c['scales'].double(), soft, c['soft_scales'].double(), a, c['sizes'], c['B'], **ld_kw(c))
    for got, k in zip(out[:4], ('loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld')):
        print(k, float(got), float(d[k]))
        assert float(got) == pytest.approx(float(d[k]), rel=1e-5), k
    assert float(out[3]) > 0 and torch.isfinite(out[3])          # (case b: one image empty, the term comes from the other)


@pytest.mark.parametrize('case', CASES)
def test_ref_gradients_equal_reference(golden, case):
    d = golden(f'ld_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    cls = AR.levels_to_flat(c['cls']).double().requires_grad_()
    raw = AR.levels_to_flat(c['reg']).double().requires_grad_()
    sc = c['scales'].double().requires_grad_()
    soft = AR.levels_to_flat(c['soft']).double().requires_grad_()
    lc, lb, ldf, lld, _ = LR.loss(cls, raw, sc, soft, c['soft_scales'].double(), a, c['sizes'], c['B'], **ld_kw(c))
    (lc + lb + ldf + lld).backward()
    for got, k in ((cls.grad, 'gcls'), (raw.grad, 'greg')):
        want = AR.levels_to_flat([T(d[f'{k}{l}']) for l in range(5)]).double()
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-7 * float(want.abs().max()) + 1e-12), k
    assert torch.allclose(sc.grad, T(d['gscales']).double(), rtol=1e-4, atol=1e-7)
    assert soft.grad is None          # the teacher receives no gradient


def test_ld_term_has_no_normaliser_and_zero_for_equal_rows(golden):
    c = load_case(golden('ld_d.npz'))
    a = ref_assign(c)
    cls, raw, soft = (AR.levels_to_flat(c[k]).double() for k in ('cls', 'reg', 'soft'))
    args = (a, c['sizes'], c['B'])
    one = LR.loss(cls, raw, c['scales'].double(), soft, c['soft_scales'].double(), *args, **ld_kw(c))
    ws = float(one[4][2])
    two = LR.loss(cls, raw, c['scales'].double(), soft, c['soft_scales'].double(), *args, world=2.0, norm=(2.0 * a['num_total'], 4.0 * ws), **ld_kw(c))
    assert float(two[3]) == float(one[3]) and float(two[1]) == pytest.approx(float(one[1]) / 2, rel=1e-12)
    same = LR.loss(cls, raw, c['scales'].double(), raw, c['scales'].double(), *args, **ld_kw(c))
    assert abs(float(same[3])) < 1e-12
    c['gts'], c['gls'] = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    none = LR.loss(cls, raw, c['scales'].double(), soft, c['soft_scales'].double(), ref_assign(c), c['sizes'], c['B'], **ld_kw(c))
    assert float(none[3]) == 0.0


# ---- configuration surface ------------------------------------------------------------------------------------------------------
def test_ld_head_builds_from_the_reference_config_dict():
    from dsl_amd import _lib as L
    from dsl_amd.detectors import GFLHead, KnowledgeDistillationKLDivLoss, LDHead
    from dsl_amd.registry import build_head
    h = build_head(ld_head_cfg())
    assert isinstance(h, LDHead) and isinstance(h, GFLHead) and isinstance(h.loss_ld, KnowledgeDistillationKLDivLoss)
    o = h.options
    assert (o.head_kind, o.reg_max, o.ld_weight, o.ld_T, o.dfl_weight, o.bbox_weight) == ('gfl', 16, 0.25, 10.0, 0.25, 2.0)
    assert o.flags() == L.HEAD_ATSS | L.HEAD_LOSS_EXT | L.HEAD_GFL | L.HEAD_LD and L.HEAD_LD == 128
    d = build_head({k: v for k, v in ld_head_cfg().items() if k != 'loss_ld'})          # the default loss_ld
    assert (d.options.ld_weight, d.options.ld_T) == (0.25, 10.0)
    # an LD head's key differs from the GFL head's, whose key is what it was
    from dsl_amd.params import HeadOptions
    g = HeadOptions(head_kind='gfl')
    assert g.ld_weight is None and g.key()[-4:] == ('gfl', 16, 2.0, 0.25) and not g.flags() & L.HEAD_LD
    assert HeadOptions(head_kind='gfl', ld_weight=0.25).key() == g.key() + (0.25, 10.0)
    assert 'ld_T' in repr(o) and 'ld_T' not in repr(g)


def test_detector_builds_with_a_gfl_teacher_from_a_dict_and_from_a_file(tmp_path):
    from dsl_amd.detectors import GFL, KnowledgeDistillationSingleStageDetector, LDHead
    m = build()
    assert isinstance(m, KnowledgeDistillationSingleStageDetector) and isinstance(m, GFL) and isinstance(m.bbox_head, LDHead)
    assert type(m.teacher_model) is GFL and m.teacher_model.store is not m.store and m.eval_teacher is True
    assert build(ld_model_cfg(teacher=gfl_model_cfg(), eval_teacher=False)).eval_teacher is False          # `model` given directly
    # a path: Config.fromfile, `_base_` followed
    (tmp_path / 'base.py').write_text('model = ' + repr(gfl_model_cfg()) + '\n')
    (tmp_path / 'teacher.py').write_text("_base_ = './base.py'\nmodel = dict(bbox_head=dict(num_classes=80))\n")
    f = build(ld_model_cfg(teacher=str(tmp_path / 'teacher.py')))
    assert type(f.teacher_model) is GFL and f.teacher_model.store.head.reg_max == 16
    # a teacher may itself be a distillation student's kind of head on another class count: only the box grid must agree
    t3 = gfl_model_cfg(num_classes=3)
    assert build(ld_model_cfg(teacher=dict(model=t3))).teacher_model.store.num_classes == 3


def _refused(cfg_kw, word, exc=NotImplementedError):
    with pytest.raises(exc, match=word):
        build(ld_model_cfg(**cfg_kw))


def test_refusals_name_the_option(tmp_path):
    from util import fcos_model_cfg
    _refused(dict(head=dict(loss_ld=dict(type='KnowledgeDistillationKLDivLoss', loss_weight=0.25, T=0.5))), r'T: a finite number >= 1 \(got 0\.5')
    _refused(dict(head=dict(loss_ld=dict(type='KnowledgeDistillationKLDivLoss', T=float('inf')))), 'T: a finite number >= 1')
    _refused(dict(head=dict(loss_ld=dict(type='KnowledgeDistillationKLDivLoss', reduction='sum'))), "reduction='mean'")
    _refused(dict(head=dict(loss_ld=dict(type='KnowledgeDistillationKLDivLoss', loss_weight=-1.0))), 'loss_weight')
    _refused(dict(head=dict(loss_ld=dict(type='DistributionFocalLoss'))), 'loss_ld: KnowledgeDistillationKLDivLoss')
    _refused(dict(teacher=dict(model=gfl_model_cfg(reg_max=7))), 'teacher reg_max 7 != student reg_max 16')
    _refused(dict(teacher=dict(model=fcos_model_cfg())), 'GFL-family head.*FCOS with FCOSHead')
    _refused(dict(head=dict(type='GFLHead')), "bbox_head type='LDHead'")
    _refused(dict(teacher_ckpt=str(tmp_path / 'absent.pth')), 'teacher_ckpt.*absent.pth.*not found', FileNotFoundError)
    # everything GFLHead refuses stays refused, fp8 towers included
    _refused(dict(head=dict(reg_max=17)), r'reg_max in 1\.\.16')
    _refused(dict(head=dict(soft_weight=1.0)), 'soft_weight')
    _refused(dict(fp8=dict(layers='towers')), 'fp8 towers')
    from dsl_amd.params import HeadOptions
    for kw, word in ((dict(head_kind='fcos', ld_weight=0.25), 'ld_weight is an option of head_kind'), (dict(head_kind='gfl', ld_weight=-1.0), 'ld_weight'),
                     (dict(head_kind='gfl', ld_weight=0.25, ld_T=0.9), 'ld_T'), (dict(head_kind='gfl', ld_weight=float('nan')), 'ld_weight')):
        with pytest.raises(NotImplementedError, match=word):
            HeadOptions(**kw)


def test_teacher_checkpoint_is_loaded_through_the_teachers_state_dict(tmp_path):
    t = build(gfl_model_cfg())
    g = torch.Generator().manual_seed(11)
    sd = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in t.state_dict().items()}
    torch.save(dict(state_dict=sd, meta=dict(epoch=12)), tmp_path / 'teacher.pth')
    m = build(ld_model_cfg(teacher_ckpt=str(tmp_path / 'teacher.pth')))
    got = m.teacher_model.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())
    assert not torch.equal(m.state_dict()['bbox_head.gfl_reg.weight'], sd['bbox_head.gfl_reg.weight'])
    torch.save(dict(state_dict={'conv1.weight': torch.zeros(3)}), tmp_path / 'other.pth')
    with pytest.raises(KeyError, match='no key of this checkpoint matches the teacher'):
        build(ld_model_cfg(teacher_ckpt=str(tmp_path / 'other.pth')))


def test_teacher_is_isolated_from_the_student():
    m, g = build(), build(gfl_model_cfg())
    assert list(m.state_dict()) == list(g.state_dict())          # no loss_ld parameter, no teacher key
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in g.named_parameters()]
    assert not [k for k in m.state_dict() if 'teacher' in k] and not [k for k, _ in m.named_parameters() if 'teacher' in k]
    ptrs = {v.data_ptr() for v in m.teacher_model.state_dict().values()}
    assert not ptrs & {v.data_ptr() for v in m.state_dict().values()} and not ptrs & {p.data_ptr() for p in m.parameters()}
    assert m.store.n_train == g.store.n_train and m.store.grad_buckets() == g.store.grad_buckets()
    assert all('teacher' not in n for n, _ in m.named_children()) and m.teacher_model not in list(m.modules())
    assert m.store.train.data_ptr() != m.teacher_model.store.train.data_ptr()
    assert m.train() is m and m.eval() is m


def test_loss_plan_descriptor_of_an_ld_head():
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    o = HeadOptions(head_kind='gfl', reg_max=16, ld_weight=0.5, ld_T=4.0)
    p = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o, max_gt=64, num_classes=3)
    assert isinstance(p.ld, L.LdDesc) and ctypes.addressof(p.ld) == ctypes.addressof(p.gfl) == ctypes.addressof(p.desc)
    assert (p.ld.T, p.ld.w_ld, p.gfl.reg_max, p.ld.gfl.w_dfl) == (4.0, 0.5, 16, 0.25) and len(p.logvec) == 5
    assert p.desc.head_flags == L.HEAD_ATSS | L.HEAD_LOSS_EXT | L.HEAD_GFL | L.HEAD_LD and not p.ld.soft
    soft, sc = torch.zeros(p.M, 68), torch.ones(5)
    p.bind_soft(soft, 68, sc)
    assert (p.ld.soft, p.ld.ld_soft, p.ld.soft_scales) == (soft.data_ptr(), 68, sc.data_ptr())
    q = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=HeadOptions(head_kind='gfl'))
    assert q.ld is None and isinstance(q.gfl, L.GflDesc) and len(q.logvec) == 4


def test_ld_desc_matches_header_layout(tmp_path):
    """tests/test_abi.py's method on the new struct: the header is compiled with gcc and asked for sizeof / offsetof."""
    from dsl_amd import _lib as L
    fields = ('gfl', 'soft', 'ld_soft', 'soft_scales', 'T', 'w_ld')
    src = tmp_path / 'sizes.c'
    body = '  printf("%zu %zu\\n", sizeof(dsl_ld_desc), sizeof(dsl_gfl_desc));\n'
    body += ''.join(f'  printf("%zu\\n", offsetof(dsl_ld_desc, {f}));\n' for f in fields)
    body += '  printf("%d\\n", DSL_HEAD_LD);\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsl_hip.h"\nint main(void) {\n' + body + '  return 0;\n}\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert ctypes.sizeof(L.LdDesc) == out[0] and ctypes.sizeof(L.GflDesc) == out[1]
    assert [getattr(L.LdDesc, f).offset for f in fields] == out[2:2 + len(fields)]
    assert out[-1] == L.HEAD_LD
    assert hasattr(L.lib, 'dsl_ld_loss')

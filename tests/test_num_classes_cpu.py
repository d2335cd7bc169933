"""Class counts other than 80 on the host side: parameter store layout, state-dict round trip and loading across class counts,
the reference's VOC configs, and the VOC mAP evaluator against the reference's eval_map (tests/golden/voc_map.npz)."""
import os

import numpy as np
import pytest
import torch

from util import fcos_model_cfg

VOC_DIR = '/root/reference/configs/fcos_semi/voc'


def build(C):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(fcos_model_cfg(num_classes=C))


@pytest.mark.parametrize('C', [1, 3, 20, 64, 65, 80, 128])
def test_store_layout_and_state_dict(C):
    from oracle import fcos_oracle as O
    m = build(C)
    cp, c4 = -(-C // 64) * 64, -(-C // 4) * 4
    assert (m.store.cls_pad, m.store.cls_ld) == (cp, c4)
    assert tuple(m.store.tview('head.cls_w').shape) == (cp, 3, 3, 256)
    assert tuple(m.store.tview('head.cls_b').shape) == (cp,)
    sd = O.synth_state_dict(0, num_classes=C)
    m.load_state_dict(sd)
    out = m.state_dict()
    assert set(out) == set(sd)
    for k, v in sd.items():
        assert tuple(out[k].shape) == tuple(v.shape) and torch.equal(out[k], v), k
    assert tuple(out['bbox_head.conv_cls.weight'].shape) == (C, 256, 3, 3)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 32021850 - (80 - C) * 2305
    # the padding rows are zero, and the [:C] views alias the flat store
    assert float(m.store.tview('head.cls_w')[C:].abs().sum()) == 0.0
    assert float(m.store.tview('head.cls_b')[C:].abs().sum()) == 0.0
    out['bbox_head.conv_cls.bias'].fill_(-1.25)
    out['bbox_head.conv_cls.weight'][C - 1].fill_(0.5)
    assert float(m.store.tview('head.cls_b')[:C].mean()) == -1.25
    assert float(m.store.tview('head.cls_w')[C - 1].mean()) == 0.5
    assert float(m.store.tview('head.cls_b')[C:].abs().sum()) == 0.0
    lo_hi = m.store.grad_buckets()
    assert lo_hi[-1][0] == 0 and lo_hi[0][1] == m.store.n_train


def test_80_classes_keep_their_layout():
    from dsl_amd.head_loss import FcosLossPlan  # noqa: F401  (import only: the plan itself allocates on the GPU)
    from dsl_amd.params import class_layout
    m = build(80)
    assert class_layout(80) == (128, 80)
    assert m.store.n_train == build(80).store.n_train
    assert m.store.wT_layout()[0]['head.cls'][1] == 256 * 9 * 128


@pytest.mark.parametrize('C', [0, 129, -3])
def test_class_count_out_of_range(C):
    with pytest.raises(NotImplementedError, match='1..128'):
        build(C)


def test_load_other_class_count():
    """An 80-class (COCO) state dict into a 20-class model: conv_cls is skipped with a warning (strict=False), an error with
    strict=True, as mmcv's load_state_dict does with a size mismatch."""
    from oracle import fcos_oracle as O
    m = build(20)
    m.load_state_dict(O.synth_state_dict(1, num_classes=20))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    sd80 = O.synth_state_dict(0)
    with pytest.raises(RuntimeError, match='conv_cls'):
        m.load_state_dict(sd80, strict=True)
    with pytest.warns(RuntimeWarning, match='conv_cls'):
        m.load_state_dict(sd80, strict=False)
    out = m.state_dict()
    for k, v in out.items():
        if k.startswith('bbox_head.conv_cls.'):
            assert torch.equal(v, before[k]), k
        else:
            assert torch.equal(v, sd80[k]), k
    assert float(m.store.tview('head.cls_w')[20:].abs().sum()) == 0.0


@pytest.mark.skipif(not os.path.isdir(VOC_DIR), reason='reference tree not present')
@pytest.mark.parametrize('name', sorted(os.listdir(VOC_DIR)) if os.path.isdir(VOC_DIR) else [])
def test_voc_configs_build_unmodified(name):
    from dsl_amd import detectors, runner  # noqa: F401
    from dsl_amd.optim import build_optimizer
    from dsl_amd.registry import Config, build_detector
    cfg = Config.fromfile(os.path.join(VOC_DIR, name))
    m = build_detector(cfg.model)
    assert m.bbox_head.num_classes == 20 and m.store.num_classes == 20
    opt = build_optimizer(m, cfg.optimizer, grad_clip=cfg.optimizer_config.get('grad_clip'))
    assert opt.max_norm == 10.0
    assert cfg.evaluation['metric'] == 'mAP'
    if m.store.backbone == 'resnet':
        assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 31883550


# ---- VOC mAP ----------------------------------------------------------------------------------------------------------
def _voc_fixture(golden):
    d = golden('voc_map.npz')
    n, C = int(d['n_img']), int(d['num_classes'])
    dets = [[d[f'det{i}_{c}'] for c in range(C)] for i in range(n)]
    anns = [{k: d[f'ann{i}_{k}'] for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore')} for i in range(n)]
    return d, dets, anns


def test_eval_map_vs_reference(golden):
    from dsl_amd.evaluation import eval_map
    d, dets, anns = _voc_fixture(golden)
    modes = set()
    for j in range(int(d['n_cases'])):
        mode, iou = str(d[f'case{j}_mode']), float(d[f'case{j}_iou'])
        ranges = [tuple(r) for r in d[f'case{j}_ranges']] or None
        modes.add((mode, ranges is None))
        mean_ap, res = eval_map(dets, anns, scale_ranges=ranges, iou_thr=iou, dataset='voc07' if mode == '11points' else None)
        np.testing.assert_allclose(np.asarray(mean_ap, np.float64), d[f'case{j}_mAP'], rtol=0, atol=1e-6)
        np.testing.assert_allclose(np.array([r['ap'] for r in res], np.float64), d[f'case{j}_ap'], rtol=0, atol=1e-6)
        assert np.array_equal(np.array([r['num_gts'] for r in res]), d[f'case{j}_num_gts'])
        for c, r in enumerate(res):
            np.testing.assert_allclose(np.asarray(r['recall'], np.float64), d[f'case{j}_rec{c}'], rtol=0, atol=1e-6)
            np.testing.assert_allclose(np.asarray(r['precision'], np.float64), d[f'case{j}_prec{c}'], rtol=0, atol=1e-6)
    assert modes == {('11points', True), ('area', True), ('11points', False), ('area', False)}
    # empty classes are left out of the mean
    assert (d['case0_num_gts'] == 0).any()


def test_voc_evaluate_and_eval_hook(golden):
    from dsl_amd.evaluation import EvalHook, VOCEvalDataset, voc_evaluate
    d, dets, anns = _voc_fixture(golden)
    ap07 = voc_evaluate(dets, anns, year=2007)
    assert list(ap07) == ['AP50', 'mAP']
    assert ap07['AP50'] == round(float(d['case0_mAP']), 3) and abs(ap07['mAP'] - float(d['case0_mAP'])) < 1e-6
    ap12 = VOCEvalDataset(anns, year=2012).evaluate(dets, metric='mAP', iou_thr=[0.5, 0.75])
    assert list(ap12) == ['AP50', 'AP75', 'mAP']
    assert abs(ap12['mAP'] - (float(d['case2_mAP']) + float(d['case3_mAP'])) / 2) < 1e-6
    with pytest.raises(KeyError):
        voc_evaluate(dets, anns, metric='bbox')

    class Runner:
        epoch, ema_flag, model, ema_model, work_dir, logger = 0, False, None, None, None, None

        def _det(self, m):
            return m

    import dsl_amd.evaluation as E
    hook = EvalHook(VOCEvalDataset(anns), metric='mAP')
    orig = E.multi_gpu_test
    E.multi_gpu_test = lambda det, loader, store=None: dets
    try:
        metrics = hook._do_evaluate(Runner())
        assert set(metrics) == {'AP50', 'mAP'} and abs(metrics['mAP'] - float(d['case0_mAP'])) < 1e-6

        class Plain:                   # no evaluate(): the hook's own VOC path
            annotations, year = anns, 2012
        metrics = EvalHook(Plain(), metric='mAP')._do_evaluate(Runner())
        assert set(metrics) == {'AP50', 'mAP'} and abs(metrics['mAP'] - float(d['case2_mAP'])) < 1e-6
    finally:
        E.multi_gpu_test = orig
    # a loader whose dataset carries COCO-form annotations: converted, then the same protocol
    from dsl_amd.evaluation import voc_annotations

    class Coco:
        cat_ids = [7, 9]
        annotations = [[dict(bbox=[10, 10, 20, 20], category_id=9, iscrowd=0), dict(bbox=[0, 0, 5, 5], category_id=7, iscrowd=1)]]
    a = voc_annotations(Coco())[0]
    assert a['bboxes'].tolist() == [[10, 10, 30, 30]] and a['labels'].tolist() == [1]
    assert a['bboxes_ignore'].tolist() == [[0, 0, 5, 5]] and a['labels_ignore'].tolist() == [0]

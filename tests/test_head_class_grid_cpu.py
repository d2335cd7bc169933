"""The configuration surface of the seven registered head classes and the seven detector classes, walked as a grid, against
tests/golden/head_class_grid.txt - the output of this file on the commit before the heads moved onto one base class in a module of
their own.  Each head is built through build_head from the bbox_head of the reference's own config for it (the *_model_cfg helpers
of the per-head tests, with train_cfg / test_cfg handed in as the detector does), alone and then with one argument at a time
changed - the arguments its constructor names, the DSL keys, the keys of the nested loss_* / anchor_generator / bbox_coder / norm_cfg / train_cfg.assigner dicts,
and one unknown key in every dict.  A line holds what the head ended up with, or the refusal.  Then every detector class is built
with its own head type and with another's."""
import copy
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]          # (run as a script, this file prints the grid)
from dsl_amd import detectors  # noqa: E402,F401 - registers the classes
from dsl_amd.registry import build_detector, build_head  # noqa: E402
from test_atss_cpu import atss_model_cfg  # noqa: E402
from test_autoassign_cpu import aa_model_cfg  # noqa: E402
from test_fovea_cpu import fovea_model_cfg  # noqa: E402
from test_gfl_cpu import gfl_model_cfg  # noqa: E402
from test_ld_cpu import ld_model_cfg  # noqa: E402
from test_paa_cpu import paa_model_cfg  # noqa: E402
from util import fcos_model_cfg  # noqa: E402

MODELS = [('FCOS', fcos_model_cfg), ('ATSS', atss_model_cfg), ('GFL', gfl_model_cfg), ('KnowledgeDistillationSingleStageDetector', ld_model_cfg),
          ('PAA', paa_model_cfg), ('FOVEA', fovea_model_cfg), ('AutoAssign', aa_model_cfg)]
DROP = object()          # a variation that removes the key
NAN, INF = float('nan'), float('inf')
FOCAL = dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.3, loss_weight=0.75)
# (path, value): applied to every head whose cfg has the dict the path leads into (a top-level argument: to every head)
VARIATIONS = [
    ('num_classes', 20), ('num_classes', 0), ('num_classes', 80.0),
    ('in_channels', 128), ('feat_channels', 128), ('stacked_convs', 2),
    ('norm_cfg', None), ('norm_cfg', dict(type='BN')), ('norm_cfg', dict(type='GN', num_groups=16)),
    ('norm_cfg.requires_grad', False),
    ('init_cfg', dict(type='Normal', layer='Conv2d', std=0.01)),
    ('loss_weight', 2.0), ('soft_weight', 0.5), ('soft_warm_up', 10), ('train_cfg', None), ('test_cfg', None),
    ('strides', [4, 8, 16, 32, 64]), ('strides', (8, 16, 32, 64, 128)), ('strides', [8, 16, 32, 64]),
    ('regress_ranges', ((-1, 32), (32, 64), (64, 128), (128, 256), (256, 1e8))), ('center_sample_radius', 2.5),
    ('center_sampling', False), ('norm_on_bbox', False), ('centerness_on_reg', False),
    ('center_sampling', True), ('norm_on_bbox', True), ('centerness_on_reg', True),
    ('conv_bias', 'auto'), ('conv_bias', False), ('conv_bias', 'yes'),
    ('dcn_on_last_conv', True), ('conv_cfg', dict(type='DCNv2')), ('reg_decoded_bbox', True), ('reg_decoded_bbox', False),
    ('loss_cls', FOCAL), ('loss_cls', dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)),
    ('loss_cls', dict(type='QualityFocalLoss', use_sigmoid=True, beta=1.5, loss_weight=0.5)),
    ('loss_cls.gamma', 1.5), ('loss_cls.gamma', -1.0), ('loss_cls.alpha', 0.3), ('loss_cls.alpha', 1.5),
    ('loss_cls.beta', 1.5), ('loss_cls.beta', -1.0),
    ('loss_cls.loss_weight', 0.75), ('loss_cls.loss_weight', -1.0), ('loss_cls.use_sigmoid', False),
    ('loss_cls.reduction', 'sum'),
    ('loss_bbox', dict(type='GIoULoss', loss_weight=1.0)), ('loss_bbox', dict(type='GIoULoss', loss_weight=2.0)),
    ('loss_bbox', dict(type='GIoULoss', loss_weight=2.0, reduction='sum')),
    ('loss_bbox', dict(type='IoULoss', loss_weight=1.0)), ('loss_bbox', dict(type='IoULoss', loss_weight=2.0)),
    ('loss_bbox', dict(type='IoULoss', linear=True, loss_weight=1.0)),
    ('loss_bbox', dict(type='DIoULoss', loss_weight=2.0)), ('loss_bbox', dict(type='CIoULoss', loss_weight=1.5, eps=1e-5)),
    ('loss_bbox', dict(type='BoundedIoULoss')),
    ('loss_bbox', dict(type='SmoothL1Loss', beta=0.2, loss_weight=1.5)), ('loss_bbox', dict(type='L1Loss')),
    ('loss_bbox.loss_weight', 0.5), ('loss_bbox.loss_weight', -1.0), ('loss_bbox.beta', 0.2),
    ('loss_bbox.beta', 0.0),
    ('loss_centerness', dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=0.5)), ('loss_centerness', FOCAL),
    ('loss_centerness.loss_weight', 0.25), ('loss_centerness.use_sigmoid', False), ('loss_centerness.class_weight', [1.0]),
    ('anchor_generator.type', 'SSDAnchorGenerator'), ('anchor_generator.ratios', [0.5, 1.0, 2.0]), ('anchor_generator.octave_base_scale', 4),
    ('anchor_generator.octave_base_scale', 0), ('anchor_generator.octave_base_scale', DROP), ('anchor_generator.scales_per_octave', 3),
    ('anchor_generator.scales', [8]), ('anchor_generator.strides', [4, 8, 16, 32, 64]), ('anchor_generator.center_offset', 0.5),
    ('anchor_generator.base_sizes', [8, 16, 32, 64, 128]), ('anchor_generator.scale_major', False),
    ('bbox_coder', None), ('bbox_coder', dict(type='DeltaXYWHBBoxCoder')), ('bbox_coder', dict(type='TBLRBBoxCoder')),
    ('bbox_coder.type', 'DistancePointBBoxCoder'), ('bbox_coder.target_means', [0.0, 0.0, 0.1, 0.0]),
    ('bbox_coder.target_stds', [0.1, 0.2, 0.3, 0.4]), ('bbox_coder.target_stds', [0.1, 0.1, 0.2]), ('bbox_coder.target_stds', [0.1, 0.1, 0.2, 0.0]),
    ('bbox_coder.target_stds', DROP), ('bbox_coder.clip_border', False), ('bbox_coder.add_ctr_clamp', True), ('bbox_coder.ctr_clamp', 32),
    ('train_cfg.assigner', DROP), ('train_cfg.assigner.type', 'ATSSAssigner'), ('train_cfg.assigner.type', 'MaxIoUAssigner'),
    ('train_cfg.assigner.topk', 5), ('train_cfg.assigner.topk', 0), ('train_cfg.assigner.topk', 17),
    ('train_cfg.assigner.ignore_iof_thr', 0.5), ('train_cfg.assigner.iou_calculator', dict(type='BboxOverlaps2D')),
    ('train_cfg.assigner.iou_calculator', dict(type='BboxDistanceMetric')),
    ('train_cfg.assigner.pos_iou_thr', 0.2), ('train_cfg.assigner.pos_iou_thr', 0.0), ('train_cfg.assigner.pos_iou_thr', True),
    ('train_cfg.assigner.neg_iou_thr', 0.2), ('train_cfg.assigner.neg_iou_thr', DROP), ('train_cfg.assigner.min_pos_iou', 0.3),
    ('train_cfg.assigner.gt_max_assign_all', False), ('train_cfg.assigner.ignore_wrt_candidates', False),
    ('train_cfg.assigner.match_low_quality', False), ('train_cfg.assigner.gpu_assign_thr', 100),
    ('train_cfg.allowed_border', 0), ('train_cfg.pos_weight', 1.0), ('train_cfg.debug', True),
    ('topk', 5), ('topk', 0), ('topk', 17), ('score_voting', False), ('covariance_type', 'full'),
    ('reg_max', 8), ('reg_max', 0), ('reg_max', 17), ('reg_max', True),
    ('loss_dfl', dict(type='DistributionFocalLoss', loss_weight=0.5)), ('loss_dfl', FOCAL), ('loss_dfl.loss_weight', -1.0),
    ('loss_ld', dict(type='KnowledgeDistillationKLDivLoss', loss_weight=0.5, T=4)), ('loss_ld', FOCAL), ('loss_ld.loss_weight', -1.0),
    ('loss_ld.T', 0.5), ('loss_ld.T', True), ('loss_ld.reduction', 'sum'),
    ('base_edge_list', (8, 16, 32, 64, 128)), ('base_edge_list', [16, 32, 64, 128]), ('base_edge_list', [16, 32, 64, 128, 0]),
    ('scale_ranges', ((8, 32), (16, 64), (32, 128), (64, 256), (128, 512))), ('scale_ranges', [[8, 32], [16, 64], [32, 128], [64, 256]]),
    ('scale_ranges', ((8, 32), (16, 64), (32, 128), (64, 256), (512, 128))),
    ('sigma', 0.5), ('sigma', 0.0), ('sigma', 1.5), ('with_deform', True), ('deform_groups', 8),
    ('force_topk', True), ('pos_loss_weight', 0.5), ('pos_loss_weight', -1.0), ('neg_loss_weight', 0.6), ('neg_loss_weight', NAN),
    ('center_loss_weight', 0.7), ('center_loss_weight', 'x'),
]


def head_cfg(model):
    """The head's cfg as the detector hands it to build_head."""
    return dict(model['bbox_head'], train_cfg=model['train_cfg'], test_cfg=model['test_cfg'])


def dict_paths(cfg, prefix=''):
    """Dotted paths of cfg itself ('') and of every dict nested in it."""
    out = [prefix]
    for k, v in cfg.items():
        if isinstance(v, dict):
            out += dict_paths(v, f'{prefix}.{k}' if prefix else k)
    return out


def vary(cfg, path, value):
    """A deep copy of cfg with `value` at the dotted path; None where the path leads through a dict the cfg does not have."""
    cfg = copy.deepcopy(cfg)
    *parents, leaf = path.split('.')
    d = cfg
    for p in parents:
        d = d.get(p)
        if not isinstance(d, dict):
            return None
    if value is DROP:
        if leaf not in d:
            return None
        del d[leaf]
    else:
        d[leaf] = copy.deepcopy(value)
    return cfg


def describe_head(cfg, base_key=None):
    """What the built head ended up with (`key=base`: options.key() equals base_key), or the refusal."""
    try:
        h = build_head(cfg)
    except Exception as e:  # noqa: BLE001 - the grid records whatever the constructor raises
        return f'{type(e).__name__}: {e}'
    key = h.options.key()
    extra = ' '.join(f'{a}={getattr(h, a)!r}' for a in ('bbox_weight', 'topk', 'with_score_voting', 'reg_max') if hasattr(h, a))
    return (f"{type(h).__name__} key={'base' if key == base_key else repr(key)} strides={h.strides!r} "
            f'weights={(h.loss_weight, h.soft_weight, h.soft_warm_up)!r} '
            f'soft={(h.effective_soft_weight(3), h.effective_soft_weight(3))!r} {extra}').rstrip()


def arguments(head_type):
    """The named constructor arguments of a registered head class and of the registered classes it derives from, and the DSL keys."""
    names = {'loss_weight', 'soft_weight', 'soft_warm_up'}
    for c in getattr(detectors, head_type).__mro__:
        if getattr(detectors, c.__name__, None) is c:
            names |= {n for n, p in inspect.signature(c.__init__).parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD or p.kind is p.KEYWORD_ONLY}
    return names


def describe_detector(cfg):
    try:
        m = build_detector(cfg)
    except Exception as e:  # noqa: BLE001
        return f'{type(e).__name__}: {e}'
    return f'{type(m).__name__} with {type(m.bbox_head).__name__}'


def grid():
    lines = []
    for _, make in MODELS:
        base = head_cfg(make())
        name = base['type']
        lines.append(f'{name} -> {describe_head(base)}')
        base_key, args = build_head(base).options.key(), arguments(name)
        cases = [(p, v) for p, v in VARIATIONS if p.split('.')[0] in args] + [((p + '.' if p else '') + 'bogus', 1) for p in dict_paths(base)]
        for path, value in cases:
            cfg = vary(base, path, value)
            if cfg is not None:
                lines.append(f"{name} {path}={'<dropped>' if value is DROP else repr(value)} -> {describe_head(cfg, base_key)}")
    for k, (det, make) in enumerate(MODELS):
        lines.append(f'{det} -> {describe_detector(make())}')
        other = MODELS[(k + 1) % len(MODELS)][1]()          # the next detector's head and train_cfg / test_cfg under this one's type
        wrong = dict(make(), bbox_head=other['bbox_head'], train_cfg=other['train_cfg'], test_cfg=other['test_cfg'])
        lines.append(f"{det} bbox_head.type={other['bbox_head']['type']!r} -> {describe_detector(wrong)}")
    return lines


def test_every_head_and_detector_class_is_in_the_grid():
    classes = {n: c for n, c in vars(detectors).items() if isinstance(c, type) and not n.startswith('_')}
    assert sorted(make()['bbox_head']['type'] for _, make in MODELS) == sorted(n for n in classes if n.endswith('Head'))
    assert sorted(det for det, _ in MODELS) == sorted(n for n, c in classes.items() if issubclass(c, detectors.FCOS))


def test_every_case_of_the_grid_equals_the_commit_before_the_base_class():
    with open(os.path.join(ROOT, 'tests', 'golden', 'head_class_grid.txt')) as fh:
        want = fh.read().splitlines()
    got = grid()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'line {k + 1}'
    assert len(got) == len(want)


if __name__ == '__main__':
    print('\n'.join(grid()))

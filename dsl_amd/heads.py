"""The registered dense heads and their loss config classes, with the reference's names and constructor arguments, so that its
configs build unmodified:

  FCOSHead                      mmdet/models/dense_heads/fcos_head.py:14-726
  ATSSHead                      mmdet/models/dense_heads/atss_head.py:14-684 with core/bbox/assigners/atss_assigner.py,
                                core/anchor/anchor_generator.py, core/bbox/coder/delta_xywh_bbox_coder.py
  PAAHead                       mmdet/models/dense_heads/paa_head.py:44-673 with core/bbox/assigners/max_iou_assigner.py
  GFLHead / LDHead              mmdet/models/dense_heads/gfl_head.py:50-647, ld_head.py:10-261
  FoveaHead                     mmdet/models/dense_heads/fovea_head.py:50-348
  AutoAssignHead                mmdet/models/dense_heads/autoassign_head.py:123-509
  FocalLoss / GIoULoss / IoULoss / DIoULoss / CIoULoss / CrossEntropyLoss / ...   mmdet/models/losses/*.py

A head class computes nothing: it validates the configuration the HIP path implements and turns it into the params.HeadOptions that
the parameter store, the plans and the kernels are built for (`options`); DenseHead holds what all of them do alike.
dsl_amd.detectors imports this module, and every name here stays importable from there.
"""
import torch.nn as nn

from .params import HeadOptions, class_layout
from .registry import HEADS, LOSSES, build_loss


def _expect(cond, msg):
    if not cond:
        raise NotImplementedError('dsl_amd hot path: ' + msg)


def _loss_weight(name, loss_weight, reduction):
    _expect(reduction == 'mean', f"{name} reduction='mean'")
    _expect(isinstance(loss_weight, (int, float)) and 0.0 <= float(loss_weight) < float('inf'),
            f'{name} loss_weight: a finite number >= 0 (got {loss_weight!r})')
    return float(loss_weight)


class _LossCfg(nn.Module):
    """loss_weight scales the reported term and its gradients in the loss kernel (dsl_fcos_desc.w_cls / w_bbox / w_ctr)."""

    def __init__(self, loss_weight=1.0, reduction='mean', **kw):
        super().__init__()
        _expect(not kw, f'{type(self).__name__}: unknown arguments {sorted(kw)}')
        self.loss_weight = _loss_weight(type(self).__name__, loss_weight, reduction)


@LOSSES.register_module()
class FocalLoss(_LossCfg):
    """mmdet/models/losses/focal_loss.py:11-56,140-180: sigmoid focal loss with gamma >= 0 and 0 <= alpha <= 1."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, **kw):
        super().__init__(**kw)
        _expect(use_sigmoid, 'FocalLoss use_sigmoid=True (the reference has no softmax focal loss either)')
        _expect(isinstance(gamma, (int, float)) and 0.0 <= float(gamma) < float('inf'), f'FocalLoss gamma >= 0 (got {gamma!r})')
        _expect(isinstance(alpha, (int, float)) and 0.0 <= float(alpha) <= 1.0, f'FocalLoss alpha in [0, 1] (got {alpha!r})')
        self.gamma, self.alpha = float(gamma), float(alpha)


@LOSSES.register_module()
class GIoULoss(_LossCfg):
    """loss_weight stays at 1.0 in the config (as IoULoss's, and IoULoss's linear=False): these three refusals are part of the
    configuration surface from before the loss family.  The kernel and params.HeadOptions(box_loss='giou' | 'iou' | 'iou_linear',
    bbox_weight=...) compute them; DIoULoss / CIoULoss take a loss_weight here."""
    box_loss = 'giou'

    def __init__(self, eps=1e-6, **kw):
        super().__init__(**kw)
        _expect(eps == 1e-6, 'GIoU eps 1e-6')
        _expect(self.loss_weight == 1.0, 'GIoULoss loss_weight=1.0 (DIoULoss / CIoULoss take a loss_weight)')
        self.eps = 1e-6


@LOSSES.register_module()
class IoULoss(nn.Module):
    """mmdet/models/losses/iou_loss.py:223-290 with its defaults: -log(clamp(iou, 1e-6)), mean over avg_factor.  linear=True and
    loss_weight != 1.0 stay refused here (see GIoULoss); params.HeadOptions(box_loss='iou_linear', bbox_weight=...) runs them."""
    box_loss = 'iou'

    def __init__(self, linear=False, eps=1e-6, reduction='mean', loss_weight=1.0, **kw):
        super().__init__()
        _expect(not linear, 'IoULoss linear=False (the log loss)')
        _expect(eps == 1e-6, 'IoULoss eps=1e-6')
        _expect(kw.get('mode', 'log') == 'log', "IoULoss mode='log'")
        _expect(not (set(kw) - {'mode'}), f'IoULoss arguments linear, eps, reduction, loss_weight (got {sorted(kw)})')
        _expect(reduction == 'mean', "IoULoss reduction='mean'")
        _expect(loss_weight == 1.0, 'IoULoss loss_weight=1.0')
        self.loss_weight, self.eps = 1.0, 1e-6


@LOSSES.register_module()
class DIoULoss(_LossCfg):
    """mmdet/models/losses/iou_loss.py:105-157,369-406."""
    box_loss = 'diou'

    def __init__(self, eps=1e-6, **kw):
        super().__init__(**kw)
        _expect(isinstance(eps, float) and 0.0 < eps < 1.0, f'{type(self).__name__} 0 < eps < 1 (got {eps!r})')
        self.eps = eps


@LOSSES.register_module()
class CIoULoss(DIoULoss):
    """mmdet/models/losses/iou_loss.py:160-219,409-446.  Where prediction and target have the same aspect (v == 0) the penalty
    v^2 / (1 - iou + v) and its gradient are 0: the reference's fp32 arithmetic gives 0/0 = NaN when the two boxes coincide."""
    box_loss = 'ciou'


@LOSSES.register_module()
class BoundedIoULoss(nn.Module):
    def __init__(self, **kw):
        super().__init__()
        _expect(False, "GIoULoss, IoULoss, DIoULoss or CIoULoss as FCOSHead's loss_bbox (BoundedIoULoss cannot be used by the "
                       "reference's FCOSHead either: its (n, 4) loss does not broadcast against the (n,) centerness weight)")


@LOSSES.register_module()
class CrossEntropyLoss(_LossCfg):
    def __init__(self, use_sigmoid=False, use_mask=False, class_weight=None, **kw):
        super().__init__(**kw)
        _expect(use_sigmoid and not use_mask and class_weight is None, 'sigmoid BCE centerness loss')


@LOSSES.register_module()
class QualityFocalLoss(_LossCfg):
    """mmdet/models/losses/gfocal_loss.py:11-52,81-133: the classification loss of GFLHead, whose target is the IoU of the decoded
    prediction with the assigned box (dsl_gfl_desc.qfl_beta, dsl_fcos_desc.w_cls)."""

    def __init__(self, use_sigmoid=True, beta=2.0, **kw):
        super().__init__(**kw)
        _expect(use_sigmoid, 'QualityFocalLoss use_sigmoid=True (the reference builds only the sigmoid form)')
        _expect(isinstance(beta, (int, float)) and 0.0 <= float(beta) < float('inf'), f'QualityFocalLoss beta >= 0 (got {beta!r})')
        self.beta = float(beta)


@LOSSES.register_module()
class DistributionFocalLoss(_LossCfg):
    """mmdet/models/losses/gfocal_loss.py:55-78,136-185: cross entropy against the two bins around the target distance
    (dsl_gfl_desc.w_dfl)."""


@LOSSES.register_module()
class KnowledgeDistillationKLDivLoss(_LossCfg):
    """mmdet/models/losses/kd_loss.py:9-87: T^2 times the KL divergence between softmax(teacher / T) and softmax(student / T),
    the loss_ld of LDHead (dsl_ld_desc.T, dsl_ld_desc.w_ld)."""

    def __init__(self, reduction='mean', loss_weight=1.0, T=10):
        super().__init__(loss_weight=loss_weight, reduction=reduction)
        _expect(isinstance(T, (int, float)) and not isinstance(T, bool) and 1.0 <= float(T) < float('inf'),
                f'KnowledgeDistillationKLDivLoss T: a finite number >= 1 (got {T!r}; kd_loss.py:50)')
        self.T = float(T)


@LOSSES.register_module()
class SmoothL1Loss(_LossCfg):
    """mmdet/models/losses/smooth_l1_loss.py:11-29,49-101: 0.5 d^2 / beta where |d| < beta, else |d| - 0.5 beta.  FoveaHead's loss_bbox
    (dsl_fovea_desc.smooth_l1_beta); the other heads refuse it."""

    def __init__(self, beta=1.0, **kw):
        super().__init__(**kw)
        _expect(isinstance(beta, (int, float)) and 0.0 < float(beta) < float('inf'), f'SmoothL1Loss beta > 0 (got {beta!r})')
        self.beta = float(beta)


def _expect_towers(in_channels, feat_channels, stacked_convs, norm_cfg, no_dcn, anchor_head=True):
    """The network every head here is built on: four 256-channel GN-32 tower convolutions, no DCN.  anchor_head: the refusals name
    AnchorHead's arguments (conv_cfg, norm_cfg), else FCOSHead's."""
    _expect(in_channels == 256 and feat_channels == 256, 'in_channels=256, feat_channels=256')
    _expect(stacked_convs == 4, 'stacked_convs=4')
    _expect(no_dcn, 'conv_cfg=None (no DCN)' if anchor_head else 'dcn_on_last_conv=False (no DCN)')
    _expect(norm_cfg is not None and norm_cfg.get('type') == 'GN' and norm_cfg.get('num_groups') == 32,
            'GN-32 towers (norm_cfg)' if anchor_head else 'GN-32 towers')


def _expect_no_dsl_keys(name, kw):
    for k in ('soft_weight', 'soft_warm_up', 'loss_weight'):
        _expect(k not in kw, f'{name}: no DSL key {k} (the scale-invariant soft term and the per-stream loss_weight are FCOSHead options)')
    _expect(not kw, f'{name}: unknown arguments {sorted(kw)}')


def _build_loss_bbox(loss_bbox, refusal, lift_weight=True):
    """(module, loss_weight) of a head's loss_bbox; `refusal` names what the head accepts.  lift_weight (ATSSHead, GFLHead): GIoULoss /
    IoULoss keep refusing a loss_weight in their own constructors (FCOSHead's configuration surface), so the weight of configs/atss and
    configs/gfl (GIoULoss(loss_weight=2.0)) is taken off the dict here; it goes to the kernel as dsl_fcos_desc.w_bbox."""
    lb, wb = dict(loss_bbox), None
    if lift_weight and lb.get('type') in ('GIoULoss', 'IoULoss'):
        wb = _loss_weight(lb['type'], lb.pop('loss_weight', 1.0), lb.get('reduction', 'mean'))
    module = build_loss(lb)
    _expect(isinstance(module, (GIoULoss, IoULoss, DIoULoss)), refusal)
    return module, module.loss_weight if wb is None else wb


def _atss_option_kw(head):
    """What the ATSS-assigned heads (ATSSHead, GFLHead) pass to HeadOptions alike."""
    return dict(box_loss=head.loss_bbox.box_loss, box_eps=head.loss_bbox.eps, cls_weight=head.loss_cls.loss_weight,
                bbox_weight=head.bbox_weight, assigner='atss')


_FCOS_LOSSES = 'FocalLoss + GIoULoss, IoULoss, DIoULoss or CIoULoss + CrossEntropyLoss'


class DenseHead(nn.Module):
    """What the heads do alike: the class count and the strides the kernels are built for, the DSL stream weights at their neutral
    values (FCOSHead has arguments for them), train_cfg / test_cfg as the detector hands them in, and no scale-invariant soft term."""
    STRIDES = (8, 16, 32, 64, 128)

    def __init__(self, num_classes, train_cfg=None, test_cfg=None, strides=STRIDES):
        super().__init__()
        class_layout(num_classes)            # 1..MAX_CLASSES, else NotImplementedError naming the range
        _expect(list(strides) == list(self.STRIDES), 'strides 8..128')
        self.num_classes, self.strides = num_classes, self.STRIDES
        self.loss_weight, self.soft_weight, self.soft_warm_up = 1.0, 0.0, 0
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def effective_soft_weight(self, batch_size):
        return 0.0


@HEADS.register_module()
class FCOSHead(DenseHead):
    def __init__(self, num_classes, in_channels, regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8)),
                 center_sampling=False, center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False,
                 loss_weight=1.0, soft_weight=0.0, soft_warm_up=0, feat_channels=256, stacked_convs=4,
                 strides=(4, 8, 16, 32, 64), dcn_on_last_conv=False, conv_bias='auto',
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), train_cfg=None, test_cfg=None,
                 init_cfg=None, **kw):
        super().__init__(num_classes, train_cfg, test_cfg, strides)
        _expect_towers(in_channels, feat_channels, stacked_convs, norm_cfg, not dcn_on_last_conv, anchor_head=False)
        # mmcv ConvModule: bias='auto' = no bias in front of a norm layer - with the GroupNorm towers, False
        _expect(conv_bias is True or conv_bias is False or conv_bias == 'auto', "conv_bias True, False or 'auto'")
        self.center_sampling, self.norm_on_bbox, self.centerness_on_reg = bool(center_sampling), bool(norm_on_bbox), bool(centerness_on_reg)
        self.conv_bias = conv_bias is True
        self.strides = tuple(strides)
        self.regress_ranges = tuple(tuple(r) for r in regress_ranges)
        self.center_sample_radius = center_sample_radius
        self.loss_weight, self.soft_weight, self.soft_warm_up = loss_weight, soft_weight, soft_warm_up
        self.cur_iter = 0                               # fcos_head.py:103
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox, wb = _build_loss_bbox(loss_bbox, _FCOS_LOSSES, lift_weight=False)
        self.loss_centerness = build_loss(loss_centerness)
        _expect(isinstance(self.loss_cls, FocalLoss) and isinstance(self.loss_centerness, CrossEntropyLoss), _FCOS_LOSSES)
        # what the kernels and the parameter layout are built for (fixed per model: ParamStore.head)
        lb = self.loss_bbox
        self.options = HeadOptions(self.center_sampling, self.norm_on_bbox, self.centerness_on_reg,
                                   isinstance(lb, IoULoss), self.conv_bias, box_loss=lb.box_loss, box_eps=lb.eps,
                                   focal_gamma=self.loss_cls.gamma, focal_alpha=self.loss_cls.alpha, cls_weight=self.loss_cls.loss_weight,
                                   bbox_weight=wb, ctr_weight=self.loss_centerness.loss_weight)

    def effective_soft_weight(self, batch_size):
        """fcos_head.py:312-327: the sisoft term exists for odd batches with soft_weight != 0; while
        cur_iter <= soft_warm_up it is scaled by 1/1000 and the counter advances."""
        if batch_size % 2 == 0 or self.soft_weight == 0.0:
            return 0.0
        w = self.soft_weight * 1.0
        if self.soft_warm_up >= self.cur_iter:
            self.cur_iter += 1
            w = self.soft_weight / 1000.0
        return w


def _cfg_get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, 'get') else getattr(cfg, key, default)


def _square_anchor_scale(anchor_generator):
    """octave_base_scale of the one square anchor per location that ATSSHead / GFLHead are built for (anchor_generator.py:99-143)."""
    ag = dict(anchor_generator)
    _expect(ag.pop('type', None) == 'AnchorGenerator', "anchor_generator type='AnchorGenerator'")
    _expect(list(ag.pop('ratios', [])) == [1.0], 'anchor_generator ratios=[1.0] (one square anchor per location)')
    _expect(ag.pop('scales_per_octave', None) == 1 and ag.get('scales') is None, 'anchor_generator scales_per_octave=1 (no scales list)')
    obs = ag.pop('octave_base_scale', None)
    _expect(isinstance(obs, (int, float)) and 0.0 < float(obs) < float('inf'), f'anchor_generator octave_base_scale > 0 (got {obs!r})')
    _expect(list(ag.pop('strides', [])) == [8, 16, 32, 64, 128], 'anchor_generator strides 8..128')
    _expect(float(ag.pop('center_offset', 0.0)) == 0.0, 'anchor_generator center_offset=0')
    ag.pop('scales', None)
    _expect(ag.pop('base_sizes', None) is None and ag.pop('centers', None) is None and ag.pop('scale_major', True),
            'anchor_generator default base_sizes / centers / scale_major')
    _expect(not ag, f'anchor_generator: unknown arguments {sorted(ag)}')
    return float(obs)


def _assigner_value(train_cfg, type_name, own, default):
    """What `own` reads out of train_cfg.assigner, an assigner of `type_name` (`default` without a train_cfg): own(asg) takes the
    assigner's own arguments off the dict, refusing what the assignment kernel does not build; what is left of the dict, and of
    train_cfg, is checked here."""
    if train_cfg is None:
        return default
    asg = dict(_cfg_get(train_cfg, 'assigner') or {})
    _expect(asg.pop('type', None) == type_name, f"train_cfg.assigner type='{type_name}'")
    value = own(asg)
    ic = asg.pop('iou_calculator', dict(type='BboxOverlaps2D'))
    _expect(dict(ic) == dict(type='BboxOverlaps2D'), 'train_cfg.assigner iou_calculator BboxOverlaps2D')
    _expect(not asg, f'train_cfg.assigner: unknown arguments {sorted(asg)}')
    _expect(_cfg_get(train_cfg, 'allowed_border', -1) == -1, 'train_cfg.allowed_border=-1')
    _expect(_cfg_get(train_cfg, 'pos_weight', -1) <= 0, 'train_cfg.pos_weight=-1')
    return value


def _atss_assigner(asg):
    """topk of an ATSSAssigner (9 without a train_cfg), with the refusals of what dsl_atss_assign does not build."""
    topk = asg.pop('topk', None)
    _expect(isinstance(topk, int) and 1 <= topk <= 16, f'train_cfg.assigner topk in 1..16 (got {topk!r})')
    _expect(float(asg.pop('ignore_iof_thr', -1)) <= 0, 'train_cfg.assigner ignore_iof_thr <= 0 (gt_bboxes_ignore is not read)')
    return topk


def _max_iou_assigner(asg):
    """pos_iou_thr of a MaxIoUAssigner as configs/paa sets it (0.1 without a train_cfg), with the refusals of what dsl_paa_assign does
    not build (max_iou_assigner.py:43-62: every other argument at its default)."""
    thr, neg = asg.pop('pos_iou_thr', None), asg.pop('neg_iou_thr', None)
    _expect(isinstance(thr, (int, float)) and not isinstance(thr, bool) and 0.0 < float(thr) < 1.0,
            f'train_cfg.assigner pos_iou_thr in (0, 1) (got {thr!r})')
    _expect(isinstance(neg, (int, float)) and float(neg) == float(thr), f'train_cfg.assigner neg_iou_thr == pos_iou_thr (got {neg!r})')
    _expect(float(asg.pop('min_pos_iou', 0.0)) == 0.0, 'train_cfg.assigner min_pos_iou=0')
    _expect(float(asg.pop('ignore_iof_thr', -1)) == -1.0, 'train_cfg.assigner ignore_iof_thr=-1 (gt_bboxes_ignore is not read)')
    _expect(asg.pop('gt_max_assign_all', True) is True, 'train_cfg.assigner gt_max_assign_all=True')
    _expect(asg.pop('ignore_wrt_candidates', True) is True, 'train_cfg.assigner ignore_wrt_candidates=True')
    _expect(asg.pop('match_low_quality', True) is True, 'train_cfg.assigner match_low_quality=True')
    _expect(float(asg.pop('gpu_assign_thr', -1)) <= 0, 'train_cfg.assigner gpu_assign_thr=-1')
    return float(thr)


@HEADS.register_module()
class ATSSHead(DenseHead):
    """mmdet/models/dense_heads/atss_head.py:14-684 on AnchorHead (anchor_head.py:36-100): the FCOS network (GN-32 towers without
    conv bias, class predictor, box predictor with centerness on the regression tower, one Scale per level) with ATSSAssigner's
    targets (dsl_atss_assign) and DeltaXYWHBBoxCoder boxes against one square anchor per location (DSL_HEAD_ATSS).  The signature
    is the reference's; what the kernels do not build is refused, naming the option."""
    REG_DECODED_BBOX = False      # (PAAHead: True - its loss works on decoded boxes)

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), init_cfg=None,
                 feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', scales=[8, 16, 32], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True, target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), train_cfg=None, test_cfg=None, **kw):
        super().__init__(num_classes, train_cfg, test_cfg)
        _expect_no_dsl_keys(type(self).__name__, kw)
        _expect_towers(in_channels, feat_channels, stacked_convs, norm_cfg, conv_cfg is None)
        _expect(bool(reg_decoded_bbox) == self.REG_DECODED_BBOX, f'reg_decoded_bbox={self.REG_DECODED_BBOX}')
        obs = _square_anchor_scale(anchor_generator)
        bc = dict(bbox_coder)
        _expect(bc.pop('type', None) == 'DeltaXYWHBBoxCoder', "bbox_coder type='DeltaXYWHBBoxCoder'")
        _expect(all(float(v) == 0.0 for v in bc.pop('target_means', (0., 0., 0., 0.))), 'bbox_coder target_means all 0')
        stds = tuple(float(v) for v in bc.pop('target_stds', (1., 1., 1., 1.)))
        _expect(len(stds) == 4 and all(0.0 < v < float('inf') for v in stds), f'bbox_coder target_stds: four numbers > 0 (got {stds})')
        _expect(bc.pop('clip_border', True) and not bc.pop('add_ctr_clamp', False), 'bbox_coder clip_border=True, add_ctr_clamp=False')
        bc.pop('ctr_clamp', None)
        _expect(not bc, f'bbox_coder: unknown arguments {sorted(bc)}')
        assigner_kw = self._assigner_options(train_cfg)
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox, self.bbox_weight = _build_loss_bbox(loss_bbox, _FCOS_LOSSES)
        self.loss_centerness = build_loss(loss_centerness)
        _expect(isinstance(self.loss_cls, FocalLoss) and isinstance(self.loss_centerness, CrossEntropyLoss), _FCOS_LOSSES)
        self.options = HeadOptions(**_atss_option_kw(self), anchor_scale=obs, focal_gamma=self.loss_cls.gamma,
                                   focal_alpha=self.loss_cls.alpha, ctr_weight=self.loss_centerness.loss_weight, delta_stds=stds,
                                   **assigner_kw)

    def _assigner_options(self, train_cfg):
        """The HeadOptions keywords that train_cfg and the subclass's own arguments decide."""
        return dict(atss_topk=_assigner_value(train_cfg, 'ATSSAssigner', _atss_assigner, 9))


@HEADS.register_module()
class PAAHead(ATSSHead):
    """mmdet/models/dense_heads/paa_head.py:44-673: ATSSHead's network, parameters, anchors and box decode - the centerness predictor
    is the IoU-prediction branch - with MaxIoUAssigner's candidates, their reassignment by a two-component Gaussian mixture of the
    candidates' losses per ground-truth box (sklearn's GaussianMixture restated in the kernel), an IoU-weighted box loss
    (dsl_paa_assign / _pos_loss / _reassign / _loss, DSL_HEAD_PAA), and at test time the sqrt(cls * iou) score with score voting.
    The signature is the reference's; what the kernels do not build is refused, naming the option."""
    REG_DECODED_BBOX = True

    def __init__(self, *args, topk=9, score_voting=True, covariance_type='diag', **kwargs):
        _expect(isinstance(topk, int) and not isinstance(topk, bool) and 1 <= topk <= 16, f'topk in 1..16 (got {topk!r})')
        _expect(covariance_type == 'diag', f"covariance_type='diag' (got {covariance_type!r})")
        self.topk, self.with_score_voting, self.covariance_type = topk, bool(score_voting), covariance_type
        super().__init__(*args, **kwargs)

    def _assigner_options(self, train_cfg):
        return dict(head_kind='paa', atss_topk=self.topk, pos_iou_thr=_assigner_value(train_cfg, 'MaxIoUAssigner', _max_iou_assigner, 0.1),
                    score_voting=self.with_score_voting)


@HEADS.register_module()
class GFLHead(DenseHead):
    """mmdet/models/dense_heads/gfl_head.py:50-647 on AnchorHead: ATSSHead's network and targets (dsl_atss_assign, one square anchor
    per location) without centerness, a box predictor of 4 (reg_max + 1) distribution logits decoded by the Integral layer, Quality
    Focal Loss, a box loss and Distribution Focal Loss weighted by the location's best class score (dsl_gfl_quality, dsl_gfl_loss,
    DSL_HEAD_GFL).  The signature is the reference's; what the kernels do not build is refused, naming the option."""

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25), reg_max=16, init_cfg=None, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', scales=[8, 16, 32], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                 bbox_coder=None, reg_decoded_bbox=False, loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), train_cfg=None, test_cfg=None, **kw):
        super().__init__(num_classes, train_cfg, test_cfg)
        _expect_no_dsl_keys('GFLHead', kw)
        _expect_towers(in_channels, feat_channels, stacked_convs, norm_cfg, conv_cfg is None)
        _expect(not reg_decoded_bbox, 'reg_decoded_bbox=False')
        _expect(isinstance(reg_max, int) and not isinstance(reg_max, bool) and 1 <= reg_max <= 16,
                f'reg_max in 1..16 (got {reg_max!r}; DSL_GFL_MAX_REG)')
        obs = _square_anchor_scale(anchor_generator)
        # (the reference's GFLHead never calls its bbox_coder: boxes are distances from the anchor centre)
        _expect(bbox_coder is None or dict(bbox_coder).get('type') == 'DeltaXYWHBBoxCoder', "bbox_coder: AnchorHead's DeltaXYWHBBoxCoder or none")
        topk = _assigner_value(train_cfg, 'ATSSAssigner', _atss_assigner, 9)
        self.reg_max = reg_max
        self.loss_cls, self.loss_dfl = build_loss(loss_cls), build_loss(loss_dfl)
        _expect(isinstance(self.loss_cls, QualityFocalLoss), 'loss_cls: QualityFocalLoss(use_sigmoid=True, beta, loss_weight)')
        _expect(isinstance(self.loss_dfl, DistributionFocalLoss), 'loss_dfl: DistributionFocalLoss(loss_weight)')
        self.loss_bbox, self.bbox_weight = _build_loss_bbox(loss_bbox, 'loss_bbox: GIoULoss, IoULoss, DIoULoss or CIoULoss')
        self.options = self._gfl_options(topk, obs)

    def _gfl_options(self, atss_topk, anchor_scale, **ld):
        """The head's HeadOptions; `ld`: the keywords of LDHead's loss term."""
        return HeadOptions(**_atss_option_kw(self), atss_topk=atss_topk, anchor_scale=anchor_scale, head_kind='gfl', reg_max=self.reg_max,
                           qfl_beta=self.loss_cls.beta, dfl_weight=self.loss_dfl.loss_weight, **ld)


@HEADS.register_module()
class LDHead(GFLHead):
    """mmdet/models/dense_heads/ld_head.py:10-261: GFLHead with one more loss term, loss_ld = KnowledgeDistillationKLDivLoss between the
    box distributions of a frozen teacher and the student's over the positives (dsl_ld_loss, DSL_HEAD_LD).  No new parameter; whatever
    GFLHead refuses stays refused.  (The reference's own default names a loss type it does not register; its configs give this one.)"""

    def __init__(self, num_classes, in_channels, loss_ld=dict(type='KnowledgeDistillationKLDivLoss', loss_weight=0.25, T=10), **kwargs):
        super().__init__(num_classes, in_channels, **kwargs)
        self.loss_ld = build_loss(loss_ld)
        _expect(isinstance(self.loss_ld, KnowledgeDistillationKLDivLoss), 'loss_ld: KnowledgeDistillationKLDivLoss(loss_weight, T)')
        gfl = self.options
        self.options = self._gfl_options(gfl.atss_topk, gfl.anchor_scale, ld_weight=self.loss_ld.loss_weight, ld_T=self.loss_ld.T)


@HEADS.register_module()
class FoveaHead(DenseHead):
    """mmdet/models/dense_heads/fovea_head.py:50-348 on AnchorFreeHead (anchor_free_head.py:40-133): FCOSHead's towers and predictor
    geometry without centerness and without Scale; painted-rectangle targets (dsl_fovea_assign), focal + SmoothL1 loss on log
    distances in units of base_edge_list (dsl_fovea_loss), base_len * exp decode clamped to img_shape - 1 (DSL_HEAD_FOVEA).  The
    signature is the reference's; what the kernels do not build is refused, naming the option."""

    def __init__(self, num_classes, in_channels, base_edge_list=(16, 32, 64, 128, 256),
                 scale_ranges=((8, 32), (16, 64), (32, 128), (64, 256), (128, 512)), sigma=0.4, with_deform=False, deform_groups=4,
                 init_cfg=None, feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64), dcn_on_last_conv=False, conv_bias='auto',
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0), conv_cfg=None, norm_cfg=None, train_cfg=None, test_cfg=None, **kw):
        super().__init__(num_classes, train_cfg, test_cfg, strides)
        _expect_no_dsl_keys('FoveaHead', kw)
        _expect(not with_deform, 'with_deform=False (FeatureAlign is a deformable convolution)')
        _expect_towers(in_channels, feat_channels, stacked_convs, norm_cfg, conv_cfg is None and not dcn_on_last_conv)
        _expect(conv_bias is True or conv_bias is False or conv_bias == 'auto', "conv_bias True, False or 'auto'")
        self.conv_bias = conv_bias is True          # (mmcv ConvModule: 'auto' = no bias in front of the GroupNorm)
        self.base_edge_list, self.scale_ranges, self.sigma = tuple(base_edge_list), tuple(tuple(r) for r in scale_ranges), sigma
        self.with_deform, self.deform_groups = False, deform_groups
        self.loss_cls, self.loss_bbox = build_loss(loss_cls), build_loss(loss_bbox)
        _expect(isinstance(self.loss_cls, FocalLoss), 'loss_cls: FocalLoss(use_sigmoid=True, gamma, alpha, loss_weight)')
        _expect(isinstance(self.loss_bbox, SmoothL1Loss), 'loss_bbox: SmoothL1Loss(beta, loss_weight)')
        self.options = HeadOptions(head_kind='fovea', sigma=sigma, base_edge_list=self.base_edge_list, scale_ranges=self.scale_ranges,
                                   smooth_l1_beta=self.loss_bbox.beta, conv_bias=self.conv_bias, focal_gamma=self.loss_cls.gamma,
                                   focal_alpha=self.loss_cls.alpha, cls_weight=self.loss_cls.loss_weight,
                                   bbox_weight=self.loss_bbox.loss_weight)


@HEADS.register_module()
class AutoAssignHead(DenseHead):
    """mmdet/models/dense_heads/autoassign_head.py:123-509 on FCOSHead: FCOS's towers (conv_bias=True forced, :151), predictors, Scale
    layers, strides and get_bboxes; points without the half-stride offset, bbox = relu(scale x) s in training and in test, and no
    hard assigner - the positive / negative / centre-prior losses over every location inside a box (dsl_aa_assign, dsl_aa_loss,
    DSL_HEAD_AUTOASSIGN).  The signature is the reference's; what the kernels do not build is refused, naming the option."""

    def __init__(self, num_classes, in_channels, force_topk=False, topk=9, pos_loss_weight=0.25, neg_loss_weight=0.75,
                 center_loss_weight=0.75, regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8)),
                 center_sampling=False, center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False,
                 feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64), dcn_on_last_conv=False, conv_cfg=None,
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), train_cfg=None, test_cfg=None, init_cfg=None, **kw):
        _expect('conv_bias' not in kw, 'AutoAssignHead: no conv_bias argument (the head passes conv_bias=True itself, autoassign_head.py:151)')
        _expect_no_dsl_keys('AutoAssignHead', kw)
        super().__init__(num_classes, train_cfg, test_cfg, strides)
        _expect(not force_topk, 'force_topk=False (the top-k centre prior of boxes that hold no point is not built; topk is then unread)')
        _expect_towers(in_channels, feat_channels, stacked_convs, norm_cfg, conv_cfg is None and not dcn_on_last_conv, anchor_head=False)
        # FCOSHead arguments that AutoAssignHead's own forward_single, get_targets and loss never read (:189-212, :314-509): the
        # class defaults only - a config that sets them expects a behaviour the head does not have
        _expect(not center_sampling and not norm_on_bbox and not centerness_on_reg,
                'center_sampling / norm_on_bbox / centerness_on_reg at their defaults (AutoAssignHead does not read them)')
        self.force_topk, self.topk = False, topk
        # loss_cls and loss_centerness are built by FCOSHead.__init__ and never called (:402-417: the head forms its own terms)
        self.loss_cls, self.loss_centerness = build_loss(loss_cls), build_loss(loss_centerness)
        self.loss_bbox, self.bbox_weight = _build_loss_bbox(loss_bbox, 'loss_bbox: GIoULoss(loss_weight)')
        _expect(isinstance(self.loss_bbox, GIoULoss), 'loss_bbox: GIoULoss(loss_weight)')
        self.options = HeadOptions(head_kind='autoassign', bbox_weight=self.bbox_weight, pos_loss_weight=pos_loss_weight,
                                   neg_loss_weight=neg_loss_weight, center_loss_weight=center_loss_weight)
        self.pos_loss_weight, self.neg_loss_weight, self.center_loss_weight = (
            self.options.pos_loss_weight, self.options.neg_loss_weight, self.options.center_loss_weight)

"""Parameter storage for the FCOS R50-caffe + FPN + FCOSHead detector, laid out for the HIP kernels.

The reference keeps 377 separate OIHW fp32 tensors.  Here every trainable
parameter lives in ONE flat fp32 buffer (`train`), with conv weights stored KRSC =
[Cout][kh][kw][Cin] so that
  * the weight-gradient kernel writes straight into the matching flat `grad` buffer,
  * SGD / EMA / gradient all-reduce are single passes over flat memory,
  * the bf16 forward pack is an element-wise cast of the same buffer (`train16`).
`state_dict()` keys, shapes and dtypes are exactly the reference's: each entry is a (permuted) view
into the flat buffers, so checkpoints and the EMA hook interoperate.

Frozen tensors (stem, layer1, every BatchNorm) live in a second flat buffer (`frozen`).
"""
import inspect
import math
from collections import namedtuple

import torch

from . import _lib as L

STAGE_BLOCKS = (3, 4, 6, 3)
STAGE_PLANES = (64, 128, 256, 512)


def _round_up(x, m):
    return (x + m - 1) // m * m


class ConvSpec:
    def __init__(self, name, cin, cout, k, stride, pad, bn=None, bias=False, trainable=True, cin_store=None, bn_train=False,
                 stage=None, no_dgrad=False):
        """cin_store: input channels of the STORED weight rows (>= cin; the extra columns are zero and stay zero: their
        inputs are zero padding) - RLA's conv1 reads cat(x, h) from one [C + 128]-wide buffer.  bn_train: the BatchNorm
        behind the conv runs in eval mode but its affine parameters train (RLA_ResNet).  stage: backward segment
        (0..3 = backbone stages) the gradients belong to."""
        self.name, self.cin, self.cout, self.k, self.stride, self.pad = name, cin, cout, k, stride, pad
        self.bn, self.bias, self.trainable = bn, bias, trainable
        self.cout_pad = _round_up(cout, 64)
        self.cin_store = cin_store or cin
        self.bn_train = bn_train and trainable
        self.stage, self.no_dgrad = stage, no_dgrad


def backbone_specs():
    """ResNet-50, caffe style, frozen_stages=1, BN frozen (mmdet/models/backbones/resnet.py:304-656)."""
    specs = [ConvSpec('backbone.conv1', 3, 64, 7, 2, 3, bn='backbone.bn1', trainable=False)]
    inpl = 64
    for li, (planes, blocks) in enumerate(zip(STAGE_PLANES, STAGE_BLOCKS)):
        tr = li >= 1
        for b in range(blocks):
            p = f'backbone.layer{li + 1}.{b}'
            s = 2 if (b == 0 and li > 0) else 1      # caffe: stride on the first 1x1 (resnet.py:153-158)
            specs.append(ConvSpec(p + '.conv1', inpl, planes, 1, s, 0, bn=p + '.bn1', trainable=tr))
            specs.append(ConvSpec(p + '.conv2', planes, planes, 3, 1, 1, bn=p + '.bn2', trainable=tr))
            specs.append(ConvSpec(p + '.conv3', planes, planes * 4, 1, 1, 0, bn=p + '.bn3', trainable=tr))
            if b == 0:
                specs.append(ConvSpec(p + '.downsample.0', inpl, planes * 4, 1, s, 0, bn=p + '.downsample.1',
                                      trainable=tr))
            inpl = planes * 4
    return specs


RLA_C = 32          # channels of the recurrent state h (resnet_rla.py: rla_channel)
RLA_PAD = 128       # cat(x, h) is stored [x | h | zeros] with C + RLA_PAD channels (multiple of the 128-channel wgrad tile)


def rla_backbone_specs():
    """RLA_ResNet (mmdet/models/backbones/resnet_rla.py:140-287), layers [3, 4, 6, 3], style 'pytorch' (the 3x3 strides),
    frozen_stages=1: stem, stage 0 and its RLA layers frozen; the BatchNorms of stages 1-3 keep trainable affine parameters
    (eval-mode statistics).  Names are the reference's module names."""
    specs = [ConvSpec('backbone.conv1', 3, 64, 7, 2, 3, bn='backbone.bn1', trainable=False)]
    inpl = 64
    for s_, (planes, blocks) in enumerate(zip(STAGE_PLANES, STAGE_BLOCKS)):
        tr = s_ >= 1
        for b in range(blocks):
            p = f'backbone.stages.{s_}.{b}'
            st = 2 if (b == 0 and s_ > 0) else 1
            first_trainable = tr and s_ == 1 and b == 0        # fed by the frozen stage 0: no data gradient needed
            specs.append(ConvSpec(p + '.conv1', inpl + RLA_C, planes, 1, 1, 0, bn=p + '.bn1', trainable=tr, bn_train=True,
                                  cin_store=inpl + RLA_PAD, stage=s_, no_dgrad=first_trainable))
            specs.append(ConvSpec(p + '.conv2', planes, planes, 3, st, 1, bn=p + '.bn2', trainable=tr, bn_train=True, stage=s_))
            specs.append(ConvSpec(p + '.conv3', planes, planes * 4, 1, 1, 0, bn=p + '.bn3', trainable=tr, bn_train=True, stage=s_))
            if b == 0:
                specs.append(ConvSpec(p + '.downsample.0', inpl, planes * 4, 1, st, 0, bn=p + '.downsample.1', trainable=tr,
                                      bn_train=True, stage=s_, no_dgrad=first_trainable))
            inpl = planes * 4
        # the stage's shared RLA convolutions: conv_out 1x1 (4*planes -> 32), recurrent 3x3 (32 -> 32, stored 64 -> 32 over a
        # zero-padded source)
        specs.append(ConvSpec(f'backbone.conv_outs.{s_}', planes * 4, RLA_C, 1, 1, 0, trainable=tr, stage=s_))
        # (stored 128 wide where it trains: the weight-gradient kernel tiles input channels by 128)
        specs.append(ConvSpec(f'backbone.recurrent_convs.{s_}', RLA_C, RLA_C, 3, 1, 1, trainable=tr, cin_store=128 if tr else 64,
                              stage=s_))
    return specs


def rla_stage_bns():
    """(name, trainable) of the per-block BatchNorm(32) layers on the recurrent path (stage_bns, resnet_rla.py:236,283);
    stage_bns.3.2 is frozen by _freeze_stages (:364-366)."""
    return [(f'backbone.stage_bns.{s_}.{b}', s_ >= 1 and not (s_ == 3 and b == 2))
            for s_, blocks in enumerate(STAGE_BLOCKS) for b in range(blocks)]


def neck_specs():
    specs = [ConvSpec(f'neck.lateral_convs.{i}.conv', c, 256, 1, 1, 0, bias=True)
             for i, c in enumerate((512, 1024, 2048))]
    specs += [ConvSpec(f'neck.fpn_convs.{i}.conv', 256, 256, 3, 1 if i < 3 else 2, 1, bias=True) for i in range(5)]
    return specs


MAX_LEVELS = 5       # DSL_MAX_SEG: the FPN levels of a head
MAX_CLASSES = 128    # the classification predictor is stored round_up(C, 64) rows wide: one or two 64-row weight tiles


def class_layout(num_classes):
    """(cp, c4) of a C-class head: the classification predictor's stored rows / gradient columns (round_up(C, 64)) and the
    row stride of its fp32 logits (round_up(C, 4), the loss / detection kernels' 4-class groups).  80 classes: (128, 80)."""
    if not (isinstance(num_classes, int) and 1 <= num_classes <= MAX_CLASSES):
        raise NotImplementedError(f'dsl_amd hot path: num_classes must be in 1..{MAX_CLASSES}, got {num_classes!r}')
    return _round_up(num_classes, 64), _round_up(num_classes, 4)


_ATSS_FIELDS = ('assigner', 'atss_topk', 'anchor_scale', 'delta_stds')
_GFL_FIELDS = ('head_kind', 'reg_max', 'qfl_beta', 'dfl_weight')
_F32, _I32 = torch.float32, torch.int32

# What the dense heads differ in, one immutable record per kind (HeadOptions.kind); every site that serves a head reads its record:
#   flags        kind flags of head_flags, beside the option flags.  A dsl_gfl_desc / dsl_paa_desc always carries the loss family
#                (HEAD_LOSS_EXT: dsl_gfl_loss reads w_cls / w_bbox / box_kind with no default to fall back to)
#   atss         the ATSS layout is forced (assigner='atss', towers without bias, ...); a dsl_atss_desc is attached, set_targets needs
#                pad_shapes and does not read ignore boxes
#   fields       the kind's options, in key() / repr order behind FIELDS [+ LOSS_FIELDS]
#   loss_desc    FcosLossPlan: the outermost ctypes struct, then the plan attributes that hold it and each wrapper nested in it as
#                first member; the dsl_fcos_desc (`desc`) is member `fcos` of the last (of the struct itself where none is named)
#   scalars      (plan attribute, descriptor field, option) set in those structs
#   buffers      (name, dtype, length attribute, fill): a plan attribute and the like-named pointer of the innermost wrapper
#   det_desc     DetectPlan: the outermost ctypes struct, then the member path to its dsl_det_desc (`desc`); the struct that holds
#                the last member holds the dsl_atss_desc pointer, set where det_mask has HEAD_ATSS
#   det_mask     dsl_det_desc.head_flags = flags() & det_mask;  det_fields: (field of the outermost struct, option)
#   dist_reg     the box predictor emits 4 (reg_max + 1) distribution logits, fp32 rows as wide; otherwise 4 (+ centerness) rows, 8 wide
#   names        module names of the class / box / centerness predictors under bbox_head
#   middle       the pass between the predictors and the loss: (op kind, direct calls, all on the innermost wrapper), or None
#   loss_entry   what FcosLossPlan.loss() calls;  loss_keys: forward_train's dict [+ loss_sisoft where `sisoft` and the
#                step's soft weight is not 0]; logvec holds them [+ loss_sisoft] + the sum
#   exchange     of stats[0:2] between ranks: 'forward' = issued behind the assignment, under the forward pass; 'middle' = behind the
#                middle pass and waited for (a GFL head's second normaliser, the sum of the positives' best class scores, exists only
#                behind the predictors, gfl_head.py:348-366); None = none, and inv_world = 1 (a PAA head normalises by this rank's own
#                stats: the reference does not reduce_mean there, paa_head.py:173-193)
#   aug_refusal  aug_test raises this
# A new head adds a record here and its kernels, a row of NOT_READ / CHECKED below for its options, a head class on heads.DenseHead and
# a two-line detector ("Head kinds").  (The records' fields are pinned by tests/test_fovea_cpu.py; what no field says - a head
# without Scale layers - HeadOptions.has_scale() reads from `flags`.)
HeadKind = namedtuple('HeadKind', 'name flags atss fields loss_desc scalars buffers det_desc det_mask det_fields dist_reg names middle '
                                  'loss_entry loss_keys sisoft exchange aug_refusal')
_FCOS = HeadKind(
    name='fcos', flags=0, atss=False, fields=(),
    loss_desc=('FcosDesc',), scalars=(), buffers=(),
    det_desc=('DetDesc',), det_mask=L.HEAD_EXP_DECODE, det_fields=(),
    dist_reg=False, names=('conv_cls', 'conv_reg', 'conv_centerness'),
    middle=None, loss_entry='dsl_fcos_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_centerness'), sisoft=True,
    exchange='forward', aug_refusal=None)
_ATSS = _FCOS._replace(
    name='atss', flags=L.HEAD_ATSS, atss=True, fields=_ATSS_FIELDS,
    det_desc=('DetAtssDesc', 'det'), det_mask=L.HEAD_EXP_DECODE | L.HEAD_ATSS,
    names=('atss_cls', 'atss_reg', 'atss_centerness'))      # (atss_head.py:83-91)
_GFL = _ATSS._replace(
    name='gfl', flags=L.HEAD_ATSS | L.HEAD_GFL | L.HEAD_LOSS_EXT, fields=_ATSS_FIELDS + _GFL_FIELDS,
    loss_desc=('GflDesc', 'gfl'),
    scalars=(('gfl', 'reg_max', 'reg_max'), ('gfl', 'qfl_beta', 'qfl_beta'), ('gfl', 'w_dfl', 'dfl_weight')),
    buffers=(('score', _F32, 'M', 0), ('weight', _F32, 'M', 0)),
    det_desc=('DetGflDesc', 'det'), det_mask=L.HEAD_GFL, det_fields=(('reg_max', 'reg_max'),),
    dist_reg=True, names=('gfl_cls', 'gfl_reg', None),      # (gfl_head.py:128-133: no centerness predictor)
    middle=(L.OP_GFL_QUALITY, ('dsl_gfl_quality',)), loss_entry='dsl_gfl_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_dfl'),
    sisoft=False, exchange='middle')
_LD = _GFL._replace(
    name='ld', flags=_GFL.flags | L.HEAD_LD, fields=_GFL.fields + ('ld_weight', 'ld_T'),
    loss_desc=('LdDesc', 'ld', 'gfl'), scalars=_GFL.scalars + (('ld', 'T', 'ld_T'), ('ld', 'w_ld', 'ld_weight')),
    loss_entry='dsl_ld_loss', loss_keys=_GFL.loss_keys + ('loss_ld',))
_PAA = _ATSS._replace(
    name='paa', flags=L.HEAD_ATSS | L.HEAD_PAA | L.HEAD_LOSS_EXT, fields=_ATSS_FIELDS + ('head_kind', 'pos_iou_thr', 'score_voting'),
    loss_desc=('PaaDesc', 'paa'), scalars=(('paa', 'pos_iou_thr', 'pos_iou_thr'),),
    buffers=(('pos_loss', _F32, 'M', 0), ('iou_target', _F32, 'M', 0), ('cand_gt', _I32, 'M', -1),
             ('gmm_iters', _I32, 'max_gt', 0), ('gmm_flags', _I32, 'max_gt', 0)),
    det_desc=('DetPaaDesc', 'atss', 'det'), det_mask=L.HEAD_EXP_DECODE | L.HEAD_ATSS | L.HEAD_PAA,
    det_fields=(('score_voting', 'score_voting'),),
    middle=(L.OP_PAA_REFINE, ('dsl_paa_pos_loss', 'dsl_paa_reassign')), loss_entry='dsl_paa_loss',
    loss_keys=('loss_cls', 'loss_bbox', 'loss_iou'), sisoft=False, exchange=None,
    aug_refusal='PAAHead does not support test-time augmentation (aug_test): PAA only supports with_nms=True (paa_head.py:536-538)')
# FoveaHead (fovea_head.py): an anchor-free head like FCOS's - same towers, strides and predictor geometry - without centerness and
# without Scale; painted-rectangle targets, focal + SmoothL1 loss, base_len * exp decode.  No reduce_mean: this rank's own normalisers
_FOVEA_FIELDS = ('head_kind', 'sigma', 'base_edge_list', 'scale_ranges', 'smooth_l1_beta')
_FOVEA = _FCOS._replace(
    name='fovea', flags=L.HEAD_FOVEA | L.HEAD_LOSS_EXT, fields=_FOVEA_FIELDS,
    loss_desc=('FoveaDesc', 'fovea'),
    scalars=(('fovea', 'sigma', 'sigma'), ('fovea', 'base_len', 'base_edge_list'), ('fovea', 'lo', 'range_lo'), ('fovea', 'hi', 'range_hi'),
             ('fovea', 'smooth_l1_beta', 'smooth_l1_beta')),
    det_desc=('DetFoveaDesc', 'det'), det_mask=L.HEAD_FOVEA, det_fields=(('base_len', 'base_edge_list'),),
    names=('conv_cls', 'conv_reg', None),      # (fovea_head.py:77-86: no centerness predictor)
    loss_entry='dsl_fovea_loss', loss_keys=('loss_cls', 'loss_bbox'), sisoft=False, exchange=None,
    aug_refusal='FoveaHead does not support test-time augmentation (aug_test): FoveaHead.get_bboxes has no with_nms argument, so '
                'aug_test_bboxes asserts (dense_test_mixins.py:62-70)')
# AutoAssignHead (autoassign_head.py): FCOS's network - towers with bias, predictors, centerness (here: objectness) on the regression
# tower, Scale - with no hard assigner: the positive, negative and centre-prior losses of dsl_aa_loss.  Its two normalisers (boxes in
# the batch, sum of the centre prior) come out of the assignment stage, so they cross the ranks under the forward pass
_AA_FIELDS = ('head_kind', 'pos_loss_weight', 'neg_loss_weight', 'center_loss_weight')
_AA = _FCOS._replace(
    name='autoassign', flags=L.HEAD_AUTOASSIGN | L.HEAD_LOSS_EXT, fields=_AA_FIELDS,
    loss_desc=('AaDesc', 'aa'),
    scalars=(('aa', 'w_pos', 'pos_loss_weight'), ('aa', 'w_neg', 'neg_loss_weight'), ('aa', 'w_center', 'center_loss_weight')),
    buffers=(('iou', _F32, 'M', 0),),
    det_mask=L.HEAD_AUTOASSIGN,
    loss_entry='dsl_aa_loss', loss_keys=('loss_pos', 'loss_neg', 'loss_center'), sisoft=False, exchange='forward', aug_refusal=None)
HEAD_KINDS = {k.name: k for k in (_FCOS, _ATSS, _GFL, _LD, _PAA, _FOVEA, _AA)}

# What HeadOptions refuses off its default instead of dropping it - an option the head does not read, or fixes itself - per value of the
# head_kind option (the 'gfl' row serves the LD head too), each row a sum of the groups of options that belong to one head.
# Known gap, kept as it is: a row holds the groups of the heads that existed when its kind was added, and FCOS / ATSS / PAA heads have
# no row - a GFL head accepts sigma=1.5, a PAA head reg_max=0, an ATSS head smooth_l1_beta=0.0 (tests/golden/head_option_grid.txt
# has every case).  Closing it changes behaviour: a pull request of its own.
_FCOS_ONLY = ('center_sampling', 'norm_on_bbox', 'centerness_on_reg', 'iou_loss')
_FOCAL = ('focal_gamma', 'focal_alpha')
_GFL_ONLY = _GFL_FIELDS[1:] + ('ld_T',)      # (ld_weight has a refusal of its own)
_PAA_ONLY = ('pos_iou_thr', 'score_voting')
NOT_READ = {
    'gfl': _FCOS_ONLY + _FOCAL + ('ctr_weight',),
    'fovea': _FCOS_ONLY + ('box_loss', 'ctr_weight') + _ATSS_FIELDS + _GFL_ONLY + _PAA_ONLY,
    'autoassign': (_FCOS_ONLY + ('conv_bias', 'box_eps') + _FOCAL + ('cls_weight', 'ctr_weight') + _ATSS_FIELDS + _GFL_ONLY + _PAA_ONLY
                   + _FOVEA_FIELDS[1:]),
}


def _like_default(v, want):
    """v as it is compared with the default `want`: a sequence option as (nested) tuples, whatever sequences it came as."""
    return tuple(_like_default(x, want[0]) for x in v) if isinstance(want, tuple) else v


# Input validation: option -> (what it must be, test of the value as given), and CHECKED: resolved kind -> the options it tests, in
# order.  A test without a type check takes whatever float() / int() takes, and what they do not take raises their own error
# (pos_iou_thr: in front of the type check).
_INF = float('inf')
_GE0 = ('a finite number >= 0', lambda v: isinstance(v, (int, float)) and 0.0 <= float(v) < _INF)
_GE0_ANY = (_GE0[0], lambda v: 0.0 <= float(v) < _INF)
_GT0 = ('a finite number > 0', lambda v: isinstance(v, (int, float)) and 0.0 < float(v) < _INF)
CHECKS = {
    'ld_weight': _GE0, 'ld_T': ('a finite number >= 1', lambda v: isinstance(v, (int, float)) and 1.0 <= float(v) < _INF),
    'reg_max': (f'an integer in 1..{L.GFL_MAX_REG}', lambda v: isinstance(v, int) and 1 <= v <= L.GFL_MAX_REG),
    'qfl_beta': _GE0_ANY, 'dfl_weight': _GE0_ANY,
    'sigma': ('a number in (0, 1]', lambda v: isinstance(v, (int, float)) and 0.0 < float(v) <= 1.0), 'smooth_l1_beta': _GT0,
    'base_edge_list': (f'{MAX_LEVELS} finite numbers > 0', lambda v: len(v) == MAX_LEVELS and all(0.0 < float(x) < _INF for x in v)),
    'scale_ranges': (f'{MAX_LEVELS} pairs (lo, hi) with lo <= hi',
                     lambda v: len(v) == MAX_LEVELS and all(len(r) == 2 and float(r[0]) <= float(r[1]) for r in v)),
    'bbox_weight': _GE0, 'pos_loss_weight': _GE0, 'neg_loss_weight': _GE0, 'center_loss_weight': _GE0,
    'pos_iou_thr': ('a number in (0, 1)', lambda v: 0.0 < float(v) < 1.0 and isinstance(v, (int, float))),
    'atss_topk': (f'in 1..{L.ATSS_MAX_TOPK}', lambda v: 1 <= int(v) <= L.ATSS_MAX_TOPK),
    'anchor_scale': (_GT0[0], lambda v: 0.0 < float(v) < _INF),
    'delta_stds': ('four finite numbers > 0', lambda v: len(v) == 4 and all(0.0 < float(x) < _INF for x in v)),
}
_ATSS_CHECKED = ('atss_topk', 'anchor_scale', 'delta_stds')
CHECKED = {
    'fcos': (), 'atss': _ATSS_CHECKED, 'gfl': _GFL_FIELDS[1:] + _ATSS_CHECKED, 'ld': ('ld_weight', 'ld_T') + _GFL_FIELDS[1:] + _ATSS_CHECKED,
    'paa': ('pos_iou_thr',) + _ATSS_CHECKED, 'fovea': ('sigma', 'smooth_l1_beta', 'base_edge_list', 'scale_ranges'),
    'autoassign': ('bbox_weight',) + _AA_FIELDS[1:],
}


class HeadOptions:
    """The FCOSHead options that reach the kernels and the parameter layout, fixed per model (a ParamStore holds one; every plan
    of that store is built for it).  The defaults are the fcos_semi "tricks" head; configs/fcos/fcos_r50_caffe_fpn_gn-head_*.py
    turn all of them off:
      center_sampling    False: a location is positive for a box it lies inside of (fcos_head.py:676-678)
      norm_on_bbox       False: distances = exp(scale * x), targets in pixels (fcos_head.py:162-167, :618)
      centerness_on_reg  False: conv_centerness reads the classification tower (fcos_head.py:155-158)
      iou_loss           True: IoULoss, -log(clamp(iou, 1e-6)) (losses/iou_loss.py:14-36); False: GIoULoss
      conv_bias          False: the eight tower convolutions have no bias ('auto' in front of GroupNorm, mmcv ConvModule)
    The loss family (dsl_fcos_desc.box_kind .. w_ctr; a head with any of them off its default is not the default head):
      box_loss           None: GIoULoss / IoULoss as iou_loss says; 'giou', 'iou', 'iou_linear' (IoULoss(linear=True)), 'diou', 'ciou'
                         (losses/iou_loss.py:105-219); iou_loss then follows it (True for the two IoULoss kinds)
      box_eps            eps of DIoULoss / CIoULoss
      focal_gamma, focal_alpha                 FocalLoss (losses/focal_loss.py:11-56)
      cls_weight, bbox_weight, ctr_weight      loss_weight of loss_cls / loss_bbox / loss_centerness
    The assigner ('fcos'; 'atss' = ATSSHead, mmdet/models/dense_heads/atss_head.py, dsl_atss_desc of include/dsl_hip.h): an ATSS head has
    the parameter layout of centerness_on_reg=True, conv_bias=False - both are forced, as are the two FCOS assignment options, which it
    does not read - and the reference's predictor names (atss_cls, atss_reg, atss_centerness):
      atss_topk          ATSSAssigner(topk), 1..16
      anchor_scale       AnchorGenerator(octave_base_scale): the one square anchor of a location has side anchor_scale * stride
      delta_stds         DeltaXYWHBBoxCoder(target_stds); the means are 0
    The head kind ('fcos'; 'gfl' = GFLHead, mmdet/models/dense_heads/gfl_head.py, dsl_gfl_desc of include/dsl_hip.h): a GFL head is an
    ATSS head (assigner='atss' is forced, and with it conv_bias=False; anchor_scale and atss_topk count, delta_stds is not read; the FCOS
    options center_sampling / norm_on_bbox / centerness_on_reg / iou_loss and focal_gamma / focal_alpha / ctr_weight are refused off their defaults) without centerness, whose box
    predictor emits 4 (reg_max + 1) distribution logits - round_up(4 (reg_max + 1), 64) stored rows, fp32 rows 4 (reg_max + 1) wide - with
    the predictor names gfl_cls / gfl_reg.  focal_gamma, focal_alpha and ctr_weight are not read:
      reg_max            bins 0..reg_max per box side, 1..16 (the reference's configs use 16)
      qfl_beta           QualityFocalLoss(beta) >= 0 (losses/gfocal_loss.py:11-52)
      dfl_weight         DistributionFocalLoss(loss_weight) (losses/gfocal_loss.py:55-78)
    Localization Distillation (LDHead, mmdet/models/dense_heads/ld_head.py, dsl_ld_desc) is a GFL head with one more loss term against
    a frozen teacher's box distributions; the network and the parameter layout are GFL's:
      ld_weight          KnowledgeDistillationKLDivLoss(loss_weight) >= 0; None (default): no LD term, a plain GFL head
      ld_T               its temperature, finite and >= 1 (losses/kd_loss.py:50)
    Probabilistic anchor assignment (head_kind 'paa' = PAAHead, mmdet/models/dense_heads/paa_head.py, dsl_paa_desc): an ATSS head in
    network, parameter layout, decode and predictor names (assigner='atss' is forced; its centerness predictor is the IoU-prediction
    branch) whose targets come from MaxIoUAssigner and the Gaussian-mixture reassignment; atss_topk is PAAHead's per-level topk:
      pos_iou_thr        MaxIoUAssigner pos_iou_thr == neg_iou_thr, in (0, 1)
      score_voting       detection: score voting behind the NMS (paa_head.py:608-673)
    FoveaBox (head_kind 'fovea' = FoveaHead, mmdet/models/dense_heads/fovea_head.py, dsl_fovea_desc): an anchor-free head with FCOS's
    towers and predictor geometry, no centerness predictor and no Scale; conv_bias, focal_gamma / focal_alpha, cls_weight and bbox_weight
    count, every other FCOS / ATSS / GFL / PAA option is refused off its default:
      sigma              the fovea's share of a box, in (0, 1]
      base_edge_list     per level: the unit of the log distances, > 0
      scale_ranges       per level: (lo, hi) bounds of sqrt(box area), lo <= hi
      smooth_l1_beta     SmoothL1Loss(beta) > 0 (losses/smooth_l1_loss.py:11-29)
    AutoAssign (head_kind 'autoassign' = AutoAssignHead, mmdet/models/dense_heads/autoassign_head.py, dsl_aa_desc): FCOS's network with
    conv_bias=True forced (:151), points without the half-stride offset and a trained per-class centre prior (the parameter region
    head.center_prior: mean, then sigma, each [C][2]); bbox_weight counts (GIoULoss(loss_weight)), box_loss must be GIoU, every other
    FCOS / ATSS / GFL / PAA / Fovea option is refused off its default:
      pos_loss_weight, neg_loss_weight, center_loss_weight      finite and >= 0 (0.25, 0.75, 0.75)
    `kind` is the record of the resolved head kind (HEAD_KINDS above): what follows from "which head is this" is read there.  Which
    options a kind refuses off their defaults is NOT_READ above, which it validates CHECKED; DEFAULTS holds the signature's defaults."""
    FIELDS = ('center_sampling', 'norm_on_bbox', 'centerness_on_reg', 'iou_loss', 'conv_bias')
    LOSS_FIELDS = ('box_loss', 'box_eps', 'focal_gamma', 'focal_alpha', 'cls_weight', 'bbox_weight', 'ctr_weight')
    BOX_KINDS = dict(giou=L.BOX_GIOU, iou=L.BOX_IOU_LOG, iou_linear=L.BOX_IOU_LINEAR, diou=L.BOX_DIOU, ciou=L.BOX_CIOU)
    FLOATS = LOSS_FIELDS[1:] + ('anchor_scale', 'qfl_beta', 'dfl_weight', 'pos_iou_thr', 'sigma', 'smooth_l1_beta') + _AA_FIELDS[1:]      # stored as float

    def __init__(self, center_sampling=True, norm_on_bbox=True, centerness_on_reg=True, iou_loss=False, conv_bias=True,
                 box_loss=None, box_eps=1e-6, focal_gamma=2.0, focal_alpha=0.25, cls_weight=1.0, bbox_weight=1.0, ctr_weight=1.0,
                 assigner='fcos', atss_topk=9, anchor_scale=8.0, delta_stds=(0.1, 0.1, 0.2, 0.2),
                 head_kind='fcos', reg_max=16, qfl_beta=2.0, dfl_weight=0.25, ld_weight=None, ld_T=10.0, pos_iou_thr=0.1, score_voting=True,
                 sigma=0.4, base_edge_list=(16, 32, 64, 128, 256), scale_ranges=((8, 32), (16, 64), (32, 128), (64, 256), (128, 512)),
                 smooth_l1_beta=0.11, pos_loss_weight=0.25, neg_loss_weight=0.75, center_loss_weight=0.75):
        given = locals()      # the options by name, as given.  This signature is the one place a default is written: DEFAULTS below reads it
        if head_kind not in ('fcos', 'gfl', 'paa', 'fovea', 'autoassign'):
            raise NotImplementedError(f"dsl_amd hot path: head_kind must be 'fcos', 'gfl', 'paa', 'fovea' or 'autoassign', got {head_kind!r}")
        if assigner not in ('fcos', 'atss'):
            raise NotImplementedError(f"dsl_amd hot path: assigner must be 'fcos' or 'atss', got {assigner!r}")
        if ld_weight is not None and head_kind != 'gfl':
            raise NotImplementedError(f"dsl_amd hot path: ld_weight is an option of head_kind='gfl' (LDHead), got head_kind={head_kind!r}")
        # the resolved kind: ld_weight makes a GFL head an LD head, assigner='atss' an FCOS head an ATSS head
        self.kind = kind = HEAD_KINDS['ld' if ld_weight is not None else assigner if head_kind == 'fcos' else head_kind]
        for name in NOT_READ.get(head_kind, ()):
            want = self.DEFAULTS[name]
            val = _like_default(given[name], want)
            if val != want:
                raise NotImplementedError(f"dsl_amd hot path: head_kind='{head_kind}' does not read {name} (got {val!r}; leave it at {want!r})")
        if head_kind == 'autoassign' and box_loss not in (None, 'giou'):
            raise NotImplementedError(f"dsl_amd hot path: head_kind='autoassign' is built for box_loss='giou' (GIoULoss), got {box_loss!r}")
        for name in CHECKED[kind.name]:
            what, ok = CHECKS[name]
            if not ok(given[name]):
                raise NotImplementedError(f'dsl_amd hot path: {name} must be {what}, got {given[name]!r}')
        self.head_kind, self.reg_max, self.score_voting = head_kind, reg_max, bool(score_voting)
        for name in self.FLOATS:
            setattr(self, name, float(given[name]))
        # (without an LD term ld_T is not read: it stays at its default)
        self.ld_weight, self.ld_T = (None, self.DEFAULTS['ld_T']) if ld_weight is None else (float(ld_weight), float(ld_T))
        self.base_edge_list = tuple(float(v) for v in base_edge_list)
        self.scale_ranges = tuple((float(lo), float(hi)) for lo, hi in scale_ranges)
        self.range_lo, self.range_hi = tuple(r[0] for r in self.scale_ranges), tuple(r[1] for r in self.scale_ranges)
        # (the default 'fcos' stands for "not given": a GFL head's targets are ATSS's, a PAA head has the anchors, valid flags, decode
        # and parameter layout of an ATSS head)
        self.assigner = 'atss' if kind.atss else assigner
        self.atss_topk, self.delta_stds = int(atss_topk), tuple(float(v) for v in delta_stds)
        if kind.atss:
            center_sampling, norm_on_bbox, centerness_on_reg, conv_bias = True, True, True, False
        self.center_sampling, self.norm_on_bbox, self.centerness_on_reg = bool(center_sampling), bool(norm_on_bbox), bool(centerness_on_reg)
        self.conv_bias = bool(conv_bias)
        self.box_loss = box_loss if box_loss is not None else ('iou' if iou_loss else 'giou')
        if self.box_loss not in self.BOX_KINDS:
            raise NotImplementedError(f'dsl_amd hot path: box_loss must be one of {sorted(self.BOX_KINDS)}, got {box_loss!r}')
        self.iou_loss = self.box_loss in ('iou', 'iou_linear')

    DEFAULTS = {name: p.default for name, p in list(inspect.signature(__init__).parameters.items())[1:]}

    def loss_key(self):
        return tuple(getattr(self, f) for f in self.LOSS_FIELDS)

    def loss_is_default(self):
        """GIoU or the IoU log loss, focal gamma 2 / alpha 0.25, unit weights: what a descriptor without HEAD_LOSS_EXT computes
        (box_eps counts for DIoU / CIoU only)."""
        return all(getattr(self, f) == self.DEFAULTS[f] for f in self.LOSS_FIELDS[2:]) and self.box_loss in ('giou', 'iou')

    def key_fields(self):
        """The five FIELDS for every head that existed before the loss family; the loss settings follow only where one is set, then the
        kind's own options."""
        return (self.FIELDS if self.loss_is_default() else self.FIELDS + self.LOSS_FIELDS) + self.kind.fields

    def key(self):
        return tuple(getattr(self, f) for f in self.key_fields())

    def is_default(self):
        return self.key() == HeadOptions().key()

    def flags(self):
        """dsl_fcos_desc.head_flags / dsl_det_desc.head_flags."""
        return ((0 if self.center_sampling else L.HEAD_INSIDE_BOX) | (0 if self.norm_on_bbox else L.HEAD_RAW_TARGETS | L.HEAD_EXP_DECODE)
                | (L.HEAD_IOU_LOSS if self.box_loss == 'iou' else 0) | (0 if self.loss_is_default() else L.HEAD_LOSS_EXT) | self.kind.flags)

    def reg_layout(self):
        """(rows, fp32 row stride) of the box predictor: conv_reg (4) + conv_centerness (1, unless it sits on the classification
        predictor), rows 8 wide; a distribution head's 4 (reg_max + 1) logits, rows exactly that wide, no centerness."""
        if self.kind.dist_reg:
            return 4 * (self.reg_max + 1), 4 * (self.reg_max + 1)
        return 5 if self.centerness_on_reg and self.kind.names[2] else 4, 8

    def has_scale(self):
        """The head has a Scale per level (parameters bbox_head.scales.i.scale, read by the loss and detection kernels); a Fovea head
        uses conv_reg's outputs raw (fovea_head.py:117-128)."""
        return not self.kind.flags & L.HEAD_FOVEA

    def has_prior(self):
        """The head has AutoAssign's centre prior (parameters bbox_head.center_prior.mean / .sigma, region head.center_prior)."""
        return bool(self.kind.flags & L.HEAD_AUTOASSIGN)

    def atss_desc(self):
        """A dsl_atss_desc with the head's settings (None for an FCOS head); the caller fills max_gt, pad_shapes and npos."""
        if not self.kind.atss:
            return None
        a = L.AtssDesc()
        a.topk, a.anchor_scale = self.atss_topk, self.anchor_scale
        for i, v in enumerate(self.delta_stds):
            a.delta_stds[i] = v
        return a

    def fill_loss_desc(self, d):
        """The loss family's fields of a dsl_fcos_desc (read by the kernel with HEAD_LOSS_EXT only)."""
        d.box_kind, d.box_eps = self.BOX_KINDS[self.box_loss], self.box_eps
        d.focal_gamma, d.focal_alpha = self.focal_gamma, self.focal_alpha
        d.w_cls, d.w_bbox, d.w_ctr = self.cls_weight, self.bbox_weight, self.ctr_weight

    def __repr__(self):
        return 'HeadOptions(' + ', '.join(f'{f}={getattr(self, f)}' for f in self.key_fields()) + ')'


def head_specs(conv_bias=True):
    specs = []
    for tower in ('cls_convs', 'reg_convs'):
        specs += [ConvSpec(f'bbox_head.{tower}.{i}.conv', 256, 256, 3, 1, 1, bias=conv_bias) for i in range(4)]
    return specs


class ParamStore:
    """Flat buffers + named views.  One instance for the student, one for the EMA teacher."""

    def __init__(self, num_classes=80, device='cpu', backbone='resnet', head=None):
        assert backbone in ('resnet', 'rla')
        self.head = head or HeadOptions()
        self.cls_pad, self.cls_ld = class_layout(num_classes)
        self.num_classes, self.backbone = num_classes, backbone
        # centerness_on_reg=False: conv_centerness is one more row of the classification predictor, behind the classes' last group
        # of four (row cls_ld; the rows between C and cls_ld are zero and stay zero, as the padding rows do), and its logit one more
        # column of that predictor's fp32 output, whose rows are four floats longer
        self.ctr_on_cls = not self.head.centerness_on_reg
        self.cls_rows = self.cls_ld + 1 if self.ctr_on_cls else num_classes     # stored rows that are computed and trained
        self.logit_ld = self.cls_ld + 4 if self.ctr_on_cls else self.cls_ld      # row stride of the fp32 logits
        if self.ctr_on_cls:
            if self.cls_ld + 4 > MAX_CLASSES:
                raise NotImplementedError(f'dsl_amd hot path: centerness_on_reg=False needs num_classes <= {MAX_CLASSES - 4} (its logit is a '
                                          f'column of the classification predictor, at most {MAX_CLASSES} columns), got {num_classes}')
            self.cls_pad = _round_up(self.cls_rows, 64)
        # the box predictor (HeadOptions.reg_layout) in 64 stored rows; a GFL head's 4 (reg_max + 1) distribution logits in one or two
        # 64-row tiles (the launch shapes of a 128-row classification predictor)
        self.reg_rows, self.reg_ld = self.head.reg_layout()
        self.reg_pad = _round_up(self.reg_rows, 64)
        self.defer_head = False       # deferred head update (FlatSGD._sync_defer decides; engine.Plan.defer reads it)
        self._pending_ev = None
        bspecs = backbone_specs() if backbone == 'resnet' else rla_backbone_specs()
        self.convs = {s.name: s for s in bspecs + neck_specs() + head_specs(self.head.conv_bias)}
        self.extra_bns = rla_stage_bns() if backbone == 'rla' else []        # BatchNorms that follow no convolution
        self.train_regions = {}     # name -> (offset, numel, shape)   (shape = storage shape)
        self.frozen_regions = {}
        toff = foff = 0

        def add(regions, off, name, shape):
            n = _round_up(int(math.prod(shape)) if len(shape) else 1, 8)
            regions[name] = (off, n, tuple(shape))
            return off + n

        # BatchNorms with TRAINABLE affine parameters (eval-mode statistics; RLA_ResNet): every gamma in one block, every
        # beta in the next, at the START of the flat buffer - i.e. inside the gradient bucket that completes last - and the
        # statistics in the same order in the frozen buffer: the per-step fold to (scale, bias) is one launch
        self.bn_train = [(s.bn, s.cout) for s in self.convs.values() if s.bn and s.bn_train] + \
                        [(n, RLA_C) for n, tr in self.extra_bns if tr]
        self.bn_train_off = {}
        if self.bn_train:
            ctot = 0
            for n, c in self.bn_train:
                self.bn_train_off[n] = (ctot, c)
                ctot += c
            self.bn_train_ch = ctot
            toff = add(self.train_regions, toff, 'bn_train.weight', (ctot,))
            toff = add(self.train_regions, toff, 'bn_train.bias', (ctot,))
            foff = add(self.frozen_regions, foff, 'bn_train.running_mean', (ctot,))
            foff = add(self.frozen_regions, foff, 'bn_train.running_var', (ctot,))
        for s in self.convs.values():
            shape = (s.cout, s.k, s.k, s.cin_store)
            if s.trainable:
                toff = add(self.train_regions, toff, s.name + '.weight', shape)
                if s.bias:
                    toff = add(self.train_regions, toff, s.name + '.bias', (s.cout,))
            else:
                foff = add(self.frozen_regions, foff, s.name + '.weight', shape)
            if s.bn and not s.bn_train:
                for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
                    foff = add(self.frozen_regions, foff, f'{s.bn}.{leaf}', (s.cout,))
        for n, tr in self.extra_bns:
            if not tr:
                for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
                    foff = add(self.frozen_regions, foff, f'{n}.{leaf}', (RLA_C,))
        # the conv kernels fetch whole weight tiles: cout_pad rows, of which a 32-channel conv stores 32.  Inside the buffers
        # the extra rows are whatever follows (their outputs are dropped); the LAST conv of the frozen buffer would read past
        # the allocation (RLA's recurrent_convs.0 did, when the next page happened to be unmapped): zero rows behind it
        over = max([(s.cout_pad - s.cout) * s.k * s.k * s.cin_store for s in self.convs.values() if not s.trainable] + [0])
        if over:
            foff = add(self.frozen_regions, foff, '_tail_pad', (over,))
        for tower in ('cls_convs', 'reg_convs'):
            for i in range(4):
                toff = add(self.train_regions, toff, f'bbox_head.{tower}.{i}.gn.weight', (256,))
                toff = add(self.train_regions, toff, f'bbox_head.{tower}.{i}.gn.bias', (256,))
        # predictors: rows padded to the kernel tile; conv_reg (4) + conv_centerness (1) share one region.  The padding rows
        # of conv_cls stay zero: their output columns' gradients are zero, so SGD / weight decay / EMA keep them at 0
        toff = add(self.train_regions, toff, 'head.cls_w', (self.cls_pad, 3, 3, 256))
        toff = add(self.train_regions, toff, 'head.cls_b', (self.cls_pad,))
        toff = add(self.train_regions, toff, 'head.regctr_w', (self.reg_pad, 3, 3, 256))
        toff = add(self.train_regions, toff, 'head.regctr_b', (self.reg_pad,))
        if self.head.has_scale():
            toff = add(self.train_regions, toff, 'head.scales', (8,))
        if self.head.has_prior():      # center_prior.mean [C][2], then center_prior.sigma [C][2]: weights (decayed, lr_mult 1), no bias, no norm
            toff = add(self.train_regions, toff, 'head.center_prior', (2, num_classes, 2))
        self.n_train, self.n_frozen = toff, foff
        self.device = torch.device(device)
        self.train = torch.zeros(toff, dtype=torch.float32, device=device)
        self.frozen = torch.zeros(foff, dtype=torch.float32, device=device)
        self.grad = torch.zeros(toff, dtype=torch.float32, device=device)
        self.nbt = {s.bn: torch.zeros((), dtype=torch.long, device=device) for s in self.convs.values() if s.bn}
        self.nbt.update({n: torch.zeros((), dtype=torch.long, device=device) for n, _ in self.extra_bns})
        # bias group mask for the optimizer's paramwise rules (bias_lr_mult / bias_decay_mult apply to
        # conv biases, not to norm layers: mmcv DefaultOptimizerConstructor, SURVEY.md §8a note)
        grp = torch.zeros(toff, dtype=torch.uint8)
        for name, (off, n, shape) in self.train_regions.items():
            if (name.endswith('.conv.bias') or name in ('head.cls_b', 'head.regctr_b')):
                grp[off:off + n] = 1
        self.group = grp.to(device)
        # derived device-side packs (built by refresh())
        self.train16 = None
        self.frozen16 = None
        self.wT16 = None
        self.bn_scale = None
        self.bn_bias = None
        self.stem16 = None
        self._views = None
        self.dirty = True

    # -- flat <-> named ---------------------------------------------------------------------------
    def tview(self, name, buf=None):
        off, n, shape = self.train_regions[name]
        buf = self.train if buf is None else buf
        return buf[off:off + int(math.prod(shape))].view(shape)

    def fview(self, name):
        off, n, shape = self.frozen_regions[name]
        return self.frozen[off:off + int(math.prod(shape))].view(shape)

    def toff(self, name):
        return self.train_regions[name][0]

    def named_views(self, buf=None):
        """OrderedDict key -> tensor view with the reference's names/shapes (OIHW for conv weights).
        `buf` selects which flat buffer the trainable views come from (train / grad)."""
        out = {}
        tb = self.train if buf is None else buf

        def conv_w(s):
            v = self.tview(s.name + '.weight', tb) if s.trainable else (self.fview(s.name + '.weight') if buf is None else None)
            if v is None:
                return None
            if s.cin_store != s.cin:      # stored rows carry zero columns behind the real input channels
                v = v[..., :s.cin]
            return v.permute(0, 3, 1, 2)

        def bn(name):
            if name in self.bn_train_off:          # trainable affine parameters: slices of the gamma / beta blocks
                o, c = self.bn_train_off[name]
                out[f'{name}.weight'] = self.tview('bn_train.weight', tb)[o:o + c]
                out[f'{name}.bias'] = self.tview('bn_train.bias', tb)[o:o + c]
                if buf is None:
                    out[f'{name}.running_mean'] = self.fview('bn_train.running_mean')[o:o + c]
                    out[f'{name}.running_var'] = self.fview('bn_train.running_var')[o:o + c]
                    out[f'{name}.num_batches_tracked'] = self.nbt[name]
                return
            if buf is not None:
                return
            for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
                out[f'{name}.{leaf}'] = self.fview(f'{name}.{leaf}')
            out[f'{name}.num_batches_tracked'] = self.nbt[name]

        for s in self.convs.values():
            w = conv_w(s)
            if w is not None:
                out[s.name + '.weight'] = w
            if s.bias:
                out[s.name + '.bias'] = self.tview(s.name + '.bias', tb)
            if s.bn:
                bn(s.bn)
            if s.name.startswith('bbox_head.') and s.name.endswith('.conv'):
                base = s.name[:-5]
                out[base + '.gn.weight'] = self.tview(base + '.gn.weight', tb)
                out[base + '.gn.bias'] = self.tview(base + '.gn.bias', tb)
        for n, _ in self.extra_bns:
            bn(n)
        cw, cb = self.tview('head.cls_w', tb), self.tview('head.cls_b', tb)
        rw, rb = self.tview('head.regctr_w', tb), self.tview('head.regctr_b', tb)
        pc, pr, pt = [n and f'bbox_head.{n}' for n in self.predictor_names()]
        out[pc + '.weight'] = cw[:self.num_classes].permute(0, 3, 1, 2)
        out[pc + '.bias'] = cb[:self.num_classes]
        nbox = self.reg_rows if self.head.kind.dist_reg else 4
        out[pr + '.weight'] = rw[:nbox].permute(0, 3, 1, 2)
        out[pr + '.bias'] = rb[:nbox]
        if pt and self.ctr_on_cls:       # (row 4 of the regression predictor is then zero and stays zero)
            out[pt + '.weight'] = cw[self.cls_ld:self.cls_ld + 1].permute(0, 3, 1, 2)
            out[pt + '.bias'] = cb[self.cls_ld:self.cls_ld + 1]
        elif pt:
            out[pt + '.weight'] = rw[4:5].permute(0, 3, 1, 2)
            out[pt + '.bias'] = rb[4:5]
        if self.head.has_scale():
            sc = self.tview('head.scales', tb)
            for i in range(5):
                out[f'bbox_head.scales.{i}.scale'] = sc[i]
        if self.head.has_prior():      # (autoassign_head.py:39-40)
            cp = self.tview('head.center_prior', tb)
            out['bbox_head.center_prior.mean'], out['bbox_head.center_prior.sigma'] = cp[0], cp[1]
        return out

    def predictor_names(self):
        """Module names of the class, box and centerness predictors under bbox_head (a GFL head has no centerness predictor)."""
        return self.head.kind.names

    def wait_pending(self):
        """Deferred head update (FlatSGD, Plan.defer): the last optimizer step may still be updating the head + FPN bucket on the
        optimizer's stream.  Training forwards wait for it inside their op lists; every other reader or writer of the parameters
        on the current stream (state_dict, EMA, evaluation, loading) calls this first."""
        ev = getattr(self, '_pending_ev', None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
            self._pending_ev = None

    def load_named(self, sd, strict=True):
        """Copy a reference-layout state dict into the store.  Keys whose shape differs (a checkpoint of another class count:
        conv_cls) follow mmcv's load_state_dict: strict=True raises, strict=False skips them with a warning."""
        self.wait_pending()
        views = self.named_views()
        missing = [k for k in views if k not in sd]
        unexpected = [k for k in sd if k not in views]
        if strict and (missing or unexpected):
            raise KeyError(f'state_dict mismatch: missing {missing[:5]}, unexpected {unexpected[:5]}')
        mismatch = [f'{k}: checkpoint {tuple(sd[k].shape)}, model {tuple(v.shape)}' for k, v in views.items()
                    if k in sd and sd[k].numel() != v.numel()]
        if mismatch:
            msg = 'size mismatch in state_dict: ' + '; '.join(mismatch)
            if strict:
                raise RuntimeError(msg)
            import warnings
            warnings.warn(msg + ' (skipped)', RuntimeWarning, stacklevel=3)
        with torch.no_grad():
            for k, v in views.items():
                if k in sd and sd[k].numel() == v.numel():
                    v.copy_(sd[k].to(v.device))
        self.dirty = True
        return missing, unexpected

    def to(self, device):
        device = torch.device(device)
        for a in ('train', 'frozen', 'grad', 'group'):
            setattr(self, a, getattr(self, a).to(device))
        self.nbt = {k: v.to(device) for k, v in self.nbt.items()}
        self.device = device
        self.dirty = True
        return self

    # -- device-side derived packs ------------------------------------------------------------------
    def wT_layout(self):
        """Offsets (bf16 elements) of the dgrad packs [Cin][kh][kw][CoutPad] of every conv that needs a
        data gradient."""
        if getattr(self, '_wT', None) is None:
            off, lay = 0, {}
            for s in self.convs.values():
                if not s.trainable or s.no_dgrad:
                    continue
                if s.name in ('backbone.layer2.0.conv1', 'backbone.layer2.0.downsample.0'):
                    continue      # fed by frozen layer1: no data gradient needed
                lay[s.name] = (off, s.cin_store * s.k * s.k * s.cout_pad)
                off += _round_up(lay[s.name][1], 8)
                if s.k == 3 and s.stride == 2 and self.backbone == 'rla' and s.name.startswith('backbone.'):
                    # (RLA_ResNet's stage-entry 3x3 / 2 convolutions; the FPN's P6 / P7 convolutions keep the general strided gather)
                    # + the four parity-class packs of its data gradient (ops.dgrad_s2_descs): [Cin][k_c * k_c][CoutPad], k_c = 1 for
                    # the even-even pixels, 2 for the rest
                    from .ops import s2_class
                    for py in (0, 1):
                        for px in (0, 1):
                            k_c = s2_class(py, px)[0]
                            lay[f'{s.name}#s2{py}{px}'] = (off, s.cin_store * k_c * k_c * s.cout_pad)
                            off += _round_up(lay[f'{s.name}#s2{py}{px}'][1], 8)
            lay['head.cls'] = (off, 256 * 9 * self.cls_pad)
            off += 256 * 9 * self.cls_pad
            lay['head.regctr'] = (off, 256 * 9 * self.reg_pad)
            off += 256 * 9 * self.reg_pad
            self._wT, self._wT_total = lay, off
        return self._wT, self._wT_total

    def refresh_frozen(self):
        """Fold the frozen BatchNorms into per-channel (scale, bias) and build the bf16 packs of the frozen
        convs.  y = gamma*(x-mean)/sqrt(var+eps)+beta = x*scale + bias  (BN eval mode, resnet.py:647-656)."""
        dev = self.device
        scs, bis, self.bn_off = [], [], {}
        off = 0
        frozen_bns = [(s.bn, s.cout) for s in self.convs.values() if s.bn and not s.bn_train] + \
                     [(n, RLA_C) for n, tr in self.extra_bns if not tr]
        for name, c in frozen_bns:
            g, b = self.fview(name + '.weight'), self.fview(name + '.bias')
            m, v = self.fview(name + '.running_mean'), self.fview(name + '.running_var')
            sc = g / torch.sqrt(v + 1e-5)
            scs.append(sc)
            bis.append(b - m * sc)
            self.bn_off[name] = off
            off += c
        # trainable-affine BatchNorms: the tail of the same arrays, re-folded after every optimizer step (refold_bn)
        self.bn_train_base = off
        if self.bn_train:
            for name, (o, c) in self.bn_train_off.items():
                self.bn_off[name] = off + o
            g, b = self.tview('bn_train.weight'), self.tview('bn_train.bias')
            m, v = self.fview('bn_train.running_mean'), self.fview('bn_train.running_var')
            sc = g / torch.sqrt(v + 1e-5)
            scs.append(sc)
            bis.append(b - m * sc)
        wp = torch.zeros(64, 7 * 64, device=dev)
        w = self.fview('backbone.conv1.weight')           # [64][7][7][3] -> [64][448], k = tap*8 + c
        wp[:, :392] = torch.cat([w, torch.zeros(64, 7, 7, 5, device=dev)], -1).reshape(64, 392)
        # the same weight for dsl_stem_pool: [22 groups][64][8], group g = the (kx, c) values 8 (g % 3) .. + 8 of tap row g / 3
        wg = torch.zeros(64, 7, 24, device=dev)
        wg[:, :, :21] = w.reshape(64, 7, 21)
        wg = torch.cat([wg.reshape(64, 21, 8).permute(1, 0, 2), torch.zeros(1, 64, 8, device=dev)], 0)
        # Execution plans bake the device addresses of these four tensors into their kernel descriptors: refresh IN
        # PLACE whenever the buffers already exist on this device (load_state_dict into a model that has already run)
        for name, val in (('bn_scale', torch.cat(scs)), ('bn_bias', torch.cat(bis)), ('frozen16', self.frozen.bfloat16()),
                          ('stem16', wp.bfloat16()), ('stem_groups16', wg.bfloat16())):
            cur = getattr(self, name, None)
            if cur is not None and cur.device == val.device and cur.shape == val.shape:
                cur.copy_(val)
            else:
                setattr(self, name, val.contiguous())
                self._pack_tab = None        # holds pointers into bn_scale
                self.generation = getattr(self, 'generation', 0) + 1    # plans built against older buffers are stale

    def refold_bn(self, sp=None):
        """Eval-mode BatchNorms whose affine parameters train (RLA_ResNet): scale = gamma / sqrt(var + eps), bias = beta -
        mean * scale, re-made on the device after every optimizer step (one launch over all their channels)."""
        if not self.bn_train:
            return
        o = self.bn_train_base * 4
        L.check(L.lib.dsl_bn_fold(L.ptr(self.tview('bn_train.weight')), L.ptr(self.tview('bn_train.bias')),
                                  L.ptr(self.fview('bn_train.running_mean')), L.ptr(self.fview('bn_train.running_var')), 1e-5,
                                  self.bn_scale.data_ptr() + o, self.bn_bias.data_ptr() + o, self.bn_train_ch,
                                  sp or L.stream_ptr()), 'dsl_bn_fold')

    def refresh_train_packs(self, stream_ptr=None):
        """bf16 forward pack (= cast of the flat buffer) and dgrad packs.  Called after load_state_dict;
        the fused SGD kernel keeps train16 current afterwards, the dgrad packs are re-made per step."""
        if self.train16 is None or self.train16.device != self.device:
            self.train16 = torch.empty(self.n_train, dtype=torch.bfloat16, device=self.device)
        sp = stream_ptr or L.stream_ptr()
        L.check(L.lib.dsl_cast_bf16(L.ptr(self.train), L.ptr(self.train16), self.n_train, sp), 'dsl_cast_bf16')
        self.repack_dgrad(sp)

    def repack_dgrad(self, sp=None, side=False):
        """All dgrad packs in ONE launch (dsl_pack_dgrad_batched) from a device-resident item table.
        side=True: the launch goes to the library's side stream behind everything queued on `sp` so far and marks named
        event SLOT_PACKS; only the backward pass reads these packs, it waits for that event (Engine: first backward op),
        and the next forward pass starts without them."""
        import ctypes as C
        lay, total = self.wT_layout()
        if self.wT16 is None or self.wT16.device != self.device:
            self.wT16 = torch.zeros(total, dtype=torch.bfloat16, device=self.device)
            self._pack_tab = self._pack_ops = None
        sp = sp or L.stream_ptr()
        self.refold_bn(sp)          # the packs fold the BatchNorm scale: keep it current first
        if getattr(self, '_pack_tab', None) is None:
            items, start = [], 0
            for name, (off, n) in lay.items():
                if name == 'head.cls':
                    w, co, cop, taps, cin, sc = self.tview('head.cls_w'), self.cls_rows, self.cls_pad, 9, 256, None
                elif name == 'head.regctr':
                    w, co, cop, taps, cin, sc = self.tview('head.regctr_w'), self.reg_rows, self.reg_pad, 9, 256, None
                else:
                    s = self.convs[name.split('#')[0]]
                    w, co, cop, taps, cin = self.tview(s.name + '.weight'), s.cout, s.cout_pad, s.k * s.k, s.cin_store
                    sc = self.bn_scale[self.bn_off[s.bn]:] if s.bn else None
                tapmap = 0
                if '#s2' in name:         # a parity-class pack: k_c * k_c out taps selected from the 9 source taps
                    from .ops import s2_class
                    k_c, _, srcs = s2_class(int(name[-2]), int(name[-1]))
                    tapmap = 9 << 16
                    for t, src in enumerate(srcs):
                        tapmap |= (src if src >= 0 else 0xF) << (4 * t)
                    taps = k_c * k_c
                it = L.PackItem()
                it.w, it.scale, it.out = w.data_ptr(), (sc.data_ptr() if sc is not None else 0), self.wT16.data_ptr() + off * 2
                it.cout, it.cout_pad, it.taps, it.cin = co, cop, taps, cin
                it.tapmap = tapmap
                it.tiles_ci, it.tiles_co, it.block_start = (cin + 63) // 64, (cop + 63) // 64, start     # 64x64 tiles (optim.hip)
                start += it.tiles_ci * it.tiles_co * taps
                items.append(it)
            arr = (L.PackItem * len(items))(*items)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
            self._pack_tab = (host.to(self.device), len(items), start)
        tab, n, blocks = self._pack_tab
        if side:
            ops_ = getattr(self, '_pack_ops', None)
            if ops_ is None:
                ops_ = (L.Op * 3)()
                ops_[0].kind, ops_[0].i[0], ops_[0].i[1] = L.OP_FORK, 1, 0
                ops_[1].kind, ops_[1].p[0], ops_[1].i[0], ops_[1].i[1], ops_[1].i[6] = L.OP_PACK_DGRAD, tab.data_ptr(), n, blocks, 1
                ops_[2].kind, ops_[2].i[0], ops_[2].i[1] = L.OP_RECORD, 1, L.SLOT_PACKS
                self._pack_ops = ops_
            L.check(L.lib.dsl_run_ops(ops_, 3, sp), 'dsl_run_ops(pack_dgrad)')
        else:
            L.check(L.lib.dsl_pack_dgrad_batched(L.ptr(tab), n, blocks, sp), 'dsl_pack_dgrad_batched')

    def refresh(self):
        assert self.device.type == 'cuda', 'the HIP packs live on the GPU'
        self.wait_pending()
        self.refresh_frozen()
        self.refresh_train_packs()
        self.dirty = False

    def grad_buckets(self):
        """Contiguous gradient ranges in the order the backward completes them: head+FPN, last backbone stage, ..., first
        trainable stage (with the trainable BatchNorm blocks in front of it).  Together they cover the whole flat gradient
        buffer exactly once."""
        r = self.train_regions
        if self.backbone == 'resnet':
            first = [r[f'backbone.layer{i}.0.conv1.weight'][0] for i in (2, 3, 4)]
        else:
            first = [0] + [r[f'backbone.stages.{i}.0.conv1.weight'][0] for i in (2, 3)]
        b = first + [r['neck.lateral_convs.0.conv.weight'][0], self.n_train]
        return [(b[3], b[4]), (b[2], b[3]), (b[1], b[2]), (b[0], b[1])]

    # -- pointers used by the plans -----------------------------------------------------------------
    def w16_ptr(self, s):
        if s.trainable:
            return self.train16.data_ptr() + self.toff(s.name + '.weight') * 2
        if s.name == 'backbone.conv1':
            return self.stem16.data_ptr()
        return self.frozen16.data_ptr() + self.frozen_regions[s.name + '.weight'][0] * 2

    def t16_ptr(self, region):
        return self.train16.data_ptr() + self.toff(region) * 2

    def t32_ptr(self, region, buf=None):
        return (self.train if buf is None else buf).data_ptr() + self.toff(region) * 4

    def scales_ptr(self, buf=None):
        """Address of the five Scale values in the flat buffer (`buf`: the gradient buffer), None for a head without Scale."""
        return self.t32_ptr('head.scales', buf) if self.head.has_scale() else None

    def prior_ptrs(self, buf=None):
        """Addresses of center_prior.mean and .sigma in the flat buffer (`buf`: the gradient buffer)."""
        base = self.t32_ptr('head.center_prior', buf)
        return base, base + 8 * self.num_classes

    def wT_ptr(self, name):
        lay, _ = self.wT_layout()
        return self.wT16.data_ptr() + lay[name][0] * 2

    def bn_ptrs(self, bn):
        o = self.bn_off[bn] * 4
        return self.bn_scale.data_ptr() + o, self.bn_bias.data_ptr() + o

    # -- reference-style initialisation (random-init weights for the benchmark) ---------------------
    def init_reference_style(self, seed=0):
        """Kaiming-normal backbone convs, Xavier-uniform FPN, Normal(0, 0.01) head with the focal prior
        bias on conv_cls (fcos_head.py:83-91), BN gamma 1 / beta 0 / running stats (0, 1), scales 1."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for k, v in self.named_views().items():
            leaf = k.rsplit('.', 1)[-1]
            shape = tuple(v.shape)
            if leaf == 'num_batches_tracked':
                t = torch.zeros((), dtype=torch.long)
            elif leaf == 'scale':
                t = torch.tensor(1.0)
            elif leaf == 'running_mean':
                t = torch.zeros(shape)
            elif leaf == 'running_var' or k == 'bbox_head.center_prior.sigma':      # (autoassign_head.py:39-40: mean 0, sigma 1)
                t = torch.ones(shape)
            elif len(shape) == 4:
                fan_in = shape[1] * shape[2] * shape[3]
                fan_out = shape[0] * shape[2] * shape[3]
                if k.startswith('backbone.'):
                    t = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_out)
                elif k.startswith('neck.'):
                    a = math.sqrt(6.0 / (fan_in + fan_out))
                    t = (torch.rand(shape, generator=g) * 2 - 1) * a
                else:
                    t = torch.randn(shape, generator=g) * 0.01
            elif leaf == 'weight':
                t = torch.ones(shape)
                if self.backbone == 'rla' and k.endswith('.bn3.weight'):
                    t = torch.zeros(shape)          # zero_init_last_bn (resnet_rla.py:251-256)
            else:
                t = torch.zeros(shape)
                if k == f'bbox_head.{self.predictor_names()[0]}.bias':      # (atss_head.py:30-42, gfl_head.py:135-142: the same prior on atss_cls / gfl_cls)
                    t = torch.full(shape, -math.log((1 - 0.01) / 0.01))
                if self.head.has_prior():      # autoassign_head.py:161-171: class bias from probability 0.02, box bias 4.0
                    if k == f'bbox_head.{self.predictor_names()[0]}.bias':
                        t = torch.full(shape, -math.log((1 - 0.02) / 0.02))
                    elif k == f'bbox_head.{self.predictor_names()[1]}.bias':
                        t = torch.full(shape, 4.0)
            sd[k] = t
        self.load_named(sd)
        return self

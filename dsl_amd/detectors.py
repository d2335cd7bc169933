"""Registered detector classes with the reference's names and constructor arguments, so that
configs/fcos_semi/*.py build unmodified:

  FCOS / SingleStageDetector   mmdet/models/detectors/{fcos,single_stage,base}.py
  ResNet                        mmdet/models/backbones/resnet.py:304-656   (depth 50, caffe, frozen BN)
  FPN                           mmdet/models/necks/fpn.py:9-202
  ATSS / GFL / PAA / FOVEA / AutoAssign / KnowledgeDistillationSingleStageDetector
                                mmdet/models/detectors/{atss,gfl,paa,fovea,autoassign,kd_one_stage}.py
The heads and their loss config classes are dsl_amd/heads.py; importing this module registers them too, and their names are
importable from here.

Unlike the reference these classes do not compute with torch ops: they validate the configuration
the HIP path implements, own the parameter store, and drive the prebuilt kernel lists of
dsl_amd.engine.  There is no CPU / PyTorch fallback: calling the hot path without the HIP library or
off-GPU raises.
"""
from collections import OrderedDict

import os
import weakref

import torch
import torch.nn as nn

from .exchange import GradExchange
from .heads import (ATSSHead, AutoAssignHead, BoundedIoULoss, CIoULoss, CrossEntropyLoss, DIoULoss, DistributionFocalLoss,  # noqa: F401
                    FCOSHead, FocalLoss, FoveaHead, GFLHead, GIoULoss, IoULoss, KnowledgeDistillationKLDivLoss, LDHead, PAAHead,
                    QualityFocalLoss, SmoothL1Loss, _expect)
from .params import ParamStore
from .registry import BACKBONES, DETECTORS, NECKS, build_backbone, build_head, build_neck


# mmcv's model-zoo aliases used by configs/fcos_semi (mmcv/model_zoo/open_mmlab.json, mmcv 1.3.10): the file a
# torch.hub download would leave in the checkpoint cache
_ZOO_FILES = {'open-mmlab://detectron2/resnet50_caffe': 'resnet50_msra-5891d200.pth',
              'open-mmlab://detectron/resnet50_caffe': 'resnet50_caffe-788b5fa3.pth'}      # (configs/fcos)


def resolve_checkpoint(uri):
    """Local file for a `checkpoint=` value: a path, or a model-zoo alias looked up in $DSL_PRETRAINED_DIR and the torch
    hub cache (there is no network on the training boxes: the file has to be there already).  None when not found."""
    import os
    if os.path.exists(uri):
        return uri
    name = _ZOO_FILES.get(uri, os.path.basename(uri))
    for d in (os.environ.get('DSL_PRETRAINED_DIR'), os.path.join(torch.hub.get_dir(), 'checkpoints'),
              os.path.expanduser('~/.cache/torch/checkpoints')):
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return None


def load_backbone_checkpoint(det, uri, strict=False):
    """Backbone-only checkpoint (keys un-prefixed: conv1.weight, layer1.0.bn1.running_mean, ...; optional
    'state_dict' wrapper and 'module.' / 'backbone.' prefixes as mmcv's load_checkpoint strips them) into the flat
    store.  A checkpoint that cannot be found is NOT silently ignored: with a frozen stem / layer1 / BatchNorms the
    model would train on random frozen features."""
    import warnings
    path = resolve_checkpoint(uri)
    if path is None:
        warnings.warn(f'dsl_amd: pretrained backbone checkpoint {uri!r} not found (looked in $DSL_PRETRAINED_DIR and the '
                      'torch hub cache; no network here): the FROZEN stem/layer1/BatchNorm tensors keep their random '
                      'reference-style initialisation', RuntimeWarning, stacklevel=2)
        return False
    ck = torch.load(path, map_location='cpu')
    sd = ck.get('state_dict', ck.get('model', ck)) if isinstance(ck, dict) else ck
    views = det.store.named_views()
    out, unexpected = {}, []
    for k, v in sd.items():
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(v)
        for pre in ('module.', 'backbone.'):
            if k.startswith(pre):
                k = k[len(pre):]
        kk = 'backbone.' + k
        if kk in views and tuple(views[kk].shape) == tuple(v.shape):
            out[kk] = v
        else:
            unexpected.append(k)
    missing = [k for k in views if k.startswith('backbone.') and k not in out and not k.endswith('num_batches_tracked')]
    if strict and (missing or unexpected):
        raise KeyError(f'backbone checkpoint mismatch: missing {missing[:5]}, unexpected {unexpected[:5]}')
    if not out:
        raise KeyError(f'{path}: no key of this checkpoint matches the backbone (first keys: {list(sd)[:5]})')
    full = {k: v for k, v in views.items()}
    full.update(out)
    det.store.load_named(full, strict=False)
    return True


@BACKBONES.register_module()
class ResNet(nn.Module):
    def __init__(self, depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch', init_cfg=None,
                 pretrained=None, **kw):
        super().__init__()
        _expect(depth == 50 and num_stages == 4 and tuple(out_indices) == (0, 1, 2, 3), 'ResNet-50, 4 stages, all outputs')
        _expect(style == 'caffe', "style='caffe' (stride on the first 1x1)")
        _expect(frozen_stages == 1 and norm_eval and not norm_cfg.get('requires_grad', True),
                'frozen_stages=1, norm_eval=True, BN requires_grad=False (configs/fcos_semi/r50_caffe_*.py:4-15)')
        _expect(not kw.get('dcn') and not kw.get('plugins') and not kw.get('with_cp', False), 'no DCN/plugins/checkpointing')
        self.init_cfg = init_cfg
        self.pretrained_checkpoint = pretrained
        if isinstance(init_cfg, dict) and init_cfg.get('type') == 'Pretrained':
            self.pretrained_checkpoint = init_cfg['checkpoint']


@BACKBONES.register_module()
class RLA_ResNet(nn.Module):
    """mmdet/models/backbones/resnet_rla.py:140-388 with the arguments of configs/fcos_semi/RLA_*.py:3-13: layers
    [3, 4, 6, 3], rla_channel 32, no SE / ECA, frozen_stages 1, norm_eval, style 'pytorch' (the 3x3 convolutions stride).
    The computation is dsl_amd/engine_rla.py; this class validates the configuration and names the checkpoint."""
    backbone_kind = 'rla'

    def __init__(self, block=None, layers=(3, 4, 6, 3), num_classes=1000, rla_channel=32, SE=False, ECA=None,
                 frozen_stages=-1, norm_eval=True, style='pytorch', zero_init_last_bn=True, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None, pretrained=None, init_cfg=None, **kw):
        super().__init__()
        _expect(block is None and list(layers) == [3, 4, 6, 3] and rla_channel == 32, 'RLA_Bottleneck, layers [3, 4, 6, 3], 32 RLA channels')
        _expect(not SE and ECA is None and groups == 1 and width_per_group == 64 and replace_stride_with_dilation is None
                and norm_layer is None, 'no SE / ECA, no groups, no dilation, BatchNorm2d')
        _expect(frozen_stages == 1 and norm_eval and style == 'pytorch', "frozen_stages=1, norm_eval=True, style='pytorch'")
        self.zero_init_last_bn = zero_init_last_bn
        self.pretrained_checkpoint = pretrained
        if isinstance(init_cfg, dict) and init_cfg.get('type') == 'Pretrained':
            self.pretrained_checkpoint = init_cfg['checkpoint']


@NECKS.register_module()
class FPN(nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest'), init_cfg=None, **kw):
        super().__init__()
        _expect(list(in_channels) == [256, 512, 1024, 2048] and out_channels == 256 and num_outs == 5 and start_level == 1,
                'FPN 256ch, start_level=1, 5 outputs')
        _expect(add_extra_convs == 'on_output' and norm_cfg is None and act_cfg is None, "add_extra_convs='on_output', no norm/act")
        # False (the class default; configs/atss): P7 = fpn_convs[4](P6) without the ReLU in front (fpn.py:196-199)
        self.relu_before_extra_convs = bool(relu_before_extra_convs)
        _expect(upsample_cfg.get('mode', 'nearest') == 'nearest' and 'scale_factor' not in upsample_cfg, 'nearest upsample')


# One stream per ROLE and device for the whole process, not per model instance (round 4).  Streams are dealt onto four hardware
# queues in creation order; which streams share a queue moves the step by up to 20 % (350 vs 427 img/s for one stream
# created too early).  The first detector of a process creates the streams in the order the measured layout came about; every later
# instance (a second model in a notebook, bench.py's extra timings, student + teacher) must find the SAME streams instead of drawing
# new ones from torch's pool - measured: the same loop on a second model in one process ran at 433 or 362 img/s depending on which
# pool stream it happened to get (profiles/r04_td_first.txt).
_ROLE_STREAMS = {}
_ROLE_IDS = dict(prefix=4, comm=5, sweep=6, optimizer=1)      # the library's stream ids (csrc/api.hip side_init)


def role_stream(role, device=None):
    """The library's own stream for `role` on `device`: created and PICKED by the C library together with its side streams (csrc/api.hip
    side_init: a spin-kernel probe finds streams on hardware queues of their own) - not drawn from torch's pool, whose streams share
    hardware queues with whatever else the process created.  The optimizer's per-bucket updates run on the weight-gradient stream itself (id 1): each follows the weight
    gradients it waits for, which is where a stream of its own ended up anyway (one hardware queue with stream 1)."""
    import ctypes as C
    from . import _lib as L
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    key = (role, dev)
    st = _ROLE_STREAMS.get(key)
    if st is None:
        h = C.c_void_p()
        with torch.cuda.device(dev):
            L.check(L.lib.dsl_streams_init(L.stream_ptr(), None), 'dsl_streams_init')     # (picks the streams against the caller's: first call only)
            L.check(L.lib.dsl_side_stream(_ROLE_IDS[role], C.byref(h)), 'dsl_side_stream')
        st = torch.cuda.ExternalStream(h.value, device=dev)
        _ROLE_STREAMS[key] = st
    return st


def _check_grad_now(det, who='total'):
    """Should this backward call verify its incoming gradient (one host sync)?  Always when the step syncs anyway or the tuning key
    asks for it; otherwise on the first three backward calls of EACH autograd bridge (`who`: one backward pass goes through
    _TotalFn and _TrainStepFn - a budget shared between them was spent within two passes)."""
    from .tuning import tune
    if not det.lazy_log or tune('check_backward_grad') != '0':
        return True
    budget = det.__dict__.setdefault('_grad_checks_left', {})
    left = budget.get(who, 3)
    if left > 0:
        budget[who] = left - 1
        return True
    return False


class _LossDict(OrderedDict):
    """The loss dict of forward_train; `.vec` (optional) holds the same scalars as one graph-connected tensor, `.vec_total` the same
    with their sum appended."""
    vec = None
    vec_total = None


class _TotalFn(torch.autograd.Function):
    """total = the last element of the step's log vector (summed by the loss kernel), connected to the graph without a device op in
    either direction: backward hands the cached one-hot gradient on (a gradient other than 1 is rejected where the step reads
    values back anyway, see _TrainStepFn.backward)."""

    @staticmethod
    def forward(ctx, vec, det):
        ctx.det, ctx.n = det, vec.numel()
        return vec[ctx.n - 1].detach()

    @staticmethod
    def backward(ctx, g):
        det = ctx.det
        if _check_grad_now(det):
            if float(g) != 1.0:
                raise NotImplementedError(f'dsl_amd: loss.backward() with a gradient of {float(g)} for the total loss: scale through '
                                          'FCOS.loss_scale (folded into the loss kernel), not by scaling the loss tensor')
        key = (ctx.n, g.device)
        oh = det._onehot.get(key)
        if oh is None:
            oh = torch.zeros(ctx.n, dtype=torch.float32, device=g.device)
            oh[ctx.n - 1] = 1.0
            det._onehot[key] = oh
        return oh, None


class _TrainStepFn(torch.autograd.Function):
    """Bridges `loss.backward()` (mmcv OptimizerHook) to the hand-written backward kernel lists."""

    @staticmethod
    def forward(ctx, anchor, det, plan):
        ctx.det, ctx.plan, ctx.eager = det, plan, det._eager_now      # were the backward lists queued already?
        kind = plan.lossplan.kind
        ctx.n_losses = len(kind.loss_keys) + (kind.sisoft and plan.lossplan.desc.soft_weight != 0.0)      # (+ loss_sisoft)
        # the loss terms in log order and, last, their sum - written by the loss kernel's finalize pass (dsl_fcos_desc.logvec)
        return plan.lossplan.logvec[:ctx.n_losses + 1].clone()

    @staticmethod
    def backward(ctx, g):
        """The backward lists compute d(sum of the losses)/d(parameters): the loss kernel already produced the head
        gradients for d(total)/d(loss_k) = grad_scale (1/world).  Any other incoming gradient - loss scaling, loss / k for
        gradient accumulation, re-weighted loss keys - is NOT representable: it is rejected instead of silently ignored.
        The check reads g back (one host sync), so it runs whenever the step syncs anyway (lazy_log False), on a detector's first
        backward calls (a loop that scales its loss does so from the first step on) and on every step under the tuning key
        check_backward_grad=1; fold a constant factor into `FCOS.loss_scale` instead."""
        det = ctx.det
        if _check_grad_now(det, 'train_step'):
            k = ctx.n_losses
            gh = g.tolist()       # d(total)/d(term) = 1 for every term: either through the terms or through the kernel's own sum
            if not (all(v == 1 for v in gh[:k]) and gh[k] == 0) and not (all(v == 0 for v in gh[:k]) and gh[k] == 1):
                raise NotImplementedError(
                    'dsl_amd: loss.backward() reached the HIP step with a gradient != 1 for its loss terms '
                    f'({gh}): scale through FCOS.loss_scale (folded into the loss kernel), not by scaling the loss tensor')
        if not ctx.eager:                 # eager: the kernels were queued right behind the loss kernel
            det._run_backward(ctx.plan)
        return None, None, None


def _forward(name):
    """A detector attribute that IS the setting `name` of its gradient exchange."""
    return property(lambda self: getattr(self.exchange, name), lambda self, value: setattr(self.exchange, name, value))


@DETECTORS.register_module()
class FCOS(nn.Module):
    """SingleStageDetector (detectors/single_stage.py:10-165) specialised by detectors/fcos.py:5-18.
    Data parallel with late exchange (FlatSGD(late_exchange=True), the default without clipping): after backward() `p.grad` holds
    this rank's local gradient until wait_grads() or the optimizer's step() has run the exchanges."""
    HEAD_TYPE = None          # a detector of one head sets its bbox_head type; FCOS itself takes any registered head

    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None, fp8=None):
        """fp8 (not a key of the reference, whose training is fp32): dict(layers='towers') runs the FORWARD of the head towers' 3x3
        convolutions on the MX-scaled fp8 MFMA (OCP e4m3 activations with a dynamic per-tensor scale 448 / max|x| of the very
        tensor, per-output-channel weight scales re-made from the fp32 weights every step; the backward pass stays bf16 on the
        bf16 tensors - straight-through).  None (default): everything bf16."""
        _expect(self.HEAD_TYPE is None or (isinstance(bbox_head, dict) and bbox_head.get('type') == self.HEAD_TYPE),
                f"{type(self).__name__} with bbox_head type='{self.HEAD_TYPE}'")
        super().__init__()
        self.backbone = build_backbone(backbone)
        self.neck = build_neck(neck)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.store = ParamStore(self.bbox_head.num_classes, 'cpu', backbone=getattr(self.backbone, 'backbone_kind', 'resnet'),
                                head=self.bbox_head.options)
        self.store.fpn_relu_extra = bool(getattr(self.neck, 'relu_before_extra_convs', True))      # engine.Plan: P7's input
        self.store.init_reference_style(0)
        if fp8:
            assert str(fp8.get('layers', 'towers')) == 'towers', "fp8: only layers='towers' is built"
            # the fp8 tower convolutions fold the layer's bias into their epilogue and were validated on the default head only
            _expect(self.bbox_head.options.is_default(),
                    f'fp8 towers with the default head options only (center_sampling, norm_on_bbox, centerness_on_reg, GIoULoss, '
                    f'conv_bias=True, default loss settings), got {self.bbox_head.options}')
            self.store.fp8 = dict(fp8)
        self._params = None
        self._engine = None
        self._anchor = None
        # data parallel: buckets, streams, pending work and every option of the gradient exchange live here; the
        # names callers know (world_size, comm_proxy, clip_partials, ... below the constructor) forward to it
        self.exchange = GradExchange(self.store)
        self.CLASSES = None
        # Product defaults = what bench.py measures (round 4; both were opt-in and only bench.py set them):
        # lazy_log True: train_step's log_vars stay 0-dim device tensors; the host reads them when it logs (TextLoggerHook: every
        # `interval` iterations, float(v)) instead of once per iteration between the forward and the backward pass
        # (detectors/base.py:175-208 calls .item() per key per iteration).  False: python floats, one host sync per iteration.
        self.lazy_log = True
        # SemiEpochBasedRunner(scale_invariant=True) may hand the batch over WITHOUT its half-scale third image: the stem kernel reads
        # it out of the second one (forward_train(half_scale_copy=True)); set it False and the runner builds the copy with framework ops
        self.half_scale_in_stem = True
        # sweep.aug_test: store -> {(number of views, test_cfg values): AugMerge}.  Weak keys: a pool (13.6 MB at full size, four
        # views) lives as long as its parameter store (this model's, a teacher's handed in by a caller) and goes with it
        self._aug_merges = weakref.WeakKeyDictionary()
        self._onehot = {}          # cached gradient of the total loss w.r.t. the step's log vector (_TotalFn)
        # eager_backward True: INSIDE train_step the backward kernel lists are queued right behind the loss kernel (and the few
        # log-variable ops) instead of when `loss.backward()` reaches the autograd bridge.  The gradient of the summed loss is 1
        # either way - the bridge ignores its incoming gradient - so only the launch order changes.  For loops that call
        # loss.backward() once per train_step, as mmcv's OptimizerHook does (mmdet/apis/train.py:126-176); a caller that scales the
        # loss tensor instead of FCOS.loss_scale must set this False (tuning key check_backward_grad=1 checks the incoming gradient on every step; by default the first three are checked).
        # A direct forward_train() call (no train_step around it) stays lazy unless eager_backward == 'always'.
        self.eager_backward = True
        self._in_train_step, self._deferred_plan, self._eager_now = False, None, False
        # The frozen prefix of the forward pass - image layout, stem, pool, layer1 - runs on its own stream; when the batch's image
        # tensor carries its producer's event (dsl_amd.data.mark_ready: resident inputs, a loader that renders on its own stream)
        # it starts under the tail of the PREVIOUS step's backward pass and optimizer step, otherwise it is ordered behind
        # everything queued on the caller's stream (always correct, no overlap)
        self.pipeline_prefix = True
        self._prefix_stream, self._prefix_plan = None, None          # (_prefix_plan: the plan whose prefix ran last)
        self.loss_scale = 1.0         # constant factor on every gradient (gradient accumulation: 1/k); the reported losses stay unscaled

    # ---- the gradient exchange's settings under the detector's names (GradExchange.__init__ says what each is) -------------------
    dist_group = _forward('group')          # (set by the DDP wrapper, with world_size)
    world_size = _forward('world_size')
    rccl = _forward('rccl')
    grad_bf16 = _forward('grad_bf16')
    comm_off = _forward('comm_off')
    comm_proxy = _forward('comm_proxy')
    comm_trace = _forward('comm_trace')
    late_exchange = _forward('late_wanted')
    clip_partials = _forward('clip_partials')

    def wait_grads(self):
        self.exchange.wait()

    # ---- nn.Module surface redirected to the flat store ------------------------------------------
    def init_weights(self):
        """tools/train.py:162,171 calls this on student and teacher: reference-style random init, then the backbone's
        `init_cfg=dict(type='Pretrained', checkpoint=...)` / `pretrained=` checkpoint (mmcv BaseModule.init_weights ->
        load_checkpoint(strict=False) on the backbone, resnet.py:372-382 / resnet_rla.py:369-377)."""
        self.store.init_reference_style(0)
        ck = getattr(self.backbone, 'pretrained_checkpoint', None)
        if ck:
            load_backbone_checkpoint(self, ck)

    def _apply(self, fn, recurse=True):
        probe = fn(torch.zeros(1, device=self.store.device))
        if probe.device != self.store.device:
            self.store.to(probe.device)
            self._params = None
            self._engine = None
            self._anchor = None
        return self

    def state_dict(self, destination=None, prefix='', keep_vars=False):
        self.store.wait_pending()
        out = OrderedDict() if destination is None else destination
        for k, v in self.store.named_views().items():
            out[prefix + k] = v
        return out

    def load_state_dict(self, state_dict, strict=True):
        return self.store.load_named(state_dict, strict)

    def named_parameters(self, prefix='', recurse=True, remove_duplicate=True):
        if self._params is None:
            tv = self.store.named_views()
            gv = self.store.named_views(self.store.grad)
            self._params = OrderedDict()
            for k, v in tv.items():
                if not v.is_floating_point() or k.rsplit('.', 1)[-1] in ('running_mean', 'running_var'):
                    continue
                p = nn.Parameter(v, requires_grad=k in gv)
                if k in gv:
                    p.grad = gv[k]
                self._params[k] = p
        for k, p in self._params.items():
            yield prefix + ('.' if prefix else '') + k, p

    def parameters(self, recurse=True):
        for _, p in self.named_parameters():
            yield p

    def _rebind_grads(self):
        if self._params is not None:
            gv = self.store.named_views(self.store.grad)
            for k, p in self._params.items():
                if k in gv and p.grad is None:
                    p.grad = gv[k]

    # ---- hot path ----------------------------------------------------------------------------------
    def _get_engine(self):
        if self.store.device.type != 'cuda':
            raise RuntimeError('dsl_amd.FCOS runs only on an MI355X: move the model to cuda (no CPU fallback)')
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine()
            self._anchor = torch.zeros(1, device=self.store.device, requires_grad=True)
        return self._engine

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, half_scale_copy=False):
        """single_stage.py:56-84 + base_dense_head.py:22-59.  Returns dict of scalar loss tensors.
        half_scale_copy: the batch has one more image than `img` holds - SemiEpochBasedRunner's scale-invariant half-size copy of
        img[-1] (semi_epoch_based_runner.py:186-204), whose metas / boxes are the lists' last entries; the stem kernel samples it
        from img[-1] (dsl_stem_pool_half), it is never written to memory."""
        eng = self._get_engine()
        if self.exchange.pending or self.exchange.todo:
            # a second training pass before step() (gradient accumulation, an aborted step): the previous backward pass's collectives
            # are queued now (late exchange) and waited for - none is dropped (the ranks would disagree on the collective sequence)
            # and none still writes store.grad under this pass.  Here and not in _run_backward: this pass's loss kernel already
            # writes the scale gradients into store.grad, and every later writer (the weight gradients) runs behind the caller's stream
            self.wait_grads()
        N, _, H, W = img.shape
        N += 1 if half_scale_copy else 0
        assert len(img_metas) == N == len(gt_bboxes) == len(gt_labels)
        if self.comm_trace is not None and img.is_cuda:
            t0 = torch.cuda.Event(enable_timing=True)
            t0.record()
            self.comm_trace.append(dict(t0=t0, buckets=[]))
        plan = eng.plan(self.store, N, H, W, training=True)
        head = self.bbox_head
        if head.loss_weight != 1.0 and gt_bboxes_ignore is None:
            raise TypeError('loss_weight != 1.0 needs gt_bboxes_ignore (fcos_head.py:223 iterates ig_labels)')
        lp = plan.lossplan
        sw = head.effective_soft_weight(N)
        ws = self.world_size
        kind = lp.kind      # (params.HEAD_KINDS: `exchange` says where the ranks' stats[0:2] are summed, None = this rank's own count)
        lp.configure(loss_weight=head.loss_weight, soft_weight=sw, grad_scale=self.loss_scale / ws,
                     inv_world=1.0 / ws if kind.exchange else 1.0)
        pipe = self.pipeline_prefix and plan.prefix is not None
        if pipe:
            # frozen prefix of THIS step on its own stream: it waits for the previous backward's data-gradient chain only (named
            # event), not for that step's weight-gradient tail / optimizer step; layer1's output alternates between two buffers
            plan.set_parity(plan._parity ^ 1)
            plan.bind_image(img, half_last=half_scale_copy)
            if self._prefix_stream is None:
                self._prefix_stream = role_stream('prefix', self.store.device)
            if img.is_cuda:
                img.record_stream(self._prefix_stream)
            ready = getattr(img, '_dsl_ready', None)          # event of the image's producer (dsl_amd.data.mark_ready)
            if ready is not None:
                # one-shot: a loader that refills this tensor in place has to mark it again (a stale, long-fired event would let the
                # prefix start before the new contents are written)
                try:
                    del img._dsl_ready
                except AttributeError:
                    pass
            staged = plan._img_ref is None                     # bind_image copied the batch into plan.img on the CALLER's stream
            if self._prefix_plan is not plan:
                # first use of this plan (or the first step at all): SLOT_TAIL was never recorded, so nothing orders the prefix
                # stream behind the caller's stream, which wrote the frozen packs (store.refresh) and possibly the image
                self._prefix_stream.wait_stream(torch.cuda.current_stream())
                self._prefix_plan = plan
            elif staged:
                # a CPU / non-fp32 / non-contiguous batch: the staging copy was queued on the caller's stream just now - whatever
                # the producer's event says, the prefix must not read plan.img before that copy has landed (round-3 advisor)
                ev = torch.cuda.Event()
                ev.record()
                self._prefix_stream.wait_event(ev)
            elif ready is not None:
                self._prefix_stream.wait_event(ready)
            elif img.is_cuda:
                # unknown producer: it can only have been queued on the caller's stream, behind the previous step - correct for
                # any caller, the prefix then simply runs after that step instead of under its tail
                ev = torch.cuda.Event()
                ev.record()
                self._prefix_stream.wait_event(ev)
            with torch.cuda.stream(self._prefix_stream):
                plan.prefix.run()
            fwd = plan.fwd_rest
        else:
            plan.bind_image(img, half_last=half_scale_copy)
            fwd = plan.fwd
        plan.fp8_warm(fwd)
        # an ATSS head's valid anchors come from each image's pad_shape (atss_head.py:615-617); absent: the batch tensor's size
        pad = [tuple(m.get('pad_shape', (H, W)))[:2] for m in img_metas] if lp.atss is not None else None
        if kind.exchange == 'forward' and ws > 1:
            # target assignment first: the reduce_mean of (num_pos, sum centerness targets) - one 2-float all-reduce
            # (fcos_head.py:264-274) - then runs under the forward pass
            lp.set_targets(gt_bboxes, gt_labels, gt_bboxes_ignore, pad)
            plan.assign_ops.run()
            work = None if self.comm_off else self.exchange.all_reduce_async(lp.stats[:2], after_current=True)
            fwd.run()
            if work is not None:
                work.wait()
        else:
            # one process: target upload + assignment go behind the forward pass on the caller's stream, into the time it
            # would otherwise spend waiting for the regression tower on the side stream.  A kind with a middle pass, on any number
            # of ranks: the same order, then that pass behind the predictors and, where the kind exchanges there, the 2-float
            # all-reduce of (num_total, the quality pass's sum), waited for in front of the loss
            fwd.run()
            lp.set_targets(gt_bboxes, gt_labels, gt_bboxes_ignore, pad)
            plan.assign_ops.run()
            if kind.middle:
                plan.quality_ops.run()
            if kind.exchange == 'middle' and ws > 1 and not self.comm_off:
                self.exchange.all_reduce_async(lp.stats[:2], after_current=True).wait()
        plan.loss_ops.run()
        eager_now = False
        if self.eager_backward and torch.is_grad_enabled():
            if self._in_train_step:       # train_step queues it behind its log-variable ops (they only need the loss kernel)
                self._deferred_plan = plan
                eager_now = True
            elif self.eager_backward == 'always':
                self._run_backward(plan)
                eager_now = True
        self._eager_now = eager_now
        out = _TrainStepFn.apply(self._anchor, self, plan)
        losses = _LossDict((k, out[i]) for i, k in enumerate(kind.loss_keys + (('loss_sisoft',) if kind.sisoft and sw != 0.0 else ())))
        losses.vec = out[:len(losses)]      # the same scalars as ONE tensor: lets _parse_losses avoid per-key device ops
        losses.vec_total = out              # ... and with their sum (the loss kernel's) as the last element: no device op at all
        return losses

    def _run_backward(self, plan):
        """Hand-written backward.  Data parallel: gradient bucket s (head+FPN, layer4, layer3, layer2) is all-reduced as
        soon as the side stream has finished its weight gradients - the communication stream waits for the named event
        the segment recorded (dsl_stream_wait_slot), not for the caller's stream, which is already running the next
        segment's data-gradient chain - so the bulk RCCL traffic overlaps the remaining backward (what torch DDP's bucket
        hooks do at mmdet/apis/train.py:92-96); only the last, smallest bucket (layer2, 5 MB) is exposed.  Or, the default
        without clipping, behind the whole pass: GradExchange says which, and does it."""
        ex = self.exchange
        ex.begin(plan)
        for ol, info in plan.bwd_segments:
            ol.run()
            ex.segment_done(info)
        ex.finish()
        self._rebind_grads()

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        """detectors/base.py:155-173."""
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def forward_test(self, imgs, img_metas, **kwargs):
        """detectors/base.py:116-153: one view -> simple_test, several (MultiScaleFlipAug) -> aug_test."""
        if isinstance(imgs, (list, tuple)):
            if len(imgs) != len(img_metas):
                raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
            if len(imgs) > 1:
                return self.aug_test(imgs, img_metas, **kwargs)
            imgs, img_metas = imgs[0], img_metas[0]
        return self.simple_test(imgs, img_metas, **kwargs)

    def simple_test(self, img, img_metas, rescale=False):
        from .sweep import simple_test
        self.store.wait_pending()          # a deferred head update of the last optimizer step (the training forward waits in its op list)
        return simple_test(self, img, img_metas, rescale)

    def aug_test(self, imgs, img_metas, rescale=False):
        """detectors/single_stage.py:109-135: `imgs` / `img_metas` hold one entry per view, each with ONE image."""
        if self.store.head.kind.aug_refusal:
            raise NotImplementedError(self.store.head.kind.aug_refusal)
        from .sweep import aug_test
        self.store.wait_pending()
        return aug_test(self, imgs, img_metas, rescale)

    def _parse_losses(self, losses):
        """detectors/base.py:175-208: total = sum of keys containing 'loss'; log vars averaged over ranks."""
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value if value.dim() == 0 else value.mean()     # the HIP head returns scalars
            else:
                log_vars[name] = sum(v.mean() for v in value)
        keys = list(log_vars.keys())
        vt = getattr(losses, 'vec_total', None)
        if vt is not None and vt.numel() == len(keys) + 1 and all('loss' in k for k in keys):
            # the HIP head: the loss kernel summed the terms itself, the total is the vector's last element
            loss = _TotalFn.apply(vt, self)
            log_vars['loss'] = loss
            keys.append('loss')
            # (the all-reduce below works in place: not on the storage `loss` is a view of)
            vec = vt.detach().clone() if (self.world_size > 1 and not self.comm_off) else vt.detach()
            return self._finish_log_vars(loss, vec, keys)
        # two device ops instead of one per key (stack + sum); the reference sums the keys containing 'loss'
        vec0 = getattr(losses, 'vec', None)
        stacked = vec0 if (vec0 is not None and vec0.numel() == len(keys)) else torch.stack([log_vars[k] for k in keys])
        if all('loss' in k for k in keys):
            loss = stacked.sum()
        else:
            loss = sum(v for k, v in log_vars.items() if 'loss' in k)
        log_vars['loss'] = loss
        keys.append('loss')
        vec = torch.cat([stacked.detach(), loss.detach().reshape(1)])
        return self._finish_log_vars(loss, vec, keys)

    def _finish_log_vars(self, loss, vec, keys):
        if self.world_size > 1 and not self.comm_off:      # ONE all-reduce for all log vars instead of one per key
            self.exchange.all_reduce_log(vec)
            vec = vec / self.world_size
        if self.lazy_log:
            log_vars = OrderedDict((k, vec[i]) for i, k in enumerate(keys))
        else:
            host = vec.tolist()
            log_vars = OrderedDict((k, host[i]) for i, k in enumerate(keys))
        return loss, log_vars

    def train_step(self, data, optimizer):
        """detectors/base.py:210-243."""
        self._in_train_step, self._deferred_plan = True, None
        try:
            losses = self(**data)
        finally:
            self._in_train_step = False
        loss, log_vars = self._parse_losses(losses)
        if self._deferred_plan is not None:
            # eager backward: its kernels go behind the handful of small device ops above instead of in front of them, where
            # those would sit between the last weight gradient and the optimizer step
            plan, self._deferred_plan = self._deferred_plan, None
            self._run_backward(plan)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))

    def val_step(self, data, optimizer=None):
        return self.train_step(data, optimizer)


@DETECTORS.register_module()
class ATSS(FCOS):
    """mmdet/models/detectors/atss.py:5-18: SingleStageDetector with an ATSSHead, on the FCOS detector's machinery (the same
    network; assignment, box decode and loss normalisers are the head's)."""
    HEAD_TYPE = 'ATSSHead'


@DETECTORS.register_module()
class GFL(FCOS):
    """mmdet/models/detectors/gfl.py:5-18: SingleStageDetector with a GFLHead, on the FCOS detector's machinery (the same network
    up to the box predictor's width; assignment, box decode, losses and their normalisers are the head's)."""
    HEAD_TYPE = 'GFLHead'


@DETECTORS.register_module()
class PAA(FCOS):
    """mmdet/models/detectors/paa.py:5-18: SingleStageDetector with a PAAHead, on the FCOS detector's machinery (ATSS's network and
    parameters; assignment, losses, normalisers and the detection score are the head's)."""
    HEAD_TYPE = 'PAAHead'


@DETECTORS.register_module()
class FOVEA(FCOS):
    """mmdet/models/detectors/fovea.py:5-18: SingleStageDetector with a FoveaHead, on the FCOS detector's machinery (the same network
    without the centerness predictor and the Scale layers; assignment, losses, normalisers and box decode are the head's)."""
    HEAD_TYPE = 'FoveaHead'


@DETECTORS.register_module()
class AutoAssign(FCOS):
    """mmdet/models/detectors/autoassign.py:5-18: SingleStageDetector with an AutoAssignHead, on the FCOS detector's machinery (the
    same network; the losses, their normalisers and the point of a location are the head's)."""
    HEAD_TYPE = 'AutoAssignHead'


@DETECTORS.register_module()
class KnowledgeDistillationSingleStageDetector(GFL):
    """mmdet/models/detectors/kd_one_stage.py:10-100 with an LDHead: a GFL student whose loss has one more term against the box
    distributions of a frozen teacher detector.  The teacher is a detector of this project with a GFL-family head on the student's
    grid (reg_max, strides and level sizes equal); it is held as a plain attribute, so that it shows up in no parameters(),
    state_dict(), flat store, EMA hook, optimizer or gradient bucket of the student, and it runs inference plans only.
    simple_test / aug_test are the student's."""
    HEAD_TYPE = 'LDHead'

    def __init__(self, backbone, neck, bbox_head, teacher_config, teacher_ckpt=None, eval_teacher=True, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None, fp8=None):
        """teacher_config: a config file's path (Config.fromfile, `_base_` followed) or a dict - a whole config with a `model` key, or
        the model's dict itself.  teacher_ckpt: a whole-detector checkpoint (resolve_checkpoint; a path that cannot be found raises,
        None loads nothing).  eval_teacher: accepted with either value - every teacher this project builds (GroupNorm towers, frozen
        BatchNorm with norm_eval) computes the same thing in both modes.  init_cfg / fp8: FCOS's (fp8 towers are refused, as for GFL)."""
        super().__init__(backbone, neck, bbox_head, train_cfg, test_cfg, pretrained, init_cfg, fp8)
        from .registry import Config, build_detector
        self.eval_teacher = bool(eval_teacher)
        if isinstance(teacher_config, (str, os.PathLike)):
            teacher_config = Config.fromfile(os.fspath(teacher_config))
        _expect(hasattr(teacher_config, '__getitem__'), f'teacher_config: a config path or a dict (got {type(teacher_config).__name__})')
        tm = teacher_config['model'] if 'model' in teacher_config else teacher_config
        teacher = build_detector(dict(tm))
        th = getattr(getattr(teacher, 'store', None), 'head', None)
        _expect(isinstance(teacher, FCOS) and th is not None and th.kind.dist_reg,
                f'teacher_config: a detector with a GFL-family head (GFLHead / LDHead), got {type(teacher).__name__} with '
                f'{type(getattr(teacher, "bbox_head", None)).__name__}')
        sh = self.store.head
        _expect(th.reg_max == sh.reg_max, f'teacher reg_max {th.reg_max} != student reg_max {sh.reg_max} (the distributions are compared bin by bin)')
        _expect(tuple(teacher.bbox_head.strides) == tuple(self.bbox_head.strides),
                f'teacher strides {tuple(teacher.bbox_head.strides)} != student strides {tuple(self.bbox_head.strides)}')
        if teacher_ckpt is not None:
            path = resolve_checkpoint(teacher_ckpt)
            if path is None:
                raise FileNotFoundError(f'teacher_ckpt {teacher_ckpt!r} not found (looked in $DSL_PRETRAINED_DIR and the torch hub cache): '
                                        'a randomly initialised teacher is never what a distillation config means')
            ck = torch.load(path, map_location='cpu')
            sd = ck.get('state_dict', ck) if isinstance(ck, dict) else ck
            # (mmcv's load_checkpoint: strict=False, 'module.' stripped; a file none of whose keys is the teacher's is refused)
            sd = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in sd.items())
            missing, _ = teacher.load_state_dict(sd, strict=False)
            if len(missing) == len(teacher.state_dict()):
                raise KeyError(f'{path}: no key of this checkpoint matches the teacher (first keys: {list(sd)[:5]})')
        self.teacher_model = teacher

    def __setattr__(self, name, value):
        """kd_one_stage.py:89-100: the teacher is a plain attribute, not a registered submodule."""
        if name == 'teacher_model':
            object.__setattr__(self, name, value)
        else:
            super().__setattr__(name, value)

    def _apply(self, fn, recurse=True):
        self.teacher_model._apply(fn)          # kd_one_stage.py:75-79 (.cuda() / .to() move the teacher too)
        return super()._apply(fn, recurse)

    def train(self, mode=True):
        self.teacher_model.train(False if self.eval_teacher else mode)
        return super().train(mode)

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        """kd_one_stage.py:43-73.  The teacher's forward is an inference plan (no loss plan, no gradient or momentum buffer) on the
        caller's stream, in front of the student's forward; its box predictor's fp32 output and its Scale values go to the student's
        loss descriptor (bind_soft), the rest is the GFL step.  loss_ld has no normaliser: data parallel adds no collective."""
        eng = self._get_engine()
        ts = self.teacher_model.store
        N, _, H, W = img.shape
        tplan = eng.plan(ts, N, H, W, training=False)
        plan = eng.plan(self.store, N, H, W, training=True)
        if [tuple(s) for s in tplan.level_sizes] != [tuple(s) for s in plan.level_sizes]:
            raise NotImplementedError(f'dsl_amd hot path: teacher level sizes {tplan.level_sizes} != student level sizes {plan.level_sizes}')
        tplan.bind_image(img)
        tplan.fwd.run()
        plan.lossplan.bind_soft(tplan.bufs['regctr'], ts.reg_ld, ts.t32_ptr('head.scales'))
        return super().forward_train(img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore)

"""Host side of the fused FCOS target assignment + loss (dsl_fcos_assign / dsl_fcos_loss).

Mirrors `FCOSHead.loss` of the reference (mmdet/models/dense_heads/fcos_head.py:170-338): same
inputs (per-image gt boxes / labels / ignore boxes), same outputs (loss_cls, loss_bbox,
loss_centerness[, loss_sisoft]); the gradients w.r.t. the head outputs are produced in the same pass.
All buffers are level-major [level][image][y][x] = the reference's flattened order."""
import ctypes as C

import torch

from . import _lib as L
from . import ops
from .params import HeadOptions, class_layout

STRIDES = (8, 16, 32, 64, 128)
REGRESS_RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8))   # fcos_head.py:61-62


class FcosLossPlan:
    """Row strides: the logits are read LD_CLS = round_up(C, 4) wide, the class gradients written LD_GCLS = round_up(C, 64)
    wide (the predictor's data / weight gradient read them as that many channels: the columns from C on stay zero)."""
    LD_RC, LD_GRC = 8, 64

    def __init__(self, n, sizes, device, strides=STRIDES, ranges=REGRESS_RANGES, num_classes=80,
                 radius=1.5, max_gt=1024, head=None):
        """head: params.HeadOptions (None = the default head).  centerness_on_reg=False: the centerness logit is column
        round_up(C, 4) of the logits' rows, which are four floats longer, and its gradient that column of g_cls.  The head's loss
        settings (box_loss, focal gamma / alpha, the loss weights) go into the descriptor: losses, logvec and the gradients are the
        weighted ones.  What the head's kind decides is in its record (params.HEAD_KINDS): the struct around `desc` and the
        attributes that hold it (`gfl`, `ld`, `paa`, `fovea`, `aa`; None on the other kinds), the box predictor's row widths, the kind's own buffers
        (`score`, `weight`; `pos_loss`, `iou_target`, `cand_gt`, `gmm_iters`, `gmm_flags`; absent on the other kinds), middle(),
        the entry of loss() and the length of logvec.  A kind with the ATSS layout: the assignment is fed the images' pad_shape
        (set_targets); `npos` holds the positives per image, stats[0] their sum_i max(npos_i, 1) (atss_head.py:554).  An LD head:
        bind_soft() names the teacher's box predictor output."""
        self.LD_GCLS, self.LD_CLS = class_layout(num_classes)
        self.head = head = head or HeadOptions()
        self.kind = kind = head.kind
        self.gfl = self.ld = self.paa = self.fovea = self.aa = self.ext = None
        inner = getattr(L, kind.loss_desc[0])()
        for attr, member in zip(kind.loss_desc[1:], kind.loss_desc[2:] + ('fcos',)):
            setattr(self, attr, inner)
            self.ext, inner = inner, getattr(inner, member)
        self.LD_RC = head.reg_layout()[1]
        self.LD_GRC = (self.LD_RC + 63) // 64 * 64
        self.ctr_col = None
        if not head.centerness_on_reg:
            self.ctr_col = self.LD_CLS
            self.LD_CLS, self.LD_GCLS = self.LD_CLS + 4, (self.LD_CLS + 1 + 63) // 64 * 64
        self.num_classes = num_classes
        self.n, self.sizes, self.strides, self.device = n, [tuple(s) for s in sizes], strides, device
        self.M = n * sum(h * w for h, w in self.sizes)
        M, dev = self.M, device
        self.labels = torch.empty(M, dtype=torch.int64, device=dev)
        self.bbox_targets = torch.empty(M, 4, dtype=torch.float32, device=dev)
        self.assign_idx = torch.empty(M, dtype=torch.int32, device=dev)
        self.cls_weight = torch.empty(M, dtype=torch.float32, device=dev)
        self.pos_weight = torch.empty(M, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(8, dtype=torch.float32, device=dev)
        self.losses = torch.zeros(4, dtype=torch.float32, device=dev)
        self.logvec = torch.zeros(5, dtype=torch.float32, device=dev)      # the loss terms in log order + their sum (dsl_fcos_desc.logvec)
        self.g_scales = torch.zeros(L.MAX_SEG, dtype=torch.float32, device=dev)
        # gradient buffers: padding columns stay zero forever (the kernels only write real columns)
        self.g_cls = torch.zeros(M, self.LD_GCLS, dtype=torch.bfloat16, device=dev)
        self.g_rc = torch.zeros(M, self.LD_GRC, dtype=torch.bfloat16, device=dev)
        self.max_gt = max_gt
        self.gt_boxes = torch.zeros(max_gt, 4, dtype=torch.float32, device=dev)
        self.gt_labels = torch.zeros(max_gt, dtype=torch.int64, device=dev)
        self.gt_off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        self.ig_boxes = torch.zeros(max_gt, 4, dtype=torch.float32, device=dev)
        self.ig_off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        # pinned staging: pageable H2D copies would block the host until the stream drains (one stall per step).
        # A ring of slots, each guarded by an event recorded behind its async copies: the host may run several steps
        # ahead of the GPU (lazy_log, no per-step sync) and must not rewrite a slot whose copy has not executed yet.
        pin = torch.cuda.is_available()
        self._slots = [dict(boxes=torch.zeros(2, max_gt, 4, dtype=torch.float32, pin_memory=pin),
                            labels=torch.zeros(max_gt, dtype=torch.int64, pin_memory=pin),
                            off=torch.zeros(2, n + 1, dtype=torch.int32, pin_memory=pin),
                            pad=torch.zeros(n, 2, dtype=torch.int32, pin_memory=pin), ev=None) for _ in range(4)]
        self._slot_i = 0
        self.desc = ops.fcos_desc(n=n, sizes=self.sizes, strides=strides, ranges=ranges, radius=radius,
                                  num_classes=num_classes, into=inner)
        ops.set_ptrs(self.desc, gt_boxes=self.gt_boxes, gt_labels=self.gt_labels, gt_off=self.gt_off,
                     labels=self.labels, bbox_targets=self.bbox_targets, assign_idx=self.assign_idx,
                     cls_weight=self.cls_weight, pos_weight=self.pos_weight, stats=self.stats,
                     norm=self.stats, g_cls=self.g_cls, g_rc=self.g_rc, g_scales=self.g_scales,
                     losses=self.losses, logvec=self.logvec)
        self.desc.ld_cls, self.desc.ld_rc = self.LD_CLS, self.LD_RC
        self.desc.ld_gcls, self.desc.ld_grc = self.LD_GCLS, self.LD_GRC
        self.desc.head_flags = head.flags()
        # box kind, focal gamma / alpha, the three loss weights, wherever HEAD_LOSS_EXT is in the flags
        if self.desc.head_flags & L.HEAD_LOSS_EXT:
            head.fill_loss_desc(self.desc)
        if self.ctr_col is not None:
            self.desc.g_ctr, self.desc.ld_gctr = self.g_cls.data_ptr() + 2 * self.ctr_col, self.LD_GCLS
        self.atss = head.atss_desc()
        if self.atss is not None:
            self.pad_shapes = torch.zeros(n, 2, dtype=torch.int32, device=dev)
            self.npos = torch.zeros(n, dtype=torch.int32, device=dev)
            self.atss.max_gt, self.atss.pad_shapes, self.atss.npos = max_gt, L.ptr(self.pad_shapes), L.ptr(self.npos)
            self.desc.atss = C.addressof(self.atss)
        for attr, field, option in kind.scalars:
            setattr(getattr(self, attr), field, getattr(head, option))
        for name, dtype, length, fill in kind.buffers:
            setattr(self, name, torch.full((getattr(self, length),), fill, dtype=dtype, device=dev))
            setattr(self.ext, name, L.ptr(getattr(self, name)))
        if self.aa is not None:
            # the per-box launches and records are sized by the capacity of gt_boxes; the centre prior (mean, then sigma, each [C][2])
            # and its gradient are the plan's own until bind_prior names the parameter store's
            self.aa.max_gt = max_gt
            self.prior = torch.cat([torch.zeros(num_classes, 2), torch.ones(num_classes, 2)]).to(dev)
            self.g_prior = torch.zeros(2 * num_classes, 2, dtype=torch.float32, device=dev)
            self.bind_prior(*(t.data_ptr() + o for t in (self.prior, self.g_prior) for o in (0, 8 * num_classes)))
        self.logvec = self.logvec[:len(kind.loss_keys) + kind.sisoft + 1]      # the terms in log order (cls, bbox, ...), their sum
        need = L.lib.dsl_fcos_workspace_bytes(C.byref(self.desc))
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.desc.workspace, self.desc.workspace_bytes = L.ptr(self.ws), need

    # -- ground truth upload (host lists -> one pinned staging copy) --------------------------------
    def set_targets(self, gt_bboxes, gt_labels, gt_bboxes_ignore=None, pad_shapes=None):
        """pad_shapes: (pad_h, pad_w) per image, required by an ATSS head (its valid anchors, atss_head.py:615-617) and not read
        otherwise; ATSS does not read gt_bboxes_ignore (ignore_iof_thr = -1)."""
        assert len(gt_bboxes) == self.n == len(gt_labels)
        if self.atss is not None:
            if pad_shapes is None or len(pad_shapes) != self.n:
                raise ValueError('an ATSS head needs the pad_shape of every image (set_targets(pad_shapes=...))')
            gt_bboxes_ignore = None
        if self.desc.head_flags & (L.HEAD_FOVEA | L.HEAD_AUTOASSIGN):      # their loss takes gt_bboxes_ignore and does not read it (fovea_head.py:134-182, autoassign_head.py:314-321)
            gt_bboxes_ignore = None
        if self.aa is not None:
            # the centre prior has one row per class: labels handed over on the host are checked here (no device read; what the
            # kernels do with an out-of-range label that arrives on the device is stated at dsl_aa_desc in include/dsl_hip.h)
            for l in gt_labels:
                if not l.is_cuda and l.numel() and not (0 <= int(l.min()) and int(l.max()) < self.num_classes):
                    raise ValueError(f'an AutoAssign head needs gt_labels in 0..{self.num_classes - 1}, got {int(l.min())}..{int(l.max())}')
        slot = self._slots[self._slot_i]
        self._slot_i = (self._slot_i + 1) % len(self._slots)
        if slot['ev'] is not None:
            slot['ev'].synchronize()          # the copies issued from this slot len(_slots) steps ago have executed

        def stage(boxes, which, dev_boxes, labels=None):
            """Offsets go through the pinned slot (shapes are host data); box/label payloads that already live on the
            GPU are concatenated there (no D2H round trip), host payloads go through the slot."""
            off, counts = slot['off'], [int(b.shape[0]) for b in boxes]
            tot = sum(counts)
            assert tot <= self.max_gt, f'more than {self.max_gt} boxes in one batch'
            off[which, 0] = 0
            for i, k in enumerate(counts):
                off[which, i + 1] = off[which, i] + k
            on_dev = tot > 0 and all(b.is_cuda for b, k in zip(boxes, counts) if k)
            if tot and on_dev:
                dev_boxes[:tot].copy_(torch.cat([b.reshape(-1, 4) for b, k in zip(boxes, counts) if k]).float())
                if labels is not None:
                    self.gt_labels[:tot].copy_(torch.cat([l.reshape(-1) for l, k in zip(labels, counts) if k]).long())
            elif tot:
                pos = 0
                for i, (b, k) in enumerate(zip(boxes, counts)):
                    if k:
                        slot['boxes'][which, pos:pos + k].copy_(b.reshape(-1, 4))
                        if labels is not None:
                            slot['labels'][pos:pos + k].copy_(labels[i].reshape(-1))
                    pos += k
                dev_boxes[:tot].copy_(slot['boxes'][which, :tot], non_blocking=True)
                if labels is not None:
                    self.gt_labels[:tot].copy_(slot['labels'][:tot], non_blocking=True)
            return tot

        stage(gt_bboxes, 0, self.gt_boxes, gt_labels)
        self.gt_off.copy_(slot['off'][0], non_blocking=True)
        if self.atss is not None:
            for i, ps in enumerate(pad_shapes):
                slot['pad'][i, 0], slot['pad'][i, 1] = int(ps[0]), int(ps[1])
            self.pad_shapes.copy_(slot['pad'], non_blocking=True)
        if gt_bboxes_ignore is not None:
            assert len(gt_bboxes_ignore) == self.n
            stage(gt_bboxes_ignore, 1, self.ig_boxes)
            self.ig_off.copy_(slot['off'][1], non_blocking=True)
            ops.set_ptrs(self.desc, ig_boxes=self.ig_boxes, ig_off=self.ig_off)
        else:
            ops.set_ptrs(self.desc, ig_boxes=None, ig_off=None)
        if self.gt_off.is_cuda:
            slot['ev'] = torch.cuda.Event()
            slot['ev'].record()

    def configure(self, loss_weight=1.0, soft_weight=0.0, grad_scale=1.0, inv_world=1.0):
        d = self.desc
        d.loss_weight, d.soft_weight, d.grad_scale, d.inv_world = loss_weight, soft_weight, grad_scale, inv_world

    def bind_outputs(self, cls_logits, regctr, scales):
        ops.set_ptrs(self.desc, cls_logits=cls_logits, regctr=regctr, scales=scales)
        if self.ctr_col is not None:
            self.desc.ctr, self.desc.ld_ctr = self.desc.cls_logits + 4 * self.ctr_col, self.LD_CLS

    def bind_prior(self, mean, sigma, g_mean, g_sigma):
        """AutoAssign only: the addresses of center_prior.mean / .sigma ([C][2] fp32 each) and of their gradients."""
        self.aa.mean, self.aa.sigma, self.aa.g_mean, self.aa.g_sigma = mean, sigma, g_mean, g_sigma

    def bind_soft(self, regctr, ld, scales):
        """LD only: the teacher's box predictor output (fp32 [M][ld], the layout of bind_outputs' regctr) and its five Scale values."""
        self.ld.soft, self.ld.ld_soft, self.ld.soft_scales = L.ptr(regctr), ld, L.ptr(scales)
        self._soft_keep = (regctr, scales)

    def assign(self):
        L.check(L.lib.dsl_head_assign(C.byref(self.desc), L.stream_ptr()), 'dsl_head_assign')

    def middle(self):
        """The kind's pass between the predictors and the loss, what its op runs.  GFL / LD: score / weight of the positives and
        stats[1] = sum of the weights; PAA: the candidates' losses, then the mixture fit and the reassignment."""
        for name in self.kind.middle[1]:
            L.check(getattr(L.lib, name)(C.byref(self.ext), L.stream_ptr()), name)

    quality = refine = middle

    def loss(self):
        """The entry point of the descriptor this plan built, not dsl_head_loss's choice by head_flags: a dsl_ld_desc whose flags lost
        DSL_HEAD_LD is then refused by dsl_ld_loss instead of running as a GFL head."""
        name = self.kind.loss_entry
        L.check(getattr(L.lib, name)(C.byref(self.desc), L.stream_ptr()), name)

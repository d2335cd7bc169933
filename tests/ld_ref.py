"""Torch (CPU) model of the LD head as include/dsl_hip.h states it (no reference files are read here): tests/gfl_ref.py's losses plus
the Localization Distillation term - a temperature-scaled KL divergence between a frozen teacher's and the student's box
distributions over the positives - in the dtype of the inputs (float64 with autograd in the tests).

Everything is level-major [level][image][y][x].  test_ld_cpu.py pins this model to the fixtures tests/golden/ld_*.npz, which hold what
the reference's own LDHead.loss computed."""
import torch

import gfl_ref as GR

STRIDES, SIZES = GR.STRIDES, GR.SIZES


def kd_rows(z, s, T):
    """[K, R] student and teacher logits (both behind their Scale) -> [K] T^2 * mean_j t_j (log t_j - log p_j), t = softmax(s / T),
    p = softmax(z / T); a term with t_j == 0 is 0.  The teacher is a constant."""
    t = (s.detach() / T).softmax(-1)
    logp = (z / T).log_softmax(-1)
    logt = (s.detach() / T).log_softmax(-1)
    term = torch.where(t > 0, t * (logt - logp), torch.zeros_like(t))
    return term.mean(-1) * (T * T)


def loss(cls, raw, scales, soft, soft_scales, asg, sizes, n, T=10.0, ld_weight=0.25, num_classes=80, reg_max=16, strides=STRIDES, **kw):
    """gfl_ref.loss plus loss_ld.  soft [M, 4 (reg_max + 1)]: the teacher's box predictor output in front of its Scale, soft_scales [5].
    loss_ld = ld_weight / 4 * sum_pos weight[m] sum_k kd(m, k): NOT divided by the weight sum (ld_head.py:253-261), so it does not
    depend on `world` / `norm`.  Returns (loss_cls, loss_bbox, loss_dfl, loss_ld) and gfl_ref's (score, weight, weight sum)."""
    l_cls, l_box, l_dfl, q = GR.loss(cls, raw, scales, asg, sizes, n, num_classes=num_classes, reg_max=reg_max, strides=strides, **kw)
    pos, _, _, _, z, lvl = GR.decode_pos(raw, scales, asg, sizes, n, reg_max, num_classes, strides)
    if len(pos) == 0:
        return l_cls, l_box, l_dfl, raw.sum() * 0, q
    R = reg_max + 1
    s = soft.detach()[pos] * soft_scales.detach()[lvl][:, None]
    kd = kd_rows(z.reshape(-1, R), s.reshape(-1, R).to(z.dtype), T).reshape(-1, 4)
    l_ld = (kd.sum(1) * q[1][pos]).sum() / 4.0 * ld_weight
    return l_cls, l_box, l_dfl, l_ld, q

"""What each head kind puts into its loss and detection descriptors, field by field, against tests/golden/head_signature.txt - the
output of this file on the commit before the head-kind table (params.HEAD_KINDS), where every site derived the kind by itself.
The existing descriptor tests spot-check a few fields per head; this one pins every field of the outermost struct, the nested
structs and the dsl_atss_desc behind the pointer, the predictors' state_dict names and HeadOptions.key() / flags() / repr().
Pointers are printed as <plan attribute>+<byte offset>, 0 (null) or H (a host structure)."""
import ctypes as C
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]          # (run as a script, this file prints the signature)
from dsl_amd import _lib as L  # noqa: E402
from dsl_amd import sweep  # noqa: E402
from dsl_amd.head_loss import FcosLossPlan  # noqa: E402
from dsl_amd.params import HeadOptions, ParamStore  # noqa: E402
import plan_signature as PS  # noqa: E402

N, SIZES, STRIDES, RANGES, MAX_GT, NUM_CLASSES = 2, [(4, 6), (2, 3)], (8, 16), ((-1, 64), (64, 1e8)), 64, 3
M = N * sum(h * w for h, w in SIZES)
HEADS = [
    ('default', lambda: HeadOptions()),
    ('plain', lambda: HeadOptions(False, False, False, True, False)),
    ('loss family', lambda: HeadOptions(box_loss='diou', box_eps=1e-5, focal_gamma=1.5, focal_alpha=0.3, cls_weight=0.75, bbox_weight=2.0,
                                        ctr_weight=0.5)),
    ('atss', lambda: HeadOptions(assigner='atss', atss_topk=5, anchor_scale=4.0, delta_stds=(0.1, 0.2, 0.3, 0.4))),
    ('gfl reg_max=15', lambda: HeadOptions(head_kind='gfl', reg_max=15, qfl_beta=1.5, dfl_weight=0.5, bbox_weight=2.0)),
    ('gfl reg_max=16', lambda: HeadOptions(head_kind='gfl', reg_max=16)),
    ('ld', lambda: HeadOptions(head_kind='gfl', reg_max=16, ld_weight=0.5, ld_T=4.0)),
    ('paa', lambda: HeadOptions(head_kind='paa', atss_topk=3, anchor_scale=4.0, bbox_weight=1.3, pos_iou_thr=0.2, score_voting=False)),
    ('fovea', lambda: HeadOptions(head_kind='fovea', sigma=0.5, base_edge_list=(8, 16, 32, 64, 128), smooth_l1_beta=0.2, conv_bias=False,
                                  focal_gamma=1.5)),
    ('autoassign', lambda: HeadOptions(head_kind='autoassign', bbox_weight=2.0, pos_loss_weight=0.5, neg_loss_weight=0.6,
                                       center_loss_weight=0.7)),
]


class Names:
    """Pointer -> '<attribute>+<offset>' of the first tensor (attributes in sorted order) that contains it."""

    def __init__(self, *holders):
        self.spans = sorted((k, t.data_ptr(), t.numel() * t.element_size()) for h in holders for k, t in h.items() if torch.is_tensor(t))

    def __call__(self, ptr):
        ptr = int(ptr or 0)
        if not ptr:
            return '0'
        return next((f'{k}+{ptr - lo}' for k, lo, nb in self.spans if lo <= ptr < lo + nb), 'H')


def detect_plan(st, bound):
    """sweep._detplan's plan for the store, bound as it binds it: the detector and the forward plan are stand-ins with what it reads."""
    det = types.SimpleNamespace(bbox_head=types.SimpleNamespace(strides=STRIDES), test_cfg=dict(nms_pre=50, max_per_img=20))
    return sweep._detplan(det, types.SimpleNamespace(level_sizes=SIZES, bufs=bound), st, N)


def struct_lines(prefix, names, s, atss_ptr=None):
    """One line per field; a nested struct's fields follow under <field>., the dsl_atss_desc behind `atss_ptr` under *atss."""
    out = []
    for n, t in s._fields_:
        if issubclass(t, C.Structure):
            out += struct_lines(f'{prefix}.{n}', names, getattr(s, n))
        elif n not in ('pad', 'pad_'):          # (alignment fillers; dsl_atss_desc.pad_shapes is a field)
            out.append(f'{prefix}.{n}={PS.val(names, t, getattr(s, n))}')
    if atss_ptr:
        out += struct_lines(f'{prefix}.*atss', names, C.cast(atss_ptr, C.POINTER(L.AtssDesc)).contents)
    return out


def signature():
    lines = []
    for name, make in HEADS:
        o = make()
        st = ParamStore(NUM_CLASSES, 'cpu', head=o)
        bound = dict(cls_logits=torch.zeros(M, st.logit_ld), regctr=torch.zeros(M, st.reg_ld), scales=torch.ones(8),
                     soft=torch.zeros(M, st.reg_ld), soft_scales=torch.ones(8))
        lp = FcosLossPlan(N, SIZES, 'cpu', strides=STRIDES, ranges=RANGES, num_classes=NUM_CLASSES, max_gt=MAX_GT, head=o)
        lp.bind_outputs(bound['cls_logits'], bound['regctr'], bound['scales'])
        if o.ld_weight is not None:
            lp.bind_soft(bound['soft'], st.reg_ld, bound['soft_scales'])
        outer = PS.head_desc(types.SimpleNamespace(desc=C.addressof(lp.desc)))
        lines.append(f'#### {name}')
        lines += struct_lines(f'loss {type(outer).__name__}', Names(vars(lp), bound), outer, lp.desc.atss)
        lines.append(f'loss logvec={lp.logvec.numel()} LD={(lp.LD_CLS, lp.LD_GCLS, lp.LD_RC, lp.LD_GRC)} ctr_col={lp.ctr_col}')
        dp = detect_plan(st, bound)
        outer = getattr(dp, '_ext', dp.desc)          # (the struct around `desc`, where the head has one)
        lines += struct_lines(f'det {type(outer).__name__}', Names(vars(dp), bound, dict(train=st.train)), outer,
                              dp.atss and C.addressof(dp.atss))
        lines.append(f'store rows={(st.cls_rows, st.cls_pad, st.logit_ld, st.reg_rows, st.reg_pad, st.reg_ld)}')
        lines.append('predictors ' + ' '.join(k for k in st.named_views() if k.startswith('bbox_head.') and '_convs.' not in k and '.scales.' not in k))
        lines += [f'key {o.key()!r}', f'flags {o.flags()}', f'repr {o!r}']
    return lines


def test_every_descriptor_field_equals_the_commit_before_the_table():
    with open(os.path.join(ROOT, 'tests', 'golden', 'head_signature.txt')) as fh:
        want = fh.read().splitlines()
    got = signature()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'line {k + 1}'
    assert len(got) == len(want)


if __name__ == '__main__':
    print('\n'.join(signature()))

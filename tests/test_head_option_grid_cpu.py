"""The configuration surface of params.HeadOptions, walked as a grid, against tests/golden/head_option_grid.txt - the output of this
file on the commit before HeadOptions took its defaults from its signature and its "does not read" refusals from one table.  Eight
bases (one per head kind, and the plain FCOS head), each alone and then with one option at a time set to each of its alternatives:
accepted values, list spellings of the sequence defaults, and every refusal the constructor has - out of range, wrong type, wrong
length, nan / inf.  A line holds the exception's type and message, or everything the resulting object answers: the kind, flags(),
reg_layout(), has_scale(), has_prior(), is_default(), key(), repr() and every instance attribute - in full for a base, for a case
those that differ from its base's, so that the file shows what an option changes.  The per-head tests spot-check
a few refusals each; this one pins which kind refuses what, the stored values and which message wins."""
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]          # (run as a script, this file prints the grid)
from dsl_amd.params import HeadOptions  # noqa: E402

NAN, INF = float('nan'), float('inf')
BASES = [
    ('fcos', dict()),
    ('plain', dict(center_sampling=False, norm_on_bbox=False, centerness_on_reg=False, iou_loss=True, conv_bias=False)),
    ('atss', dict(assigner='atss')),
    ('gfl', dict(head_kind='gfl')),
    ('ld', dict(head_kind='gfl', ld_weight=0.25)),
    ('paa', dict(head_kind='paa')),
    ('fovea', dict(head_kind='fovea')),
    ('autoassign', dict(head_kind='autoassign')),
]
RANGES = ((8, 32), (16, 64), (32, 128), (64, 256), (128, 512))
# per option: an accepted value off the default (where there is one), the list spellings of the sequence defaults, and one value per
# distinct refusal - out of range, nan or inf, wrong type, wrong length
ALTERNATIVES = [
    ('center_sampling', (False, True)),
    ('norm_on_bbox', (False, True)),
    ('centerness_on_reg', (False, True)),
    ('iou_loss', (True, False)),
    ('conv_bias', (False, True)),
    ('box_loss', ('giou', 'iou_linear', 'diou', 'l1')),
    ('box_eps', (1e-5,)),
    ('focal_gamma', (1.5,)),
    ('focal_alpha', (0.3,)),
    ('cls_weight', (0.75,)),
    ('bbox_weight', (2.0, -1.0, NAN, 'x')),
    ('ctr_weight', (0.5,)),
    ('assigner', ('atss', 'max_iou')),
    ('atss_topk', (5, 0, 17)),
    ('anchor_scale', (4.0, 0.0, INF)),
    ('delta_stds', ((0.1, 0.2, 0.3, 0.4), [0.1, 0.1, 0.2, 0.2], (0.1, 0.1, 0.2), (0.1, 0.1, 0.2, 0.0), (0.1, 0.1, 0.2, NAN))),
    ('head_kind', ('gfl', 'paa', 'fovea', 'autoassign', 'retina')),
    ('reg_max', (15, 0, 17, 8.0)),
    ('qfl_beta', (1.5, -1.0, INF)),
    ('dfl_weight', (0.5, -1.0, NAN)),
    ('ld_weight', (0.5, -1.0, INF, 'x')),
    ('ld_T', (4.0, 0.5, NAN, 'x')),
    ('pos_iou_thr', (0.2, 1.0, NAN, 'x')),
    ('score_voting', (False,)),
    ('sigma', (0.5, 0.0, 1.5, NAN, 'x')),
    ('base_edge_list', ((8, 16, 32, 64, 128), [16, 32, 64, 128, 256], (16, 32, 64, 128), (16, 32, 64, 128, 0), (16, 32, 64, 128, INF))),
    ('scale_ranges', (((1, 64), (32, 128), (64, 256), (128, 512), (256, 2048)), [[8, 32], [16, 64], [32, 128], [64, 256], [128, 512]],
                      RANGES[:4], RANGES[:4] + ((128, 512, 1024),), RANGES[:4] + ((512, 128),))),
    ('smooth_l1_beta', (0.2, 0.0, INF, 'x')),
    ('pos_loss_weight', (0.5, -1.0, NAN, 'x')),
    ('neg_loss_weight', (0.6, -1.0)),
    ('center_loss_weight', (0.7, -1.0)),
]


def facts(kw):
    """Everything HeadOptions(**kw) answers, as (name, text) pairs in a fixed order; or the exception's type and message."""
    try:
        o = HeadOptions(**kw)
    except Exception as e:  # noqa: BLE001 - the grid records whatever the constructor raises
        return f'{type(e).__name__}: {e}'
    return ([('kind', o.kind.name), ('flags', o.flags()), ('reg_layout', o.reg_layout()), ('has_scale', o.has_scale()),
             ('has_prior', o.has_prior()), ('is_default', o.is_default()), ('key', o.key()), ('repr', repr(o))]
            + [('.' + k, v) for k, v in sorted(vars(o).items()) if k != 'kind'])


def grid():
    """A base's line holds all its facts; a case's line the refusal, or the facts that differ from its base's (every other fact,
    instance attributes included, equals the base's)."""
    lines = []
    for base, kw in BASES:
        ref = facts(kw)
        lines.append(f'{base} -> ' + ' '.join(f'{k}={v!r}' for k, v in ref))
        for name, values in ALTERNATIVES:
            for v in values:
                if name in kw and kw[name] == v:
                    continue          # (the base itself)
                got = facts(dict(kw, **{name: v}))
                if not isinstance(got, str):
                    assert [k for k, _ in got] == [k for k, _ in ref]
                    got = ' '.join(f'{k}={a!r}' for (k, a), (_, b) in zip(got, ref) if repr(a) != repr(b)) or 'as the base'
                lines.append(f'{base} {name}={v!r} -> {got}')
    return lines


def test_the_alternatives_cover_every_option():
    options = [p for p in inspect.signature(HeadOptions.__init__).parameters if p != 'self']
    assert len(options) == 31 and [name for name, _ in ALTERNATIVES] == options
    assert all(name in options for _, kw in BASES for name in kw)


def test_every_case_of_the_grid_equals_the_commit_before_the_table():
    with open(os.path.join(ROOT, 'tests', 'golden', 'head_option_grid.txt')) as fh:
        want = fh.read().splitlines()
    got = grid()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'line {k + 1}'
    assert len(got) == len(want)


if __name__ == '__main__':
    print('\n'.join(grid()))

"""dsl_groupnorm_relu_fwd / dsl_groupnorm_relu_bwd through the C ABI against the float64 references of tests/op_ref.py (gn_fwd_ref,
gn_bwd_ref) under op_ref's own bars (BF16_REL, BETA['gn']), at the geometries gn_check admits beyond the training step's: other
channel counts and group sizes, ragged and one-pixel levels, up to 255 (level, image) rows, groups of zero variance - on the inputs
of tests/gn_cases.py (offset groups, dY correlated with xhat, no ReLU decision on the edge, gamma with zeros and negative entries,
beta that switches channels off and on).

Every case: workspace filled with 0xff bytes and every output with NaN before each launch, both launches under op_ref.run_checked
(every output's worst |err| / bound <= 1, no byte outside the declared outputs and the workspace changed), then both launches once
more from the same poisoned state with bit-identical outputs (the reductions are fixed-order).

Measured on an MI355X, worst |err| / bound per output class over all cases (each test prints its own figures):
  y 0.989 and dx 0.991: the bf16 rounding of the output itself, which the bar's 2^-8 |ref| part prices at its worst case;
  (mean, rstd) 0.019 (64 channels in 2 groups; 0.018 at 2048 in 32, at most 0.011 elsewhere), at |mean| / sigma up to 20;
  dgamma 0.0071, dbeta 0.0040, dbias 0.0092 (all three in case F's zero image; 0.0058, 0.0037, 0.0040 elsewhere).
  A zero-variance group's rstd has a bar of 0: case F runs at eps = 2^-16, where 1 / sqrt(eps) = 256 is an fp32 value.
  Controls: dbias without m1 4619 / 79 (case A / 65 rows), without m2 461 / 74, dx with a foreign m1 5.7e4 / 4.8e4.
  Before the parameter-gradient row of gn_bwd_apply_kernel summed more group-sum columns than it has threads, dbias (and nothing
  else) of case D stood at 9.7e12 (65 rows), 1.9e31 (130), 58.5 (255) and 2.2e22 (130 rows, 16 channels per group) of its bar,
  with 60 rows at 6.4e-5; now 9.0e-5, 8.6e-5, 7.5e-5 and 1.1e-4.
"""
import ctypes as C
import functools

import pytest
import torch

import gn_cases
import op_ref
from gn_cases import CHANNELS, FIVE, TINY5

pytestmark = pytest.mark.gpu
F64 = torch.float64
OUTPUTS = ('y', 'stats', 'dx', 'dgamma', 'dbeta', 'dbias')


@pytest.fixture(scope='module')
def K():
    from dsl_amd import _lib as L
    from dsl_amd import ops
    assert torch.cuda.is_available()
    return L, ops


def _tensors(n, segs, c, G, inputs):
    tot = sum(n * h * w for h, w in segs)
    t = dict(zip(('x', 'gamma', 'beta', 'dy'), (v.cuda() for v in inputs)))
    t['y'] = torch.empty(tot * c, dtype=torch.bfloat16, device='cuda')
    t['dx'] = torch.empty_like(t['y'])
    t['stats'] = torch.empty(len(segs) * n * G * 2, device='cuda')
    t['dgamma'], t['dbeta'], t['dbias'] = (torch.empty(c, device='cuda') for _ in range(3))
    return t


def _desc(K, t, n, segs, c, G, dbias=True, eps=1e-5):
    L, ops = K
    d = ops.gn_desc(t['x'], t['y'], t['gamma'], t['beta'], t['stats'], n=n, hw=list(segs), c=c, groups=G, eps=eps, dy=t['dy'], dx=t['dx'],
                    dgamma=t['dgamma'], dbeta=t['dbeta'], dbias=t['dbias'] if dbias else None)
    t['workspace'] = d._keep[5]
    return d


def _poison(t):
    t['workspace'].fill_(0xff)
    for k in OUTPUTS:
        t[k].fill_(float('nan'))


def _bits(v):
    return v.view(torch.uint8).clone()


@functools.lru_cache(maxsize=None)
def _run(n, segs, c=256, G=32, dbias=True, seed=0, zero=(), eps=1e-5):
    """Both launches of one case under the check, then once more for the bits.  -> (results [(output, worst ratio, elements over
    the bar, index)], the tensors, the resolver, the backward's LaunchRef); cached, so that tests which share a case launch it once."""
    from dsl_amd import _lib as L
    from dsl_amd import ops
    t = _tensors(n, segs, c, G, gn_cases.gn_inputs(n, segs, c, G, seed=seed, zero=zero, eps=eps))
    d = _desc((L, ops), t, n, segs, c, G, dbias, eps)
    mem = op_ref.Memory({'t': t})

    def fwd():
        L.check(L.lib.dsl_groupnorm_relu_fwd(C.byref(d), L.stream_ptr()), 'dsl_groupnorm_relu_fwd')
        torch.cuda.synchronize()

    def bwd():
        L.check(L.lib.dsl_groupnorm_relu_bwd(C.byref(d), L.stream_ptr()), 'dsl_groupnorm_relu_bwd')
        torch.cuda.synchronize()

    _poison(t)
    res = op_ref.run_checked(mem, op_ref.gn_fwd_ref(mem, d), fwd)
    lr = op_ref.gn_bwd_ref(mem, d)                     # (from the stored statistics)
    t['workspace'].fill_(0xff)
    res += op_ref.run_checked(mem, lr, bwd)
    first = {k: _bits(t[k]) for k in OUTPUTS}
    _poison(t)
    fwd()
    t['workspace'].fill_(0xff)
    bwd()
    same = {k: bool(torch.equal(first[k], _bits(t[k]))) for k in OUTPUTS}
    if not dbias:                                      # not asked for: not written
        assert bool(torch.isnan(t['dbias']).all())
    return res, same, t, mem, lr


def _assert_case(tag, n, segs, **kw):
    res, same, *_ = _run(n, tuple(segs), **kw)
    over = []
    for name, ratio, nbad, worst in res:
        print(f'GN {tag} {name} worst |err| / bound = {ratio:.4g} ({nbad} over, at {worst})')
        if not ratio <= 1.0:
            over.append((name, ratio, nbad))
    assert not over, (tag, over)
    assert all(same.values()), (tag, 'a second launch gave other bits', same)


RAGGED = ((3, 43), (8, 16), (1, 127), (1, 1), (1, 17))
SMALL2 = ((5, 7), (2, 3))


def test_case_a_shipped_geometry(K):
    """N = 2, C = 256 / 32 groups, five small levels, with dbias."""
    _assert_case('A', 2, FIVE, seed=1)


def test_case_b_full_blocks_beside_ragged_tails(K):
    """hw 129 / 128 / 127 / 1 / 17: gn_stats_kernel's full-block fast path beside a one-pixel tail block, a 127-pixel block, a
    one-pixel level, and blocks of the grid that lie past their level's end."""
    _assert_case('B', 3, RAGGED, seed=2)


@pytest.mark.parametrize('segs', [((16, 24),), ((1, 1),)], ids=['three-blocks', 'cnt8'])
def test_case_c_single_segment(K, segs):
    """one level, one image: exactly three blocks; and one pixel, the smallest group there is (8 elements).  Without dbias."""
    _assert_case('C', 1, segs, seed=3, dbias=False)


@pytest.mark.parametrize('n,c', [(12, 256), (13, 256), (26, 256), (51, 256), (26, 512)])
def test_case_d_many_rows(K, n, c):
    """S = 5 n (level, image) rows: 60, 65 (the first at which the parameter-gradient row's group sums no longer fit one column per
    thread with 8 channels per group), 130, 255 (gn_check's limit); 130 with 16 channels per group."""
    _assert_case(f'D{5 * n}/C{c}', n, TINY5, c=c, seed=4)


@pytest.mark.parametrize('c,G', CHANNELS)
def test_case_e_channel_counts(K, c, G):
    """other channel counts and group sizes; (1024, 128): gn_sum_records with as many values as threads; (2048, 32): one pixel
    per iteration."""
    _assert_case(f'E{c}/{G}', 2, SMALL2, c=c, G=G, seed=5)


ZERO = dict(group=((1, 1, 3),), image=((None, 0, None),))


@pytest.mark.parametrize('what', ['group', 'image'])
def test_case_f_zero_variance(K, what):
    """case A with x = 0 over one (level, image, group) and over one whole image: var = 0, rstd = 1 / sqrt(eps), y = relu(beta),
    dx = rstd (dz gamma - m1).  At var = 0 op_ref's bar for rstd is beta * rstd * k with k = E[x^2] / (var + eps) = 0: the stored
    rstd has to EQUAL the float64 1 / sqrt(eps).  No fp32 value does that at eps = 1e-5 (measured there: ratio inf on exactly the
    zero groups' rstd, 1 and 160 elements, the value itself within 2^-22 of 1 / sqrt(eps)), so this case runs at eps = 2^-16, where
    1 / sqrt(eps) = 256 is an fp32 value and the reference, not the number format, decides: mean 0 and rstd 256 to the bit."""
    _assert_case('F' + what, 2, FIVE, seed=1, zero=ZERO[what], eps=2.0 ** -16)
    _, _, t, _, _ = _run(2, FIVE, seed=1, zero=ZERO[what], eps=2.0 ** -16)
    stats = t['stats'].view(5, 2, 32, 2)
    z = (stats[1, 1, 3] if what == 'group' else stats[:, 0]).reshape(-1, 2)
    assert bool((z[:, 0] == 0).all()) and bool((z[:, 1] == 256).all())


# ------------------------------------------------------------------------------------------------------------------------------
# the bars see the errors these cases are about
def _backward_variants(t, n, segs, c, G):
    """float64, from the launch's own inputs and stored statistics: dx and dbias as they are, dbias without its m1 term, dbias
    without its m2 term, dx with m1 of the neighbouring group."""
    cpg = c // G
    g4, b4 = t['gamma'].to(F64).view(1, 1, G, cpg), t['beta'].to(F64).view(1, 1, G, cpg)
    stats = t['stats'].to(F64).view(len(segs), n, G, 2)
    dx, dx_m1n, dbias, no_m1, no_m2 = [], [], 0, 0, 0
    off = 0
    for s, (h, w) in enumerate(segs):
        hw = h * w
        xs = t['x'][off * c:(off + n * hw) * c].to(F64).view(n, hw, G, cpg)
        gs = t['dy'][off * c:(off + n * hw) * c].to(F64).view(n, hw, G, cpg)
        off += n * hw
        mean, rstd = stats[s, :, :, 0].view(n, 1, G, 1), stats[s, :, :, 1].view(n, 1, G, 1)
        xh = (xs - mean) * rstd
        dzg = gs * (xh * g4 + b4 > 0) * g4
        m1 = dzg.sum((1, 3), keepdim=True) / (hw * cpg)
        m2 = (dzg * xh).sum((1, 3), keepdim=True) / (hw * cpg)
        dx.append((rstd * (dzg - m1 - xh * m2)).reshape(-1, c))
        dx_m1n.append((rstd * (dzg - m1.roll(1, 2) - xh * m2)).reshape(-1, c))
        dbias = dbias + dx[-1].sum(0)
        no_m1 = no_m1 + (rstd * (dzg - xh * m2)).sum((0, 1)).reshape(c)
        no_m2 = no_m2 + (rstd * (dzg - m1)).sum((0, 1)).reshape(c)
    return torch.cat(dx), dbias, no_m1, no_m2, torch.cat(dx_m1n)


@pytest.mark.parametrize('n,segs,seed', [(2, FIVE, 1), (13, TINY5, 4)], ids=['A', 'D65'])
def test_the_bars_flag_a_missing_or_foreign_group_mean(K, n, segs, seed):
    """dbias without m1, dbias without m2, and dx with the neighbouring group's m1, put in the reference's place: check_out must
    flag the kernel's output against each (and does not against the same formulas left whole)."""
    res, same, t, mem, lr = _run(n, segs, seed=seed)
    o = {k.name.split('.')[-1]: k for k in lr.outs}
    dx, dbias, no_m1, no_m2, dx_m1n = _backward_variants(t, n, segs, 256, 32)
    assert torch.allclose(dx, o['dx'].ref, rtol=1e-12, atol=1e-12 * float(dx.abs().max()))
    assert torch.allclose(dbias, o['dbias'].ref, rtol=1e-12, atol=1e-12 * float(dbias.abs().max()))
    for name, like, ref in (('dbias without m1', 'dbias', no_m1), ('dbias without m2', 'dbias', no_m2),
                            ('dx with a foreign m1', 'dx', dx_m1n)):
        k = o[like]
        wrong = op_ref.Out(k.name, k.ptr, k.dtype, k.idx, ref.view_as(k.ref), k.S, k.beta)
        ratio, nbad, _ = op_ref.check_out(mem, wrong)
        print(f'GN control {name}: worst |err| / bound = {ratio:.4g}, {nbad} of {k.ref.numel()} over')
        assert nbad > 0 and ratio > 1, name


# ------------------------------------------------------------------------------------------------------------------------------
# what gn_check refuses (before any launch: the outputs stay as they were)
REFUSALS = {
    '260 rows': (dict(n=52, segs=TINY5, c=256, G=32), 'more than 256'),
    '4 channels per group': (dict(n=2, segs=SMALL2, c=128, G=32), 'channels per group'),
    'C = 96': (dict(n=2, segs=SMALL2, c=96, G=4), 'unsupported C=96'),
    '256 groups': (dict(n=2, segs=SMALL2, c=2048, G=256), '2*groups=512'),
    'conv_stats with 16 channels per group': (dict(n=2, segs=SMALL2, c=512, G=32, conv_stats=1), 'conv_stats needs 8 channels per group'),
    'workspace one byte short': (dict(n=2, segs=SMALL2, c=256, G=32, short=1), 'workspace too small'),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refusals(K, what):
    L, ops = K
    (geo, text), extra = REFUSALS[what], {}
    geo = dict(geo)
    for k in ('conv_stats', 'short'):
        extra[k] = geo.pop(k, 0)
    n, segs, c, G = geo['n'], geo['segs'], geo['c'], geo['G']
    tot = sum(n * h * w for h, w in segs)
    inputs = (torch.zeros(tot * c, dtype=torch.bfloat16), torch.ones(c), torch.zeros(c), torch.zeros(tot * c, dtype=torch.bfloat16))
    t = _tensors(n, segs, c, G, inputs)
    d = _desc(K, t, n, segs, c, G)
    d.conv_stats = extra['conv_stats']
    d.workspace_bytes -= extra['short']
    _poison(t)
    for fn in (L.lib.dsl_groupnorm_relu_fwd, L.lib.dsl_groupnorm_relu_bwd):
        assert fn(C.byref(d), L.stream_ptr()) != 0
        assert text in L.lib.dsl_last_error().decode(), L.lib.dsl_last_error().decode()
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bool(torch.isnan(t[k]).all()), k
    assert bool((t['workspace'] == 0xff).all())

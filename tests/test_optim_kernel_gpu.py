"""dsl_optim_step through the C ABI against the float64 restatement, element by element.

The bound is not a flat rtol: tests/optim_ref.py follows optim_kernel (dsl_amd/csrc/optim.hip) operation by operation.  Each fp32
multiply, add, divide and square root is within u = 2^-24 of its own result (no fast-math: / and sqrtf are correctly rounded;
FMA contraction only removes roundings), and the operands' bounds travel through each operation's derivative.  Written out for
one element of group k with table row (lr, wd), e(x) the bound of x, inputs exact:
    clip  = min(max_norm / (sqrt(gnorm_sq) + 1e-6), 1)       e = 3 u clip  (sqrt, add, divide; none without clipping)
    d0    = g clip                                           e = |g| e(clip) + u |d0|
  SGD
    d     = d0 + wd p                                        e = e(d0) + u |wd p| + u |d|
    m'    = d (first step) or mom m + d                      e = e(d) [+ u |mom m| + u |m'|]
    upd   = m', Nesterov: d + mom m'                         e = e(d) + mom e(m') + u |mom m'| + u |upd|
    p'    = p - lr upd                                       e = lr e(upd) + u |lr upd| + u |p'|
  Adam kinds  (step = lr step_scale, e = u step;  AdamW: p <- p (1 - lr wd), three roundings, and d = d0)
    m'    = b1 m + (1 - b1) d                                e = u |b1 m| + u |1 - b1| |d| + (1 - b1) e(d) + u |(1 - b1) d| + u |m'|
    v'    = b2 v + ((1 - b2) d) d                            likewise, d's bound entering twice
    den   = sqrt(v') rsqrt_bc2 + eps                         e = rsqrt_bc2 (sqrt(v') e(v') / (2 v') + u sqrt(v')) + u |sqrt(v') rsqrt_bc2| + u den
    q     = m' / den                                         e = (e(m') + |q| e(den)) / den + u |q|
    p'    = p - step q                                       e = e(p) + step e(q) + |q| e(step) + u |step q| + u |p'|
The bounds of m' and v' are thereby carried into p' (the kernel's update reads the moments it stores), as HostRef.check of
test_bucket_update_gpu.py carries lr_e * em.  The bar is TWICE the bound: the margin for the second-order terms.  Inputs keep every
intermediate normal (|g| in [1e-12, 1e3] or exactly 0, |p| in [1e-3, 10], v >= 1e-12 or 0), so u |z| holds for every operation.
(optim_ref adds 2^-149 per operation for a result that underflows all the same: the step tests feed real gradients.)
p16 = bf16(p') bit for bit; where a zero gradient meets zero moments the bound is a few denormals wide, i.e. the result is exact."""
import ctypes as C

import pytest
import torch

import optim_ref as R
from optim_ref import REFUSALS, refused_call

pytestmark = pytest.mark.gpu

# sgd_kernel's and optim_kernel's grid is nblocks(n / 4, 4096) x 256: one float4 | a ragged second block | the smallest n at which
# the grid stride wraps (about 17 MB per fp32 buffer)
SIZES = [4, 1028, 4 * (4096 * 256 + 3)]
KINDS = ['sgd', 'nesterov', 'adam', 'adamw']
LR0, WD0 = 2e-3, 1e-4


def _table():
    """16 groups, each its own rate; a quarter of them without decay."""
    return [LR0 * (0.5 + k / 8) for k in range(16)], [WD0 * (k % 4) / 2 for k in range(16)]


def _logu(gen, n, lo, hi):
    return 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo)


def _sign(gen, n):
    return torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()


def _inputs(n, later, seed):
    gen = torch.Generator().manual_seed(seed)
    g = _logu(gen, n, -12, 3) * _sign(gen, n)
    g[torch.rand(n, generator=gen) < 0.1] = 0.0
    p = _logu(gen, n, -3, 1) * _sign(gen, n)
    if later:
        m = _logu(gen, n, -6, 1) * _sign(gen, n)
        v = _logu(gen, n, -12, 2)
    else:
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    grp = torch.randint(0, 16, (n,), generator=gen, dtype=torch.uint8)
    grp[:4] = torch.tensor([0, 5, 10, 15], dtype=torch.uint8)          # four ids inside one float4
    if n >= 64:
        grp[n - 16:] = torch.arange(16, dtype=torch.uint8)             # all 16 present
        assert grp.unique().numel() == 16
    return [t.float() for t in (p, g, m, v)] + [grp]


def _desc(kind, later, clip):
    from dsl_amd import _lib as L
    d = L.OptimDesc()
    d.kind = dict(sgd=L.OPT_SGD, nesterov=L.OPT_SGD, adam=L.OPT_ADAM, adamw=L.OPT_ADAMW)[kind]
    d.n_groups = 16
    lr, wd = _table()
    for k in range(16):
        d.lr[k], d.wd[k] = lr[k], wd[k]
    d.momentum, d.nesterov, d.first_step = 0.9, int(kind == 'nesterov'), int(not later)
    hp = R.adam_hp(0.9, 0.999, 1e-8, 100000 if later else 1)
    d.beta1, d.beta2, d.eps, d.step_scale, d.rsqrt_bc2 = hp['beta1'], hp['beta2'], hp['eps'], hp['step_scale'], hp['rsqrt_bc2']
    # clip: None | 'above' (coefficient 500: clipped to exactly 1) | 'below' (0.35)
    d.max_norm = dict(above=1e3, below=0.7).get(clip, 0.0)
    if kind in ('sgd', 'nesterov'):
        hp = R.sgd_hp(0.9, kind == 'nesterov', not later)
    return d, hp


def _launch(d, p, g, m, v, p16, grp, gn):
    from dsl_amd import _lib as L
    L.check(L.lib.dsl_optim_step(C.byref(d), L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p16), L.ptr(grp), p.numel(), L.ptr(gn),
                                 L.stream_ptr()), 'dsl_optim_step')


def _run(kind, n, later, clip, with_p16, seed, worst):
    p0, g, m0, v0, grp = _inputs(n, later, seed)
    d, hp = _desc(kind, later, clip)
    adam = kind in ('adam', 'adamw')
    dev = [t.cuda() for t in (p0, g, m0, v0, grp)]
    p16 = torch.full((n,), 7.0, dtype=torch.bfloat16, device='cuda') if with_p16 else None
    gn = torch.tensor([4.0], device='cuda') if clip else None
    _launch(d, dev[0], dev[1], dev[2], dev[3] if adam else None, p16, dev[4], gn)
    torch.cuda.synchronize()
    lr, wd = _table()
    lr_e = torch.tensor([R.f32(x) for x in lr], dtype=torch.float64)[grp.long()]
    wd_e = torch.tensor([R.f32(x) for x in wd], dtype=torch.float64)[grp.long()]
    ref = R.update(dict(sgd=R.SGD, nesterov=R.SGD, adam=R.ADAM, adamw=R.ADAMW)[kind], hp, p0.double(), g.double(), m0.double(),
                   v0.double() if adam else None, lr_e, wd_e, R.clip_coef(4.0, d.max_norm) if clip else None)
    where = f'{kind} n={n} later={later} clip={clip} p16={with_p16}'
    for name, got in (('p', dev[0]), ('m', dev[2])) + ((('v', dev[3]),) if adam else ()):
        err = (got.cpu().double() - ref[name].x).abs()
        bad = err > 2 * ref[name].e
        assert not bool(bad.any()), f'{where}: {name} beyond twice the rounding bound on {int(bad.sum())} elements, first {int(bad.nonzero()[0])}: ' \
            f'err {float(err[bad][0]):.3e} bound {float(ref[name].e[bad][0]):.3e}'
        nz = ref[name].e > 0
        if nz.any():
            worst[name] = max(worst.get(name, 0.0), float((err[nz] / ref[name].e[nz]).max()))
    if not adam:
        assert torch.equal(dev[3].cpu(), v0), f'{where}: the SGD kind touched v'
    assert bool((dev[0].cpu() != p0).float().mean() > 0.25), f'{where}: the update did not run'
    assert torch.equal(dev[1].cpu(), g) and torch.equal(dev[4].cpu(), grp), f'{where}: an input buffer changed'
    if with_p16:
        assert torch.equal(p16.view(torch.int16), dev[0].bfloat16().view(torch.int16)), f'{where}: p16 != bf16(p)'
    return dev


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_optim_step_vs_float64_restatement(kind, n):
    """First and later step (Adam kinds: t = 1 and t = 100000) x no clip / coefficient above 1 / below 1 x p16 given or NULL;
    the 4 M-element size runs the two combinations that between them cover every option."""
    combos = [(later, clip, p16) for later in (False, True) for clip in (None, 'above', 'below') for p16 in (True, False)]
    if n > 100000:
        combos = [(False, 'below', True), (True, None, False)]
    worst = {}
    for i, (later, clip, with_p16) in enumerate(combos):
        _run(kind, n, later, clip, with_p16, 100 + i, worst)
    print(f'{kind} n={n}: worst |err| / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('kind', KINDS)
def test_all_zero_buffers_stay_zero(kind):
    n = 1028
    d, _ = _desc(kind, True, None)
    bufs = [torch.zeros(n, device='cuda') for _ in range(4)]
    p16 = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    grp = (torch.arange(n) % 16).to(torch.uint8).cuda()
    _launch(d, *bufs, p16, grp, None)
    torch.cuda.synchronize()
    for name, t in zip('pgmv', bufs):
        assert not bool(t.view(torch.int32).any()), f'{kind}: {name} is not all zero bits'
    assert not bool(p16.view(torch.int16).any())


@pytest.mark.parametrize('kind', KINDS)
def test_two_runs_give_identical_bits(kind):
    outs = []
    for _ in range(2):
        dev = _run(kind, 4 * 5000 + 4, True, 'below', True, 7, {})
        outs.append([t.cpu().clone() for t in dev[:4]])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_refusals_launch_nothing():
    """Every refusal of the entry, with real buffers: non-zero, its word in dsl_last_error(), and no buffer changes."""
    n = 16
    bufs = dict(p=torch.full((n,), 1.0, device='cuda'), g=torch.full((n,), 2.0, device='cuda'), m=torch.full((n,), 3.0, device='cuda'),
                v=torch.full((n,), 4.0, device='cuda'), group=torch.ones(n, dtype=torch.uint8, device='cuda'))
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    fake = dict(p=0x10000, g=0x20000, m=0x30000, v=0x40000, group=0x50000)
    for case, word in REFUSALS:
        case = dict(case)
        for k in ('p', 'g', 'm', 'v', 'group'):          # (a misaligned argument: the same offset from the real buffer)
            if isinstance(case.get(k), int):
                case[k] = ptrs[k] + case[k] - fake[k]
        rc, err = refused_call(case, bufs=ptrs)
        assert rc != 0 and b'dsl_optim_step' in err and word in err, (case, rc, err)
    torch.cuda.synchronize()
    for (k, t), want in zip(bufs.items(), (1.0, 2.0, 3.0, 4.0, 1)):
        assert bool((t == want).all()), f'a refused call wrote {k}'

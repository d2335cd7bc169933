"""The optimizer family restated in float64, for the tests of dsl_optim_step and of FlatSGD / FlatAdam beyond plain momentum SGD.

update(): the three formulas of include/dsl_hip.h (torch's single-tensor ones).  Every quantity is a V: its float64 value and a
first-order bound on how far the fp32 kernel (dsl_amd/csrc/optim.hip optim_kernel) may be from it.  The bound follows the kernel
operation by operation: the result z of an fp32 multiply, add, divide or square root is within u = 2^-24 of |z| (round to nearest;
the library is built without fast-math, so / and sqrtf are correctly rounded; a contraction to FMA only removes a rounding), and
the operands' own bounds travel through the operation's derivative:
    x y          |x| e_y + |y| e_x + u |z|
    x + y        e_x + e_y + u |z|
    x / y        (e_x + |z| e_y) / |y| + u |z|
    sqrt(x)      z e_x / (2 x) + u z                  (x > 0; exact at 0)
    min(x, c)    e_x
and, for results below the normal range (gradual underflow: fp32 denormals are kept), each operation adds ETA = 2^-149 absolute.
Inputs (the buffers and the descriptor's fp32 fields) are exact.  The moments the kernel stores are those its weight update reads,
so their bounds are carried into the weight's, as HostRef.check of test_bucket_update_gpu.py carries lr_e * em.  The bound holds
while no intermediate is subnormal (the tests' inputs see to that); a test's bar is TWICE the bound, the margin for the
second-order terms dropped here.  With every bound ignored the values are the plain float64 restatement (test_optim_family_cpu.py
holds it against torch.optim).

mults(): mmcv 1.3.x DefaultOptimizerConstructor's rules restated from parameter names (from memory, as SURVEY section 8a)."""
import ctypes
import math

import torch

U = 2.0 ** -24
ETA = 2.0 ** -149          # the smallest fp32 denormal: what a result that underflows may lose beside u |z|
SGD, ADAM, ADAMW = 0, 1, 2
KINDS = dict(SGD=SGD, Adam=ADAM, AdamW=ADAMW)


def f32(x):
    """The float64 value of x rounded to fp32 (what a c_float field of the descriptor holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


class V:
    def __init__(self, x, e=0.0):
        self.x = torch.as_tensor(x, dtype=torch.float64)
        self.e = torch.as_tensor(e, dtype=torch.float64)

    def __mul__(self, o):
        o = o if isinstance(o, V) else V(o)
        z = self.x * o.x
        return V(z, self.x.abs() * o.e + o.x.abs() * self.e + U * z.abs() + ETA)

    def __add__(self, o):
        o = o if isinstance(o, V) else V(o)
        z = self.x + o.x
        return V(z, self.e + o.e + U * z.abs() + ETA)

    def __sub__(self, o):
        o = o if isinstance(o, V) else V(o)
        z = self.x - o.x
        return V(z, self.e + o.e + U * z.abs() + ETA)

    def __truediv__(self, o):
        o = o if isinstance(o, V) else V(o)
        z = self.x / o.x
        return V(z, (self.e + z.abs() * o.e) / o.x.abs() + U * z.abs() + ETA)

    def sqrt(self):
        z = self.x.sqrt()
        rel = torch.where(self.x > 0, self.e / (2 * self.x.clamp(min=1e-300)), torch.zeros_like(self.x))
        return V(z, z * rel + U * z + ETA)


def clip_coef(gnorm_sq, max_norm):
    """The kernel's clip coefficient from the fp32 squared norm: min(max_norm / (sqrt(gnorm_sq) + 1e-6), 1) - torch's
    clip_grad_norm_, oracle.fcos_oracle.clip_coef's definition."""
    c = V(f32(max_norm)) / (V(f32(gnorm_sq)).sqrt() + f32(1e-6))
    return V(c.x.clamp(max=1.0), c.e)


def update(kind, hp, p, g, m, v, lr, wd, clip=None):
    """One step.  kind: SGD / ADAM / ADAMW; hp: the descriptor's scalars as Python floats ALREADY rounded to what the kernel gets
    (momentum, nesterov, first_step | beta1, beta2, eps, step_scale, rsqrt_bc2); p, g, m, v: float64 tensors (v None for SGD);
    lr, wd: per element (the table row of each element's group), float64; clip: V from clip_coef, or None.  Returns dict(p, m, v)
    of V."""
    p, g, m = V(p), V(g), V(m)
    lr, wd = V(lr), V(wd)
    d0 = g * clip if clip is not None else g          # (the kernel multiplies by exactly 1.0 without clipping)
    if kind == SGD:
        mom = hp['momentum']
        d = d0 + wd * p
        m1 = d if hp['first_step'] else m * mom + d
        upd = d + m1 * mom if hp['nesterov'] else m1
        return dict(p=p - lr * upd, m=m1, v=None)
    v = V(v)
    b1, b2 = V(hp['beta1']), V(hp['beta2'])
    omb1, omb2 = V(1.0) - b1, V(1.0) - b2
    step = lr * hp['step_scale']
    if kind == ADAM:
        d = d0 + wd * p
    else:
        d = d0
        p = p * (V(1.0) - lr * wd)
    m1 = m * b1 + omb1 * d
    v1 = v * b2 + omb2 * d * d
    den = v1.sqrt() * hp['rsqrt_bc2'] + hp['eps']
    return dict(p=p - step * (m1 / den), m=m1, v=v1)


def adam_hp(beta1, beta2, eps, t, fp32=True):
    """The Adam kinds' scalars for step t = 1, 2, ..: the bias corrections in double, then (fp32=True) rounded as the descriptor does."""
    r = f32 if fp32 else float
    return dict(beta1=r(beta1), beta2=r(beta2), eps=r(eps), step_scale=r(1.0 / (1.0 - beta1 ** t)),
                rsqrt_bc2=r(1.0 / math.sqrt(1.0 - beta2 ** t)))


def sgd_hp(momentum, nesterov, first_step, fp32=True):
    return dict(momentum=(f32 if fp32 else float)(momentum), nesterov=bool(nesterov), first_step=bool(first_step))


# ---- parameter groups from names ----------------------------------------------------------------------------------------------
def is_norm(name):
    return ('.gn.' in name) or ('.bn' in name) or ('downsample.1' in name) or ('.stage_bns.' in name)


def mults(name, pw):
    """(lr_mult, decay_mult) of a parameter by its state-dict name.  custom_keys first (alphabetical, then longest first; the first
    key contained in the name decides alone); else bias_lr_mult for a non-norm leaf `bias`; decay: norm_decay_mult for norm
    layers, else bias_decay_mult for a leaf `bias`."""
    ck = pw.get('custom_keys') or {}
    for key in sorted(sorted(ck.keys()), key=len, reverse=True):
        if key in name:
            return float(ck[key].get('lr_mult', 1.0)), float(ck[key].get('decay_mult', 1.0))
    bias = name.endswith('.bias')
    lm = float(pw.get('bias_lr_mult', 1.0)) if bias and not is_norm(name) else 1.0
    if is_norm(name):
        dm = float(pw.get('norm_decay_mult', 1.0))
    else:
        dm = float(pw.get('bias_decay_mult', 1.0)) if bias else 1.0
    return lm, dm


# ---- dsl_optim_step's refusals: one table for the CPU test (fake addresses) and the GPU test (real buffers) -----------------------
P, G, M, V2, GR = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000          # aligned, never dereferenced: every call is refused before a launch


def refusal_desc(kind=0, n_groups=2, **kw):
    from dsl_amd import _lib as L
    d = L.OptimDesc()
    d.kind, d.n_groups, d.momentum = kind, n_groups, 0.9
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSALS = [
    (dict(p=None), b'p is null'), (dict(g=None), b'g is null'), (dict(m=None), b'm is null'), (dict(group=None), b'group is null'),
    (dict(d=None), b'd is null'), (dict(d=refusal_desc, kind=1, v=None), b'v is null'), (dict(d=refusal_desc, kind=2, v=None), b'v is null'),
    (dict(n=0), b'n=0'), (dict(n=-4), b'n=-4'), (dict(n=18), b'multiple of 4'),
    (dict(p=P + 4), b'aligned'), (dict(g=G + 8), b'aligned'), (dict(m=M + 4), b'aligned'), (dict(d=refusal_desc, kind=1, v=V2 + 8), b'aligned'),
    (dict(p16=0x60004), b'aligned'), (dict(group=GR + 2), b'aligned'),
    (dict(d=refusal_desc, kind=-1), b'kind=-1'), (dict(d=refusal_desc, kind=3), b'kind=3'), (dict(d=refusal_desc, n_groups=0), b'n_groups=0'),
    (dict(d=refusal_desc, n_groups=17), b'n_groups=17'), (dict(d=refusal_desc, nesterov=1, momentum=0.0), b'nesterov'),
]


def refused_call(case, bufs=None):
    """One refused dsl_optim_step call: `case` overrides the good arguments (d=refusal_desc plus descriptor fields, or an argument by name).
    bufs: real device pointers for the GPU test (dict p, g, m, v, p16, group), else the fake aligned addresses."""
    from dsl_amd import _lib as L
    case = dict(case)
    a = dict(p=P, g=G, m=M, v=V2, p16=None, group=GR, n=16)
    a.update(bufs or {})
    fields = {k: case.pop(k) for k in list(case) if k in ('kind', 'n_groups', 'nesterov', 'momentum')}
    d = refusal_desc(**fields)
    if 'd' in case and case.pop('d') is None:
        d = None
    a.update(case)
    rc = L.lib.dsl_optim_step(ctypes.byref(d) if d is not None else None, a['p'], a['g'], a['m'], a['v'], a['p16'], a['group'], a['n'], None, None)
    return rc, L.lib.dsl_last_error()

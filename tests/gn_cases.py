"""Inputs for the GroupNorm + ReLU checks (test helper, like op_ref.py): CPU tensors, bf16-representable, built so that the float64
reference and not luck decides each output (tests/test_groupnorm_gpu.py, tests/test_op_ref_cpu.py).

  - x: per (level, image, group) its own mean and spread: sigma log-uniform (stratified) in [0.05, 8], |mean| / sigma cycling through
    MEAN_OVER_SIGMA (the one-pass variance E[x^2] - mean^2 cancels, and a convolution's output is not centred);
  - gamma: zeros, negative entries, the rest 0.25 .. 2 in size; beta: a few channels near -10 (ReLU off everywhere) and near + 10
    (on everywhere);
  - no ReLU decision on the edge: elements with |gamma xhat + beta| <= EDGE (xa |gamma| + |beta|) in float64 are moved up one
    bf16 value at a time until none is left (EDGE = 2^-16, 16 x the band in which op_ref itself counts a decision as open);
  - dy = a + b xhat + noise with a, b of size 0.5 .. 1.5 per (level, image, group): the group means m1, m2 of the backward are as
    large as dz gamma itself, so a wrong m1 or m2 moves dx and dbias at every level.
"""
import torch

F64 = torch.float64
MEAN_OVER_SIGMA = (0.0, 4.0, 16.0)
EDGE = 2.0 ** -16
EPS = 1e-5


def _bf16_up(v):
    """the next bf16 value above every element of the bf16 tensor v (finite values)"""
    b = v.view(torch.int16).to(torch.int32)
    neg = b < 0
    mag = b & 0x7fff
    mag = torch.where(neg & (mag > 0), mag - 1, mag + 1)              # (-0 and +0 both go to the smallest positive value)
    neg = neg & (mag > 0) & ((b & 0x7fff) > 0)
    return torch.where(neg, mag - 0x8000, mag).to(torch.int16).view(torch.bfloat16)


def _segments(t, n, segs, c):
    off = 0
    for h, w in segs:
        yield t[off * c:(off + n * h * w) * c]
        off += n * h * w


def gn_pre(x, gamma, beta, n, segs, c, G, eps=EPS):
    """float64 per level: (xhat, gamma xhat + beta, xa |gamma| + |beta|), each [n][hw][G][cpg]"""
    cpg = c // G
    g4, b4 = gamma.to(F64).view(1, 1, G, cpg), beta.to(F64).view(1, 1, G, cpg)
    out = []
    for (h, w), xs in zip(segs, _segments(x, n, segs, c)):
        xs = xs.to(F64).view(n, h * w, G, cpg)
        mean = xs.mean((1, 3), keepdim=True)
        rstd = ((xs - mean).pow(2).mean((1, 3), keepdim=True) + eps).rsqrt()
        xh = (xs - mean) * rstd
        xa = (xs.abs() + mean.abs()) * rstd
        out.append((xh, xh * g4 + b4, xa * g4.abs() + b4.abs()))
    return out


def edge_elements(x, gamma, beta, n, segs, c, G, eps=EPS):
    """bool mask over x: ReLU decisions inside the EDGE band"""
    return torch.cat([(pre.abs() <= EDGE * mag).reshape(-1) for _, pre, mag in gn_pre(x, gamma, beta, n, segs, c, G, eps)])


def gn_inputs(n, segs, c, G, seed=0, zero=(), eps=EPS):
    """-> x [tot * c] bf16, gamma [c], beta [c] fp32, dy [tot * c] bf16 (level-major [level][image][pixel][channel]).
    zero: (level, image, group) triples whose x is 0 throughout; None stands for every level / group.  eps: the launch's."""
    g = torch.Generator().manual_seed(seed)
    cpg = c // G
    ch = torch.arange(c)
    gamma = (0.25 + 1.75 * torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
    beta = 0.3 * torch.randn(c, generator=g)
    gamma[ch % 8 == 3] = 0.0
    gamma[ch % 8 == 5] = -gamma[ch % 8 == 5].abs()
    off_ch, on_ch = (ch % 16 == 1) | ((ch % 8 == 1) & (c == 8)), (ch % 16 == 14) | ((ch % 8 == 6) & (c == 8))
    beta[off_ch] = -10.0 + 0.1 * torch.randn(int(off_ch.sum()), generator=g)
    beta[on_ch] = 10.0 + 0.1 * torch.randn(int(on_ch.sum()), generator=g)
    gamma[off_ch | on_ch] = gamma[off_ch | on_ch].clamp(-1.25, 1.25)          # |gamma xhat| stays below 10 on these
    xs, i = [], 0
    for s, (h, w) in enumerate(segs):
        u = (torch.randperm(n * G, generator=g) + torch.rand(n * G, generator=g)) / (n * G)         # one per stratum of the range
        sigma = torch.exp(-2.9957 + 5.0751 * u).view(n, 1, G, 1)                                   # ln 0.05 .. ln 8
        ratio = torch.tensor([MEAN_OVER_SIGMA[(i + k) % 3] for k in range(n * G)]).view(n, 1, G, 1)
        i += n * G + 2
        sign = torch.where(torch.rand(n, 1, G, 1, generator=g) < 0.5, -1.0, 1.0)
        v = sigma * (ratio * sign + torch.randn(n, h * w, G, cpg, generator=g))
        for zs, zi, zg in zero:
            if zs is None or zs == s:
                v[zi, :, slice(None) if zg is None else zg] = 0.0
        xs.append(v.reshape(-1))
    x = torch.cat(xs).bfloat16()
    for it in range(64):
        m = edge_elements(x, gamma, beta, n, segs, c, G, eps)
        if not bool(m.any()):
            break
        x = torch.where(m, _bf16_up(x), x)
    assert not bool(edge_elements(x, gamma, beta, n, segs, c, G, eps).any())
    dys = []
    for xh, _, _ in gn_pre(x, gamma, beta, n, segs, c, G, eps):
        a, b = (torch.where(torch.rand(n, 1, G, 1, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(n, 1, G, 1, generator=g))
                for _ in range(2))
        dys.append((a + b * xh.float() + 0.5 * torch.randn(xh.shape, generator=g)).reshape(-1))
    return x, gamma, beta, torch.cat(dys).bfloat16()


def group_statistics(x, n, segs, c, G):
    """float64 (|mean| / sigma, sigma) of every (level, image, group), flattened"""
    r, sg = [], []
    for (h, w), xs in zip(segs, _segments(x, n, segs, c)):
        xs = xs.to(F64).view(n, h * w, G, c // G)
        mean = xs.mean((1, 3))
        sd = (xs - mean.view(n, 1, G, 1)).pow(2).mean((1, 3)).sqrt()
        r.append((mean.abs() / sd.clamp_min(1e-30)).reshape(-1))
        sg.append(sd.reshape(-1))
    return torch.cat(r), torch.cat(sg)


FIVE = ((12, 20), (6, 10), (3, 5), (2, 3), (1, 2))
TINY5 = ((2, 3), (1, 2), (1, 1), (1, 1), (1, 1))
CHANNELS = ((8, 1), (64, 8), (64, 2), (128, 16), (512, 32), (1024, 128), (2048, 32))

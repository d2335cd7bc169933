"""Float64 reference interpreter for op-list entries (test helper, like util.py).

Every launch of a training step is one `dsl_op` (include/dsl_hip.h) whose descriptor states its arithmetic field by field.  This module
recomputes that arithmetic in float64 from the descriptor alone - explicit per-tap gather + matmul, never F.conv2d (on ROCm that is
MIOpen in fp32) - reading the launch's real inputs from device memory, and checks the launch's outputs elementwise:

    bf16 output:  |got - ref| <= 2^-8 |ref| + beta S          fp32 output:  |got - ref| <= beta S

2^-8 is bf16's worst-case half ulp.  S is the same computation on absolute values: for a convolution the gather + matmul of |src| and
|w| through |scale|, plus |bias| and |addend|; for a weight gradient |scale| x the sum of |dY| |X|.  beta (BETA, per op class, never
above BETA_MAX = 2^-13) prices fp32 accumulation.  The other classes:
  - GroupNorm forward: y and the stored (mean, rstd) come from fp32 E[x], E[x^2]; with xa = (|x| + |mean|) rstd and
    k = E[x^2] / var (the cancellation factor of the one-pass variance):  S_y = |gamma| (xa k + E|x| rstd) + |beta|,
    S_mean = E|x|, S_rstd = rstd k.
  - GroupNorm backward (dz = dy [gamma xhat + beta > 0], xhat from the stored statistics): S_dx = rstd (|dz gamma| + (A1 + xa A2) / cnt)
    with A1 = sum |dz gamma|, A2 = sum |dz gamma| xa over the group; S_dgamma = sum |dz| xa, S_dbeta = sum |dz|, S_dbias = the sum of
    S_dx over the channel's pixels.  An element whose ReLU decision the fp32 rounding of gamma xhat + beta can flip counts with either
    decision: its |dy| enters S.
  - Pools: max is exact (bound 0); the fused stem's pooled output is bounded by the window's largest conv bound; sums have
    S = sum |inputs|.

Outputs are checked where the descriptor declares them; every other byte of their allocations must be unchanged by the launch, apart
from the descriptor's own workspace (split-K partials, block records, a GroupNorm record area named by gn_ws).
"""
import ctypes as C
import types

import torch

BF16_REL = 2.0 ** -8
BETA_MAX = 2.0 ** -13
# wgrad: 2^-14.  A weight-gradient accumulator sums a whole split's pixels (thousands of products) in one fp32 chain, so its error
# grows with the partial sum, not with sqrt(n): the N = 3 towers' group measured 2^-15.7 S where dW ~ S (coherent terms), 1.4x a
# 2^-16 bar.  2^-14 still flags one 32-pixel K stage of the 3 x 44 800-pixel towers' gradient (test_step_replay_gpu.py controls).
BETA = dict(conv=2.0 ** -16, wgrad=2.0 ** -14, gn=2.0 ** -16, pool=2.0 ** -16)
F64 = torch.float64

# op kinds (mirror include/dsl_hip.h; kept here so that the CPU tests need no library)
OP_CONV, OP_WGRAD, OP_GN_FWD, OP_GN_BWD, OP_MAXPOOL, OP_SUM2X2, OP_COLSUM, OP_MEMSET, OP_PACK_IMAGE = range(1, 10)
OP_ASSIGN, OP_LOSS, OP_FORK, OP_JOIN, OP_WGRAD_GROUP, OP_RECORD, OP_WAIT = range(10, 17)
OP_RLA, OP_PACK_DGRAD, OP_WGRAD_MULTI, OP_PROF = 17, 18, 19, 21
OP_QUANT_FP8, OP_QUANT_FP8_W, OP_FP8_COMB, OP_STEM_POOL, OP_BNECK, OP_FP8_PREP, OP_QUANT_FP8_DELAYED = 22, 23, 24, 25, 26, 27, 28
KIND_NAMES = {OP_CONV: 'CONV', OP_WGRAD: 'WGRAD', OP_GN_FWD: 'GN_FWD', OP_GN_BWD: 'GN_BWD', OP_MAXPOOL: 'MAXPOOL', OP_SUM2X2: 'SUM2X2',
              OP_COLSUM: 'COLSUM', OP_MEMSET: 'MEMSET', OP_PACK_IMAGE: 'PACK_IMAGE', OP_ASSIGN: 'ASSIGN', OP_LOSS: 'LOSS', OP_FORK: 'FORK',
              OP_JOIN: 'JOIN', OP_WGRAD_GROUP: 'WGRAD_GROUP', OP_RECORD: 'RECORD', OP_WAIT: 'WAIT', OP_RLA: 'RLA',
              OP_PACK_DGRAD: 'PACK_DGRAD', OP_WGRAD_MULTI: 'WGRAD_MULTI', OP_PROF: 'PROF', OP_QUANT_FP8: 'QUANT_FP8',
              OP_QUANT_FP8_W: 'QUANT_FP8_W', OP_FP8_COMB: 'FP8_COMB', OP_STEM_POOL: 'STEM_POOL', OP_BNECK: 'BNECK',
              OP_FP8_PREP: 'FP8_PREP', OP_QUANT_FP8_DELAYED: 'QUANT_FP8_DELAYED'}
CHECKED = {OP_CONV, OP_WGRAD, OP_WGRAD_GROUP, OP_WGRAD_MULTI, OP_BNECK, OP_GN_FWD, OP_GN_BWD, OP_STEM_POOL, OP_MAXPOOL, OP_SUM2X2,
           OP_COLSUM, OP_MEMSET, OP_PACK_IMAGE}
CONV_RELU_OUT, CONV_RELU_IN, CONV_OUT_F32, CONV_MASK_FIRST, CONV_MASK_LAST, CONV_ADD_UPSAMPLE, CONV_SMALL_C, CONV_FP8 = \
    1, 2, 4, 8, 16, 32, 64, 128


class PointerError(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------------------
# pointer resolver
class Alloc:
    def __init__(self, name, t):
        st = t.untyped_storage()
        self.name, self.start, self.nbytes = name, st.data_ptr(), st.nbytes()
        self.base = torch.empty(0, dtype=torch.uint8, device=t.device).set_(st)      # the whole allocation as bytes

    def __repr__(self):
        return f'{self.name}[{self.nbytes} B]'


def _walk(obj, path, out, seen, depth):
    if depth > 9 or id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        if obj.untyped_storage().nbytes() > 0:
            out.append((path, obj))
        return
    if isinstance(obj, dict):
        for k, v in list(obj.items()):
            _walk(v, f'{path}[{k}]', out, seen, depth + 1)
        return
    if isinstance(obj, (list, tuple, set, frozenset)):
        for k, v in enumerate(obj):
            _walk(v, f'{path}[{k}]', out, seen, depth + 1)
        return
    if isinstance(obj, (str, bytes, int, float, type, types.ModuleType, types.FunctionType, C.Structure, C.Array)) or obj is None:
        return
    if hasattr(obj, 'valuerefs') and hasattr(obj, 'items'):          # weakref.WeakValueDictionary
        for k, v in list(obj.items()):
            _walk(v, f'{path}[{k}]', out, seen, depth + 1)
        return
    mod = type(obj).__module__ or ''
    if (mod.startswith('dsl_amd') or mod.startswith('torch.nn') or depth == 0) and hasattr(obj, '__dict__'):
        for k, v in list(vars(obj).items()):
            _walk(v, f'{path}.{k}', out, seen, depth + 1)


class Memory:
    """Maps raw pointers (descriptor fields) to the live tensor allocations reachable from `roots` ({name: object}): plan, store,
    loss plan, optimizer, the ops caches.  The walk follows vars() recursively, so no buffer is listed by hand."""

    def __init__(self, roots):
        found, seen = [], set()
        for name, obj in roots.items():
            _walk(obj, name, found, seen, 0)
        by_start = {}
        for path, t in found:
            a = Alloc(path, t)
            old = by_start.get(a.start)
            if old is None or a.nbytes > old.nbytes:
                by_start[a.start] = a
        self.allocs = sorted(by_start.values(), key=lambda a: a.start)

    def find(self, ptr, nbytes, what):
        ptr = int(ptr or 0)
        for a in self.allocs:
            if a.start <= ptr < a.start + a.nbytes:
                if ptr + nbytes > a.start + a.nbytes:
                    raise PointerError(f'{what}: extent {nbytes} B at offset {ptr - a.start} runs past the end of {a}')
                return a, ptr - a.start
        raise PointerError(f'{what}: pointer 0x{ptr:x} lies in no known allocation')

    def device_of(self, ptr, what):
        return self.find(ptr, 0, what)[0].base.device

    def typed(self, ptr, dtype, numel, what):
        """1-D view of `numel` elements of `dtype` at `ptr` (shares the allocation)."""
        es = torch.empty(0, dtype=dtype).element_size()
        a, off = self.find(ptr, int(numel) * es, what)
        assert off % es == 0, (what, off, es)
        return a.base[off:off + int(numel) * es].view(dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# outputs and the check
class Out:
    """One checked output: elements idx (element indices from ptr) of dtype, expected ref (float64) within the bar built on S."""

    def __init__(self, name, ptr, dtype, idx, ref, S, beta, exact=False, bound=None):
        self.name, self.ptr, self.dtype, self.idx, self.ref, self.S, self.beta = name, int(ptr), dtype, idx, ref, S, beta
        self.exact, self.bound_ = exact, bound

    def bound(self):
        if self.exact:
            return torch.zeros_like(self.ref)
        if self.bound_ is not None:
            return self.bound_
        b = self.beta * self.S
        if self.dtype == torch.bfloat16:
            b = b + BF16_REL * self.ref.abs()
        return b

    def got(self, mem):
        n = int(self.idx.max()) + 1 if self.idx.numel() else 0
        return mem.typed(self.ptr, self.dtype, n, self.name).view(-1)[self.idx].to(F64)


def compare(got, ref, bound):
    """(worst |err| / bound, number of elements over the bar, flat index of the worst)."""
    err = (got.to(F64) - ref).abs()
    bad = err > bound
    nbad = int(bad.sum())
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    worst = int(ratio.argmax()) if ratio.numel() else 0
    return (float(ratio.view(-1)[worst]) if ratio.numel() else 0.0), nbad, worst


def check_out(mem, o, got=None):
    got = o.got(mem) if got is None else got
    return compare(got, o.ref, o.bound())


class LaunchRef:
    """What one launch must do: `outs` (checked before/after), `post` (callables run after the launch that return more Outs - the
    later stages of a fused launch, fed the launch's own earlier outputs), `allowed` (byte ranges it may scribble on)."""

    def __init__(self, kind):
        self.kind, self.outs, self.post, self.allowed, self.extra = kind, [], [], [], {}


def _allow(mem, lr, ptr, nbytes, what, whole=False):
    if not ptr:
        return
    a, off = mem.find(ptr, 0 if whole else nbytes, what)
    lr.allowed.append((a.start, a.start + a.nbytes) if whole else (ptr, ptr + nbytes))


# ------------------------------------------------------------------------------------------------------------------------------
# descriptor snapshots (plain Python: references never read ctypes memory that a later edit could change)
def _ns(d):
    out = types.SimpleNamespace()
    for f in d._fields_:
        v = getattr(d, f[0])
        if isinstance(v, C.Array):
            v = list(v)
        out.__dict__[f[0]] = v if isinstance(v, list) else (v or 0)
    return out


def _grid(n, gh, gw, dev):
    img = torch.arange(n, device=dev).view(n, 1, 1).expand(n, gh, gw).reshape(-1)
    y = torch.arange(gh, device=dev).view(1, gh, 1).expand(n, gh, gw).reshape(-1)
    x = torch.arange(gw, device=dev).view(1, 1, gw).expand(n, gh, gw).reshape(-1)
    return img, y, x


def _gather_rows(flat, pix, ld, c):
    """rows pix (long, -1 = zero row) of c elements at stride ld -> float64 [len(pix)][c]."""
    ok = pix >= 0
    idx = pix.clamp_min(0).view(-1, 1) * ld + torch.arange(c, device=pix.device).view(1, -1)
    v = flat[idx].to(F64)
    return v * ok.view(-1, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# DSL_OP_CONV
def conv_geometry(d, dev):
    """Per segment: (img, y, x) of the compute grid, destination pixel index, addend pixel index, and per tap the source pixel index
    (-1 = outside / not divisible).  Segment offsets: level-major [segment][image][y][x] (dsl_hip.h conventions)."""
    segs = []
    so = do = ao = 0
    up = bool(d.flags & CONV_ADD_UPSAMPLE)
    for s in range(d.nseg):
        gh, gw, sh, sw, dh, dw = d.gh[s], d.gw[s], d.sh[s], d.sw[s], d.dh[s], d.dw[s]
        ah, aw = (d.ah[s], d.aw[s]) if up else (dh, dw)
        img, y, x = _grid(d.n, gh, gw, dev)
        oy, ox = y * d.os, x * d.os
        dpix = do + (img * dh + oy) * dw + ox
        apix = ao + (img * ah + oy * ah // dh) * aw + ox * aw // dw if up else dpix
        taps = []
        for r in range(d.kh):
            for c_ in range(d.kw):
                if d.mode == 0:
                    sy, sx, ok = y * d.stride + r - d.pad, x * d.stride + c_ - d.pad, torch.ones_like(y, dtype=torch.bool)
                else:
                    ty, tx = y + d.pad - r, x + d.pad - c_
                    ok = (ty % d.stride == 0) & (tx % d.stride == 0)
                    sy, sx = torch.div(ty, d.stride, rounding_mode='floor'), torch.div(tx, d.stride, rounding_mode='floor')
                ok = ok & (sy >= 0) & (sy < sh) & (sx >= 0) & (sx < sw)
                taps.append(torch.where(ok, so + (img * sh + sy) * sw + sx, torch.full_like(sy, -1)))
        segs.append(dict(img=img, y=y, x=x, dpix=dpix, apix=apix, taps=taps))
        so += d.n * sh * sw
        do += d.n * dh * dw
        ao += d.n * ah * aw
    return segs


def conv_ref(mem, d, name='conv', beta=None, drop=None):
    """Reference of one dsl_conv_desc (ctypes struct or namespace).  drop: test hook, (segment, pixel index set or callable(seg, tap)
    -> bool mask of grid pixels whose tap is removed) - negative controls perturb the reference, never a launch."""
    d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
    beta = BETA['conv'] if beta is None else beta
    fp8 = bool(d.flags & CONV_FP8)
    esrc = torch.float8_e4m3fn if fp8 else torch.bfloat16
    dev = mem.device_of(d.src, f'{name}.src')
    lds = d.lds or d.cs
    segs = conv_geometry(d, dev)
    # extents: the largest index the descriptor reaches (an os > 1 launch starts at an offset pointer and reaches less than its
    # destination's pixel count)
    top = lambda key: max(int(g[key].max()) for g in segs) + 1
    src_top = max(int(t.max()) for g in segs for t in g['taps']) + 1
    src = mem.typed(d.src, esrc, (src_top - 1) * lds + d.cs, f'{name}.src')
    taps = d.kh * d.kw
    wrow = taps * d.cs
    if d.flags & CONV_SMALL_C:
        wrow = (taps * d.cs + 63) // 64 * 64
    wgt = mem.typed(d.wgt, esrc, (d.cd_pad - 1) * wrow + taps * d.cs, f'{name}.wgt').view(-1)
    W = wgt[torch.arange(d.cd, device=wgt.device).view(-1, 1) * wrow + torch.arange(taps * d.cs, device=wgt.device).view(1, -1)]
    W = W.to(F64).view(d.cd, taps, d.cs)
    Wa = W.abs()
    out_f32 = bool(d.flags & CONV_OUT_F32)
    scale = mem.typed(d.scale, torch.float32, d.cd, f'{name}.scale').to(F64) if d.scale else None
    bias = mem.typed(d.bias, torch.float32, d.cd, f'{name}.bias').to(F64) if d.bias else None
    add = mem.typed(d.addend, torch.bfloat16, (top('apix') - 1) * d.lda + d.cd, f'{name}.addend') if d.addend else None
    has_mask = bool(d.mask) and bool(d.flags & (CONV_MASK_FIRST | CONV_MASK_LAST))
    mask = mem.typed(d.mask, torch.bfloat16, (top('dpix') - 1) * d.ldm + d.cd, f'{name}.mask') if has_mask else None
    mem.find(d.dst, ((top('dpix') - 1) * d.ldd + d.cd) * (4 if out_f32 else 2), f'{name}.dst')
    refs, Ss, idxs = [], [], []
    for si, g in enumerate(segs):
        acc = torch.zeros(g['img'].numel(), d.cd, dtype=F64, device=dev)
        sacc = torch.zeros_like(acc)
        for t in range(taps):
            pix = g['taps'][t]
            if drop is not None:
                pix = torch.where(drop(si, t, g), torch.full_like(pix, -1), pix)
            X = _gather_rows(src, pix, lds, d.cs)
            if d.flags & CONV_RELU_IN:
                X = X.clamp_min(0)
            acc += X @ W[:, t, :].T
            sacc += X.abs() @ Wa[:, t, :].T
        v, S = acc, sacc
        if scale is not None:
            v, S = v * scale, S * scale.abs()
        if bias is not None:
            v, S = v + bias, S + bias.abs()
        cols = torch.arange(d.cd, device=dev).view(1, -1)
        if mask is not None:
            m = (mask[g['dpix'].view(-1, 1) * d.ldm + cols].to(F64) > 0).to(F64)
        if d.flags & CONV_MASK_FIRST and mask is not None:
            v, S = v * m, S * m
        if add is not None:
            a = add[g['apix'].view(-1, 1) * d.lda + cols].to(F64)
            v, S = v + a, S + a.abs()
        if d.flags & CONV_MASK_LAST and mask is not None:
            v, S = v * m, S * m
        if d.flags & CONV_RELU_OUT:
            v = v.clamp_min(0)
        refs.append(v)
        Ss.append(S)
        idxs.append(g['dpix'].view(-1, 1) * d.ldd + cols)
    lr = LaunchRef('CONV')
    lr.outs.append(Out(f'{name}.dst', d.dst, torch.float32 if out_f32 else torch.bfloat16, torch.cat(idxs), torch.cat(refs),
                       torch.cat(Ss), beta))
    if d.workspace and d.workspace_bytes:
        _allow(mem, lr, d.workspace, d.workspace_bytes, f'{name}.workspace')
    if getattr(d, 'gn_ws', 0):
        _allow(mem, lr, d.gn_ws, 0, f'{name}.gn_ws', whole=True)
    lr.extra['segs'] = segs
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# weight gradients
def wgrad_member(mem, d, name='wgrad', drop_img=None, drop_stage=None, dev=None):
    """(dW ref, S, db ref, db S) of one dsl_wgrad_desc: dW[co][r][s][ci] = scale[co] sum_p dY[p][co] X[p@(r,s)][ci] (fp32, KRSC).
    drop_img: negative-control hook - image index left out; drop_stage: (first pixel, count) of the flat pixel order left out."""
    dev = dev or mem.device_of(d.dy, f'{name}.dy')
    ldx = d.ldx or d.cs
    tot_g = sum(d.n * d.gh[s] * d.gw[s] for s in range(d.nseg))
    tot_s = sum(d.n * d.sh[s] * d.sw[s] for s in range(d.nseg))
    dy = mem.typed(d.dy, torch.bfloat16, (tot_g - 1) * d.cy + d.cd, f'{name}.dy')
    x = mem.typed(d.x, torch.bfloat16, (tot_s - 1) * ldx + d.cs, f'{name}.x')
    taps = d.kh * d.kw
    dW = torch.zeros(d.cd, taps, d.cs, dtype=F64, device=dev)
    SW = torch.zeros_like(dW)
    db = torch.zeros(d.cd, dtype=F64, device=dev)
    Sdb = torch.zeros_like(db)
    go = so = 0
    for s in range(d.nseg):
        gh, gw, sh, sw = d.gh[s], d.gw[s], d.sh[s], d.sw[s]
        img, y, xx = _grid(d.n, gh, gw, dev)
        p = go + torch.arange(img.numel(), device=dev)
        keep = torch.ones_like(p, dtype=torch.bool)
        if drop_img is not None:
            keep &= img != drop_img
        if drop_stage is not None:
            keep &= ~((p >= drop_stage[0]) & (p < drop_stage[0] + drop_stage[1]))
        DY = _gather_rows(dy, torch.where(keep, p, torch.full_like(p, -1)), d.cy, d.cd)
        DYa = DY.abs()
        db += DY.sum(0)
        Sdb += DYa.sum(0)
        for t in range(taps):
            r, c_ = divmod(t, d.kw)
            sy, sx = y * d.stride + r - d.pad, xx * d.stride + c_ - d.pad
            ok = (sy >= 0) & (sy < sh) & (sx >= 0) & (sx < sw)
            X = _gather_rows(x, torch.where(ok, so + (img * sh + sy) * sw + sx, torch.full_like(sy, -1)), ldx, d.cs)
            dW[:, t] += DY.T @ X
            SW[:, t] += DYa.T @ X.abs()
        go += img.numel()
        so += d.n * sh * sw
    if d.scale:
        sc = mem.typed(d.scale, torch.float32, d.cd, f'{name}.scale').to(F64).view(-1, 1, 1)
        dW, SW = dW * sc, SW * sc.abs()
    return dW.view(d.cd, -1), SW.view(d.cd, -1), db, Sdb


def wgrad_ref(mem, descs, name='wgrad', beta=None, drop=None, workspace=None):
    """descs: dsl_wgrad_desc structs of one launch (single, group or a multi launch's flattened sub-launches).  `shared` members are
    summed into one dw.  drop: {member index: dict(drop_img=.., drop_stage=..)} (negative controls)."""
    beta = BETA['wgrad'] if beta is None else beta
    lr = LaunchRef('WGRAD')
    acc = {}
    for k, d in enumerate(descs):
        d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
        dW, SW, db, Sdb = wgrad_member(mem, d, f'{name}[{k}]', **((drop or {}).get(k, {})))
        key = d.dw if d.shared else (d.dw, k)
        if key in acc:
            acc[key][1].add_(dW)
            acc[key][2].add_(SW)
        else:
            acc[key] = [d, dW, SW, k]
        if d.db:
            mem.find(d.db, d.cd * 4, f'{name}[{k}].db')
            lr.outs.append(Out(f'{name}[{k}].db', d.db, torch.float32, torch.arange(d.cd, device=db.device), db, Sdb, beta))
        if k == 0 and d.workspace and d.workspace_bytes:
            _allow(mem, lr, d.workspace, d.workspace_bytes, f'{name}.workspace')
    for d, dW, SW, k in acc.values():
        n = dW.numel()
        mem.find(d.dw, n * 4, f'{name}[{k}].dw')
        lr.outs.append(Out(f'{name}[{k}].dw', d.dw, torch.float32, torch.arange(n, device=dW.device).view(dW.shape), dW, SW, beta))
    if workspace is not None:
        _allow(mem, lr, workspace[0], workspace[1], f'{name}.workspace')
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU
def _gn_layout(d, dev):
    off, segs = 0, []
    for s in range(d.nseg):
        hw = d.h[s] * d.w[s]
        segs.append((off, hw))
        off += d.n * hw
    return segs, off


def gn_fwd_ref(mem, d, name='gn', beta=None):
    d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
    beta = BETA['gn'] if beta is None else beta
    dev = mem.device_of(d.x, f'{name}.x')
    segs, tot = _gn_layout(d, dev)
    c, G = d.c, d.groups
    cpg = c // G
    x = mem.typed(d.x, torch.bfloat16, tot * c, f'{name}.x').to(F64).view(tot, c)
    gam = mem.typed(d.gamma, torch.float32, c, f'{name}.gamma').to(F64)
    bet = mem.typed(d.beta, torch.float32, c, f'{name}.beta').to(F64)
    mem.find(d.y, tot * c * 2, f'{name}.y')
    mem.find(d.stats, d.nseg * d.n * G * 8, f'{name}.stats')
    ys, Sy, st, Sst = [], [], [], []
    for off, hw in segs:
        xs = x[off:off + d.n * hw].view(d.n, hw, G, cpg)
        mean = xs.mean((1, 3))                                        # [n][G]
        var = (xs - mean.view(d.n, 1, G, 1)).pow(2).mean((1, 3))
        ex2 = xs.pow(2).mean((1, 3))
        eabs = xs.abs().mean((1, 3))
        rstd = (var + d.eps).rsqrt()
        k = ex2 / (var + d.eps)
        xh = (xs - mean.view(d.n, 1, G, 1)) * rstd.view(d.n, 1, G, 1)
        xa = (xs.abs() + mean.abs().view(d.n, 1, G, 1)) * rstd.view(d.n, 1, G, 1)
        g4, b4 = gam.view(1, 1, G, cpg), bet.view(1, 1, G, cpg)
        ys.append((xh * g4 + b4).clamp_min(0).reshape(-1, c))
        Sy.append((g4.abs() * (xa * k.view(d.n, 1, G, 1) + (eabs * rstd).view(d.n, 1, G, 1)) + b4.abs()).reshape(-1, c))
        st.append(torch.stack([mean, rstd], -1).reshape(-1))
        Sst.append(torch.stack([eabs, rstd * k], -1).reshape(-1))
    lr = LaunchRef('GN_FWD')
    lr.outs.append(Out(f'{name}.y', d.y, torch.bfloat16, torch.arange(tot * c, device=dev).view(tot, c), torch.cat(ys), torch.cat(Sy), beta))
    lr.outs.append(Out(f'{name}.stats', d.stats, torch.float32, torch.arange(d.nseg * d.n * G * 2, device=dev), torch.cat(st),
                       torch.cat(Sst), beta))
    _allow(mem, lr, d.workspace, d.workspace_bytes, f'{name}.workspace')
    if d.y8:
        def post(mem=mem, d=d, tot=tot, c=c):
            # the fp8 copy: y8 = e4m3(clamp(bf16(y) * y8_scale, +-448)) of the launch's own y; y8_amax = block maxima of bf16(y)
            y = mem.typed(d.y, torch.bfloat16, tot * c, f'{name}.y').float().view(tot, c)
            s8 = float(mem.typed(d.y8_scale, torch.float32, 1, f'{name}.y8_scale')[0])
            q = (y * s8).clamp(-448, 448).to(torch.float8_e4m3fn).to(F64)
            outs = [Out(f'{name}.y8', d.y8, torch.float8_e4m3fn, torch.arange(tot * c, device=y.device).view(tot, c), q, q, 0.0,
                        exact=True)]
            nblk = (max(hw for _, hw in segs) + 127) // 128
            idx, ref = [], []
            for s, (off, hw) in enumerate(segs):
                for im in range(d.n):
                    rows = y[off + im * hw: off + (im + 1) * hw]
                    for b in range((hw + 127) // 128):
                        idx.append((s * d.n + im) * nblk + b)
                        ref.append(rows[b * 128:(b + 1) * 128].max())
            ref = torch.stack(ref).to(F64)
            outs.append(Out(f'{name}.y8_amax', d.y8_amax, torch.float32, torch.tensor(idx, device=y.device), ref, ref, 0.0, exact=True))
            return outs
        mem.find(d.y8, tot * c, f'{name}.y8')
        lr.post.append(post)
    return lr


def gn_bwd_ref(mem, d, name='gn_bwd', beta=None):
    d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
    beta = BETA['gn'] if beta is None else beta
    dev = mem.device_of(d.x, f'{name}.x')
    segs, tot = _gn_layout(d, dev)
    c, G = d.c, d.groups
    cpg = c // G
    x = mem.typed(d.x, torch.bfloat16, tot * c, f'{name}.x').to(F64).view(tot, c)
    dy = mem.typed(d.dy, torch.bfloat16, tot * c, f'{name}.dy').to(F64).view(tot, c)
    gam = mem.typed(d.gamma, torch.float32, c, f'{name}.gamma').to(F64)
    bet = mem.typed(d.beta, torch.float32, c, f'{name}.beta').to(F64)
    stats = mem.typed(d.stats, torch.float32, d.nseg * d.n * G * 2, f'{name}.stats').to(F64).view(d.nseg, d.n, G, 2)
    mem.find(d.dx, tot * c * 2, f'{name}.dx')
    dxs, Sdx = [], []
    dg, db, dbi = (torch.zeros(c, dtype=F64, device=dev) for _ in range(3))
    Sdg, Sdb, Sdbi = (torch.zeros(c, dtype=F64, device=dev) for _ in range(3))
    g4, b4 = gam.view(1, 1, G, cpg), bet.view(1, 1, G, cpg)
    for s, (off, hw) in enumerate(segs):
        xs = x[off:off + d.n * hw].view(d.n, hw, G, cpg)
        gs = dy[off:off + d.n * hw].view(d.n, hw, G, cpg)
        mean, rstd = stats[s, :, :, 0].view(d.n, 1, G, 1), stats[s, :, :, 1].view(d.n, 1, G, 1)
        xh = (xs - mean) * rstd
        xa = (xs.abs() + mean.abs()) * rstd
        pre = xh * g4 + b4
        amb = pre.abs() <= 2.0 ** -20 * (xa * g4.abs() + b4.abs())       # fp32 rounding may flip this ReLU decision
        dz = gs * (pre > 0)
        dza = gs.abs() * ((pre > 0) | amb)
        cnt = hw * cpg
        s1 = (dz * g4).sum((1, 3), keepdim=True)
        s2 = (dz * g4 * xh).sum((1, 3), keepdim=True)
        a1 = (dza * g4.abs()).sum((1, 3), keepdim=True)
        a2 = (dza * g4.abs() * xa).sum((1, 3), keepdim=True)
        dx = rstd * (dz * g4 - (s1 + xh * s2) / cnt)
        S = rstd * (dza * g4.abs() + (a1 + xa * a2) / cnt)
        dxs.append(dx.reshape(-1, c))
        Sdx.append(S.reshape(-1, c))
        dg += (dz * xh).sum((0, 1)).reshape(c)
        Sdg += (dza * xa).sum((0, 1)).reshape(c)
        db += dz.sum((0, 1)).reshape(c)
        Sdb += dza.sum((0, 1)).reshape(c)
        dbi += dx.sum((0, 1)).reshape(c)
        Sdbi += S.sum((0, 1)).reshape(c)
    lr = LaunchRef('GN_BWD')
    lr.outs.append(Out(f'{name}.dx', d.dx, torch.bfloat16, torch.arange(tot * c, device=dev).view(tot, c), torch.cat(dxs), torch.cat(Sdx), beta))
    ar = torch.arange(c, device=dev)
    lr.outs.append(Out(f'{name}.dgamma', d.dgamma, torch.float32, ar, dg, Sdg, beta))
    lr.outs.append(Out(f'{name}.dbeta', d.dbeta, torch.float32, ar, db, Sdb, beta))
    if d.dbias:
        lr.outs.append(Out(f'{name}.dbias', d.dbias, torch.float32, ar, dbi, Sdbi, beta))
    _allow(mem, lr, d.workspace, d.workspace_bytes, f'{name}.workspace')
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# the fused bottleneck (three convolutions, folded BatchNorms, identity)
def bneck_ref(mem, d, name='bneck', beta=None):
    d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
    P = d.planes
    base = dict(nseg=1, n=d.n, gh=[d.h], gw=[d.w], dh=[d.h], dw=[d.w], ah=[0], aw=[0], mode=0, os=1, pad=0, mask=0, ldm=0,
                workspace=0, workspace_bytes=0, gn_ws=0, lda=0, addend=0)
    c1 = types.SimpleNamespace(**base, sh=[d.hin], sw=[d.win], cs=d.cin, cd=P, cd_pad=P, ldd=P, kh=1, kw=1, stride=d.stride,
                               flags=CONV_RELU_OUT, src=d.x, wgt=d.w1, dst=d.a1, scale=d.s1, bias=d.b1, lds=d.ldx)
    c2 = types.SimpleNamespace(**base, sh=[d.h], sw=[d.w], cs=P, cd=P, cd_pad=P, ldd=P, kh=3, kw=3, stride=1, flags=CONV_RELU_OUT,
                               src=d.a1, wgt=d.w2, dst=d.a2, scale=d.s2, bias=d.b2, lds=0)
    c2.pad = 1
    c3 = types.SimpleNamespace(**base, sh=[d.h], sw=[d.w], cs=P, cd=4 * P, cd_pad=4 * P, ldd=d.ldo, kh=1, kw=1, stride=1,
                               flags=CONV_RELU_OUT, src=d.a2, wgt=d.w3, dst=d.out, scale=d.s3, bias=d.b3, lds=0)
    c3.addend, c3.lda = d.idt, d.ldi
    lr = conv_ref(mem, c1, f'{name}.conv1', beta)
    lr.kind = 'BNECK'
    # conv2 / conv3 read the launch's own a1 / a2: evaluated after it (teacher forcing inside the fused launch)
    lr.post.append(lambda: conv_ref(mem, c2, f'{name}.conv2', beta).outs)
    lr.post.append(lambda: conv_ref(mem, c3, f'{name}.conv3', beta).outs)
    lr.later = [c2.dst, c3.dst]      # (their allocations are snapshotted before the launch too)
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# small ops
def maxpool_ref(mem, x_ptr, y_ptr, n, h, w, c, ldy, name='maxpool'):
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = mem.typed(x_ptr, torch.bfloat16, n * h * w * c, f'{name}.x').to(F64).view(n, h, w, c)
    mem.find(y_ptr, ((n * oh * ow - 1) * ldy + c) * 2, f'{name}.y')
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float('-inf'))
    ref = torch.nn.functional.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1).reshape(-1, c)
    idx = torch.arange(n * oh * ow, device=x.device).view(-1, 1) * ldy + torch.arange(c, device=x.device).view(1, -1)
    lr = LaunchRef('MAXPOOL')
    lr.outs.append(Out(f'{name}.y', y_ptr, torch.bfloat16, idx, ref, ref.abs(), 0.0, exact=True))
    return lr


def sum2x2_ref(mem, g_ptr, out_ptr, n, h, w, ch, cw, c, name='sum2x2', beta=None):
    beta = BETA['pool'] if beta is None else beta
    g = mem.typed(g_ptr, torch.bfloat16, n * ch * cw * c, f'{name}.g').to(F64).view(n, ch, cw, c)
    mem.find(out_ptr, n * h * w * c * 2, f'{name}.out')
    ref = torch.zeros(n, h, w, c, dtype=F64, device=g.device)
    S = torch.zeros_like(ref)
    for a in (0, 1):
        for b in (0, 1):
            ys, xs = torch.arange(h) * 2 + a, torch.arange(w) * 2 + b
            ys, xs = ys[ys < ch], xs[xs < cw]
            part = g[:, ys][:, :, xs]
            ref[:, :len(ys), :len(xs)] += part
            S[:, :len(ys), :len(xs)] += part.abs()
    lr = LaunchRef('SUM2X2')
    lr.outs.append(Out(f'{name}.out', out_ptr, torch.bfloat16, torch.arange(n * h * w * c, device=g.device).view(-1, c),
                       ref.view(-1, c), S.view(-1, c), beta))
    return lr


def colsum_ref(mem, x_ptr, out_ptr, rows, c, ld, name='colsum', beta=None):
    beta = BETA['pool'] if beta is None else beta
    x = _gather_rows(mem.typed(x_ptr, torch.bfloat16, (rows - 1) * ld + c, f'{name}.x'),
                     torch.arange(rows, device=mem.device_of(x_ptr, f'{name}.x')), ld, c)
    mem.find(out_ptr, c * 4, f'{name}.out')
    lr = LaunchRef('COLSUM')
    lr.outs.append(Out(f'{name}.out', out_ptr, torch.float32, torch.arange(c, device=x.device), x.sum(0), x.abs().sum(0), beta))
    return lr


def memset_ref(mem, ptr, nbytes, value, name='memset'):
    mem.find(ptr, nbytes, f'{name}.dst')
    dev = mem.device_of(ptr, f'{name}.dst')
    lr = LaunchRef('MEMSET')
    ref = torch.full((nbytes,), value & 0xff, dtype=F64, device=dev)
    lr.outs.append(Out(f'{name}.dst', ptr, torch.uint8, torch.arange(nbytes, device=dev), ref, ref, 0.0, exact=True))
    return lr


def pack_image_ref(mem, img_ptr, out_ptr, n, h, w, name='pack_image'):
    img = mem.typed(img_ptr, torch.float32, n * 3 * h * w, f'{name}.img').view(n, 3, h, w)
    mem.find(out_ptr, n * h * w * 8 * 2, f'{name}.out')
    ref = torch.zeros(n, h, w, 8, dtype=F64, device=img.device)
    ref[..., :3] = img.permute(0, 2, 3, 1).bfloat16().to(F64)
    lr = LaunchRef('PACK_IMAGE')
    lr.outs.append(Out(f'{name}.out', out_ptr, torch.bfloat16, torch.arange(ref.numel(), device=img.device).view(-1, 8),
                       ref.view(-1, 8), ref.view(-1, 8), 0.0, exact=True))
    return lr


def stem_image(mem, img_ptr, n, h, w, half_last, name='stem'):
    """The stem's bf16 input images [n][3][h][w]: with half_last, image n - 1 is F.interpolate(bilinear) of the last stored image
    at half size in the top-left corner of a zero canvas (dsl_stem_pool_half)."""
    nm = n - 1 if half_last else n
    img = mem.typed(img_ptr, torch.float32, nm * 3 * h * w, f'{name}.img').view(nm, 3, h, w)
    if half_last:
        half = torch.nn.functional.interpolate(img[-1:], size=(h // 2, w // 2), mode='bilinear', align_corners=False)
        extra = torch.zeros(1, 3, h, w, dtype=img.dtype, device=img.device)
        extra[:, :, :h // 2, :w // 2] = half
        img = torch.cat([img, extra])
    return img.bfloat16().to(F64)


def stem_pool_ref(mem, img_ptr, wg_ptr, scale_ptr, bias_ptr, out_ptr, ld_out, n, h, w, half_last, name='stem', beta=None):
    """conv1 7x7 / 2 / pad 3 (3 -> 64) + folded BN + ReLU on bf16(img), then max pool 3x3 / 2 / pad 1.  The pooled value's bound is
    the largest per-element conv bound of its window (max is 1-Lipschitz)."""
    beta = BETA['conv'] if beta is None else beta
    x = stem_image(mem, img_ptr, n, h, w, half_last, name)
    wg = mem.typed(wg_ptr, torch.bfloat16, 22 * 64 * 8, f'{name}.w_groups').to(F64).view(22, 64, 8)
    W = wg[:21].view(7, 3, 64, 8).permute(2, 0, 1, 3).reshape(64, 7, 24)[:, :, :21].reshape(64, 7, 7, 3)   # [co][ky][kx][c]
    sc = mem.typed(scale_ptr, torch.float32, 64, f'{name}.scale').to(F64)
    bi = mem.typed(bias_ptr, torch.float32, 64, f'{name}.bias').to(F64)
    sh, sw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ph, pw = (sh - 1) // 2 + 1, (sw - 1) // 2 + 1
    mem.find(out_ptr, ((n * ph * pw - 1) * ld_out + 64) * 2, f'{name}.out')
    xp = torch.nn.functional.pad(x, (3, 3, 3, 3))
    acc = torch.zeros(n, sh, sw, 64, dtype=F64, device=x.device)
    sacc = torch.zeros_like(acc)
    for ky in range(7):
        for kx in range(7):
            patch = xp[:, :, ky:ky + 2 * sh - 1:2, kx:kx + 2 * sw - 1:2].permute(0, 2, 3, 1)   # [n][sh][sw][3]
            acc += patch @ W[:, ky, kx, :].T
            sacc += patch.abs() @ W[:, ky, kx, :].abs().T
    v = (acc * sc + bi).clamp_min(0)
    S = sacc * sc.abs() + bi.abs()
    bnd = BF16_REL * v.abs() + beta * S
    pool = lambda t, fill: torch.nn.functional.max_pool2d(
        torch.nn.functional.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1), value=fill), 3, 2).permute(0, 2, 3, 1).reshape(-1, 64)
    ref, bound = pool(v, float('-inf')), pool(bnd, 0.0)
    idx = torch.arange(n * ph * pw, device=x.device).view(-1, 1) * ld_out + torch.arange(64, device=x.device).view(1, -1)
    lr = LaunchRef('STEM_POOL')
    lr.outs.append(Out(f'{name}.out', out_ptr, torch.bfloat16, idx, ref, ref.abs(), beta, bound=bound))
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch over one dsl_op
def op_ref(mem, op, multis=None, name=None):
    """LaunchRef of one dsl_op (ctypes), or None for kinds without a reference.  multis: {table_host pointer: ops.WgradMulti}."""
    from dsl_amd import _lib as L
    k = op.kind
    nm = name or KIND_NAMES.get(k, str(k))
    if k == OP_CONV:
        return conv_ref(mem, C.cast(op.desc, C.POINTER(L.ConvDesc)).contents, nm)
    if k == OP_WGRAD:
        return wgrad_ref(mem, [C.cast(op.desc, C.POINTER(L.WgradDesc)).contents], nm)
    if k == OP_WGRAD_GROUP:
        arr = C.cast(op.desc, C.POINTER(L.WgradDesc))
        lr = wgrad_ref(mem, [arr[g] for g in range(op.i[0])], nm)
        lr.kind = 'WGRAD_GROUP'
        return lr
    if k == OP_WGRAD_MULTI:
        m = multis[op.p[0]]
        ws = m._keep[1]
        lr = wgrad_ref(mem, [m.descs[g] for g in range(len(m.descs))], nm, workspace=(ws.data_ptr(), ws.numel() * ws.element_size()))
        lr.kind = 'WGRAD_MULTI'
        return lr
    if k == OP_BNECK:
        return bneck_ref(mem, C.cast(op.desc, C.POINTER(L.BneckDesc)).contents, nm)
    if k == OP_GN_FWD:
        return gn_fwd_ref(mem, C.cast(op.desc, C.POINTER(L.GnDesc)).contents, nm)
    if k == OP_GN_BWD:
        return gn_bwd_ref(mem, C.cast(op.desc, C.POINTER(L.GnDesc)).contents, nm)
    if k == OP_MAXPOOL:
        return maxpool_ref(mem, op.p[0], op.p[1], *op.i[:4], op.i[4] if op.i[4] > 0 else op.i[3], name=nm)
    if k == OP_SUM2X2:
        return sum2x2_ref(mem, op.p[0], op.p[1], *op.i[:6], name=nm)
    if k == OP_COLSUM:
        return colsum_ref(mem, op.p[0], op.p[1], op.l[0], op.i[0], op.i[1], name=nm)
    if k == OP_MEMSET:
        return memset_ref(mem, op.p[0], op.l[0], op.i[0], name=nm)
    if k == OP_PACK_IMAGE:
        return pack_image_ref(mem, op.p[0], op.p[1], *op.i[:3], name=nm)
    if k == OP_STEM_POOL:
        return stem_pool_ref(mem, op.p[0], op.p[1], op.l[0], op.l[1], op.p[2], op.i[0], op.i[1], op.i[2], op.i[3], op.i[4], name=nm)
    return None


# ------------------------------------------------------------------------------------------------------------------------------
# running one launch under the check
def _declared_bytes(mem, o, mark):
    a, off = mem.find(o.ptr, 0, o.name)
    es = torch.empty(0, dtype=o.dtype).element_size()
    idx = o.idx.reshape(-1).to(mark.device)
    b = (off + idx * es).view(-1, 1) + torch.arange(es, device=mark.device).view(1, -1)
    mark[b.view(-1)] = True


def run_checked(mem, lr, launch):
    """Snapshot the outputs' allocations, launch, compare.  Returns [(out name, worst ratio, elements over the bar)] and raises
    AssertionError naming the allocation if a byte outside every declared region and workspace changed."""
    outs = list(lr.outs)
    allocs = {}
    for o in outs:
        a, _ = mem.find(o.ptr, 0, o.name)
        allocs[a.start] = a
    for ptr in getattr(lr, 'later', []):
        a, _ = mem.find(ptr, 0, f'{lr.kind}.later')
        allocs[a.start] = a
    snaps = {s: a.base.clone() for s, a in allocs.items()}
    launch()
    for post in lr.post:
        outs += post()
    res = [(o.name,) + check_out(mem, o) for o in outs]
    for s, a in allocs.items():
        changed = a.base != snaps[s]
        if not bool(changed.any()):
            continue
        mark = torch.zeros_like(changed)
        for o in outs:
            if mem.find(o.ptr, 0, o.name)[0] is a:
                _declared_bytes(mem, o, mark)
        for lo, hi in lr.allowed:
            if a.start <= lo < a.start + a.nbytes or a.start < hi <= a.start + a.nbytes:
                mark[max(lo - a.start, 0):min(hi - a.start, a.nbytes)] = True
        stray = changed & ~mark
        if bool(stray.any()):
            first = int(stray.nonzero()[0])
            raise AssertionError(f'{lr.kind}: {int(stray.sum())} bytes of {a} outside the declared outputs changed (first at byte {first})')
    return res

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
# loss: the FCOS loss kernel's bf16 gradients; loss_sum: its fp32 sums (losses, g_scales, the assignment's centerness sum), added
# in block records of 256: measured at most 0.009 of a 2^-16 bar over the seven replay legs, hence 2^-20.
BETA = dict(conv=2.0 ** -16, wgrad=2.0 ** -14, gn=2.0 ** -16, pool=2.0 ** -16, loss=2.0 ** -16, loss_sum=2.0 ** -20)
F64 = torch.float64
DSL_MAX_SEG = 5

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
           OP_COLSUM, OP_MEMSET, OP_PACK_IMAGE, OP_ASSIGN, OP_LOSS, OP_QUANT_FP8, OP_QUANT_FP8_W, OP_FP8_COMB, OP_FP8_PREP,
           OP_QUANT_FP8_DELAYED}
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
# FCOS target assignment (csrc/fcos_loss.hip assign_kernel): bit-exact fp32 restatement, kernel operation order
FCOS_INF = 1e8


def _fcos_locations(d):
    """Level-major [lvl][img][y][x] locations of a dsl_fcos_desc: (lvl, img, y, x) long tensors (CPU) and mstart[nlvl + 1]."""
    lv, im, ys, xs, ms = [], [], [], [], [0]
    for l in range(d.nlvl):
        img, y, x = _grid(d.n, d.h[l], d.w[l], 'cpu')
        lv.append(torch.full_like(img, l))
        im.append(img)
        ys.append(y)
        xs.append(x)
        ms.append(ms[-1] + img.numel())
    return torch.cat(lv), torch.cat(im), torch.cat(ys), torch.cat(xs), ms


def _assign_boxes(px, py, rs, lo, hi, boxes):
    """assign_one over rows of locations against boxes [G][4] (fp32, CPU): (best area, first argmin, ltrb of that box)."""
    x, y = px.view(-1, 1), py.view(-1, 1)
    x1, y1, x2, y2 = (boxes[:, i].view(1, -1) for i in range(4))
    area = (x2 - x1) * (y2 - y1)
    l, tp, r, b = x - x1, y - y1, x2 - x, y2 - y
    cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    rr = rs.view(-1, 1)
    xmin, ymin, xmax, ymax = cx - rr, cy - rr, cx + rr, cy + rr
    c0 = torch.where(xmin > x1, xmin, x1)
    c1 = torch.where(ymin > y1, ymin, y1)
    c2 = torch.where(xmax > x2, x2, xmax)
    c3 = torch.where(ymax > y2, y2, ymax)
    cmin = torch.minimum(torch.minimum(x - c0, y - c1), torch.minimum(c2 - x, c3 - y))
    mx = torch.maximum(torch.maximum(l, tp), torch.maximum(r, b))
    ok = (cmin > 0) & (mx >= lo.view(-1, 1)) & (mx <= hi.view(-1, 1))
    area = torch.where(ok, area.expand_as(ok), torch.full_like(mx, FCOS_INF))
    best, idx = area.min(1)               # first index of the minimum (the kernel's `g == g0 || area < best`)
    ar = torch.arange(px.numel())
    t = torch.stack([v.expand_as(mx)[ar, idx] for v in (l, tp, r, b)], 1)
    return best, idx, t


def assign_ref(mem, d, name='assign', radius=None):
    """dsl_fcos_assign: labels, assign_idx, bbox_targets (/ stride; background rows: gt 0's ltrb, zeros for an image without gt),
    cls_weight (0 for background locations that an ignore box claims by the same rule, x loss_weight for images >= n / 2),
    pos_weight, stats[0] (exact count), stats[1] (sum of centerness targets, beta S), stats[2..7] = 0.  radius: negative-control
    hook (the centre-sampling radius in place of the descriptor's)."""
    d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
    dev = mem.device_of(d.labels, f'{name}.labels')
    f32 = torch.float32
    lvl, img, y, x, ms = _fcos_locations(d)
    M, C = ms[-1], d.num_classes
    s = torch.tensor([d.stride[l] for l in range(d.nlvl)])[lvl]
    px = x.to(f32) * s.to(f32) + (s // 2).to(f32)
    py = y.to(f32) * s.to(f32) + (s // 2).to(f32)
    rad = torch.tensor(d.radius if radius is None else radius, dtype=f32)
    rs = s.to(f32) * rad
    lo = torch.tensor([d.range_lo[l] for l in range(d.nlvl)], dtype=f32)[lvl]
    hi = torch.tensor([d.range_hi[l] for l in range(d.nlvl)], dtype=f32)[lvl]
    gt_off = mem.typed(d.gt_off, torch.int32, d.n + 1, f'{name}.gt_off').cpu().long()
    G = int(gt_off[-1])
    boxes = mem.typed(d.gt_boxes, f32, 4 * G, f'{name}.gt_boxes').cpu().view(G, 4)
    glab = mem.typed(d.gt_labels, torch.int64, G, f'{name}.gt_labels').cpu()
    ig = None
    if d.ig_boxes and d.ig_off:
        ig_off = mem.typed(d.ig_off, torch.int32, d.n + 1, f'{name}.ig_off').cpu().long()
        ig = (ig_off, mem.typed(d.ig_boxes, f32, 4 * int(ig_off[-1]), f'{name}.ig_boxes').cpu().view(-1, 4))
    labels = torch.full((M,), C, dtype=torch.int64)
    aidx = torch.full((M,), -1, dtype=torch.int64)
    tgt = torch.zeros(M, 4, dtype=f32)
    wgt = torch.ones(M, dtype=f32)
    for i in range(d.n):
        sel = (img == i).nonzero().view(-1)
        g0, g1 = int(gt_off[i]), int(gt_off[i + 1])
        if g1 > g0:
            best, idx, t = _assign_boxes(px[sel], py[sel], rs[sel], lo[sel], hi[sel], boxes[g0:g1])
            pos = best != FCOS_INF
            labels[sel[pos]] = glab[g0 + idx[pos]]
            aidx[sel[pos]] = idx[pos]
            tgt[sel] = t
        if ig is not None and int(ig[0][i + 1]) > int(ig[0][i]):
            bi, _, _ = _assign_boxes(px[sel], py[sel], rs[sel], lo[sel], hi[sel], ig[1][int(ig[0][i]):int(ig[0][i + 1])])
            wgt[sel[(bi != FCOS_INF) & (labels[sel] == C)]] = 0.0
    tgt = tgt / s.to(f32).view(-1, 1)
    sw = torch.ones(M, dtype=f32)
    if torch.tensor(d.loss_weight, dtype=f32) != 1.0:
        sw[img >= d.n // 2] = torch.tensor(d.loss_weight, dtype=f32)
    pos = labels < C
    tp = tgt[pos]
    ctr = torch.sqrt((torch.minimum(tp[:, 0], tp[:, 2]) / torch.maximum(tp[:, 0], tp[:, 2])) *
                     (torch.minimum(tp[:, 1], tp[:, 3]) / torch.maximum(tp[:, 1], tp[:, 3]))).to(F64)
    ar = lambda n: torch.arange(n, device=dev)
    on = lambda t: t.to(dev).to(F64)
    lr = LaunchRef('ASSIGN')
    for nm, ptr, dt, idx, ref in (('labels', d.labels, torch.int64, ar(M), labels), ('assign_idx', d.assign_idx, torch.int32, ar(M), aidx),
                                  ('bbox_targets', d.bbox_targets, f32, ar(4 * M).view(M, 4), tgt),
                                  ('cls_weight', d.cls_weight, f32, ar(M), wgt * sw), ('pos_weight', d.pos_weight, f32, ar(M), sw)):
        mem.find(ptr, idx.numel() * torch.empty(0, dtype=dt).element_size(), f'{name}.{nm}')
        lr.outs.append(Out(f'{name}.{nm}', ptr, dt, idx, on(ref), on(ref).abs(), 0.0, exact=True))
    mem.find(d.stats, 32, f'{name}.stats')
    st = torch.zeros(8, dtype=F64)
    st[0], st[1] = float(pos.sum()), float(ctr.sum())
    Sst = torch.zeros(8, dtype=F64)
    Sst[1] = float(ctr.abs().sum())
    lr.outs.append(Out(f'{name}.stats', d.stats, f32, ar(8), on(st), on(Sst), BETA['loss_sum']))
    _allow(mem, lr, d.workspace, d.workspace_bytes, f'{name}.workspace')
    lr.extra.update(pos=int(pos.sum()), M=M)
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# the fused FCOS loss (csrc/fcos_loss.hip loss_kernel + fcos_finalize_kernel), float64 from the launch's own inputs
FOCAL_ALPHA = 0.25


def loss_ref(mem, d, name='loss', beta=None, partner_level=-1, relu_mask=True):
    """dsl_fcos_loss.  Focal (alpha 0.25, gamma 2) x cls_weight / num_pos; GIoU on distance2bbox(point, relu(raw x scale)) against
    the targets, x centerness target x pos_weight / denorm, torch's 0.5 / 0.5 split of max / min gradients on ties and its eps
    clamps; centerness BCE x pos_weight / num_pos; sisoft (soft_weight != 0, n odd >= 3): mean (x[lvl][n-2] - x[lvl-1][n-1][:h, :w])^2
    over levels >= 1, gradients both ways; gradients x grad_scale; num_pos = max(norm[0] inv_world, 1), denorm = max(norm[1]
    inv_world, 1e-6) from the norm[] in device memory.  The max / min decisions of the GIoU are taken on the fp32 box corners
    (point -+ distance, rounded as the kernel forms them: they differ in the last bit of a 1000-pixel coordinate); everything else is
    float64.  Outputs: g_cls (columns C .. ld_gcls zero), g_rc (columns 5 .. 7 zero), g_scales[5], losses[4], logvec (post: the fp32
    recombination fcos_finalize_kernel documents, bit for bit, of the losses the launch wrote).
    S: the sum of the absolute term contributions; a positive's focal term also carries 2^-8 |d term / d q| (q = 1 - p is formed in
    fp32: an absolute error of 2^-24 = 2^-8 beta).  partner_level / relu_mask: negative-control hooks (sisoft partner level offset,
    the ReLU mask of the box gradient)."""
    d = d if isinstance(d, types.SimpleNamespace) else _ns(d)
    beta = BETA['loss'] if beta is None else beta
    bsum = BETA['loss_sum']
    dev = mem.device_of(d.cls_logits, f'{name}.cls_logits')
    f32 = torch.float32
    lvl, img, y, x, ms = _fcos_locations(d)
    lvl, img, y, x = (t.to(dev) for t in (lvl, img, y, x))
    M, C, C4 = ms[-1], d.num_classes, (d.num_classes + 3) // 4 * 4
    logits = _gather_rows(mem.typed(d.cls_logits, f32, (M - 1) * d.ld_cls + C4, f'{name}.cls_logits'), torch.arange(M, device=dev),
                          d.ld_cls, C)
    rc = _gather_rows(mem.typed(d.regctr, f32, (M - 1) * d.ld_rc + 5, f'{name}.regctr'), torch.arange(M, device=dev), d.ld_rc, 5)
    labels = mem.typed(d.labels, torch.int64, M, f'{name}.labels')
    tg = mem.typed(d.bbox_targets, f32, 4 * M, f'{name}.bbox_targets').view(M, 4)
    cw = mem.typed(d.cls_weight, f32, M, f'{name}.cls_weight').to(F64)
    pw = mem.typed(d.pos_weight, f32, M, f'{name}.pos_weight').to(F64)
    scales = mem.typed(d.scales, f32, d.nlvl, f'{name}.scales')
    norm = mem.typed(d.norm, f32, 2, f'{name}.norm').clone()
    iw = torch.tensor(d.inv_world, dtype=f32, device=dev)
    num_pos = float(torch.clamp_min(norm[0] * iw, 1.0))
    denorm = float(torch.clamp_min(norm[1] * iw, 1e-6))
    gs = float(torch.tensor(d.grad_scale, dtype=f32))
    sw = float(torch.tensor(d.soft_weight, dtype=f32))
    a = FOCAL_ALPHA
    # -- focal
    t = labels.view(-1, 1) == torch.arange(C, device=dev).view(1, -1)
    p, q = torch.sigmoid(logits), torch.sigmoid(-logits)
    sp_pos, sp_neg = torch.nn.functional.softplus(-logits), torch.nn.functional.softplus(logits)
    l_el = torch.where(t, a * q * q * sp_pos, (1 - a) * p * p * sp_neg)
    g_el = torch.where(t, -a * q * q * (2 * p * sp_pos + q), (1 - a) * p * p * (2 * q * sp_neg + p))
    cond_g = torch.where(t, a * (2 * q * (2 * p * sp_pos + q) + q * q) * BF16_REL, torch.zeros_like(q))
    cond_l = torch.where(t, a * 2 * q * sp_pos * BF16_REL, torch.zeros_like(q))
    k = (cw / num_pos * gs).view(-1, 1)
    g_cls = g_el * k
    S_cls = (g_el.abs() + cond_g) * k.abs()
    L_cls = (l_el * cw.view(-1, 1)).sum() / num_pos
    S_Lcls = ((l_el.abs() + cond_l) * cw.abs().view(-1, 1)).sum() / num_pos
    # -- sisoft
    L_soft = S_soft = 0.0
    if sw != 0.0 and d.n % 2 == 1 and d.n >= 3:
        for l in range(1, d.nlvl):
            pl = l + partner_level
            h, w = d.h[l], d.w[l]
            yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
            ma = ms[l] + ((d.n - 2) * h + yy.reshape(-1)) * w + xx.reshape(-1)
            mb = ms[pl] + ((d.n - 1) * d.h[pl] + yy.reshape(-1)) * d.w[pl] + xx.reshape(-1)
            cnt = C * h * w
            dd = logits[ma] - logits[mb]
            L_soft += float((dd * dd).sum()) / cnt * sw
            S_soft += float((dd * dd).sum()) / cnt * abs(sw)
            gterm = 2 * dd / cnt * sw * gs
            g_cls.index_add_(0, ma, gterm)
            g_cls.index_add_(0, mb, -gterm)
            S_cls.index_add_(0, ma, gterm.abs())
            S_cls.index_add_(0, mb, gterm.abs())
    # -- boxes and centerness at the positives
    pos = (labels < C).nonzero().view(-1)
    g_rc = torch.zeros(M, 8, dtype=F64, device=dev)
    S_rc = torch.zeros_like(g_rc)
    g_sc = torch.zeros(DSL_MAX_SEG, dtype=F64, device=dev)
    S_sc = torch.zeros_like(g_sc)
    L_box = S_box = L_ctr = S_ctr = 0.0
    if pos.numel():
        lv = lvl[pos]
        s = torch.tensor([d.stride[l] for l in range(d.nlvl)], device=dev)[lv]
        px = (x[pos].to(f32) * s.to(f32) + (s // 2).to(f32)).view(-1, 1)
        py = (y[pos].to(f32) * s.to(f32) + (s // 2).to(f32)).view(-1, 1)
        sc32 = scales[lv].view(-1, 1)
        raw32 = mem.typed(d.regctr, f32, (M - 1) * d.ld_rc + 5, f'{name}.regctr').view(-1)[
            pos.view(-1, 1) * d.ld_rc + torch.arange(4, device=dev).view(1, -1)]
        d32 = torch.clamp_min(raw32 * sc32, 0.0)
        t32 = tg[pos]
        # fp32 corners (the kernel's), then float64
        P1 = torch.cat([px - d32[:, :1], py - d32[:, 1:2], px + d32[:, 2:3], py + d32[:, 3:4]], 1).to(F64)
        T1 = torch.cat([px - t32[:, :1], py - t32[:, 1:2], px + t32[:, 2:3], py + t32[:, 3:4]], 1).to(F64)
        raw, sc, t64 = raw32.to(F64), sc32.to(F64), t32.to(F64)
        # the centerness target in fp32, as the kernel and the reference (fcos_head.py:707-726 on fp32 targets) form it
        ct32 = torch.sqrt((torch.minimum(t32[:, 0], t32[:, 2]) / torch.maximum(t32[:, 0], t32[:, 2])) *
                          (torch.minimum(t32[:, 1], t32[:, 3]) / torch.maximum(t32[:, 1], t32[:, 3])))
        ct = ct32.to(F64)
        x1, y1, x2, y2 = P1.unbind(1)
        X1, Y1, X2, Y2 = T1.unbind(1)
        eps = float(torch.tensor(1e-6, dtype=f32))
        dmax = lambda u, v: torch.where(u > v, 1.0, torch.where(u == v, 0.5, 0.0)).to(F64)
        dmin = lambda u, v: torch.where(u < v, 1.0, torch.where(u == v, 0.5, 0.0)).to(F64)
        a1, a2 = (x2 - x1) * (y2 - y1), (X2 - X1) * (Y2 - Y1)
        w0, h0 = torch.minimum(x2, X2) - torch.maximum(x1, X1), torch.minimum(y2, Y2) - torch.maximum(y1, Y1)
        iw_, ih = w0.clamp_min(0), h0.clamp_min(0)
        ov = iw_ * ih
        u0 = a1 + a2 - ov
        U = u0.clamp_min(eps)
        ew0, eh0 = torch.maximum(x2, X2) - torch.minimum(x1, X1), torch.maximum(y2, Y2) - torch.minimum(y1, Y1)
        ew, eh = ew0.clamp_min(0), eh0.clamp_min(0)
        e0 = ew * eh
        E = e0.clamp_min(eps)
        giou = ov / U - (E - U) / E
        wb = (ct32 * pw[pos].float()).to(F64)           # (an fp32 product in the kernel and the reference alike)
        L_box = float((wb * (1 - giou)).sum()) / denorm
        S_box = float((wb.abs() * (1 + ov / U + (E - U).abs() / E)).sum()) / denorm
        cw_, ch_ = (w0 >= 0).to(F64), (h0 >= 0).to(F64)
        dov = torch.stack([ih * -dmax(x1, X1) * cw_, iw_ * -dmax(y1, Y1) * ch_, ih * dmin(x2, X2) * cw_, iw_ * dmin(y2, Y2) * ch_], 1)
        da1 = torch.stack([-(y2 - y1), -(x2 - x1), y2 - y1, x2 - x1], 1)
        ug = torch.where(u0 > eps, 1.0, torch.where(u0 == eps, 0.5, 0.0)).to(F64).view(-1, 1)
        eg = torch.where(e0 > eps, 1.0, torch.where(e0 == eps, 0.5, 0.0)).to(F64).view(-1, 1)
        cew, ceh = (ew0 >= 0).to(F64), (eh0 >= 0).to(F64)
        de = torch.stack([eh * -dmin(x1, X1) * cew, ew * -dmin(y1, Y1) * ceh, eh * dmax(x2, X2) * cew, ew * dmax(y2, Y2) * ceh], 1) * eg
        dU = (da1 - dov) * ug
        U_, E_, ov_ = U.view(-1, 1), E.view(-1, 1), ov.view(-1, 1)
        dg = dov / U_ - ov_ * dU / (U_ * U_) + dU / E_ - U_ * de / (E_ * E_)
        Sdg = dov.abs() / U_ + ov_ * (da1.abs() + dov.abs()) * ug / (U_ * U_) + (da1.abs() + dov.abs()) * ug / E_ + U_ * de.abs() / (E_ * E_)
        coef = (-wb / denorm * gs).view(-1, 1)
        sign = torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=F64, device=dev)
        dd = coef * dg * sign
        Sdd = coef.abs() * Sdg
        on = (raw * sc > 0).to(F64) if relu_mask else torch.ones_like(raw)
        g_rc[pos, :4] = dd * on * sc
        S_rc[pos, :4] = Sdd * on * sc.abs()
        g_sc.index_add_(0, lv, (dd * on * raw).sum(1))
        S_sc.index_add_(0, lv, (Sdd * on * raw.abs()).sum(1))
        cl = rc[pos, 4]
        ppw = pw[pos]
        ce = torch.clamp_min(cl, 0) - cl * ct + torch.log1p(torch.exp(-cl.abs()))
        L_ctr = float((ce * ppw).sum()) / num_pos
        S_ctr = float(((torch.clamp_min(cl, 0) + (cl * ct).abs() + torch.log1p(torch.exp(-cl.abs()))) * ppw.abs()).sum()) / num_pos
        sig = torch.sigmoid(cl)
        g_rc[pos, 4] = (sig - ct) * ppw / num_pos * gs
        S_rc[pos, 4] = (sig + ct) * (ppw / num_pos * gs).abs()
    # -- outputs
    ar = lambda n: torch.arange(n, device=dev)
    lr = LaunchRef('LOSS')
    G = torch.zeros(M, d.ld_gcls, dtype=F64, device=dev)
    SG = torch.zeros_like(G)
    G[:, :C], SG[:, :C] = g_cls, S_cls
    mem.find(d.g_cls, M * d.ld_gcls * 2, f'{name}.g_cls')
    lr.outs.append(Out(f'{name}.g_cls', d.g_cls, torch.bfloat16, ar(M * d.ld_gcls).view(M, d.ld_gcls), G, SG, beta))
    mem.find(d.g_rc, ((M - 1) * d.ld_grc + 8) * 2, f'{name}.g_rc')
    lr.outs.append(Out(f'{name}.g_rc', d.g_rc, torch.bfloat16, ar(M).view(-1, 1) * d.ld_grc + ar(8).view(1, -1), g_rc, S_rc, beta))
    lr.outs.append(Out(f'{name}.g_scales', d.g_scales, f32, ar(DSL_MAX_SEG), g_sc, S_sc, bsum))
    losses = torch.tensor([L_cls, L_box, L_ctr, L_soft], dtype=F64, device=dev)
    S_l = torch.tensor([float(S_Lcls), S_box, S_ctr, S_soft], dtype=F64, device=dev)
    lr.outs.append(Out(f'{name}.losses', d.losses, f32, ar(4), losses, S_l, bsum))
    if d.logvec:
        def post(mem=mem, d=d):
            lo = mem.typed(d.losses, f32, 4, f'{name}.losses').clone()
            terms = [lo[0], lo[1], lo[2]] + ([lo[3]] if sw != 0.0 else [])
            tot = (lo[0] + lo[1]) + lo[2]
            if sw != 0.0:
                tot = tot + lo[3]
            ref = torch.stack(terms + [tot]).to(F64)
            return [Out(f'{name}.logvec', d.logvec, f32, ar(ref.numel()), ref, ref.abs(), 0.0, exact=True)]
        mem.find(d.logvec, 20, f'{name}.logvec')
        lr.post.append(post)
    _allow(mem, lr, d.workspace, d.workspace_bytes, f'{name}.workspace')
    lr.extra.update(pos=int(pos.numel()), num_pos=num_pos, denorm=denorm)
    return lr


# ------------------------------------------------------------------------------------------------------------------------------
# fp8 quantisers (csrc/optim.hip): bytes bit-exact against torch's e4m3 cast, scales and maxima in fp32
E4M3_MAX = 448.0


def e4m3_bytes(v32, scale32):
    """clamp(v x scale, +-448) cast by torch.float8_e4m3fn (RNE), as bytes -> float64 (v, scale fp32: one fp32 product)."""
    return (v32 * scale32).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8).to(F64)


def e4m3_scale(m):
    """448 / m as the kernels form it: one correctly rounded fp32 division (IEEE divide; torch's `448.0 / tensor` is a reciprocal
    and a product, two roundings), 1 where m == 0."""
    return torch.where(m > 0, torch.full_like(m, E4M3_MAX) / m, torch.ones_like(m))


def e4m3_inv(a):
    """a / 448, correctly rounded (a tensor divisor: on the GPU torch divides by a scalar as a product with its reciprocal), 1 where
    a == 0."""
    return torch.where(a > 0, a / torch.full_like(a, E4M3_MAX), torch.ones_like(a))


def _bf16_rows(mem, ptr, rows, c, ld, what):
    return _gather_rows(mem.typed(ptr, torch.bfloat16, (rows - 1) * ld + c, what), torch.arange(rows, device=mem.device_of(ptr, what)),
                        ld, c).float()


def _block_max(xa, rows, c, per, grid):
    """max over the per-element chunks that each of `grid` grid-stride workgroups of 256 threads visits (chunk j -> block
    (j // 256) % grid) of |x| [rows][c] (fp32)."""
    ch = xa.reshape(rows * (c // per), per).amax(1)
    blk = (torch.arange(ch.numel(), device=xa.device) // 256) % grid
    out = torch.zeros(grid, dtype=xa.dtype, device=xa.device)
    return out.scatter_reduce(0, blk, ch, 'amax', include_self=True)


def _fbits(bits):
    return float(torch.tensor([bits & 0xffffffff], dtype=torch.int64).to(torch.int32).view(torch.float32)[0])


def quant_fp8_ref(mem, x_ptr, y_ptr, rows, c, ld_x, scale_bits, partials=0, n_partials=0, name='quant_fp8', scale_mul=1.0):
    """DSL_OP_QUANT_FP8: fixed scale (the float whose bits are l[1]), or absmax block maxima + scale = 448 / max.  scale_mul:
    negative-control hook."""
    x = _bf16_rows(mem, x_ptr, rows, c, ld_x, f'{name}.x')
    dev = x.device
    lr = LaunchRef('QUANT_FP8')
    if partials:
        pm = _block_max(x.abs(), rows, c, 8, n_partials)
        amax = pm.max()
        scale = e4m3_scale(amax)
        lr.outs.append(Out(f'{name}.partials', partials, torch.float32, torch.arange(n_partials, device=dev), pm.to(F64), pm.to(F64), 0.0,
                           exact=True))
    else:
        scale = torch.tensor(_fbits(scale_bits), dtype=torch.float32, device=dev)
    q = e4m3_bytes(x, scale * scale_mul)
    mem.find(y_ptr, rows * c, f'{name}.y')
    lr.outs.insert(0, Out(f'{name}.y', y_ptr, torch.uint8, torch.arange(rows * c, device=dev).view(rows, c), q, q, 0.0, exact=True))
    return lr


def _w8_rows(w, cout, cout_pad, k, inv_act, bn=None):
    """quantised weight rows [cout_pad][k] (bytes, float64) and comb [cout_pad] (fp32 arithmetic, the kernels' order) of fp32 w
    [cout][k]; padding rows zero."""
    s = e4m3_scale(w.abs().amax(1))
    w8 = torch.zeros(cout_pad, k, dtype=F64, device=w.device)
    w8[:cout] = e4m3_bytes(w, s.view(-1, 1))
    comb = torch.zeros(cout_pad, dtype=torch.float32, device=w.device)
    comb[:cout] = inv_act / s * (bn if bn is not None else 1.0)
    return w8, comb.to(F64)


def quant_fp8_w_ref(mem, w_ptr, w8_ptr, comb_ptr, bn_ptr, cout, cout_pad, k, inv_bits, name='quant_fp8_w'):
    w = mem.typed(w_ptr, torch.float32, cout * k, f'{name}.w').view(cout, k)
    bn = mem.typed(bn_ptr, torch.float32, cout, f'{name}.bn_scale') if bn_ptr else None
    inv = torch.tensor(_fbits(inv_bits), dtype=torch.float32, device=w.device)
    w8, comb = _w8_rows(w, cout, cout_pad, k, inv, bn)
    mem.find(w8_ptr, cout_pad * k, f'{name}.w8')
    lr = LaunchRef('QUANT_FP8_W')
    ar = lambda n: torch.arange(n, device=w.device)
    lr.outs.append(Out(f'{name}.w8', w8_ptr, torch.uint8, ar(cout_pad * k).view(cout_pad, k), w8, w8, 0.0, exact=True))
    lr.outs.append(Out(f'{name}.comb', comb_ptr, torch.float32, ar(cout_pad), comb, comb, 0.0, exact=True))
    return lr


def fp8_comb_ref(mem, winv_ptr, comb_ptr, n, partials, n_partials, name='fp8_comb'):
    winv = mem.typed(winv_ptr, torch.float32, n, f'{name}.winv')
    amax = mem.typed(partials, torch.float32, n_partials, f'{name}.partials').max()
    inv = e4m3_inv(amax)
    ref = (winv * inv).to(F64)
    lr = LaunchRef('FP8_COMB')
    lr.outs.append(Out(f'{name}.comb', comb_ptr, torch.float32, torch.arange(n, device=winv.device), ref, ref, 0.0, exact=True))
    return lr


class Fp8PrepItem(C.Structure):
    """dsl_fp8_prep_item (mirrors include/dsl_hip.h and dsl_amd/_lib.py; kept here so that the CPU tests need no library)"""
    _fields_ = [('w', C.c_void_p), ('w8', C.c_void_p), ('comb', C.c_void_p), ('amax', C.c_void_p), ('scale', C.c_void_p),
                ('n_amax', C.c_int32), ('cout', C.c_int32)]


def fp8_prep_ref(mem, items_ptr, n_items, cout_pad, k, margin_bits, name='fp8_prep'):
    """DSL_OP_FP8_PREP over the item table in device memory: per item a = margin x max(amax[0 .. n_amax)), scale[0] = 448 / a (1 when
    a == 0: nothing recorded yet), w8 / comb = the weight rows quantised with comb[co] = (a / 448 or 1) / s_w[co]; rows >= cout zero."""
    sz = C.sizeof(Fp8PrepItem)
    raw = bytes(mem.typed(items_ptr, torch.uint8, n_items * sz, f'{name}.items').cpu().numpy().tobytes())
    margin = torch.tensor(_fbits(margin_bits), dtype=torch.float32)
    lr = LaunchRef('FP8_PREP')
    lr.extra['cold'] = 0
    for j in range(n_items):
        it = Fp8PrepItem.from_buffer_copy(raw[j * sz:(j + 1) * sz])
        w = mem.typed(it.w, torch.float32, it.cout * k, f'{name}[{j}].w').view(it.cout, k)
        dev = w.device
        a = mem.typed(it.amax, torch.float32, it.n_amax, f'{name}[{j}].amax').max() * margin.to(dev)
        scale = e4m3_scale(a)
        inv_act = e4m3_inv(a)
        lr.extra['cold'] += int(not bool(a > 0))
        w8, comb = _w8_rows(w, it.cout, cout_pad, k, inv_act)
        ar = lambda n: torch.arange(n, device=dev)
        mem.find(it.w8, cout_pad * k, f'{name}[{j}].w8')
        lr.outs.append(Out(f'{name}[{j}].w8', it.w8, torch.uint8, ar(cout_pad * k).view(cout_pad, k), w8, w8, 0.0, exact=True))
        lr.outs.append(Out(f'{name}[{j}].comb', it.comb, torch.float32, ar(cout_pad), comb, comb, 0.0, exact=True))
        sc64 = scale.view(1).to(F64)
        lr.outs.append(Out(f'{name}[{j}].scale', it.scale, torch.float32, ar(1), sc64, sc64, 0.0, exact=True))
    return lr


def quant_fp8_delayed_ref(mem, x_ptr, y_ptr, partials, scale_ptr, rows, c, ld_x, n_partials, name='quant_fp8_delayed', scale_mul=1.0):
    """y = e4m3(clamp(x x scale[0], +-448)) with the scale in device memory; partials[b] = max |x| over the 16-element chunks
    workgroup b visits (n_partials workgroups, grid-stride)."""
    x = _bf16_rows(mem, x_ptr, rows, c, ld_x, f'{name}.x')
    dev = x.device
    scale = mem.typed(scale_ptr, torch.float32, 1, f'{name}.scale')[0].clone()
    q = e4m3_bytes(x, scale * scale_mul)
    pm = _block_max(x.abs(), rows, c, 16, n_partials).to(F64)
    mem.find(y_ptr, rows * c, f'{name}.y')
    lr = LaunchRef('QUANT_FP8_DELAYED')
    lr.outs.append(Out(f'{name}.y', y_ptr, torch.uint8, torch.arange(rows * c, device=dev).view(rows, c), q, q, 0.0, exact=True))
    lr.outs.append(Out(f'{name}.partials', partials, torch.float32, torch.arange(n_partials, device=dev), pm, pm, 0.0, exact=True))
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
    if k == OP_ASSIGN:
        return assign_ref(mem, C.cast(op.desc, C.POINTER(L.FcosDesc)).contents, nm)
    if k == OP_LOSS:
        return loss_ref(mem, C.cast(op.desc, C.POINTER(L.FcosDesc)).contents, nm)
    if k == OP_QUANT_FP8:
        return quant_fp8_ref(mem, op.p[0], op.p[1], op.l[0], op.i[0], op.i[1], op.l[1], op.p[2] or 0, op.i[2], name=nm)
    if k == OP_QUANT_FP8_W:
        return quant_fp8_w_ref(mem, op.p[0], op.p[1], op.p[2], op.p[3] or 0, op.i[0], op.i[1], op.i[2], op.l[1], name=nm)
    if k == OP_FP8_COMB:
        return fp8_comb_ref(mem, op.p[0], op.p[1], op.i[0], op.p[2], op.i[2], name=nm)
    if k == OP_FP8_PREP:
        return fp8_prep_ref(mem, op.p[0], op.i[0], op.i[1], op.i[2], op.l[1], name=nm)
    if k == OP_QUANT_FP8_DELAYED:
        return quant_fp8_delayed_ref(mem, op.p[0], op.p[1], op.p[2], op.p[3], op.l[0], op.i[0], op.i[1], op.i[2], name=nm)
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

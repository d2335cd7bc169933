"""The float64 op-list interpreter (tests/op_ref.py) against fp64 torch on the CPU, its negative controls and its pointer resolver.

op_ref is what tests/test_step_replay_gpu.py holds every launch of a real step to, so it is itself checked here against an
independent formulation (F.conv2d / autograd / F.group_norm in float64) at every flag and mode combination the engines emit."""
import types

import pytest
import torch
import torch.nn.functional as F

import gn_cases
import op_ref as R

F64 = torch.float64
torch.manual_seed(0)


def _pad5(v):
    return list(v) + [0] * (5 - len(v))


def cdesc(**kw):
    d = dict(nseg=1, n=1, ah=[], aw=[], mode=0, os=1, flags=0, scale=0, bias=0, addend=0, mask=0, lda=0, ldm=0, workspace=0,
             workspace_bytes=0, gn_ws=0, lds=0, stride=1, pad=0, cs_real=0)
    d.update(kw)
    for k in ('gh', 'gw', 'sh', 'sw', 'dh', 'dw', 'ah', 'aw'):
        d[k] = _pad5(d[k])
    return types.SimpleNamespace(**d)


def wdesc(**kw):
    d = dict(nseg=1, n=1, scale=0, db=0, workspace=0, workspace_bytes=0, ldx=0, shared=0, stride=1, pad=0)
    d.update(kw)
    for k in ('gh', 'gw', 'sh', 'sw'):
        d[k] = _pad5(d[k])
    return types.SimpleNamespace(**d)


def mem_of(**ts):
    return R.Memory({'t': ts})


def rows_to_nchw(rows, n, h, w, c):
    return rows[:n * h * w].view(n, h, w, -1)[..., :c].permute(0, 3, 1, 2).to(F64)


def seg_rows(t, segs, n, ld):
    """split a level-major [segment][image][y][x][ld] buffer into per-segment [n*h*w][ld] views"""
    out, o = [], 0
    for h, w in segs:
        out.append(t[o * ld:(o + n * h * w) * ld].view(n * h * w, ld))
        o += n * h * w
    return out


def store_(dst, idx, v):
    dst.view(-1)[idx.reshape(-1)] = v.reshape(-1).to(dst.dtype)


def fill_conv_dst(lr, dst, vals):
    store_(dst, lr.outs[0].idx, vals)


# ------------------------------------------------------------------------------------------------------------------------------
# DSL_OP_CONV, forward mode, three segments with an odd last level, channel-sliced source, padded destination rows
@pytest.mark.parametrize('variant', ['affine_mask_first_addend', 'mask_last_relu_f32', 'relu_in', 'upsample_addend'])
def test_conv_mode0_matches_fp64_conv2d(variant):
    n, cs, lds, cd, cd_pad, ldd = 2, 64, 96, 40, 64, 48
    src_hw = [(17, 25), (9, 13), (5, 7)]
    out_hw = [((h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1) for h, w in src_hw]        # (9, 13), (5, 7), (3, 4)
    kh, stride, pad = 3, 2, 1
    if variant == 'upsample_addend':
        src_hw = out_hw = [(10, 14), (5, 7)]
        kh, stride, pad = 1, 1, 0
    npx_s = sum(n * h * w for h, w in src_hw)
    npx_d = sum(n * h * w for h, w in out_hw)
    src = torch.randn(npx_s * lds).bfloat16()
    wgt = (torch.randn(cd_pad * kh * kh * cs) * 0.1).bfloat16()
    dst = torch.full((npx_d * ldd,), 7.0, dtype=torch.float32 if variant == 'mask_last_relu_f32' else torch.bfloat16)
    scale, bias = torch.rand(cd) + 0.5, torch.randn(cd)
    lda, ldm = 44, 48
    add_hw = [(5, 7), (3, 4)] if variant == 'upsample_addend' else out_hw
    addend = torch.randn(sum(n * h * w for h, w in add_hw) * lda).bfloat16()
    mask = torch.randn(npx_d * ldm).bfloat16()
    flags = {'affine_mask_first_addend': R.CONV_MASK_FIRST | R.CONV_RELU_OUT, 'mask_last_relu_f32': R.CONV_MASK_LAST | R.CONV_RELU_OUT |
             R.CONV_OUT_F32, 'relu_in': R.CONV_RELU_IN, 'upsample_addend': R.CONV_ADD_UPSAMPLE}[variant]
    use_add = variant in ('affine_mask_first_addend', 'mask_last_relu_f32', 'upsample_addend')
    use_mask = variant in ('affine_mask_first_addend', 'mask_last_relu_f32')
    mem = mem_of(src=src, wgt=wgt, dst=dst, scale=scale, bias=bias, addend=addend, mask=mask)
    d = cdesc(nseg=len(out_hw), n=n, gh=[h for h, _ in out_hw], gw=[w for _, w in out_hw], sh=[h for h, _ in src_hw],
              sw=[w for _, w in src_hw], dh=[h for h, _ in out_hw], dw=[w for _, w in out_hw], ah=[h for h, _ in add_hw],
              aw=[w for _, w in add_hw], cs=cs, cd=cd, cd_pad=cd_pad, ldd=ldd, lda=lda, ldm=ldm, kh=kh, kw=kh, stride=stride, pad=pad,
              flags=flags, src=src.data_ptr(), wgt=wgt.data_ptr(), dst=dst.data_ptr(), scale=scale.data_ptr(), bias=bias.data_ptr(),
              addend=addend.data_ptr() if use_add else 0, mask=mask.data_ptr() if use_mask else 0, lds=lds)
    lr = R.conv_ref(mem, d)
    # independent: F.conv2d in float64 per segment, then the header's epilogue
    W = wgt.view(cd_pad, kh, kh, cs)[:cd].permute(0, 3, 1, 2).to(F64)
    refs = []
    for s, ((sh, sw), (oh, ow), (ah, aw), srows, arows, mrows) in enumerate(zip(
            src_hw, out_hw, add_hw, seg_rows(src, src_hw, n, lds), seg_rows(addend, add_hw, n, lda), seg_rows(mask, out_hw, n, ldm))):
        x = rows_to_nchw(srows, n, sh, sw, cs)
        if variant == 'relu_in':
            x = x.clamp_min(0)
        v = F.conv2d(x, W, stride=stride, padding=pad).permute(0, 2, 3, 1) * scale.to(F64) + bias.to(F64)
        m = (rows_to_nchw(mrows, n, oh, ow, cd).permute(0, 2, 3, 1) > 0).to(F64)
        if variant == 'affine_mask_first_addend':
            v = v * m
        if use_add:
            a = rows_to_nchw(arows, n, ah, aw, cd)
            if (ah, aw) != (oh, ow):
                a = F.interpolate(a, size=(oh, ow), mode='nearest')
            v = v + a.permute(0, 2, 3, 1)
        if variant == 'mask_last_relu_f32':
            v = v * m
        if flags & R.CONV_RELU_OUT:
            v = v.clamp_min(0)
        refs.append(v.reshape(-1, cd))
    ref = torch.cat(refs)
    assert torch.allclose(lr.outs[0].ref, ref, rtol=1e-12, atol=1e-12)
    # a correctly rounded output passes, and nothing else in its allocation may change
    res = R.run_checked(mem, lr, lambda: fill_conv_dst(lr, dst, ref))
    assert res[0][1] <= 1.0 and res[0][2] == 0, res
    assert (dst.view(-1, ldd)[:, cd:] == 7.0).all()


def test_conv_fp8_operands_decode_as_e4m3():
    n, h, w, cs, cd = 1, 6, 7, 128, 64
    src = (torch.randn(n * h * w * cs) * 4).to(torch.float8_e4m3fn)
    wgt = (torch.randn(cd * 9 * cs) * 4).to(torch.float8_e4m3fn)
    scale = torch.rand(cd) * 1e-2
    dst = torch.zeros(n * h * w * cd, dtype=torch.bfloat16)
    mem = mem_of(src=src, wgt=wgt, dst=dst, scale=scale)
    d = cdesc(n=n, gh=[h], gw=[w], sh=[h], sw=[w], dh=[h], dw=[w], cs=cs, cd=cd, cd_pad=cd, ldd=cd, kh=3, kw=3, pad=1,
              flags=R.CONV_FP8, src=src.data_ptr(), wgt=wgt.data_ptr(), dst=dst.data_ptr(), scale=scale.data_ptr())
    lr = R.conv_ref(mem, d)
    x = src.to(F64).view(n, h, w, cs).permute(0, 3, 1, 2)
    W = wgt.to(F64).view(cd, 3, 3, cs).permute(0, 3, 1, 2)
    ref = (F.conv2d(x, W, padding=1).permute(0, 2, 3, 1) * scale.to(F64)).reshape(-1, cd)
    assert torch.allclose(lr.outs[0].ref, ref, rtol=1e-12, atol=1e-12)


def _dgrad_case(stride, k=3, pad=1, n=2, h=11, w=9, cin=64, cout=48, cout_pad=64):
    x = torch.randn(n, cin, h, w, dtype=F64, requires_grad=True)
    Wt = (torch.randn(cout, cin, k, k) * 0.1).bfloat16().to(F64)
    y = F.conv2d(x, Wt, stride=stride, padding=pad)
    dy = torch.randn_like(y).bfloat16().to(F64)
    dx, = torch.autograd.grad(y, x, dy)
    return x, Wt, dy, dx


def test_conv_mode1_strided_data_gradient_matches_autograd():
    """mode 1 (transposed gather) with stride 2: the data gradient of a 3x3 / 2 / pad 1 convolution from the CRSK pack."""
    n, h, w, cin, cout, cout_pad = 2, 11, 9, 64, 48, 64
    x, Wt, dy, dx = _dgrad_case(2, n=n, h=h, w=w, cin=cin, cout=cout, cout_pad=cout_pad)
    oh, ow = dy.shape[2:]
    src = torch.zeros(n * oh * ow * cout_pad, dtype=torch.bfloat16)          # dY rows padded to 64 channels (cs = 64)
    src.view(n, oh, ow, cout_pad)[..., :cout] = dy.permute(0, 2, 3, 1).bfloat16()
    pack = torch.zeros(cin, 3, 3, cout_pad, dtype=torch.bfloat16)
    pack[..., :cout] = Wt.permute(1, 2, 3, 0).bfloat16()
    dst = torch.zeros(n * h * w * cin, dtype=torch.bfloat16)
    mem = mem_of(src=src, pack=pack, dst=dst)
    d = cdesc(n=n, gh=[h], gw=[w], sh=[oh], sw=[ow], dh=[h], dw=[w], cs=cout_pad, cd=cin, cd_pad=cin, ldd=cin, kh=3, kw=3, stride=2,
              pad=1, mode=1, src=src.data_ptr(), wgt=pack.data_ptr(), dst=dst.data_ptr())
    lr = R.conv_ref(mem, d)
    assert torch.allclose(lr.outs[0].ref, dx.permute(0, 2, 3, 1).reshape(-1, cin), rtol=1e-12, atol=1e-12)


def test_conv_mode1_parity_classes_with_output_stride():
    """RLA's stride-2 data gradient as four stride-1 mode-1 launches with os = 2 (ops.dgrad_s2_descs): together they equal autograd."""
    from dsl_amd import ops
    n, h, w, cin, cout = 2, 11, 9, 64, 64
    x, Wt, dy, dx = _dgrad_case(2, n=n, h=h, w=w, cin=cin, cout=cout, cout_pad=cout)
    oh, ow = dy.shape[2:]
    src = dy.permute(0, 2, 3, 1).contiguous().bfloat16().view(-1)
    packs, keep = {}, []
    for py in (0, 1):
        for px in (0, 1):
            k, _, taps = ops.s2_class(py, px)
            p = torch.zeros(cin, k * k, cout, dtype=torch.bfloat16)
            for t, st in enumerate(taps):
                if st >= 0:
                    p[:, t] = Wt.permute(1, 2, 3, 0).reshape(cin, 9, cout)[:, st].bfloat16()
            packs[(py, px)] = p.data_ptr()
            keep.append(p)
    dst = torch.zeros(n * h * w * cin, dtype=torch.bfloat16)
    mem = mem_of(src=src, dst=dst, packs=keep)
    descs = ops.dgrad_s2_descs(src, packs, dst, n=n, dy_hw=(oh, ow), dst_hw=(h, w), cs=cout, cd=cin)
    assert len(descs) == 4
    for d in descs:
        lr = R.conv_ref(mem, d)
        R.run_checked(mem, lr, lambda: store_(dst.view(-1)[(d.dst - dst.data_ptr()) // 2:], lr.outs[0].idx, lr.outs[0].ref))
    assert torch.allclose(dst.to(F64), dx.permute(0, 2, 3, 1).reshape(-1).bfloat16().to(F64), rtol=2 ** -7, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------------
# weight gradients
def _wgrad_case(n, segs_in, k, stride, pad, cs, ldx, cd, cy, seed=0):
    g = torch.Generator().manual_seed(seed)
    segs_out = [((h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1) for h, w in segs_in]
    x = torch.randn(sum(n * h * w for h, w in segs_in) * ldx, generator=g).bfloat16()
    dy = torch.randn(sum(n * h * w for h, w in segs_out) * cy, generator=g).bfloat16()
    dW = torch.zeros(cd, cs, k, k, dtype=F64)
    for (h, w), (oh, ow), xr, gr in zip(segs_in, segs_out, seg_rows(x, segs_in, n, ldx), seg_rows(dy, segs_out, n, cy)):
        W = torch.zeros(cd, cs, k, k, dtype=F64, requires_grad=True)
        y = F.conv2d(rows_to_nchw(xr, n, h, w, cs), W, stride=stride, padding=pad)
        dW += torch.autograd.grad(y, W, rows_to_nchw(gr, n, oh, ow, cd))[0]
    db = sum(gr[:, :cd].to(F64).sum(0) for gr in seg_rows(dy, segs_out, n, cy))
    return x, dy, segs_out, dW.permute(0, 2, 3, 1).reshape(cd, -1), db


def test_wgrad_matches_autograd_with_scale_db_and_channel_slice():
    n, segs, k, cs, ldx, cd, cy = 2, [(13, 17), (7, 9), (4, 5)], 3, 64, 96, 40, 64
    x, dy, so, dW, db = _wgrad_case(n, segs, k, 1, 1, cs, ldx, cd, cy)
    scale = torch.rand(cd) + 0.5
    dw = torch.zeros(cd * k * k * cs)
    dbb = torch.zeros(cd)
    mem = mem_of(x=x, dy=dy, dw=dw, db=dbb, scale=scale)
    d = wdesc(nseg=3, n=n, gh=[h for h, _ in so], gw=[w for _, w in so], sh=[h for h, _ in segs], sw=[w for _, w in segs], cs=cs, cy=cy,
              cd=cd, kh=k, kw=k, stride=1, pad=1, dy=dy.data_ptr(), x=x.data_ptr(), scale=scale.data_ptr(), dw=dw.data_ptr(),
              db=dbb.data_ptr(), ldx=ldx)
    lr = R.wgrad_ref(mem, [d])
    outs = {o.name.split('.')[-1]: o for o in lr.outs}
    assert torch.allclose(outs['dw'].ref, dW * scale.to(F64).view(-1, 1), rtol=1e-12, atol=1e-10)
    assert torch.allclose(outs['db'].ref, db, rtol=1e-12, atol=1e-10)


def test_wgrad_strided_and_shared_group():
    """stride 2 (the FPN's P6 / P7 geometry) and a `shared` pair: two applications of one convolution summed into one dw."""
    n, segs, k, cs, cd, cy = 1, [(9, 11)], 3, 64, 64, 64
    a = _wgrad_case(n, segs, k, 2, 1, cs, cs, cd, cy, seed=1)
    b = _wgrad_case(n, segs, k, 2, 1, cs, cs, cd, cy, seed=2)
    dw = torch.zeros(cd * k * k * cs)
    mem = mem_of(x1=a[0], dy1=a[1], x2=b[0], dy2=b[1], dw=dw)
    so = a[2]
    mk = lambda x, dy: wdesc(n=n, gh=[so[0][0]], gw=[so[0][1]], sh=[segs[0][0]], sw=[segs[0][1]], cs=cs, cy=cy, cd=cd, kh=k, kw=k,
                             stride=2, pad=1, dy=dy.data_ptr(), x=x.data_ptr(), dw=dw.data_ptr(), shared=1)
    lr = R.wgrad_ref(mem, [mk(a[0], a[1]), mk(b[0], b[1])])
    assert len(lr.outs) == 1
    assert torch.allclose(lr.outs[0].ref, a[3] + b[3], rtol=1e-12, atol=1e-10)


# ------------------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU, 32 groups, two segments
def _gn_case(n=2, segs=((6, 10), (3, 5)), c=256, G=32, seed=3, structured=False):
    g = torch.Generator().manual_seed(seed)
    tot = sum(n * h * w for h, w in segs)
    if structured:         # the inputs of tests/test_groupnorm_gpu.py: offset groups, dy correlated with xhat, no ReLU decision on the edge
        return (n, list(segs), c, G, tot) + gn_cases.gn_inputs(n, segs, c, G, seed=seed)
    x = (torch.randn(tot * c, generator=g) * 2 + 0.5).bfloat16()
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    dy = torch.randn(tot * c, generator=g).bfloat16()
    return n, list(segs), c, G, tot, x, gamma, beta, dy


def _gn_torch(n, segs, c, G, x, gamma, beta, dy):
    outs, dxs, st = [], [], []
    dg, db = torch.zeros(c, dtype=F64), torch.zeros(c, dtype=F64)
    gam, bet = gamma.to(F64).requires_grad_(), beta.to(F64).requires_grad_()
    for (h, w), xr, gr in zip(segs, seg_rows(x, segs, n, c), seg_rows(dy, segs, n, c)):
        xx = rows_to_nchw(xr, n, h, w, c).requires_grad_()
        y = F.group_norm(xx, G, gam, bet, eps=1e-5).relu()
        g_ = rows_to_nchw(gr, n, h, w, c)
        dx, dga, dbe = torch.autograd.grad(y, (xx, gam, bet), g_)
        outs.append(y.detach().permute(0, 2, 3, 1).reshape(-1, c))
        dxs.append(dx.permute(0, 2, 3, 1).reshape(-1, c))
        dg += dga
        db += dbe
        xg = xx.detach().reshape(n, G, -1)
        st.append(torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-5).rsqrt()], -1).reshape(-1))
    return torch.cat(outs), torch.cat(st), torch.cat(dxs), dg, db


def _gn_desc(n, segs, c, G, x, y, gamma, beta, stats, **kw):
    d = dict(nseg=len(segs), n=n, c=c, groups=G, h=_pad5([h for h, _ in segs]), w=_pad5([w for _, w in segs]), eps=1e-5,
             x=x.data_ptr(), y=y.data_ptr() if y is not None else 0, gamma=gamma.data_ptr(), beta=beta.data_ptr(),
             stats=stats.data_ptr(), dy=0, dx=0, dgamma=0, dbeta=0, dbias=0, workspace=0, workspace_bytes=0, conv_stats=0, y8=0,
             y8_scale=0, y8_amax=0)
    d.update({k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    return types.SimpleNamespace(**d)


# the one earlier geometry with its centred inputs, then what tests/test_groupnorm_gpu.py leans on the references for: its (C, groups)
# pairs and its 65-row five-level geometry, on its inputs
GN_GEOMETRIES = [dict()] + [dict(n=2, segs=((5, 7), (2, 3)), c=c, G=G, seed=11 + i, structured=True)
                            for i, (c, G) in enumerate(gn_cases.CHANNELS)] + \
    [dict(n=13, segs=gn_cases.TINY5, c=256, G=32, seed=19, structured=True)]


@pytest.mark.parametrize('geo', GN_GEOMETRIES, ids=lambda g: 'N{n}-C{c}-G{G}'.format(**g) if g else 'centred')
def test_groupnorm_forward_and_backward_match_autograd(geo):
    n, segs, c, G, tot, x, gamma, beta, dy = _gn_case(**geo)
    y_t, st_t, dx_t, dg_t, db_t = _gn_torch(n, segs, c, G, x, gamma, beta, dy)
    y = torch.zeros(tot * c, dtype=torch.bfloat16)
    stats = st_t.float()
    dx = torch.zeros_like(y)
    dg, db, dbias = torch.zeros(c), torch.zeros(c), torch.zeros(c)
    mem = mem_of(x=x, y=y, gamma=gamma, beta=beta, stats=stats, dy=dy, dx=dx, dg=dg, db=db, dbias=dbias)
    f = R.gn_fwd_ref(mem, _gn_desc(n, segs, c, G, x, y, gamma, beta, stats))
    assert torch.allclose(f.outs[0].ref, y_t, rtol=1e-12, atol=1e-12)
    assert torch.allclose(f.outs[1].ref, st_t, rtol=1e-12, atol=1e-12)
    b = R.gn_bwd_ref(mem, _gn_desc(n, segs, c, G, x, None, gamma, beta, stats, dy=dy, dx=dx, dgamma=dg, dbeta=db, dbias=dbias))
    o = {k.name.split('.')[-1]: k for k in b.outs}
    # (the reference takes the stored fp32 statistics, autograd the exact ones: 2^-24-relative apart.  On the offset inputs that moves
    # xhat by 2^-24 xa with xa = (|x| + |mean|) rstd up to 40, 2.4e-6, and each term of dx, dgamma and dbias by that share of its
    # size: the absolute bars there are 4e-5 of the output's largest element.  No ReLU decision can differ: the inputs keep
    # every one 2^-16 relative from the edge.)
    if geo.get('structured'):
        ratio, sigma = gn_cases.group_statistics(x, n, segs, c, G)
        assert float(ratio.max()) > 12 and float(ratio.min()) < 1
        assert sigma.numel() < 16 or (float(sigma.min()) < 0.2 and float(sigma.max()) > 2)
        assert bool((gamma == 0).any()) and bool((gamma < 0).any()) and bool((beta < -9).any()) and bool((beta > 9).any())
        a_dx, a_dg, a_dbi = (4e-5 * float(t.abs().max()) for t in (dx_t, dg_t, dx_t.sum(0)))
    else:
        a_dx, a_dg, a_dbi = 1e-6, 1e-5, 1e-5
    assert torch.allclose(o['dx'].ref, dx_t, rtol=1e-5, atol=a_dx)
    assert torch.allclose(o['dgamma'].ref, dg_t, rtol=1e-5, atol=a_dg)
    assert torch.allclose(o['dbeta'].ref, db_t, rtol=1e-9, atol=1e-9)
    assert torch.allclose(o['dbias'].ref, dx_t.sum(0), rtol=1e-5, atol=a_dbi)
    for oo in b.outs:          # the autograd values pass their own bars
        ref = {'dx': dx_t, 'dgamma': dg_t, 'dbeta': db_t, 'dbias': dx_t.sum(0)}[oo.name.split('.')[-1]]
        assert R.compare(ref.view_as(oo.ref).to(oo.dtype).to(F64), oo.ref, oo.bound())[1] == 0, oo.name


# ------------------------------------------------------------------------------------------------------------------------------
# small ops
def test_maxpool_sum2x2_colsum_stem():
    n, h, w, c = 2, 9, 11, 64
    x = torch.randn(n * h * w * c).bfloat16()
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.zeros(n * oh * ow * 72, dtype=torch.bfloat16)
    mem = mem_of(x=x, y=y)
    lr = R.maxpool_ref(mem, x.data_ptr(), y.data_ptr(), n, h, w, c, 72)
    ref = F.max_pool2d(x.to(F64).view(n, h, w, c).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, c)
    assert torch.equal(lr.outs[0].ref, ref)
    # sum2x2: the backward of the nearest 2x upsample (ch, cw odd: the last children are missing)
    ch, cw = 2 * h - 1, 2 * w
    g = torch.randn(n * ch * cw * c).bfloat16()
    out = torch.zeros(n * h * w * c, dtype=torch.bfloat16)
    mem = mem_of(g=g, out=out)
    lr = R.sum2x2_ref(mem, g.data_ptr(), out.data_ptr(), n, h, w, ch, cw, c)
    src = torch.zeros(n, c, h, w, dtype=F64, requires_grad=True)
    up = F.interpolate(src, scale_factor=2, mode='nearest')[:, :, :ch, :cw]
    ref, = torch.autograd.grad(up, src, g.to(F64).view(n, ch, cw, c).permute(0, 3, 1, 2))
    assert torch.allclose(lr.outs[0].ref, ref.permute(0, 2, 3, 1).reshape(-1, c), rtol=1e-12, atol=1e-12)
    # colsum over padded rows
    xs = torch.randn(37 * 72).bfloat16()
    o = torch.zeros(64)
    lr = R.colsum_ref(mem_of(xs=xs, o=o), xs.data_ptr(), o.data_ptr(), 37, 64, 72)
    assert torch.allclose(lr.outs[0].ref, xs.view(37, 72)[:, :64].to(F64).sum(0), rtol=1e-12)
    # the fused stem: bf16(image) -> conv1 7x7 / 2 + BN + ReLU -> max pool 3x3 / 2, weights in the [22][64][8] group layout
    H, W_ = 30, 38
    img = torch.randn(2, 3, H, W_) * 30
    wt = (torch.randn(64, 7, 7, 3) * 0.05)
    wg = torch.zeros(64, 7, 24)
    wg[:, :, :21] = wt.reshape(64, 7, 21)
    wg = torch.cat([wg.reshape(64, 21, 8).permute(1, 0, 2), torch.zeros(1, 64, 8)], 0).bfloat16().contiguous()
    sc, bi = torch.rand(64) + 0.5, torch.randn(64)
    ph, pw = ((H - 1) // 2) // 2 + 1, ((W_ - 1) // 2) // 2 + 1
    out = torch.zeros(2 * ph * pw * 64, dtype=torch.bfloat16)
    mem = mem_of(img=img, wg=wg, sc=sc, bi=bi, out=out)
    lr = R.stem_pool_ref(mem, img.data_ptr(), wg.data_ptr(), sc.data_ptr(), bi.data_ptr(), out.data_ptr(), 64, 2, H, W_, 0)
    v = F.conv2d(img.bfloat16().to(F64), wt.bfloat16().to(F64).permute(0, 3, 1, 2), stride=2, padding=3)
    v = (v * sc.to(F64).view(1, -1, 1, 1) + bi.to(F64).view(1, -1, 1, 1)).relu()
    ref = F.max_pool2d(v, 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, 64)
    assert torch.allclose(lr.outs[0].ref, ref, rtol=1e-12, atol=1e-12)
    # with half_last, image 1 is the bilinear half-size copy of image 0 on a zero canvas
    lr = R.stem_pool_ref(mem, img.data_ptr(), wg.data_ptr(), sc.data_ptr(), bi.data_ptr(), out.data_ptr(), 64, 2, H, W_, 1)
    half = torch.zeros(1, 3, H, W_)
    half[:, :, :H // 2, :W_ // 2] = F.interpolate(img[:1], size=(H // 2, W_ // 2), mode='bilinear', align_corners=False)
    v = F.conv2d(torch.cat([img[:1], half]).bfloat16().to(F64), wt.bfloat16().to(F64).permute(0, 3, 1, 2), stride=2, padding=3)
    v = (v * sc.to(F64).view(1, -1, 1, 1) + bi.to(F64).view(1, -1, 1, 1)).relu()
    assert torch.allclose(lr.outs[0].ref, F.max_pool2d(v, 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, 64), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------------
# negative controls: the checker flags each defect applied to a copy of a correct output
def _flags(o, got):
    ratio, nbad, _ = R.compare(got.to(o.dtype).to(F64), o.ref, o.bound())
    return nbad > 0


def test_negative_controls_weight_gradient():
    n, segs, k, cs, cd, cy = 2, [(40, 56)], 3, 64, 64, 64
    x, dy, so, dW, db = _wgrad_case(n, segs, k, 1, 1, cs, cs, cd, cy, seed=4)
    dw = torch.zeros(cd * k * k * cs)
    mem = mem_of(x=x, dy=dy, dw=dw)
    d = wdesc(n=n, gh=[so[0][0]], gw=[so[0][1]], sh=[segs[0][0]], sw=[segs[0][1]], cs=cs, cy=cy, cd=cd, kh=k, kw=k, pad=1,
              dy=dy.data_ptr(), x=x.data_ptr(), dw=dw.data_ptr())
    o = R.wgrad_ref(mem, [d]).outs[0]
    assert not _flags(o, dW.float())                                           # the correct fp32 gradient passes
    no_img1 = R.wgrad_ref(mem, [d], drop={0: dict(drop_img=1)}).outs[0].ref
    assert _flags(o, no_img1.float()), 'one image missing'
    no_stage = R.wgrad_ref(mem, [d], drop={0: dict(drop_stage=(32 * 37, 32))}).outs[0].ref
    assert _flags(o, no_stage.float()), 'one 32-pixel K stage missing'


def _conv3x3(n=2, h=12, w=14, cs=64, cd=64, flags=0, mask=None, seed=5):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(n * h * w * cs, generator=g).bfloat16()
    wgt = (torch.randn(cd * 9 * cs, generator=g) * 0.1).bfloat16()
    dst = torch.zeros(n * h * w * cd, dtype=torch.bfloat16)
    ts = dict(src=src, wgt=wgt, dst=dst)
    if mask is not None:
        ts['mask'] = mask
    mem = mem_of(**ts)
    d = cdesc(n=n, gh=[h], gw=[w], sh=[h], sw=[w], dh=[h], dw=[w], cs=cs, cd=cd, cd_pad=cd, ldd=cd, ldm=cd, kh=3, kw=3, pad=1,
              flags=flags, src=src.data_ptr(), wgt=wgt.data_ptr(), dst=dst.data_ptr(), mask=mask.data_ptr() if mask is not None else 0)
    return mem, d, dst


def test_negative_controls_convolution():
    n, h, w, c = 2, 12, 14, 64
    mem, d, dst = _conv3x3(n, h, w)
    o = R.conv_ref(mem, d).outs[0]
    assert not _flags(o, o.ref)
    # tap (0, 0) missing on the border row (the last row: there the tap reads real data)
    bad = R.conv_ref(mem, d, drop=lambda s, t, g: (t == 0) & (g['y'] == h - 1)).outs[0].ref
    assert _flags(o, bad), 'border tap missing'
    bad = R.conv_ref(mem, d, drop=lambda s, t, g: g['img'] == 1).outs[0].ref
    assert _flags(o, bad), 'one image missing'
    # a one-pixel shift of the ReLU mask (MASK_FIRST: the data gradient through a ReLU)
    mask = torch.randn(n * h * w * c).bfloat16()
    mem, d, dst = _conv3x3(n, h, w, flags=R.CONV_MASK_FIRST, mask=mask)
    o = R.conv_ref(mem, d).outs[0]
    shifted = mask.view(n, h, w, c).roll(1, 2).reshape(-1).clone()
    mem2, d2, _ = _conv3x3(n, h, w, flags=R.CONV_MASK_FIRST, mask=shifted)
    assert _flags(o, R.conv_ref(mem2, d2).outs[0].ref), 'ReLU mask shifted by one pixel'


def test_negative_control_write_into_row_padding():
    n, h, w, cs, cd, ldd = 1, 5, 6, 64, 40, 48
    src = torch.randn(n * h * w * cs).bfloat16()
    wgt = torch.randn(64 * cs).bfloat16()
    dst = torch.zeros(n * h * w * ldd, dtype=torch.bfloat16)
    mem = mem_of(src=src, wgt=wgt, dst=dst)
    d = cdesc(n=n, gh=[h], gw=[w], sh=[h], sw=[w], dh=[h], dw=[w], cs=cs, cd=cd, cd_pad=64, ldd=ldd, kh=1, kw=1, src=src.data_ptr(),
              wgt=wgt.data_ptr(), dst=dst.data_ptr())
    lr = R.conv_ref(mem, d)
    R.run_checked(mem, lr, lambda: fill_conv_dst(lr, dst, lr.outs[0].ref))

    def stray():
        fill_conv_dst(lr, dst, lr.outs[0].ref)
        dst.view(-1, ldd)[3, cd] = 1.0           # one element past cd, in the padding of row 3

    with pytest.raises(AssertionError, match='outside the declared outputs'):
        R.run_checked(mem, R.conv_ref(mem, d), stray)


def test_negative_control_groupnorm_channel_with_foreign_statistics():
    n, segs, c, G, tot, x, gamma, beta, dy = _gn_case()
    y_t, st_t, *_ = _gn_torch(n, segs, c, G, x, gamma, beta, dy)
    y, stats = torch.zeros(tot * c, dtype=torch.bfloat16), st_t.float()
    mem = mem_of(x=x, y=y, gamma=gamma, beta=beta, stats=stats)
    o = R.gn_fwd_ref(mem, _gn_desc(n, segs, c, G, x, y, gamma, beta, stats)).outs[0]
    assert not _flags(o, y_t)
    # channel 8 (group 1) normalised with group 0's statistics
    bad = y_t.clone()
    off = 0
    for (h, w), xr in zip(segs, seg_rows(x, segs, n, c)):
        xs = xr.to(F64).view(n, h * w, c)
        g0 = xs[:, :, :8]
        m, r = g0.mean((1, 2)), (g0.var((1, 2), unbiased=False) + 1e-5).rsqrt()
        v = ((xs[:, :, 8] - m.view(-1, 1)) * r.view(-1, 1) * gamma[8].double() + beta[8].double()).relu()
        bad[off:off + n * h * w, 8] = v.reshape(-1)
        off += n * h * w
    assert _flags(o, bad), 'GN channel with another group statistics'


# ------------------------------------------------------------------------------------------------------------------------------
def test_resolver_reports_stray_pointers_and_overruns():
    a, b = torch.zeros(100), torch.zeros(64, dtype=torch.bfloat16)
    mem = mem_of(a=a, nested=dict(inner=[b]))
    assert mem.find(a.data_ptr() + 40, 360, 'x')[1] == 40
    assert 'nested' in mem.find(b.data_ptr(), 128, 'y')[0].name
    with pytest.raises(R.PointerError, match='conv.src: pointer .* lies in no known allocation'):
        mem.find(a.data_ptr() + 4096 * 1024, 4, 'conv.src')
    with pytest.raises(R.PointerError, match='wgrad.dw: extent 404 B .* runs past the end'):
        mem.typed(a.data_ptr(), torch.float32, 101, 'wgrad.dw')
    # a descriptor whose extent overruns its allocation is refused by the reference, naming the field
    mem2, d, dst = _conv3x3(1, 4, 4)
    d.ldd = 80
    with pytest.raises(R.PointerError, match=r'conv\.dst: extent'):
        R.conv_ref(mem2, d)
    d.ldd, d.src = 64, d.src + (1 << 30)
    with pytest.raises(R.PointerError, match=r'conv\.src: pointer'):
        R.conv_ref(mem2, d)


# ------------------------------------------------------------------------------------------------------------------------------
# DSL_OP_ASSIGN / DSL_OP_LOSS against the oracle (fp32 assignment, fp64 autograd of oracle.fcos_loss)
FCOS_SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
FCOS_RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8))


CTR_TOL = torch.tensor([1e-9] * 4 + [2.0 ** -20] + [1e-9] * 3, dtype=F64)


def fcos_case(B=3, C=80, ig=True, loss_weight=3.0, soft_weight=1.0, grad_scale=0.5, world=8, seed=0, empty=(), out_of_range=()):
    """A small FCOS batch whose box corners are exact in fp32 (quarter-pixel gt boxes, raw / 64 regressions, power-of-two scales):
    the kernel's fp32 corners equal the oracle's float64 ones, so the references can be held to float64 agreement.
    empty: images without gt; out_of_range: images whose only gt lies outside every regression range's reach."""
    import numpy as np
    from oracle import fcos_oracle as O
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    H, W = 128, 192
    gtb, gtl, igb = [], [], []
    for i in range(B):
        if i in empty:
            b = np.zeros((0, 4), 'float32')
        elif i in out_of_range:
            b = np.array([[60.0, 60.0, 61.0, 61.0]], 'float32')          # 1 x 1: inside no centre region of any level's points
        else:
            b = np.round(O.synth_boxes(rng, 5, H=H, W=W, lo=8, hi=150) * 4) / 4
        gtb.append(torch.from_numpy(b.astype('float32')))
        gtl.append(torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')))
        igb.append(torch.from_numpy((np.round(O.synth_boxes(rng, 2, H=H, W=W, lo=16, hi=100) * 4) / 4).astype('float32')))
    cls = [(torch.randn(B, C, h, w, generator=g, dtype=F64) - 2).float().double() for h, w in FCOS_SIZES]
    raw = [(torch.randint(-128, 640, (B, 4, h, w), generator=g) / 64.0).double() for h, w in FCOS_SIZES]
    ctr = [torch.randn(B, 1, h, w, generator=g, dtype=F64).float().double() for h, w in FCOS_SIZES]
    scales = torch.tensor([1.0, 0.5, 2.0, 1.0, 0.25], dtype=F64)
    return dict(B=B, C=C, gtb=gtb, gtl=gtl, igb=igb if ig else None, cls=cls, raw=raw, ctr=ctr, scales=scales, loss_weight=loss_weight,
                soft_weight=soft_weight, grad_scale=grad_scale, world=world)


def flat_lv(ts):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts])


def fcos_buffers(case, pad_nan=False):
    """The launch's buffers (CPU) and a dsl_fcos_desc namespace over them, as FcosLossPlan lays them out."""
    B, C = case['B'], case['C']
    M = B * sum(h * w for h, w in FCOS_SIZES)
    ld_cls, ld_gcls = (C + 3) // 4 * 4, (C + 63) // 64 * 64
    logits = torch.zeros(M, ld_cls)
    if pad_nan:
        logits[:, C:] = float('nan')
    logits[:, :C] = flat_lv(case['cls']).float()
    rc = torch.zeros(M, 8)
    rc[:, :4] = flat_lv(case['raw']).float()
    rc[:, 4] = flat_lv(case['ctr'])[:, 0].float()
    cat = lambda ts: torch.cat(ts) if ts else torch.zeros(0, 4)
    off = lambda ts: torch.tensor([0] + [int(sum(t.shape[0] for t in ts[:i + 1])) for i in range(len(ts))], dtype=torch.int32)
    b = dict(logits=logits, rc=rc, scales=case['scales'].float(), gt_boxes=cat(case['gtb']).reshape(-1, 4).contiguous() + 0,
             gt_labels=torch.cat(case['gtl']), gt_off=off(case['gtb']),
             labels=torch.full((M,), -7, dtype=torch.int64), bbox_targets=torch.full((M, 4), -7.0), assign_idx=torch.full((M,), -7, dtype=torch.int32),
             cls_weight=torch.full((M,), -7.0), pos_weight=torch.full((M,), -7.0), stats=torch.full((8,), -7.0), norm=torch.zeros(2),
             g_cls=torch.full((M, ld_gcls), 3.0, dtype=torch.bfloat16), g_rc=torch.full((M, 64), 3.0, dtype=torch.bfloat16),
             g_scales=torch.full((8,), 3.0), losses=torch.full((4,), 3.0), logvec=torch.full((5,), 3.0), ws=torch.zeros(4096))
    if case['igb'] is not None:
        b['ig_boxes'], b['ig_off'] = cat(case['igb']).reshape(-1, 4).contiguous() + 0, off(case['igb'])
    if b['gt_boxes'].numel() == 0:
        b['gt_boxes'], b['gt_labels'] = torch.zeros(1, 4), torch.zeros(1, dtype=torch.int64)
    p = lambda k: b[k].data_ptr() if k in b else 0
    d = types.SimpleNamespace(nlvl=5, n=B, h=[h for h, _ in FCOS_SIZES], w=[w for _, w in FCOS_SIZES], stride=[8, 16, 32, 64, 128],
                              range_lo=[r[0] for r in FCOS_RANGES], range_hi=[r[1] for r in FCOS_RANGES], radius=1.5, num_classes=C,
                              gt_boxes=p('gt_boxes'), gt_labels=p('gt_labels'), gt_off=p('gt_off'), ig_boxes=p('ig_boxes'), ig_off=p('ig_off'),
                              labels=p('labels'), bbox_targets=p('bbox_targets'), assign_idx=p('assign_idx'), cls_weight=p('cls_weight'),
                              pos_weight=p('pos_weight'), stats=p('stats'), loss_weight=case['loss_weight'], cls_logits=p('logits'),
                              regctr=p('rc'), ld_cls=ld_cls, ld_rc=8, scales=p('scales'), norm=p('norm'), g_cls=p('g_cls'), ld_gcls=ld_gcls,
                              g_rc=p('g_rc'), ld_grc=64, g_scales=p('g_scales'), losses=p('losses'), soft_weight=case['soft_weight'],
                              grad_scale=case['grad_scale'], inv_world=1.0 / case['world'], workspace=p('ws'), workspace_bytes=4 * 4096,
                              logvec=p('logvec'))
    return b, d, R.Memory({'b': b})


def fill_outs(outs):
    """Writes each Out's reference, rounded to its dtype, into its buffer (a correctly rounding launch)."""
    def go(mem):
        for o in outs:
            n = int(o.idx.max()) + 1
            v = o.ref.to(torch.float32).to(o.dtype) if o.dtype in (torch.bfloat16, torch.float32) else o.ref.to(o.dtype)
            mem.typed(o.ptr, o.dtype, n, o.name).view(-1)[o.idx.reshape(-1)] = v.reshape(-1)
    return go


def oracle_loss(case):
    """fp64 autograd of oracle.fcos_loss through Scale + ReLU; num_pos / denorm go through fp32 as the norm buffer holds them."""
    from oracle import fcos_oracle as O
    cls = [c.clone().requires_grad_() for c in case['cls']]
    raw = [r.clone().requires_grad_() for r in case['raw']]
    ctr = [c.clone().requires_grad_() for c in case['ctr']]
    sc = case['scales'].clone().requires_grad_()
    reg = [torch.relu(r * sc[i]) for i, r in enumerate(raw)]
    out, aux = O.fcos_loss(cls, reg, ctr, case['gtb'], case['gtl'], case['igb'], loss_weight=case['loss_weight'],
                           soft_weight=case['soft_weight'], num_classes=case['C'], world_mean=lambda t: t.float().double(), return_aux=True)
    (sum(out.values()) * case['grad_scale']).backward()
    return out, aux, cls, raw, ctr, sc


def run_fcos_refs(case, norm=None, **kw):
    """norm: the (num_pos, centerness sum) one rank contributes (default: the assignment's stats); norm[] holds `world` times it."""
    b, d, mem = fcos_buffers(case, **kw)
    la = R.assign_ref(mem, d)
    res = R.run_checked(mem, la, lambda: fill_outs(la.outs)(mem))
    b['norm'][:] = (b['stats'][:2] if norm is None else torch.tensor(norm, dtype=torch.float32)) * case['world']
    ll = R.loss_ref(mem, d)

    def launch():
        fill_outs(ll.outs)(mem)
        lo, n = b['losses'], 4 if case['soft_weight'] else 3
        b['logvec'][:n] = lo[:n]
        b['logvec'][n] = ((lo[0] + lo[1]) + lo[2]) + (lo[3] if n == 4 else 0.0)
    res += R.run_checked(mem, ll, launch)
    return b, d, mem, la, ll, res


def _close(o, ref, tol=1e-9):
    """o.ref == ref to float64 rounding (tol may be a tensor broadcast over o.ref: the oracle's centerness BCE takes the dtype of
    its fp32 target and runs in fp32)."""
    bound = tol * (o.S.abs() + o.ref.abs()) + 1e-300
    ratio, nbad, worst = R.compare(o.ref, ref.to(F64).reshape(o.ref.shape), bound)
    assert nbad == 0, (o.name, ratio, worst, float(o.ref.reshape(-1)[worst]), float(ref.reshape(-1)[worst]))


@pytest.mark.parametrize('C,ig,lw,soft,gs,world', [(80, True, 3.0, 1.0, 0.5, 8), (3, False, 1.0, 1.0, 1.0, 1), (1, True, 2.0, 0.0, 2.0, 8)])
def test_assign_and_loss_refs_match_oracle_autograd(C, ig, lw, soft, gs, world):
    case = fcos_case(C=C, ig=ig, loss_weight=lw, soft_weight=soft, grad_scale=gs, world=world, empty=(1,) if C == 3 else ())
    out, aux, cls, raw, ctr, sc = oracle_loss(case)
    # (the oracle's centerness sum is an fp32 torch sum: the loss reads the norm[] it is given, whatever order made it)
    b, d, mem, la, ll, res = run_fcos_refs(case, norm=[aux['num_pos'], aux['ctr_denorm']], pad_nan=C % 4 != 0)
    assert all(r[2] == 0 for r in res), res
    assert float(b['stats'][1]) == pytest.approx(float(aux['ctr_targets'].double().sum()), rel=2 ** -20)
    o = {x.name.split('.')[-1]: x for x in la.outs + ll.outs}
    # assignment: bit for bit at every location (background rows: gt 0's ltrb / stride, zeros for an image without gt)
    assert torch.equal(b['labels'], aux['labels'])
    assert torch.equal(b['assign_idx'].long(), aux['assign_idx'])
    assert torch.equal(b['bbox_targets'], aux['bbox_targets'])
    assert torch.equal(b['cls_weight'], aux['cls_weight'].float())
    assert float(b['stats'][0]) == len(aux['pos_inds']) > 0 and not b['stats'][2:].any()
    if ig:
        assert bool((b['cls_weight'] == 0).any())
    # the stream weight: loss_weight on images >= n / 2 (the unlabeled stream), 1 elsewhere
    img = R._fcos_locations(d)[1]
    want_pw = torch.where(img >= case['B'] // 2, torch.tensor(lw), torch.tensor(1.0))
    assert torch.equal(b['pos_weight'], want_pw)
    ig_zero = torch.zeros_like(b['cls_weight'], dtype=torch.bool) if aux['cls_weight'] is None else aux['cls_weight'] == 0
    assert torch.equal(b['cls_weight'], torch.where(ig_zero, torch.tensor(0.0), want_pw))
    # loss: float64 agreement with autograd
    _close(o['g_cls'], torch.cat([flat_lv([c.grad for c in cls]), torch.zeros(b['g_cls'].shape[0], b['g_cls'].shape[1] - C, dtype=F64)], 1))
    g_rc = torch.zeros(b['g_rc'].shape[0], 8, dtype=F64)
    g_rc[:, :4], g_rc[:, 4] = flat_lv([r.grad for r in raw]), flat_lv([c.grad for c in ctr])[:, 0]
    _close(o['g_rc'], g_rc, CTR_TOL)
    _close(o['g_scales'], sc.grad)
    want = [out['loss_cls'], out['loss_bbox'], out['loss_centerness'], out.get('loss_sisoft', torch.zeros((), dtype=F64))]
    _close(o['losses'], torch.stack([w.detach().double().reshape(()) for w in want]), torch.tensor([1e-9, 1e-9, 2.0 ** -20, 1e-9]))
    assert ('loss_sisoft' in out) == (soft != 0.0)
    # logvec: the fp32 recombination of the written losses
    lv = b['logvec']
    n = 4 if soft else 3
    assert torch.equal(lv[:n], b['losses'][:n]) and float(lv[n]) == float(((b['losses'][0] + b['losses'][1]) + b['losses'][2]) +
                                                                        (b['losses'][3] if soft else 0.0))


def test_loss_ref_edges_ties_zero_relu_no_gt():
    """predicted box == target (GIoU max / min ties split 0.5 / 0.5, as torch), raw x scale == 0 exactly (ReLU passes nothing), an
    image without gt and one whose gt is out of every range."""
    case = fcos_case(B=4, C=3, soft_weight=0.0, empty=(2,), out_of_range=(3,))
    b, d, mem = fcos_buffers(case)
    la = R.assign_ref(mem, d)
    fill_outs(la.outs)(mem)
    pos = (b['labels'] < 3).nonzero().view(-1)
    assert pos.numel() > 4 and not bool((b['labels'][pos] < 0).any())
    lvl = R._fcos_locations(d)[0]
    # ties: the first positives regress exactly their targets; the next ones have raw == 0 in one coordinate
    sc = case['scales'][lvl[pos[:4]]].view(-1, 1)
    exact = (b['bbox_targets'][pos[:4]].double() / sc)
    for j, r_ in enumerate(exact):
        m = int(pos[j])
        b['rc'][m, :4] = r_.float()
    b['rc'][pos[4:8], 1] = 0.0
    # mirror into the case tensors for the oracle
    M = b['rc'].shape[0]
    o_ = 0
    for l, (h, w) in enumerate(FCOS_SIZES):
        n_ = case['B'] * h * w
        case['raw'][l] = b['rc'][o_:o_ + n_, :4].double().view(case['B'], h, w, 4).permute(0, 3, 1, 2).contiguous()
        o_ += n_
    assert o_ == M
    assert torch.equal((b['rc'][pos[:4], :4] * b['scales'][lvl[pos[:4]]].view(-1, 1)), b['bbox_targets'][pos[:4]])
    out, aux, cls, raw, ctr, scg = oracle_loss(case)
    b['norm'][:] = torch.tensor([aux['num_pos'], aux['ctr_denorm']], dtype=torch.float32) * case['world']
    ll = R.loss_ref(mem, d)
    g_rc = torch.zeros(M, 8, dtype=F64)
    g_rc[:, :4], g_rc[:, 4] = flat_lv([r.grad for r in raw]), flat_lv([c.grad for c in ctr])[:, 0]
    _close(ll.outs[1], g_rc, CTR_TOL)
    _close(ll.outs[2], scg.grad)
    assert not bool(ll.outs[1].ref[pos[4:8], 1].any())
    # images 2 (no gt) and 3 (gt out of range): background everywhere, zero box gradient
    assert not bool(((R._fcos_locations(d)[1] >= 2) & (b['labels'] < 3)).any())


def test_negative_controls_assign_loss():
    case = fcos_case(C=80)
    b, d, mem, la, ll, res = run_fcos_refs(case)
    got = lambda o: o.got(mem)
    # ASSIGN with radius 1.0
    bad = R.assign_ref(mem, d, radius=1.0)
    assert R.compare(got(la.outs[0]), bad.outs[0].ref, la.outs[0].bound())[1] > 0
    # LOSS: sisoft partner from level lvl instead of lvl - 1
    bad = R.loss_ref(mem, d, partner_level=0)
    assert R.compare(got(ll.outs[0]), bad.outs[0].ref, ll.outs[0].bound())[1] > 0
    # LOSS: ReLU mask dropped from g_rc
    bad = R.loss_ref(mem, d, relu_mask=False)
    assert R.compare(got(ll.outs[1]), bad.outs[1].ref, ll.outs[1].bound())[1] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# fp8 quantisers against torch's e4m3 cast
def test_fp8_refs_match_torch_cast():
    rows, c, ld = 300, 48, 64
    x = (torch.randn(rows, ld) * 3).bfloat16()
    x[5, 7] = 200.0                                       # saturates at scale 4
    y = torch.zeros(rows * c, dtype=torch.uint8)
    part = torch.full((7,), -1.0)
    scale = torch.tensor([4.0])
    mem = mem_of(x=x, y=y, part=part, scale=scale)
    lr = R.quant_fp8_delayed_ref(mem, x.data_ptr(), y.data_ptr(), part.data_ptr(), scale.data_ptr(), rows, c, ld, 7)
    want = (x[:, :c].float() * 4.0).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(lr.outs[0].ref.to(torch.uint8).view(rows, c), want.view(torch.uint8))
    assert int(lr.outs[0].ref.view(rows, c)[5, 7]) == 0x7e                # +448
    chunks = x[:, :c].float().abs().reshape(-1, 16).amax(1)
    pm = torch.tensor([chunks[[j for j in range(chunks.numel()) if (j // 256) % 7 == b]].max() if b < (chunks.numel() + 255) // 256 else 0.0
                       for b in range(7)])
    assert torch.equal(lr.outs[1].ref.float(), pm) and float(pm.max()) == float(x[:, :c].float().abs().max())
    # scale doubled: flagged
    bad = R.quant_fp8_delayed_ref(mem, x.data_ptr(), y.data_ptr(), part.data_ptr(), scale.data_ptr(), rows, c, ld, 7, scale_mul=2.0)
    R.run_checked(mem, lr, lambda: fill_outs(lr.outs)(mem))
    assert R.compare(lr.outs[0].got(mem), bad.outs[0].ref, lr.outs[0].bound())[1] > 0
    # fixed-scale and dynamic quantisers
    s_bits = int(torch.tensor([0.75]).view(torch.int32)[0])
    lr = R.quant_fp8_ref(mem, x.data_ptr(), y.data_ptr(), rows, c, ld, s_bits)
    assert torch.equal(lr.outs[0].ref.to(torch.uint8).view(rows, c), (x[:, :c].float() * 0.75).to(torch.float8_e4m3fn).view(torch.uint8))
    lr = R.quant_fp8_ref(mem, x.data_ptr(), y.data_ptr(), rows, c, ld, 0, part.data_ptr(), 7)
    s = (448.0 / x[:, :c].double().abs().max()).float()             # correctly rounded quotient (the kernel's IEEE divide)
    assert torch.equal(lr.outs[0].ref.to(torch.uint8).view(rows, c), (x[:, :c].float() * s).to(torch.float8_e4m3fn).view(torch.uint8))


def test_fp8_weight_refs_prep_and_cold_scale():
    cout, cout_pad, k = 5, 8, 36
    w = torch.randn(cout, k)
    w[3] = 0.0                                                  # a zero row: s = 1
    w8 = torch.full((cout_pad * k,), 9, dtype=torch.uint8)
    comb = torch.full((cout_pad,), 9.0)
    bn = torch.rand(cout) + 0.5
    amax_rec = torch.tensor([0.5, 3.0, 2.0])
    amax_cold = torch.zeros(3)
    scale = torch.full((2,), -1.0)
    comb2, w82 = torch.full((cout_pad,), 9.0), torch.full((cout_pad * k,), 9, dtype=torch.uint8)
    items = (R.Fp8PrepItem * 2)()
    for j, (am, cb, q) in enumerate(((amax_rec, comb, w8), (amax_cold, comb2, w82))):
        items[j].w, items[j].w8, items[j].comb, items[j].amax = w.data_ptr(), q.data_ptr(), cb.data_ptr(), am.data_ptr()
        items[j].scale, items[j].n_amax, items[j].cout = scale.data_ptr() + 4 * j, 3, cout
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
    mem = mem_of(w=w, w8=w8, comb=comb, bn=bn, a=amax_rec, z=amax_cold, scale=scale, c2=comb2, w82=w82, table=table)
    mbits = int(torch.tensor([1.25]).view(torch.int32)[0])
    lr = R.fp8_prep_ref(mem, table.data_ptr(), 2, cout_pad, k, mbits)
    o = {x.name: x for x in lr.outs}
    a = torch.tensor(3.0) * 1.25
    sw = (448.0 / w.double().abs().amax(1)).float()                  # correctly rounded quotients (the kernel's IEEE divide)
    sw[3] = 1.0
    assert float(o['fp8_prep[0].scale'].ref[0]) == float((448.0 / a.double()).float())
    assert float(o['fp8_prep[1].scale'].ref[0]) == 1.0 and lr.extra['cold'] == 1          # nothing recorded yet
    assert torch.equal(o['fp8_prep[0].comb'].ref[:cout].float(), (a / 448.0) / sw) and not o['fp8_prep[0].comb'].ref[cout:].any()
    assert torch.equal(o['fp8_prep[1].comb'].ref[:cout].float(), 1.0 / sw)
    q = o['fp8_prep[0].w8'].ref.to(torch.uint8)
    assert torch.equal(q[:cout], (w * sw.view(-1, 1)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    assert not q[cout:].any() and not q[3].any()
    lr = R.quant_fp8_w_ref(mem, w.data_ptr(), w8.data_ptr(), comb.data_ptr(), bn.data_ptr(), cout, cout_pad, k,
                           int(torch.tensor([0.5]).view(torch.int32)[0]))
    assert torch.equal(lr.outs[1].ref[:cout].float(), 0.5 / sw * bn)
    assert lr.outs[0].exact and lr.outs[1].exact
    lr = R.fp8_comb_ref(mem, bn.data_ptr(), comb.data_ptr(), cout, amax_rec.data_ptr(), 3)
    assert torch.equal(lr.outs[0].ref.float(), bn * (torch.tensor(3.0) / 448.0))
    lr = R.fp8_comb_ref(mem, bn.data_ptr(), comb.data_ptr(), cout, amax_cold.data_ptr(), 3)
    assert torch.equal(lr.outs[0].ref.float(), bn)

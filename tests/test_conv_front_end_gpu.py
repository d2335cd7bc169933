"""The front end of conv_pipe_kernel / conv_f8_kernel / conv_splitk_epilogue_kernel: the tile decode and
the first weight tile are addressed from scalar kernel parameters in front of the parameter struct, and tile kt0's weight DMA is
issued before the pixel decode.  Each case is the smallest shape at which that prologue can be wrong, run for every tile
configuration the `force` test hook (dsl_conv_desc.flags bits 8-11; bits 12-15 force a split-K factor) can put on it, against fp32
torch-CPU references on bf16-representable inputs with the tolerances tests/test_kernels_gpu.py uses for the same comparisons."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import _multiseg, bf, from_nhwc, nhwc, pack_w, pack_w_dgrad, rnd, sync

pytestmark = pytest.mark.gpu

BCO = {1: 256, 2: 256, 3: 128, 4: 128, 5: 64, 6: 128, 7: 64, 8: 64}        # cout tile of forced configuration 1..8 (kConvTiles, conv.hip)


def forces(cd_pad):
    """0 = the planner's own choice, then every tile configuration whose cout tile divides cd_pad."""
    return [0] + [f for f, b in BCO.items() if cd_pad % b == 0]


@pytest.fixture(scope='module')
def K():
    from dsl_amd import _lib as L
    from dsl_amd import ops
    assert torch.cuda.is_available()
    return L, ops


def close_fwd(got, ref):          # test_conv_forward's two assertions (bf16 output, split-K launches included)
    assert torch.allclose(got, ref, rtol=1e-2, atol=1e-2), (got - ref).abs().max()
    assert (got - bf(ref)).abs().max() <= 2 ** -7 * ref.abs().max()


def close_dgrad(got, ref):        # test_conv_dgrad_transposed's assertion
    assert torch.allclose(got, ref, rtol=1e-2, atol=2e-2), (got - ref).abs().max()


def workspace():
    return torch.empty(8 << 20, dtype=torch.uint8, device='cuda')


# ---- split-K with kt0 > 0: the first weight tile of split bz, w_soff of a non-zero kt0 ------------------------------------------
@pytest.fixture(scope='module')
def splitk_1x1():
    g = torch.Generator().manual_seed(101)
    N, Ci, Co, H, W = 2, 512, 128, 6, 7
    x, w = rnd(N, Ci, H, W, g=g), rnd(Co, Ci, 1, 1, g=g, scale=1 / math.sqrt(Ci))
    return x, w, F.conv2d(x, w)


@pytest.mark.parametrize('force', forces(128))
@pytest.mark.parametrize('splits', [2, 4])
def test_split_k_1x1_first_weight_tile_of_every_split(K, splitk_1x1, splits, force):
    L, ops = K
    x, w, ref = splitk_1x1
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    outs = []
    for sp in (1, splits):                       # 1: no workspace, so the same launch runs unsplit
        y = torch.empty(N, H, W, Co, dtype=torch.bfloat16, device='cuda')
        ops.conv2d(nhwc(x), pack_w(w, Co), y, n=N, grid=[(H, W)], src_hw=[(H, W)], dst_hw=[(H, W)], cs=Ci, cd=Co, cd_pad=Co, ldd=Co,
                   kh=1, kw=1, flags=(force << 8) | ((sp << 12) if sp > 1 else 0), workspace=workspace() if sp > 1 else None)
        sync()
        outs.append(from_nhwc(y))
        close_fwd(outs[-1], ref)
    # the split sum is the same fp32 products in another order: at most one bf16 rounding step at the largest magnitude apart
    assert (outs[0] - outs[1]).abs().max() <= 2 ** -7 * ref.abs().max()


# ---- 3x3 split-K: tap_r, tap_s, cidx at entry (3 splits of 18 K tiles start on a tap, 4 splits of 5 tiles start mid-tap) ---------
@pytest.fixture(scope='module')
def splitk_3x3():
    g = torch.Generator().manual_seed(102)
    N, Cc, H, W = 2, 128, 9, 11
    x = rnd(N, Cc, H, W, g=g).requires_grad_()
    w = rnd(Cc, Cc, 3, 3, g=g, scale=1 / math.sqrt(Cc * 9))
    yref = F.conv2d(x, w, None, 1, 1)
    dy = rnd(N, Cc, H, W, g=g)
    yref.backward(dy)
    return x.detach(), w, yref.detach(), dy, x.grad.clone()


@pytest.mark.parametrize('force', forces(128))
@pytest.mark.parametrize('splits', [3, 4])
@pytest.mark.parametrize('mode', [0, 1])
def test_split_k_3x3_tap_state_at_entry(K, splitk_3x3, mode, splits, force):
    L, ops = K
    x, w, yref, dy, dxref = splitk_3x3
    N, Cc, H, W = x.shape
    out = torch.empty(N, H, W, Cc, dtype=torch.bfloat16, device='cuda')
    src, wp, ref = (nhwc(x), pack_w(w, Cc), yref) if mode == 0 else (nhwc(dy), pack_w_dgrad(w, Cc), dxref)
    ops.conv2d(src, wp, out, n=N, grid=[(H, W)], src_hw=[(H, W)], dst_hw=[(H, W)], cs=Cc, cd=Cc, cd_pad=Cc, ldd=Cc, kh=3, kw=3,
               stride=1, pad=1, mode=mode, flags=(force << 8) | (splits << 12), workspace=workspace())
    sync()
    (close_fwd if mode == 0 else close_dgrad)(from_nhwc(out), ref)


# ---- five level segments, ragged last pixel tile: 258 pixels, tiles straddle segments and images --------------------------------
SIZES5 = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]


@pytest.fixture(scope='module')
def five_levels():
    g = torch.Generator().manual_seed(103)
    N, Ci, Co = 2, 64, 256
    xs = [rnd(N, Ci, h, w, g=g) for h, w in SIZES5]
    w = rnd(Co, Ci, 3, 3, g=g, scale=1 / math.sqrt(Ci * 9))
    b = torch.randn(Co, generator=g)
    ref = torch.cat([F.conv2d(x, w, b, 1, 1).permute(0, 2, 3, 1).reshape(-1, Co) for x in xs])
    # mode 1: the data gradient of a 256 -> 64 convolution is a 64 -> 256 launch
    wt = rnd(Ci, Co, 3, 3, g=g, scale=1 / math.sqrt(Ci * 9))          # OIHW of that forward convolution
    dref = torch.cat([F.conv_transpose2d(x, wt, None, 1, 1).permute(0, 2, 3, 1).reshape(-1, Co) for x in xs])
    return xs, w, b, ref, wt, dref


@pytest.mark.parametrize('force', forces(256))
@pytest.mark.parametrize('records', [False, True])
def test_five_segments_ragged_tile_with_and_without_groupnorm_records(K, five_levels, records, force):
    L, ops = K
    xs, w, b, ref, _, _ = five_levels
    N, Co = 2, 256
    P = ref.shape[0]
    y = torch.empty(P, Co, dtype=torch.bfloat16, device='cuda')
    cd = ops.conv_desc(_multiseg(xs), pack_w(w, Co), y, n=N, grid=SIZES5, src_hw=SIZES5, dst_hw=SIZES5, cs=64, cd=Co, cd_pad=Co, ldd=Co,
                       kh=3, kw=3, stride=1, pad=1, flags=force << 8, bias=b.cuda())
    if records:
        ga, be = torch.ones(Co, device='cuda'), torch.zeros(Co, device='cuda')
        yn = torch.empty_like(y)
        stats = torch.empty(5 * N * 32, 2, device='cuda')
        gd = ops.gn_desc(y, yn, ga, be, stats, n=N, hw=SIZES5)
        assert L.lib.dsl_conv2d_gn_fusable(C.byref(cd)) == 1
        cd.gn_ws = gd.workspace
        gd.conv_stats = 1
        gd._keep[5].fill_(0xff)                  # an unwritten record would read NaN
    L.check(L.lib.dsl_conv2d(C.byref(cd), L.stream_ptr()), 'dsl_conv2d')
    sync()
    got = y.float().cpu()
    close_fwd(got, ref)
    if records:                                  # the records give the statistics of the two-pass GroupNorm on the same output
        L.check(L.lib.dsl_groupnorm_relu_fwd(C.byref(gd), L.stream_ptr()), 'gn')
        stats2 = torch.empty_like(stats)
        gd2 = ops.gn_desc(y, torch.empty_like(y), ga, be, stats2, n=N, hw=SIZES5)
        L.check(L.lib.dsl_groupnorm_relu_fwd(C.byref(gd2), L.stream_ptr()), 'gn')
        sync()
        assert torch.allclose(stats, stats2, rtol=2e-5, atol=2e-6), (stats - stats2).abs().max()     # (test_groupnorm_statistics_...)


@pytest.mark.parametrize('force', [0, 1, 2])     # the backward records are instantiated for the two 256-cout tiles
def test_five_segments_ragged_tile_backward_records_instantiation(K, five_levels, force):
    L, ops = K
    xs, _, _, _, wt, dref = five_levels
    N, Cc = 2, 256
    P = dref.shape[0]
    g = torch.Generator().manual_seed(104)
    xin = _multiseg([rnd(N, Cc, h, w, g=g, scale=2.0) for h, w in SIZES5])      # the norm's input of the forward pass
    ga, be = (1 + 0.2 * torch.randn(Cc, generator=g)).cuda(), (0.3 * torch.randn(Cc, generator=g)).cuda()
    yn = torch.empty(P, Cc, dtype=torch.bfloat16, device='cuda')
    stats = torch.empty(5 * N * 32, 2, device='cuda')
    L.check(L.lib.dsl_groupnorm_relu_fwd(C.byref(ops.gn_desc(xin, yn, ga, be, stats, n=N, hw=SIZES5)), L.stream_ptr()))
    wp = pack_w_dgrad(wt, 64)
    outs = []
    for fused in (0, 1):
        dy = torch.zeros(P, Cc, dtype=torch.bfloat16, device='cuda')
        dx = torch.empty_like(dy)
        dgam, dbet, dbias = (torch.full((Cc,), float('nan'), device='cuda') for _ in range(3))
        gd = ops.gn_desc(xin, yn, ga, be, stats, n=N, hw=SIZES5, dy=dy, dx=dx, dgamma=dgam, dbeta=dbet, dbias=dbias)
        cd = ops.conv_desc(_multiseg(xs), wp, dy, n=N, grid=SIZES5, src_hw=SIZES5, dst_hw=SIZES5, cs=64, cd=Cc, cd_pad=Cc, ldd=Cc,
                           kh=3, kw=3, stride=1, pad=1, mode=1, flags=force << 8)
        if fused:
            cd.gn_x = L.ptr(xin)
            assert L.lib.dsl_conv2d_gn_fusable(C.byref(cd)) == 1
            cd.gn_ws, cd.gn_gamma, cd.gn_beta, cd.gn_stats = gd.workspace, L.ptr(ga), L.ptr(be), L.ptr(stats)
            gd.conv_stats = 1
            gd._keep[5].fill_(0xff)
        L.check(L.lib.dsl_conv2d(C.byref(cd), L.stream_ptr()), 'dsl_conv2d')
        L.check(L.lib.dsl_groupnorm_relu_bwd(C.byref(gd), L.stream_ptr()), 'gn bwd')
        sync()
        outs.append([t.clone() for t in (dy, dx, dgam, dbet, dbias)])
    a, b_ = outs
    close_dgrad(a[0].float().cpu(), dref)
    assert torch.equal(a[0], b_[0])              # the data gradient itself does not change with the records
    # (test_groupnorm_backward_records_from_the_data_gradient_epilogue's bounds)
    assert float((a[1].float() - b_[1].float()).abs().max()) <= 2 ** -7 * float(a[1].float().abs().max())
    for u, v in zip(a[2:], b_[2:]):
        assert torch.allclose(u, v, rtol=1e-4, atol=1e-4 * float(u.abs().max())), (u - v).abs().max()


# ---- cout not filling the last cout tile: 80 channels stored as 128 (conv_cls), weight rows beyond cout --------------------------
@pytest.fixture(scope='module')
def cout80():
    g = torch.Generator().manual_seed(105)
    N, Ci, Co, H, W = 2, 256, 80, 7, 9
    x, w, b = rnd(N, Ci, H, W, g=g), rnd(Co, Ci, 3, 3, g=g, scale=0.02), torch.randn(Co, generator=g)
    return x, w, b, F.conv2d(x, w, b, 1, 1)


@pytest.mark.parametrize('force', forces(128))
def test_cout_80_stored_as_128(K, cout80, force):
    L, ops = K
    x, w, b, ref = cout80
    N, Ci, H, W = x.shape
    y = torch.full((N, H, W, 80), -7.0, dtype=torch.float32, device='cuda')
    ops.conv2d(nhwc(x), pack_w(w, 128), y, n=N, grid=[(H, W)], src_hw=[(H, W)], dst_hw=[(H, W)], cs=Ci, cd=80, cd_pad=128, ldd=80,
               kh=3, kw=3, stride=1, pad=1, flags=L.CONV_OUT_F32 | (force << 8), bias=b.cuda())
    sync()
    got = from_nhwc(y)
    assert torch.allclose(got, ref, rtol=2e-3, atol=2e-3), (got - ref).abs().max()       # (test_conv_multilevel_fp32_out_ragged_channels)


# ---- lds > cs: the source is a channel slice of wider rows ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def wide_rows():
    g = torch.Generator().manual_seed(106)
    N, Cw, Ci, Co, H, W = 2, 192, 128, 64, 7, 9
    xw, w = rnd(N, Cw, H, W, g=g), rnd(Co, Ci, 3, 3, g=g, scale=1 / math.sqrt(Ci * 9))
    return xw, w, F.conv2d(xw[:, 64:], w, None, 1, 1)


@pytest.mark.parametrize('force', forces(64))
def test_source_is_a_channel_slice_of_wider_rows(K, wide_rows, force):
    L, ops = K
    xw, w, ref = wide_rows
    N, Cw, H, W = xw.shape
    rows = nhwc(xw)
    y = torch.empty(N, H, W, 64, dtype=torch.bfloat16, device='cuda')
    ops.conv2d(rows.view(-1, Cw)[:, 64:], pack_w(w, 64), y, n=N, grid=[(H, W)], src_hw=[(H, W)], dst_hw=[(H, W)], cs=128, cd=64,
               cd_pad=64, ldd=64, kh=3, kw=3, stride=1, pad=1, flags=force << 8, lds=Cw)
    sync()
    close_fwd(from_nhwc(y), ref)


# ---- the stem instantiation (8-channel source) ----------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [0, 5])        # instantiated for the 64 x 256 tile
def test_stem_instantiation(K, force):
    L, ops = K
    g = torch.Generator().manual_seed(107)
    N, H, W = 2, 32, 40
    x, w = rnd(N, 3, H, W, g=g), rnd(64, 3, 7, 7, g=g, scale=0.1)
    ref = F.relu(F.conv2d(x, w, None, 2, 3))
    Ho, Wo = ref.shape[2:]
    x8 = torch.empty(N, H, W, 8, dtype=torch.bfloat16, device='cuda')
    x_d = x.cuda()
    L.check(L.lib.dsl_pack_image(L.ptr(x_d), L.ptr(x8), N, H, W, L.stream_ptr()))
    wp = torch.zeros(64, 7 * 64)                 # K = 49 taps * 8 channels = 392, padded to 448
    wp[:, :392] = torch.cat([w.permute(0, 2, 3, 1), torch.zeros(64, 7, 7, 5)], -1).reshape(64, 392)
    y = torch.empty(N, Ho, Wo, 64, dtype=torch.bfloat16, device='cuda')
    ops.conv2d(x8, wp.bfloat16().cuda(), y, n=N, grid=[(Ho, Wo)], src_hw=[(H, W)], dst_hw=[(Ho, Wo)], cs=8, cd=64, cd_pad=64, ldd=64,
               kh=7, kw=7, stride=2, pad=3, flags=L.CONV_RELU_OUT | L.CONV_SMALL_C | (force << 8))
    sync()
    assert torch.allclose(from_nhwc(y), ref, rtol=1e-2, atol=1e-2)                      # (test_conv_stem_small_c)


# ---- conv_f8_kernel (part of every build of the library, as in tests/test_fp8_gpu.py: nothing to skip) ---------------------------
@pytest.mark.parametrize('force', [0, 1, 2, 4])  # instantiated for 256 x 192, 256 x 128, 128 x 128
def test_fp8_kernel(K, force):
    L, ops = K
    F8 = torch.float8_e4m3fn
    n, ci, co, k, lv = 2, 256, 256, 3, [(6, 8)]
    g = torch.Generator().manual_seed(108)
    P = sum(h * w for h, w in lv) * n
    x = torch.relu(torch.randn(P, ci, generator=g)).bfloat16()
    w = torch.randn(co, k, k, ci, generator=g) * 0.05
    sx = 16.0
    xd, wd = x.cuda(), w.reshape(co, -1).contiguous().cuda()
    x8 = torch.zeros(P, ci, dtype=torch.uint8, device='cuda')
    w8 = torch.zeros(co, k * k * ci, dtype=torch.uint8, device='cuda')
    comb = torch.zeros(co, device='cuda')
    bias = torch.randn(co, generator=g).cuda()
    L.check(L.lib.dsl_quant_fp8(L.ptr(xd), L.ptr(x8), P, ci, ci, sx, L.stream_ptr()))
    L.check(L.lib.dsl_quant_fp8_weights(L.ptr(wd), L.ptr(w8), L.ptr(comb), None, co, co, k * k * ci, 1.0 / sx, L.stream_ptr()))
    y = torch.zeros(P, co, device='cuda')
    d = ops.conv_desc(x8, w8, y, n=n, grid=lv, src_hw=lv, dst_hw=lv, cs=ci, cd=co, cd_pad=co, ldd=co, kh=k, kw=k, stride=1, pad=1,
                      flags=L.CONV_FP8 | L.CONV_OUT_F32 | (force << 8), scale=comb, bias=bias)
    L.check(L.lib.dsl_conv2d(C.byref(d), L.stream_ptr()), 'dsl_conv2d fp8')
    sync()
    xq = x8.cpu().view(F8).float().reshape(n, 6, 8, ci).permute(0, 3, 1, 2)
    wq = w8.cpu().view(F8).float().reshape(co, k, k, ci).permute(0, 3, 1, 2)
    r = F.conv2d(xq.double(), wq.double(), None, 1, 1).permute(0, 2, 3, 1).reshape(-1, co)
    ref = (r * comb.cpu().double() + bias.cpu().double()).float()
    got = y.cpu()
    assert torch.allclose(got, ref, rtol=2e-5, atol=2e-5 * float(ref.abs().max())), float((got - ref).abs().max())   # (test_conv_fp8_vs_torch_...)


# ---- run-to-run bits: a first-tile wait that is one piece short reads a stale or half-filled ring slot ---------------------------
@pytest.mark.parametrize('force', forces(128))
def test_two_runs_into_a_nan_filled_buffer_give_the_same_bits(K, splitk_3x3, force):
    L, ops = K
    x, w, yref, _, _ = splitk_3x3
    N, Cc, H, W = x.shape
    y = torch.empty(N, H, W, Cc, dtype=torch.bfloat16, device='cuda')
    d = ops.conv_desc(nhwc(x), pack_w(w, Cc), y, n=N, grid=[(H, W)], src_hw=[(H, W)], dst_hw=[(H, W)], cs=Cc, cd=Cc, cd_pad=Cc, ldd=Cc,
                      kh=3, kw=3, stride=1, pad=1, flags=force << 8)
    runs = []
    for _ in range(2):
        y.view(torch.int16).fill_(-1)            # 0xffff: a NaN bit pattern in every element
        L.check(L.lib.dsl_conv2d(C.byref(d), L.stream_ptr()), 'dsl_conv2d')
        sync()
        runs.append(y.clone())
    assert not bool(torch.isnan(runs[0].float()).any())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    close_fwd(from_nhwc(runs[0]), yref)

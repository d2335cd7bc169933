"""Convolution descriptors whose launch plans tests/test_conv_plan_cpu.py pins (tests/golden/conv_plan.json): every convolution
geometry of the benchmark step (N = 2, 800 x 1344) and of the special paths, built over integer dummy pointers - the plan query
dsl_conv2d_plan is host-only.  tools/gen_conv_plan_golden.py writes the fixture from these same descriptors."""
import ctypes as C

from dsl_amd import _lib as L
from dsl_amd import ops

N = 2
LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
# 16-byte aligned dummies (the in-register addend epilogue, ConvK.addfast, asks for that); UNALIGNED is 8-byte aligned only
SRC, WGT, DST, ADD, MASK, SCALE, BIAS, WS, GNWS, GNX, GAMMA, BETA, STATS = [(i + 1) << 32 for i in range(13)]
UNALIGNED = ADD + 8
WS_BYTES = 128 << 20

# (name, cin, cout, k, stride, source sizes): the rows of tools/bench_conv.py, repeated ones included
BENCH_SHAPES = [
    ('head tower 3x3 256 (5 lvls)', 256, 256, 3, 1, LEVELS),
    ('fpn 3x3 256 @P3', 256, 256, 3, 1, LEVELS[:1]),
    ('l1 3x3 64->64 @200x336', 64, 64, 3, 1, [(200, 336)]),
    ('l1 1x1 64->256', 64, 256, 1, 1, [(200, 336)]),
    ('l1 1x1 256->64', 256, 64, 1, 1, [(200, 336)]),
    ('l2 3x3 128 @100x168', 128, 128, 3, 1, [(100, 168)]),
    ('l2 1x1 128->512', 128, 512, 1, 1, [(100, 168)]),
    ('l2 1x1 512->128', 512, 128, 1, 1, [(100, 168)]),
    ('l3 3x3 256 @50x84', 256, 256, 3, 1, [(50, 84)]),
    ('l3 1x1 256->1024', 256, 1024, 1, 1, [(50, 84)]),
    ('l3 1x1 1024->256', 1024, 256, 1, 1, [(50, 84)]),
    ('l4 3x3 512 @25x42', 512, 512, 3, 1, [(25, 42)]),
    ('l4 1x1 2048->512', 2048, 512, 1, 1, [(25, 42)]),
    ('l4 1x1 512->2048', 512, 2048, 1, 1, [(25, 42)]),
    ('l4 3x3 512 @25x42 (2)', 512, 512, 3, 1, [(25, 42)]),
    ('l4 1x1 512->2048 (2)', 512, 2048, 1, 1, [(25, 42)]),
    ('l4 1x1 2048->512 (2)', 2048, 512, 1, 1, [(25, 42)]),
    ('l3.0 ds 1x1 s2 512->1024', 512, 1024, 1, 2, [(100, 168)]),
]


def _out(sizes, k, s):
    p = k // 2
    return [((h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1) for h, w in sizes]


def _fwd(ci, co, k, s, sizes, flags=L.CONV_RELU_OUT, cd_pad=None, ldd=None, **kw):
    so = _out(sizes, k, s)
    return ops.conv_desc(SRC, WGT, DST, n=N, grid=so, src_hw=sizes, dst_hw=so, cs=ci, cd=co, cd_pad=cd_pad or co, ldd=ldd or co,
                         kh=k, kw=k, stride=s, pad=k // 2, flags=flags, **kw)


def _dgrad(ci, co, k, s, sizes, flags=L.CONV_MASK_LAST, **kw):
    """data gradient of the forward convolution ci -> co over `sizes`: dY (co channels) -> dX (ci channels), masked by the input"""
    so = _out(sizes, k, s)
    return ops.conv_desc(SRC, WGT, DST, n=N, grid=sizes, src_hw=so, dst_hw=sizes, cs=co, cd=ci, cd_pad=ci, ldd=ci, kh=k, kw=k,
                         stride=s, pad=k // 2, mode=1, mask=MASK, ldm=ci, flags=flags, **kw)


def _with(d, **fields):
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def cases():
    """{name: dsl_conv_desc}, in a fixed order"""
    out = {}
    for name, ci, co, k, s, sizes in BENCH_SHAPES:
        out['bench fwd   ' + name] = _fwd(ci, co, k, s, sizes)
        out['bench dgrad ' + name] = _dgrad(ci, co, k, s, sizes)
    gn_bwd = dict(gn_ws=GNWS, gn_x=GNX, gn_gamma=GAMMA, gn_beta=BETA, gn_stats=STATS)
    out['tower'] = _fwd(256, 256, 3, 1, LEVELS, flags=0, bias=BIAS)
    out['tower gn_ws'] = _with(_fwd(256, 256, 3, 1, LEVELS, flags=0, bias=BIAS), gn_ws=GNWS)
    out['tower dgrad gn_x'] = _with(_dgrad(256, 256, 3, 1, LEVELS, flags=0), mask=None, ldm=0, **gn_bwd)
    out['tower dgrad gn_x without gn_ws'] = _with(_dgrad(256, 256, 3, 1, LEVELS, flags=0), mask=None, ldm=0, gn_x=GNX)
    out['tower fp8'] = _fwd(256, 256, 3, 1, LEVELS, flags=L.CONV_FP8, scale=SCALE, bias=BIAS)
    out['tower fp8 gn_ws'] = _with(_fwd(256, 256, 3, 1, LEVELS, flags=L.CONV_FP8, scale=SCALE, bias=BIAS), gn_ws=GNWS)
    out['predictor cd 80 of 128 f32'] = _fwd(256, 80, 3, 1, LEVELS, flags=L.CONV_OUT_F32, cd_pad=128, ldd=80, bias=BIAS)
    out['fpn lateral add_upsample'] = _fwd(512, 256, 1, 1, LEVELS[:1], flags=L.CONV_ADD_UPSAMPLE, bias=BIAS, addend=ADD, lda=256,
                                           add_hw=LEVELS[1:2])
    out['p7 relu_in'] = _fwd(256, 256, 3, 2, LEVELS[3:4], flags=L.CONV_RELU_IN, bias=BIAS)
    out['dgrad 3x3 stride 2'] = _dgrad(256, 256, 3, 2, LEVELS[:1])
    for i, d in enumerate(ops.dgrad_s2_descs(SRC, {(py, px): WGT + ((2 * py + px) << 24) for py in (0, 1) for px in (0, 1)}, DST, n=N,
                                             dy_hw=LEVELS[1], dst_hw=LEVELS[0], cs=256, cd=256, mask=MASK, addend=ADD,
                                             flags=L.CONV_MASK_LAST)):
        out['dgrad_s2_descs class %d' % i] = d
    out['stem 7x7 small_c'] = _fwd(8, 64, 7, 2, [(800, 1344)], flags=L.CONV_RELU_OUT | L.CONV_SMALL_C, scale=SCALE, bias=BIAS)
    out['channel slice lds 256 of cs 128'] = _fwd(128, 128, 1, 1, LEVELS[:1], lds=256)
    # the in-register addend epilogue and what turns it off
    out['residual add'] = _fwd(128, 512, 1, 1, LEVELS[:1], scale=SCALE, bias=BIAS, addend=ADD, lda=512)
    out['residual add unaligned'] = _fwd(128, 512, 1, 1, LEVELS[:1], scale=SCALE, bias=BIAS, addend=UNALIGNED, lda=512)
    out['residual add staged'] = _fwd(128, 512, 1, 1, LEVELS[:1], flags=L.CONV_RELU_OUT | L.CONV_EPI_STAGED, scale=SCALE, bias=BIAS,
                                      addend=ADD, lda=512)
    return out


FORCES = list(range(9)) + [15]
FORCE_SPLITS = [0, 2, 4]
WORKSPACES = [WS_BYTES, 0]
PLAN_FIELDS = ['kernel', 'cfg', 'bco', 'bpx', 'threads', 'splits', 'grid0', 'grid1', 'grid2', 'ident', 'addfast', 'lds_bytes',
               'workspace_bytes']


def variants():
    return [(f, s, w) for f in FORCES for s in FORCE_SPLITS for w in WORKSPACES]


def plan(d, force, force_split, ws_bytes, lib=None):
    """The plan of `d` under the test hooks: the 13 PLAN_FIELDS, or [rc, error text] where the launch is refused."""
    lib = lib or L.lib
    f0, w0 = d.flags, (d.workspace, d.workspace_bytes)
    d.flags = (f0 & ~0xff00) | (force << 8) | (force_split << 12)
    d.workspace, d.workspace_bytes = (WS if ws_bytes else None), ws_bytes
    p = L.ConvPlan()
    rc = lib.dsl_conv2d_plan(C.byref(d), C.byref(p))
    d.flags, (d.workspace, d.workspace_bytes) = f0, w0
    if rc != 0:
        return [rc, lib.dsl_last_error().decode()]
    return [p.kernel, p.cfg, p.bco, p.bpx, p.threads, p.splits, p.grid[0], p.grid[1], p.grid[2], p.ident, p.addfast, p.lds_bytes,
            p.workspace_bytes]

"""The convolution launch planner (csrc/conv.hip: conv_validate, conv_fill_k, conv_plan) on the geometries of the benchmark step and of
the special paths, without a device through dsl_conv2d_plan - the function dsl_conv2d itself takes its kernel, grid, block and LDS
size from.  tests/golden/conv_plan.json holds what the library answered BEFORE the tile table / single launch path refactor (written
by tools/gen_conv_plan_golden.py from that build): a plan that differs is a changed launch and has to be meant.  The quiet rules of
the force hooks are pinned with the rest: forced rows 9..14 are no force, a forced small tile on a strided data gradient falls to the
v1 kernel, an infeasible forced split is ignored."""
import ctypes as C
import json
import os

import pytest

import conv_plan_cases as P
from dsl_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plan.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g['fields'] == P.PLAN_FIELDS and [tuple(v) for v in g['variants']] == P.variants()
    return g['plans']


CASES = P.cases()


def test_fixture_covers_exactly_the_cases(golden):
    assert list(golden) == list(CASES)
    assert len(CASES) >= 36 + 19 and len(P.variants()) == 10 * 3 * 2


@pytest.mark.parametrize('name', list(CASES))
def test_plan_is_pinned(golden, name):
    d = CASES[name]
    for v, want in zip(P.variants(), golden[name]):
        assert P.plan(d, *v) == want, (name, dict(force=v[0], force_split=v[1], workspace_bytes=v[2]))


def test_every_kernel_generation_and_refusal_is_in_the_fixture(golden):
    plans = [p for ps in golden.values() for p in ps]
    assert {p[0] for p in plans if len(p) == 13} == {0, 1, 2, 3, 4, 5}
    assert {p[1] for p in plans if len(p) == 13} == {-1, 0, 1, 2, 3, 4, 5, 6, 7}
    assert any(len(p) == 2 and p[0] != 0 for p in plans)


def test_rows_9_to_14_are_no_force():
    for name in ('tower', 'bench dgrad l2 3x3 128 @100x168', 'dgrad 3x3 stride 2'):
        d = CASES[name]
        for force in range(9, 15):
            assert P.plan(d, force, 0, P.WS_BYTES) == P.plan(d, 0, 0, P.WS_BYTES)


def test_forced_rows_the_tools_ask_for():
    """ops.conv_forced_rows (tools/plan_check.py, tools/bench_conv.py): the rows each kernel generation is instantiated for"""
    from dsl_amd import ops
    assert ops.conv_forced_rows(CASES['tower']) == [1, 2, 3, 4, 5, 6, 7, 8]                   # pipelined kernel: every row
    assert ops.conv_forced_rows(CASES['dgrad 3x3 stride 2']) == [1, 2, 3, 4, 5]             # general-gather kernel
    assert ops.conv_forced_rows(CASES['tower fp8']) == [1, 2, 4]
    assert ops.conv_forced_rows(CASES['tower dgrad gn_x']) == [1, 2]                         # backward GroupNorm records
    assert ops.conv_forced_rows(CASES['stem 7x7 small_c']) == [5]
    assert ops.conv_forced_rows(CASES['bench fwd   l1 3x3 64->64 @200x336']) == [5, 7, 8]    # 64 couts: the 64-cout tiles
    assert ops.conv_forced_rows(CASES['p7 relu_in']) == []                                   # v1 kernel only


def test_plan_agrees_with_the_workspace_query():
    """dsl_conv2d_workspace_bytes is what the plan uses of a workspace that is large enough for it"""
    some = 0
    for name, d in CASES.items():
        want = L.lib.dsl_conv2d_workspace_bytes(C.byref(d))
        assert want <= P.WS_BYTES, name
        assert P.plan(d, 0, 0, P.WS_BYTES)[-1] == want, name
        some += want > 0
    assert some >= 3


def test_plan_refuses_what_the_launch_refuses():
    d = L.ConvDesc()
    p = L.ConvPlan()
    assert L.lib.dsl_conv2d_plan(C.byref(d), C.byref(p)) != 0 and b'nseg' in L.lib.dsl_last_error()
    assert L.lib.dsl_conv2d_plan(C.byref(CASES['tower']), None) != 0

"""psld_amd/score_routes.py against the kernel choices the executor made before they were gathered there.

``tests/golden/routes.json`` was written at commit e4f7cc2 - the last one at which ``_Exec.resblock`` (``lp0`` / ``lp1`` /
``fuse0`` / ``fuse1`` / the ``part_for`` arguments), ``_Exec.conv3``, ``dgrad``, ``wgrad``, ``_resblock_cat_bwd`` and
``_cat_ok`` each tested the ``ops`` predicates themselves - by a throw-away script that evaluated those expressions,
copied verbatim, over the grid below (the library built, no GPU: the predicates are host functions).  A later pull request
that changes a policy or a kernel's shape coverage regenerates the file from the route functions (``_row`` below is the
row format) and reviews the diff.

Grid: ``PSLD_WINOGRAD`` 0 / 1 / 2 x recording or not on the limb kernels (fused-GroupNorm and Winograd weight-gradient
policies at their defaults), and for ``PSLD_WINOGRAD=1`` also math mode f32 (``split`` False) and a tape-less forward with
dropout active; c1 in 128 / 160 / 256 / 384, cout in 128 / 160 / 256, square maps of 8 .. 128, batch 2 / 16 / 128, no
resampling / up (not from 128) / down; a second source of 128 or 256 channels for blocks that do not resample: its rows
record ``cat=0`` where the parent refused the unmaterialised concatenation, else ``cat=1`` and the block's pattern."""
import json
import os

import pytest

from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def routes():
    from psld_amd import ops, score_routes as R
    ops.lib()
    with open(os.path.join(GOLDEN, "routes.json")) as f:
        doc = json.load(f)
    yield ops, R, doc
    ops.set_winograd(None)
    ops.set_fused_gn(None)
    ops.set_wgrad_winograd(None)
    ops.conv3x3_wino_gn_wanted.cache_clear()


def _shapes(grid):
    for c1 in grid["c1"]:
        for cout in grid["cout"]:
            for b in grid["b"]:
                for hw in grid["hw"]:
                    for c2 in grid["c2"]:
                        yield c1, c2, b, hw, cout, False, False
                    if hw != 128:
                        yield c1, 0, b, hw, cout, True, False
                    yield c1, 0, b, hw, cout, False, True


def _row(R, plan, split, record, c1, c2, b, ho, wo, cout):
    """A plan in the fixture's row format (its ``fields``)."""
    f = [int(bool(plan.lp0)), int(bool(plan.lp1)),
         int(bool(R.conv3_route(True, c1, c2, b, ho, wo, cout, True) == R.LIMB)),       # part_for's "limb kernel" arguments
         int(bool(R.conv3_route(True, cout, 0, b, ho, wo, cout, True) == R.LIMB)),
         int(bool(plan.part0)), int(bool(plan.part1)), plan.conv0, plan.conv1]
    if record:
        f += [plan.wgrad0, plan.wgrad1, "+".join(plan.dgrad0), plan.dgrad1]
    return " ".join(str(v) for v in f)


def _check_invariants(R, plan, record, dropout, c2):
    for lp, conv, wgrad in ((plan.lp0, plan.conv0, plan.wgrad0), (plan.lp1, plan.conv1, plan.wgrad1)):
        if lp:
            assert conv == R.LIMB
            assert not record or wgrad == R.LIMB
        if conv == R.WINO_GN:
            assert not record
        assert conv in (R.WINO, R.LIMB, R.TILE, R.WINO_GN)
    assert plan.conv1 != R.WINO_GN or not dropout
    if record:
        assert plan.wgrad0 in (R.WINO, R.LIMB, R.TILE) and plan.wgrad1 in (R.WINO, R.LIMB, R.TILE)
        assert len(plan.dgrad0) == (2 if c2 else 1) and plan.dgrad1 in (R.WINO, R.LIMB, R.TILE)
        if c2:
            assert plan.dgrad0 in ((R.WINO, R.WINO), (R.LIMB, R.LIMB))
    else:
        assert plan.wgrad0 is None and plan.wgrad1 is None and plan.dgrad0 == () and plan.dgrad1 is None


def test_routes_reproduce_the_parent_on_the_grid(routes):
    ops, R, doc = routes
    patterns, shapes = doc["patterns"], list(_shapes(doc["grid"]))
    seen, n = set(), 0
    for sl in doc["slices"]:
        split, record, dropout = sl["split"], sl["record"], sl["dropout"]
        ops.set_winograd(sl["winograd"])
        ops.set_fused_gn(1)
        ops.set_wgrad_winograd(1)
        ops.conv3x3_wino_gn_wanted.cache_clear()       # set_winograd leaves this cache as it is
        assert len(sl["rows"]) == len(shapes)
        for (c1, c2, b, hw, cout, up, down), idx in zip(shapes, sl["rows"]):
            want = patterns[idx]
            where = (sl["winograd"], split, record, dropout, c1, c2, b, hw, cout, up, down)
            if c2:
                ok = R.cat_ok(split, record, c1, c2, b, hw, hw, cout, up, down, c1 + c2 != cout or up or down)
                assert bool(ok) == want.startswith("cat=1"), where
                if not ok:
                    continue
                want = want[len("cat=1 "):]
            plan = R.block_plan(split, True, record, dropout, c1, c2, b, hw, hw, cout, up, down)
            ho = hw // 2 if down else (hw * 2 if up else hw)
            assert _row(R, plan, split, record, c1, c2, b, ho, ho, cout) == want, where
            _check_invariants(R, plan, record, dropout, c2)
            # the stand-alone route functions - what conv3 / dgrad / wgrad look up for a caller without a plan
            if plan.conv0 != R.WINO_GN:
                assert R.conv3_route(split, c1, c2, b, ho, ho, cout, plan.lp0) == plan.conv0, where
            if plan.conv1 != R.WINO_GN:
                assert R.conv3_route(split, cout, 0, b, ho, ho, cout, plan.lp1) == plan.conv1, where
            if record:
                assert R.wgrad_route(split, cout, c1, c2, b, ho, ho, plan.lp0) == plan.wgrad0, where
                assert R.wgrad_route(split, cout, cout, 0, b, ho, ho, plan.lp1) == plan.wgrad1, where
                assert R.conv3_route(split, cout, 0, b, ho, ho, cout) == plan.dgrad1, where
                if not c2:
                    assert R.conv3_route(split, cout, 0, b, ho, ho, c1) == plan.dgrad0[0], where
            seen.update((plan.conv0, plan.conv1, plan.wgrad0, plan.wgrad1))
            n += 1
    # the fixture discriminates: every route occurs
    assert seen >= {R.WINO, R.LIMB, R.TILE, R.WINO_GN} and n > 5000, (seen, n)


def test_two_source_weight_gradient_nothing_takes_is_named(routes):
    ops, R, _ = routes
    ops.set_wgrad_winograd(1)
    # math mode f32: no limb kernel, and the tile engine reads one source
    assert R.wgrad_route(False, 128, 128, 128, 2, 16, 16, False) == R.NONE
    assert R.wgrad_route(False, 128, 128, 0, 2, 16, 16, False) == R.TILE


def test_routes_module_keeps_no_cache_of_its_own(routes):
    """set_winograd() must take effect on the next plan: the tests and tools switch it inside one process."""
    ops, R, _ = routes
    shape = (256, 0, 128, 32, 32, 256)
    got = []
    for mode in (0, 2, 0):
        ops.set_winograd(mode)
        got.append(R.conv3_route(True, *shape))
    assert got == [R.LIMB, R.WINO, R.LIMB]


def test_a_shape_left_fused_by_the_uncleared_cache_is_not_given_limb_planes(routes):
    """set_winograd() leaves conv3x3_wino_gn_wanted's cache alone (behaviour this module keeps): a shape fused
    under PSLD_WINOGRAD=2 stays fused after a switch to 0 in the same process, while the Winograd question itself now
    answers no.  The fused launch reads the raw fp32 tensor, so the plan must not ask for limb planes there (the AFHQv2-128
    forward tests walk through exactly this state)."""
    ops, R, _ = routes
    shape = (256, 0, 1, 64, 64, 256, True, False)        # an upsampling block: Conv_1 on a 128x128 map
    ops.set_fused_gn(1)
    ops.set_winograd(2)
    ops.conv3x3_wino_gn_wanted.cache_clear()
    assert R.block_plan(True, True, False, False, *shape).conv1 == R.WINO_GN
    ops.set_winograd(0)
    stale = R.block_plan(True, True, False, False, *shape)
    assert stale.conv1 == R.WINO_GN and not stale.lp1
    ops.conv3x3_wino_gn_wanted.cache_clear()
    fresh = R.block_plan(True, True, False, False, *shape)
    assert fresh.conv1 == R.LIMB and fresh.lp1

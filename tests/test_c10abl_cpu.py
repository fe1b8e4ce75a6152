"""The four-level CIFAR-10 networks (maps 32, 16, 8 and 4x4) without a GPU: the ``c10_ablation`` / ``c10_vpsde`` presets
against the configurations captured from the reference (tests/golden/c10abl_meta.json, tools/gen_golden_c10abl.py), the CPU
oracle against the reference's forward of both networks, the 4x4 answers of the Winograd kernels' host-side predicates, and a
dry run of the executor (tools/launch_trace's stand-in library) showing which entry points the 4x4 level's 3x3 convolutions
reach."""
import json
import os

import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests.conftest import GOLDEN
from tests.synth import synth_state_dict

T = torch.from_numpy
PRESETS = ("c10_ablation", "c10_vpsde")


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "c10abl_meta.json")) as fh:
        return json.load(fh)


# ---- presets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRESETS)
def test_preset_equals_the_reference_configuration(meta, name):
    cfg, ref = getattr(C, name)(), meta[name]["diffusion"]
    nodes = {"data": cfg.data, "score_fn": cfg.model.score_fn, "sde": cfg.model.sde, "optimizer": cfg.training.optimizer,
             "training": cfg.training, "loss": cfg.training.loss, "evaluation": cfg.evaluation}
    assert set(ref) == set(nodes)
    for node, want in ref.items():
        for key, value in want.items():
            assert key in nodes[node], (node, key)
            assert nodes[node][key] == value, (node, key, nodes[node][key], value)
    # whole nodes of the model: the preset carries no key the reference does not have
    assert set(cfg.model.score_fn) == set(ref["score_fn"])
    assert set(cfg.model.sde) == set(ref["sde"])


def test_presets_are_the_four_level_networks():
    for name, nres, ch in (("c10_ablation", 2, 6), ("c10_vpsde", 4, 3)):
        sf = getattr(C, name)().model.score_fn
        assert (sf.nf, list(sf.ch_mult), sf.num_res_blocks, sf.in_ch, sf.out_ch) == (128, [1, 2, 2, 2], nres, ch, ch)
        assert getattr(C, name)().data.image_size // 2 ** (len(sf.ch_mult) - 1) == 4


@pytest.mark.parametrize("name", PRESETS)
def test_state_dict_census(meta, name):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    net = get_module("score_fn", "ncsnpp")(getattr(C, name)())
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == meta[name]["keys"]
    assert sum(v.numel() for v in net.state_dict().values()) == meta[name]["n_params"]


def test_conv_census_of_the_4x4_level():
    """The 3x3 stride-1 convolutions on 4x4 maps, counted from the modules: 2 in the block that resamples 8 -> 4, 2 nres in the
    level, 4 in the middle, 2 (nres + 1) on the way up = 16 at nres = 2, 24 at nres = 4."""
    import psld_amd
    from psld_amd.score_modules import ResnetBlockBigGANpp
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    for name, nres in (("c10_ablation", 2), ("c10_vpsde", 4)):
        net = get_module("score_fn", "ncsnpp")(getattr(C, name)())
        size, n4 = 32, 0
        for m in net.all_modules:
            if not isinstance(m, ResnetBlockBigGANpp):
                continue
            if m.down:
                size //= 2
            if m.up:
                size *= 2
            if size == 4:
                n4 += 2
        assert n4 == 2 + 2 * nres + 4 + 2 * (nres + 1) == {2: 16, 4: 24}[nres], (name, n4)


# ---- oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRESETS)
def test_oracle_forward_against_the_reference(meta, golden, name):
    g = golden(f"net_{name}.npz")
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta[name]["keys"]], meta[name]["seed"])
    with torch.no_grad():
        y = O.ncsnpp_forward(sd, getattr(C, name)(), T(g["x"]), T(g["t"]))
    assert rel_l2(y, T(g["y"])) < 2e-6


# ---- predicates (the loaded library; no device) ----------------------------------------------------------------------------
def test_forward_predicate_takes_4x4_maps():
    from psld_amd import ops
    for b in (1, 8, 9, 32):
        assert ops.conv3x3_wino_supported(256, 0, b, 4, 4, 256), b
        assert ops.conv3x3_wino_supported(256, 256, b, 4, 4, 256), b
        assert ops.conv3x3_wino_supported(384, 0, b, 4, 4, 512), b
    assert ops.conv3x3_wino_supported(160, 0, 3, 4, 4, 160)                 # channel tail
    # channel rules unchanged
    assert not ops.conv3x3_wino_supported(256, 0, 8, 4, 4, 64)
    assert not ops.conv3x3_wino_supported(240, 0, 8, 4, 4, 256)
    # GroupNorm-fused staging: one image per workgroup region only
    assert not ops.conv3x3_wino_gn_supported(256, 0, 8, 4, 4, 256)


def test_wgrad_predicate_takes_4x4_maps_in_batches_of_eight():
    from psld_amd import ops
    for b, want in ((8, True), (32, True), (1, False), (12, False)):
        assert ops.conv3x3_wgrad_wino_supported(256, 256, 0, b, 4, 4) == want, b
    assert ops.conv3x3_wgrad_wino_supported(256, 256, 256, 16, 4, 4)
    assert ops.conv3x3_wgrad_wino_supported(512, 384, 0, 24, 4, 4)


def test_other_maps_answer_as_before():
    from psld_amd import ops
    lib = ops.lib()
    # 4x8 (four images per region) and 8x8 forward; 8x4 and 4x16 were and are refused
    assert ops.conv3x3_wino_supported(256, 0, 3, 4, 8, 256) and ops.conv3x3_wino_supported(256, 0, 3, 8, 8, 256)
    assert not ops.conv3x3_wino_supported(256, 0, 3, 8, 4, 256)
    assert not ops.conv3x3_wino_supported(256, 0, 3, 2, 4, 256)
    assert ops.conv3x3_wino_supported(256, 0, 3, 4, 16, 256) == bool(128 % (4 * 16) == 0)
    # weight gradient: square maps only, 8x8 in batches of two
    assert not ops.conv3x3_wgrad_wino_supported(256, 256, 0, 8, 4, 8)
    assert ops.conv3x3_wgrad_wino_supported(256, 256, 0, 2, 8, 8) and not ops.conv3x3_wgrad_wino_supported(256, 256, 0, 3, 8, 8)
    # the direct limb kernels keep refusing 4x4 maps
    assert not ops.conv3x3_split_supported(256, 0, 8, 4, 4, 256)
    # split-chunk plan of an 8x8 launch: as many pixel tiles as before (two images each)
    assert lib.psld_conv3x3_wino_ksplit(512, 0, 8, 8, 8, 256) == lib.psld_conv3x3_wino_ksplit(512, 0, 7, 8, 8, 256)


def test_split_chunk_plan_counts_seven_images_per_workgroup():
    """(b = 8, 512 -> 256) at 4x4: two workgroups per channel tile, so the 16 chunks split 8 ways at most (two chunks each)
    on any device with at least 64 CUs; the workspace holds one [b * 16][cout] slab per split."""
    from psld_amd import ops
    ks = ops.lib().psld_conv3x3_wino_ksplit(512, 0, 8, 4, 4, 256)
    assert ks == 8
    assert ops.conv3x3_wino_ws_bytes(512, 0, 8, 4, 4, 256) == ks * 8 * 16 * 256 * 4


def test_policy_modes():
    """4x4 maps have their own opt-in, ops.set_winograd_4x4: off (the default) they stay on the tile engine under every
    PSLD_WINOGRAD / PSLD_WGRAD_WINOGRAD mode - the routes of every existing configuration are what they were; 2 takes every
    supported shape, 1 the measured batches; mode 0 of a direction switches it off whatever the opt-in says."""
    from psld_amd import ops, score_routes as R
    try:
        assert ops.winograd_4x4() == 0
        for mode in (0, 1, 2):
            ops.set_winograd(mode)
            ops.set_wgrad_winograd(mode)
            for b in (8, 32, 128):
                assert not ops.conv3x3_wino_wanted(256, 0, b, 4, 4, 256, True)
                assert not ops.conv3x3_wgrad_wino_wanted(256, 256, 0, b, 4, 4)
                assert R.conv3_route(True, 256, 0, b, 4, 4, 256) == R.TILE and R.wgrad_route(True, 256, 256, 0, b, 4, 4, False) == R.TILE
                assert not R.cat_ok(True, True, 256, 256, b, 4, 4, 256, False, False, True)
        ops.set_winograd_4x4(2)
        for mode in (1, 2):
            ops.set_winograd(mode)
            ops.set_wgrad_winograd(mode)
            assert ops.conv3x3_wino_wanted(256, 0, 1, 4, 4, 256, True) and ops.conv3x3_wino_wanted(256, 256, 9, 4, 4, 256)
            assert ops.conv3x3_wgrad_wino_wanted(256, 256, 256, 8, 4, 4)
            assert not ops.conv3x3_wgrad_wino_wanted(256, 256, 0, 12, 4, 4)        # not supported: no mode takes it
            assert R.cat_ok(True, True, 256, 256, 8, 4, 4, 256, False, False, True)
            assert not R.cat_ok(True, True, 256, 256, 12, 4, 4, 256, False, False, True)     # no two-source weight gradient
            assert R.cat_ok(True, False, 256, 256, 16, 4, 4, 256, False, False, True)
        ops.set_winograd(0)
        ops.set_wgrad_winograd(0)
        assert not ops.conv3x3_wino_wanted(256, 0, 32, 4, 4, 256, True)
        assert not ops.conv3x3_wgrad_wino_wanted(256, 256, 0, 32, 4, 4)
        ops.set_winograd(1)
        ops.set_wgrad_winograd(1)
        ops.set_winograd_4x4(1)
        # the measured thresholds, never the "direct kernels win below one round" rule of larger maps
        for b in (1, 7, 8, 32, 128):
            assert ops.conv3x3_wino_wanted(256, 0, b, 4, 4, 256, True) == (b >= ops.WINO_4X4_MIN_BATCH == 8)
        for b in (8, 32, 128):
            assert ops.conv3x3_wgrad_wino_wanted(256, 256, 0, b, 4, 4)
        # larger maps do not see the opt-in
        ops.set_winograd_4x4(0)
        big = [ops.conv3x3_wino_wanted(256, 0, b, 8, 8, 256, True) for b in (2, 16, 128)]
        ops.set_winograd_4x4(2)
        assert big == [ops.conv3x3_wino_wanted(256, 0, b, 8, 8, 256, True) for b in (2, 16, 128)]
    finally:
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
        ops.set_winograd_4x4(0)


# ---- launch dry run --------------------------------------------------------------------------------------------------------
_SIG_CACHE = {}


def _arg(row, name):
    """Argument ``name`` of a recorded row, by the C prototype's parameter order in include/psld_hip.h."""
    import re
    fn = row[0]
    if fn not in _SIG_CACHE:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "include", "psld_hip.h")) as fh:
            text = fh.read()
        m = re.search(r"^int %s\s*\(([^)]*)\)" % re.escape(fn), text, re.M)
        assert m, fn
        _SIG_CACHE[fn] = [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]
    return row[1 + _SIG_CACHE[fn].index(name)]


_CASE = dict(tiny=dict(image_size=16, nf=128, ch_mult=(1, 2, 2)), batch=8, mode="bf16x6", pin="residual", dropout=0.0)
_TRACE = os.path.join(GOLDEN, "c10abl_launch_trace.json")


def _run_case(wino, patch=setattr):
    """(eval rows, recorded rows) of the local case - maps 16, 8, 4 at batch 8; not an entry of tools.launch_trace.CASES - with
    the three Winograd switches at ``wino`` (0 or 2).  The caller has applied ``tools.launch_trace.patches()``."""
    from psld_amd import ops
    from tools import launch_trace as LT
    ops.lib()
    LT.CASES["c10abl_4x4"] = LT.Case(_CASE["tiny"], _CASE["batch"], _CASE["mode"], _CASE["pin"], _CASE["dropout"], wino)
    ops.set_wgrad_winograd(wino)
    ops.set_winograd_4x4(wino)
    try:
        return LT.run_case("c10abl_4x4", patch)
    finally:
        del LT.CASES["c10abl_4x4"]
        ops.set_wgrad_winograd(None)
        ops.set_winograd_4x4(0)


def _dry_run(monkeypatch, wino):
    from tools import launch_trace as LT
    for obj, attr, val in LT.patches():
        monkeypatch.setattr(obj, attr, val)
    ev, tr = _run_case(wino, monkeypatch.setattr)
    return ev + tr


def write_trace_fixture():
    """``python -m tests.test_c10abl_cpu``: (re)write tests/golden/c10abl_launch_trace.json - per switch setting what
    tools/launch_trace keeps of a case (row counts, count per entry point, SHA-256 of the rows).  A pull request that changes a
    launch of this case on purpose regenerates the file and reviews the counts."""
    import contextlib
    from unittest import mock

    from tools import launch_trace as LT
    with contextlib.ExitStack() as stack:
        for obj, attr, val in LT.patches():
            stack.enter_context(mock.patch.object(obj, attr, val))
        doc = {"case": {**_CASE, "tiny": {k: list(v) if isinstance(v, tuple) else v for k, v in _CASE["tiny"].items()}},
               "switches_0": LT.summary(*_run_case(0)), "switches_2": LT.summary(*_run_case(2))}
    with open(_TRACE, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", _TRACE)


def _tile_3x3_on_4x4(rows):
    """Tile-engine rows that carry a 3x3 kernel on a 4x4 output map with at least 128 input channels."""
    out = []
    for r in rows:
        if r[0].startswith("psld_conv2d_nhwc") and r[0].endswith("_f32"):
            if _arg(r, "kh") == 3 and _arg(r, "oh") == 4 and _arg(r, "ow") == 4 and _arg(r, "stride") == 1 and \
                    _arg(r, "c1") + _arg(r, "c2") >= 128:
                out.append(r)
        elif r[0] == "psld_conv2d_wgrad_nhwc_f32":
            if _arg(r, "kh") == 3 and _arg(r, "oh") == 4 and _arg(r, "ow") == 4 and _arg(r, "stride") == 1 and _arg(r, "cin") >= 128:
                out.append(r)
    return out


def test_dry_run_4x4_level_on_the_winograd_kernels(monkeypatch):
    rows = _dry_run(monkeypatch, 2)
    assert _tile_3x3_on_4x4(rows) == []
    fwd = [r for r in rows if r[0].startswith("psld_conv3x3_wino") and "pack" not in r[0] and _arg(r, "h") == 4 and _arg(r, "w") == 4]
    wg = [r for r in rows if r[0].startswith("psld_conv3x3_wgrad_wino") and _arg(r, "h") == 4 and _arg(r, "w") == 4]
    assert fwd and wg
    assert any(_arg(r, "c2") > 0 for r in fwd), "no two-source forward launch on a 4x4 map"
    assert any(_arg(r, "cin2") > 0 for r in wg), "no two-source weight gradient on a 4x4 map"
    # no launch asks for GroupNorm partial sums of a 16-pixel image (epilogue fields in the order of _lib.Epilogue)
    from psld_amd import _lib
    gp = [n for n, _ in _lib.Epilogue._fields_].index("gn_part")
    for r in fwd:
        epi = _arg(r, "epi")
        assert epi is None or epi[gp] == [True, True], r[0]


def _against_fixture(rows_pair, key):
    from tools import launch_trace as LT
    with open(_TRACE) as fh:
        want = json.load(fh)[key]
    got = LT.summary(*rows_pair)
    assert got["eval_rows"] == want["eval_rows"] and got["rows"] == want["rows"]
    assert got["counts"] == want["counts"]
    assert got["sha256"] == want["sha256"], "same launches, other arguments: regenerate with python -m tests.test_c10abl_cpu and review"


def test_dry_run_mode_0_keeps_todays_rows(monkeypatch):
    """With the three switches at 0 the executor makes the launches it made before the 4x4 geometry existed: the fixture's
    ``switches_0`` entry (tests/golden/c10abl_launch_trace.json: row counts, count per entry point and digest, in the format
    of tests/golden/launch_trace.json) was reproduced bit for bit by the same dry run on the parent commit, where the case's
    3x3 convolutions on 4x4 maps are tile-engine rows; with the 4x4 opt-in at its default the rows are the same whatever the
    other two switches say there."""
    from tools import launch_trace as LT
    for obj, attr, val in LT.patches():
        monkeypatch.setattr(obj, attr, val)
    ev, tr = _run_case(0, monkeypatch.setattr)
    rows = ev + tr
    assert not [r for r in rows if r[0].startswith("psld_conv3x3_wino") or r[0].startswith("psld_conv3x3_wgrad_wino")]
    tile = _tile_3x3_on_4x4(rows)
    assert tile and all(r[0].startswith("psld_conv2d_") for r in tile)
    _against_fixture((ev, tr), "switches_0")


def test_dry_run_rows_with_the_switches_at_2_are_the_fixtures(monkeypatch):
    from tools import launch_trace as LT
    for obj, attr, val in LT.patches():
        monkeypatch.setattr(obj, attr, val)
    _against_fixture(_run_case(2, monkeypatch.setattr), "switches_2")


if __name__ == "__main__":
    write_trace_fixture()

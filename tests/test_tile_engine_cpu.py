"""The fp32 tile engine's launch plans and the case table of tests/tile_cases.py, without a GPU.

The four entry points of psld_amd/csrc/tile_engine.hip choose between many kernels; the psld_*_plan queries run the host
code the launches select with.  Here: every case of the table reaches the form it claims (so a GPU test knows which kernel
it ran), the table reaches every form and every split count (a threshold change that un-covers one fails here), the
operands are admissible for exact comparison, every reference reacts to the mistakes an implicit GEMM can make, and no
split convolution is planned with an empty K range.
"""
import ctypes as C

import pytest
import torch

from tests import tile_cases as T


def _cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.mark.parametrize("key", T.case_ids())
def test_case_plans_its_form(ops, key):
    case = T.CASES[key]
    form, ns = T.Call(ops, T.operands(key)).plan()
    assert (T.form_name(form), ns) == (T.form_name(case.form), case.nsplit), str(case)
    assert form == case.form


def test_table_reaches_every_form():
    for entry, forms in T.ALL_FORMS.items():
        reached = {(c.layout, c.form) for c in T.CASES.values() if c.entry == entry}
        assert reached == forms, (entry, [(l, T.form_name(f)) for l, f in reached ^ forms])
    splits = {c.nsplit for c in T.CASES.values() if c.entry == "conv" and c.nsplit > 1}
    assert splits == T.SPLIT_COUNTS
    # ... and each split count once with the whole epilogue (accumulation included) into strided rows
    full = {c.nsplit for c in T.CASES.values() if c.entry == "conv" and c.nsplit > 1 and c.epi and c.epi.accumulate
            and c.epi.residual and c.epi.rows_per_img and c.p.get("ldy3")}
    assert full == T.SPLIT_COUNTS
    # the whole epilogue on every fast GEMM form, on the wave-uniform row-bias path (rows_per_img % 32 == 0) and off it
    for uniform in (True, False):
        got = {(c.layout, c.form) for c in T.CASES.values() if c.entry == "gemm" and c.epi and c.epi.accumulate
               and (c.epi.rows_per_img % 32 == 0) == uniform}
        assert got >= {f for f in T.ALL_FORMS["gemm"] if f[1] & T.L.TILE_KIND_MASK != T.GENERIC}, uniform


def test_fast_gemm_grids():
    """The cases named after a tile count have that many 128 x 128 tiles per image (grid.x of the XCD swizzle: 1, 9 = 8 + 1
    and 27 = 3 x 8 + 3), and the large-grid NT case is above the 256 tiles at which 64-row tiles stop."""
    seen = set()
    for c in T.CASES.values():
        if "tiles" in c.p:
            assert _cdiv(c.p["M"], 128) * _cdiv(c.p["N"], 128) == c.p["tiles"], str(c)
            seen.add((c.layout, c.p["tiles"]))
    assert seen == {("NN", 1), ("NN", 9), ("NN", 27), ("TN", 1), ("TN", 9), ("TN", 27), ("NT", 9)}
    big = T.CASES["gemm:nt-fast128-261tiles"].p
    assert big["tiles"] * big["batch"] == 261


def test_one_dense_case_per_form():
    for entry, forms in T.ALL_FORMS.items():
        dense = [(c.layout, c.form) for c in T.CASES.values() if c.entry == entry and c.dense]
        assert sorted(dense) == sorted(forms), entry


@pytest.mark.parametrize("key", T.case_ids())
def test_operands_are_admissible(key):
    """Integers in the documented ranges, K <= 4608, powers of two in the epilogue - and the fp64 reference is an fp32
    number below 2^24 in units of its last place, so equality with it is a fair demand."""
    case, o = T.CASES[key], T.operands(key)
    lim = {"A": 4, "x1": 4, "x2": 4, "dy": 4, "B": 3, "w": 3, "x": 3, "bias": 8, "rowbias": 8, "res": 8, "prev": 8}
    for name, t in o.logical.items():
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= lim[name], (name, key)
        assert float(t.abs().max()) == lim[name], (name, key)         # the range is used, not a corner of it
    p = case.p
    K = {"gemm": lambda: p["K"], "tn": lambda: p["K"], "conv": lambda: p["kh"] * p["kw"] * (p["c1"] + p["c2"]),
         "wgrad": lambda: p["b"] * p["oh"] * p["ow"]}[case.entry]()
    assert K <= 4608
    if case.epi is not None:
        assert case.epi.alpha in (1.0, 0.5, 0.25) and case.epi.out_scale in (1.0, 2.0)
    ref = T.reference(o)
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) * 8 < 2 ** 24
    if case.entry == "gemm" and case.epi is not None and case.epi.rows_per_img:
        # the last 32-row block of the last tile lies wholly beyond M, and the row bias has not one row to spare
        tile = 64 if case.form & T.L.TILE_KIND_MASK == T.FAST64 else 128
        assert -(-p["M"] // tile) * tile - p["M"] >= 32
        assert o.logical["rowbias"].shape[0] == -(-p["M"] // case.epi.rows_per_img)


@pytest.mark.parametrize("key", T.case_ids())
def test_reference_is_sensitive(key):
    """The reference of every case changes when the last four k are dropped, the two sources are swapped, the taps are
    transposed or the row bias is taken from the next image - a kernel that did any of it would not equal it."""
    case, o = T.CASES[key], T.operands(key)
    ref = T.reference(o)
    tried = 0
    for mut in T.MUTATIONS:
        if not T.applicable(case, mut):
            continue
        other = T.reference(o, mut)
        assert other.shape == ref.shape and not torch.equal(other, ref), (key, mut)
        assert int((other != ref).sum()) >= min(ref.shape[-1], 8), (key, mut)
        tried += 1
    assert tried >= 1


def test_every_mutation_is_exercised():
    for mut in T.MUTATIONS:
        for entry in {"drop_k4": ("gemm", "tn", "conv", "wgrad"), "swap_sources": ("conv",),
                      "transpose_taps": ("conv", "wgrad"), "shift_rowbias": ("gemm", "conv")}[mut]:
            assert any(T.applicable(c, mut) for c in T.CASES.values() if c.entry == entry), (mut, entry)


def test_split_plan_has_no_empty_range(ops):
    """psld_conv2d_plan over 12..160 K-steps and 1..256 tiles of 64 rows (a 1x1 convolution of 32 * ksteps channels on
    ``tiles`` 8x8 images, 64 output channels, a full workspace): a planned split never has an empty K range - the
    workgroups of one would stage K-step ``ksteps``, beyond the weight rows and, with one source, through the null second
    source.  The rule min(768 / tiles, 8, ksteps / 6) alone has exactly one such plan: 49 steps in 8 ranges of 7."""
    lib = ops.lib()
    ptr = 1 << 20                       # any aligned non-null address: the plan never dereferences
    holes = []
    for ksteps in range(12, 161):
        for tiles in range(1, 257):
            ns, kper = C.c_int(0), C.c_int(0)
            wsb = lib.psld_conv2d_workspace_bytes(tiles, 8, 8, 64)
            form = lib.psld_conv2d_plan(ptr, 32 * ksteps, None, 0, tiles, 8, 8, ptr, 64, 1, 1, 1, 0, 1, 8, 8, ptr, 64, None, ptr,
                                        wsb, C.byref(ns), C.byref(kper))
            rule = min(768 // tiles, 8, ksteps // 6)
            if tiles == 1:              # M = 64: never split, 64-row tiles need more than 64 rows
                assert (form, ns.value) == (T.FAST128 | T.V, 1)
                continue
            want_kind = T.SPLITK if ns.value > 1 else (T.FAST64 if _cdiv(tiles, 2) <= 256 else T.FAST128)
            assert form == want_kind | T.V, (ksteps, tiles, T.form_name(form))
            if rule >= 2 and (rule - 1) * _cdiv(ksteps, rule) >= ksteps:
                holes.append((ksteps, rule))
                assert ns.value == rule - 1, (ksteps, tiles, ns.value)
            else:
                assert ns.value == max(rule, 1), (ksteps, tiles, ns.value, rule)
            if ns.value > 1:
                assert kper.value == _cdiv(ksteps, ns.value) * 32
                assert (ns.value - 1) * _cdiv(ksteps, ns.value) < ksteps, (ksteps, tiles, ns.value)
    assert set(holes) == {(49, 8)}


def test_plans_refuse_what_the_launches_refuse(ops):
    lib = ops.lib()
    assert lib.psld_gemm_plan(0, 1, 8, 8, 0, 256, 8, 0, 256, 8, 0, 256, 8, 0, 1, None) == -1
    assert b"psld_gemm_f32" in lib.psld_last_error()
    assert lib.psld_gemm_tn_splitk_plan(8, 8, 8, 256, 8, 256, 8, 256, 0) == -1
    assert lib.psld_conv2d_wgrad_plan(None, 8, 8, 256, 8, 1, 8, 8, 3, 3, 1, 1, 8, 8, 256, 8, 0, 1) == -1
    assert lib.psld_conv2d_plan(256, 8, None, 4, 1, 8, 8, 256, 8, 3, 3, 1, 1, 1, 8, 8, 256, 8, None, None, 0, None, None) == -1

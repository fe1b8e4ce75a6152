"""``ops.pass_arith`` against the three booleans the executor used to derive from the four math settings, and the suffix
table that produces the derived weights' cache tags and batch families.  No GPU: the settings are host state of the library, the weights
are packed by a stand-in library (``_lib.set_proxy``) that records every call with a pointer argument and answers 0."""
import itertools

import pytest

from psld_amd import _lib
from tools import launch_trace as LT


@pytest.fixture()
def ops():
    from psld_amd import ops as o
    o.lib()
    return o


def test_pass_arith_is_the_three_booleans(ops):
    """All 48 combinations of math mode x record math x eval math x record f16 x record: the ladder is ('f16' if f16 or f16r) +
    ('x3' if x3) + ('x6'), () under 'f32' - x3, f16, f16r as _ExecBase.__init__ computed them before the ladder replaced them."""
    saved = ops.math_mode(), ops.record_math(), ops.eval_math(), ops.record_f16()
    seen = 0
    try:
        for mode, rmath, emath, rf16, record in itertools.product(ops.MATH_MODES, ("bf16x6", "bf16x3"), ops.EVAL_MATHS,
                                                                  (False, True), (False, True)):
            ops.set_math_mode(mode)
            ops.set_record_math(rmath)
            ops.set_eval_math(emath)
            ops.set_record_f16(rf16)
            split = mode in ("bf16x6", "bf16x3")
            x3 = (mode == "bf16x3" and not record) or (record and split and ops.record_math() == "bf16x3")
            f16 = split and not record and ops.eval_math() == "f16"
            f16r = record and split and ops.record_math() == "bf16x3" and ops.record_f16()
            want = ((("f16",) if f16 or f16r else ()) + (("x3",) if x3 else ()) + ("x6",)) if split else ()
            assert ops.pass_arith(record) == want, (mode, rmath, emath, rf16, record)
            assert not f16r or x3           # record f16 without record math 'bf16x3' has no effect
            seen += 1
    finally:
        ops.set_math_mode(saved[0])
        ops.set_record_math(saved[1])
        ops.set_eval_math(saved[2])
        ops.set_record_f16(saved[3])
    assert seen == 48


# cache tag -> (batch family, read by the replayed inference forward) of every derived weight that exists per arithmetic
_TAGS = {
    "x6": {"wfrag": ("wino", True), "dwfrag": ("wino", False), "fwd": ("limb", True), "dgrad": ("limb", False),
           "s2fwd": (None, True), "s2dgrad": (None, True), "qkv_f": ("limb", True), "qkv_d": ("limb", False),
           "qkv": ("qkv_bias", True)},
    "x3": {"wfrag_x3": ("wino_x3", True), "wfrag_d_x3": ("wino_x3", False), "fwd_x3": ("limb_x3", True),
           "dgrad_x3": ("limb_x3", False), "s2fwd_x3": (None, True), "s2dgrad_x3": (None, True),
           "qkv_set_x3": (None, False), "qkv_set_d_x3": (None, False), "qkv_f_x3": ("limb_x3", True),
           "qkv_d_x3": ("limb_x3", False)},
    "f16": {"wfrag_f16": ("wino_f16", True), "wfrag_d_f16": ("wino_f16", False), "fwd_f16": ("limb_f16", True),
            "dgrad_f16": ("limb_f16", False), "s2fwd_f16": (None, True), "s2dgrad_f16": (None, True),
            "qkv_set_f16": (None, False), "qkv_set_d_f16": (None, False), "qkv_f_f16": ("limb_f16", True),
            "qkv_d_f16": ("limb_f16", False)},
}


def test_cache_tags_and_families_per_arithmetic(ops, monkeypatch):
    """Every derived weight with a form per arithmetic, fetched the way the executor fetches it: the cache tags, batch families and
    ``graph`` flags are the literal ones above (tests and DESIGN.md name them; the batched refresh groups by family)."""
    import psld_amd
    from psld_amd import config as cfgs
    from psld_amd.registry import get_module
    from psld_amd.score_modules import AttnBlockpp, ResnetBlockBigGANpp
    from psld_amd.score_weights import PointwiseWeight
    for obj, attr, val in LT.patches():
        monkeypatch.setattr(obj, attr, val)
    psld_amd.import_modules_into_registry()
    rec = LT._Recorder(_lib.load_real())
    _lib.set_proxy(rec)
    try:
        net = get_module("score_fn", "ncsnpp")(cfgs.tiny(nf=128))
        net.flatten_parameters()
        assert sorted(net._wcache.families) == sorted(
            ["limb", "wino", "limb_x3", "wino_x3", "limb_f16", "wino_f16", "limb_tail", "qkv_bias", "temb"])
        block = next(m for m in net.all_modules if isinstance(m, ResnetBlockBigGANpp))
        attn = next(m for m in net.all_modules if isinstance(m, AttnBlockpp))
        conv2 = block.Conv_1        # any 3x3 weight of whole tiles stands for the pyramid's stride-2 convolution ("ohwi")
        c = attn.NIN_0.W.shape[0]
        co, ci = conv2.weight.shape[:2]
        for arith in ops.ARITHS:
            before = set(net._wcache.entries)
            weights = [PointwiseWeight(net, attn.NIN_3.W, c, c, "io"), PointwiseWeight(net, conv2, co, 9 * ci, "ohwi"),
                       PointwiseWeight(net, attn, 3 * c, c, "qkv", net._qkv_frags(attn))]
            for dgrad in (False, True):
                net._wfrag(block.Conv_0, dgrad, arith)
                for w in weights:
                    w.frag(dgrad, arith)
            got = {}
            for key in set(net._wcache.entries) - before:
                e = net._wcache.entries[key]
                assert got.setdefault(key[1], (e.family, e.graph)) == (e.family, e.graph), key[1]
            got.pop("pack", None)       # the OHWI copy the pyramid's fragments are packed from
            assert got == _TAGS[arith], arith
    finally:
        _lib.set_proxy(None)
    packers = {r[0] for r in rec.rows}
    assert {"psld_pack_conv3x3_wino", "psld_pack_conv3x3_wino_x3", "psld_pack_conv3x3_wino_dgrad_x3", "psld_pack_conv3x3_wino_f16",
            "psld_pack_conv3x3_wino_dgrad_f16", "psld_pack_gemm_frag", "psld_pack_gemm_frag_x3", "psld_pack_gemm_frag_f16",
            "psld_pack_frag_batch", "psld_pack_frag_batch_x3", "psld_pack_frag_batch_f16"} <= packers, sorted(packers)

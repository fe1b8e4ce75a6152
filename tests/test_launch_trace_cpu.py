"""The executor's launch sequence against the one recorded before its pointwise sites were gathered behind
``_ExecBase.pw_fwd`` / ``pw_dgrad`` / ``pw_wgrad``.

``tests/golden/launch_trace.json`` was written by ``python -m tools.launch_trace --write`` in a scratch checkout of commit
d13ebeb (the library built, ``tools/launch_trace.py`` copied in, no GPU: the executor is dry-run on CPU tensors against a
stand-in library that records every call with a pointer argument and forwards the host-side predicates).  Per case it keeps
the number of rows, the count per entry point and a SHA-256 of the rows of one eval forward followed by one recorded forward
+ backward of the same network (the second forward therefore packs no weight the first one packed).  A row pins the entry
point, every integer and float argument, every epilogue field, and for pointers into the flat parameter / gradient buffer
their element offset - which weight a launch reads, which gradient it writes.

The cases that set record math, eval math, record f16 and a loss divisor were added the same way from commit 2d67725, before
the executor's ``x3`` / ``f16`` / ``f16r`` booleans became ``ops.pass_arith``'s ladder; that run reproduced the digests of the
eight older cases.

A pull request that changes a launch on purpose regenerates the file and reviews ``--dump CASE`` against the parent's."""
import collections
import json

import pytest

from tools import launch_trace as LT

_ROWS = {}


def _rows(name, monkeypatch):
    if name not in _ROWS:
        from psld_amd import ops
        ops.lib()
        for obj, attr, val in LT.patches():
            monkeypatch.setattr(obj, attr, val)
        _ROWS[name] = LT.run_case(name, monkeypatch.setattr)
    return _ROWS[name]


@pytest.fixture(scope="module")
def golden():
    with open(LT.FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_the_cases(golden):
    assert list(golden) == list(LT.CASES)


@pytest.mark.parametrize("name", list(LT.CASES))
def test_launch_trace(name, golden, monkeypatch):
    got, want = LT.summary(*_rows(name, monkeypatch)), golden[name]
    assert got["eval_rows"] == want["eval_rows"] and got["rows"] == want["rows"]
    assert got["counts"] == want["counts"]
    assert got["sha256"] == want["sha256"], f"same launches, other arguments: python -m tools.launch_trace --dump {name}"


# entry point -> condition on its row (arguments from index 1, in the order of _lib.SIGNATURES); every one must occur
_NULL = [True, True]
_WANTED = {
    "psld_gemm_split_f32 (second source)": ("psld_gemm_split_f32", lambda r: r[3] != _NULL),
    "psld_gemm_split_tail_f32": ("psld_gemm_split_tail_f32", None),
    "psld_gemm_split_x3_f32": ("psld_gemm_split_x3_f32", None),
    "psld_gemm_tn_split_f32": ("psld_gemm_tn_split_f32", None),
    "psld_gemm_tn_split_tail_f32": ("psld_gemm_tn_split_tail_f32", None),
    "psld_gemm_tn_splitk_f32": ("psld_gemm_tn_splitk_f32", None),
    "psld_conv2d_nhwc_ws_f32 (kh = 1)": ("psld_conv2d_nhwc_ws_f32", lambda r: r[10] == 1),
    "psld_conv3x3_wino_f32": ("psld_conv3x3_wino_f32", None),
    "psld_conv3x3_wino_ws_f32": ("psld_conv3x3_wino_ws_f32", None),
    "psld_conv3x3_wino_gn_f32 / _ws": ("psld_conv3x3_wino_gn_f32 psld_conv3x3_wino_gn_ws_f32", None),
    "psld_conv3x3_wino_x3_f32": ("psld_conv3x3_wino_x3_f32", None),
    "psld_bgemm_split_f32": ("psld_bgemm_split_f32", None),
    "psld_attn_fwd_split_f32": ("psld_attn_fwd_split_f32", None),
    # record math 'bf16x3', eval math 'f16', record f16 (the *_f16s rows carry the operand shift)
    "psld_conv3x3_wino_f16_f32": ("psld_conv3x3_wino_f16_f32", None),
    "psld_conv3x3_wino_f16s_f32": ("psld_conv3x3_wino_f16s_f32", None),
    "psld_conv3x3_wino_gn_x3_f32": ("psld_conv3x3_wino_gn_x3_f32", None),
    "psld_conv3x3_wino_gn_f16_f32": ("psld_conv3x3_wino_gn_f16_f32", None),
    "psld_gemm_split_f16_f32": ("psld_gemm_split_f16_f32", None),
    "psld_gemm_split_f16s_f32": ("psld_gemm_split_f16s_f32", None),
    "psld_conv3x3_wgrad_wino_x3_f32": ("psld_conv3x3_wgrad_wino_x3_f32", None),
    "psld_pack_conv3x3_wino_dgrad_x3": ("psld_pack_conv3x3_wino_dgrad_x3", None),
    "psld_pack_conv3x3_wino_dgrad_f16": ("psld_pack_conv3x3_wino_dgrad_f16", None),
    "psld_pack_frag_batch_x3": ("psld_pack_frag_batch_x3", None),
    "psld_pack_frag_batch_f16": ("psld_pack_frag_batch_f16", None),
}


def test_cases_cover_the_dispatch(monkeypatch):
    """The union of the cases runs every pointwise form and both 3x3 front-end families: a condition on the case list
    (and so on the fixture), checked on the rows themselves."""
    by_name = collections.defaultdict(list)
    for name in LT.CASES:
        for row in sum(_rows(name, monkeypatch), []):
            by_name[row[0]].append(row)
    # the math modes, widths, pyramid forms, dropout and Winograd switches the case list must span
    specs = list(LT.CASES.values())
    assert {s[2] for s in specs} == {"f32", "bf16x6", "bf16x3"}
    assert {s[0]["nf"] for s in specs} >= {32, 128, 160}
    assert {s[3] for s in specs} == {"residual", "none"}
    assert any(s[4] > 0 for s in specs) and {s[5] for s in specs} >= {0, 2}
    assert {(s.record_math, s.eval_math, s.record_f16) for s in specs} >= {
        ("bf16x6", "limb", False), ("bf16x3", "limb", False), ("bf16x6", "f16", False), ("bf16x3", "limb", True),
        ("bf16x3", "f16", True)}
    assert {s.divisor for s in specs if s.record_f16} >= {196608, 1000}        # operand shifts 18 and 10
    missing = [what for what, (names, cond) in _WANTED.items()
               if not any(cond is None or cond(r) for n in names.split() for r in by_name[n])]
    assert not missing, missing

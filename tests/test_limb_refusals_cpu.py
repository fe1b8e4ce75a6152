"""The limb kernels' entry points refuse what they refused, in the same words, and their shape predicates answer what they
answered, before psld_amd/csrc/conv_split.hip put each kernel family's checks into one builder.

``tests/golden/limb_refusals.json`` (tools/limb_refusals.py, which documents the row format) was written at commit d6221a2.
It covers the twelve launching entry points that go through a builder - the two 3x3 forwards, the two 3x3 weight
gradients, the two ``gemm_tn`` forms, the three ``gemm_split`` forms and the three batched packers - with, where the entry
has such a check: a null required pointer, a null second source with ``c2`` / ``k2`` / ``n2`` > 0, unsupported shapes,
misaligned pointers, an ``nsplit`` that leaves empty slabs, ``ldy < n`` and a ``gn_part`` epilogue on the tail GEMM, short
row strides on the ``gemm_tn`` forms, and rows that break two checks at once (the first one speaks).  Every row is refused
with PSLD_ERR_ARG in front of the entry's first HIP runtime call.

The calls are made in a fresh child process that sees no device (``HIP_VISIBLE_DEVICES`` empty): a row that a broken
builder lets through then comes back as a launch error (status 2) instead of launching anything."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import GOLDEN, ROOT

ENTRIES = {"psld_conv3x3_split_f32", "psld_conv3x3_limb_f32", "psld_conv3x3_wgrad_split_f32", "psld_conv3x3_wgrad_xlimb_f32",
           "psld_gemm_tn_split_f32", "psld_gemm_tn_split_tail_f32", "psld_gemm_split_f32", "psld_gemm_split_x3_f32",
           "psld_gemm_split_tail_f32", "psld_pack_frag_batch", "psld_pack_frag_batch_x3", "psld_pack_frag_batch_tail"}


@pytest.fixture(scope="module")
def replayed():
    with open(os.path.join(GOLDEN, "limb_refusals.json")) as f:
        doc = json.load(f)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "tools.limb_refusals", "--replay"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return doc, json.loads(r.stdout)


def test_every_refusal_keeps_its_status_and_message(replayed):
    doc, got = replayed
    assert len(got["rows"]) == len(doc["rows"]) >= 150
    assert {r["entry"] for r in doc["rows"]} == ENTRIES
    for row, (status, error) in zip(doc["rows"], got["rows"]):
        assert row["status"] == 1, row                        # the fixture holds no answer that depends on the machine
        assert (status, error) == (row["status"], row["error"]), row


def test_the_fixture_covers_each_kind_of_refusal():
    with open(os.path.join(GOLDEN, "limb_refusals.json")) as f:
        rows = json.load(f)["rows"]
    said = {}
    for r in rows:
        said.setdefault(r["entry"], set()).add(r["error"].split(": ", 1)[1].split(" ")[0])
    for entry, words in said.items():
        if "pack_frag_batch" in entry:
            assert words == {"bad"}, (entry, words)
            continue
        assert words >= {"unsupported", "unaligned"} and words & {"null", "bad"}, (entry, words)
        if "wgrad" in entry or "gemm_tn" in entry:
            assert "nsplit" in words, (entry, words)
    assert {"ldy", "no"} <= said["psld_gemm_split_tail_f32"]                  # ldy < n; no GroupNorm partial sums
    for entry in ("psld_gemm_tn_split_f32", "psld_gemm_tn_split_tail_f32"):    # short row strides: aligned, too short
        assert any(r["entry"] == entry and "odd" not in r["args"] and r["args"][4] % 4 == 0 and r["args"][4] < r["args"][0]
                   for r in rows), entry                                      # args: m, n, k, a, lda, ...


def test_the_shape_predicates_answer_as_before(replayed):
    doc, got = replayed
    assert set(got["sweep"]) == set(doc["sweep"]) and len(doc["sweep"]) == 9
    for name, want in doc["sweep"].items():
        assert len(want) >= 256
        assert got["sweep"][name] == want, name
        if name.endswith("_supported"):
            assert "0" in want and "1" in want, name         # the grid discriminates

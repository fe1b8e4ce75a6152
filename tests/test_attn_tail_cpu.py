"""Attention at 480 channels without a GPU: what the two predicates answer, what psld_bgemm_split_tail_f32 refuses (in a
child process that sees no device), where score_routes.batched_route sends the attention block's batched products, and
the register / scratch report of the new kernel instances."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from psld_amd import ops
    return ops.lib()


def test_fused_attention_predicate(lib):
    f = lib.psld_attn_fwd_split_supported
    assert f(256, 480) == 1 and f(64, 480) == 1
    # as before: the widths with an instance, and the pairs tests/test_abi_cpu.py asks
    assert [f(hw, c) for hw in (256, 64) for c in (256, 128)] == [1, 1, 1, 1]
    assert f(1024, 256) == 0 and f(256, 64) == 0
    assert [f(hw, c) for hw, c in ((1024, 480), (256, 160), (256, 320), (64, 320), (64, 64), (128, 480))] == [0] * 6


def test_tail_predicate(lib):
    f, full = lib.psld_bgemm_split_tail_supported, lib.psld_bgemm_split_supported
    for ta, tb in ((0, 1), (0, 0), (1, 0)):
        for n in (160, 192, 480):
            for k in (32, 96, 256):
                assert f(ta, tb, 128, n, k) == 1 and f(ta, tb, 256, n, k) == 1 and full(ta, tb, 256, n, k) == 0
        assert f(ta, tb, 64, 480, 256) == 0
        assert f(ta, tb, 256, 96, 256) == 0
        assert f(ta, tb, 256, 256, 256) == 0 and full(ta, tb, 256, 256, 256) == 1     # the full-tile kernel's
        assert f(ta, tb, 256, 480, 48) == 0
        assert f(ta, tb, 256, 0, 32) == 0 and f(ta, tb, 0, 160, 32) == 0 and f(ta, tb, 128, 160, 0) == 0
    assert f(1, 1, 256, 480, 256) == 0
    # the full-tile predicate is what it was (test_bgemm_split pins m = 64 -> 0)
    assert full(0, 0, 64, 128, 32) == 0 and full(0, 0, 128, 160, 32) == 0 and full(1, 1, 128, 128, 32) == 0


_CHILD = """
import ctypes as C, json, sys
from tools.limb_refusals import _load_lib
mod, lib = _load_lib()
buf = (C.c_char * 256)()
ok = C.addressof(buf) + (-C.addressof(buf)) % 64          # never dereferenced: every row is refused on the host
ptr = {"null": None, "ok": ok, "odd": ok + 4}
out = []
for row in json.loads(sys.argv[1]):
    st = lib.psld_bgemm_split_tail_f32(*[ptr[a] if isinstance(a, str) else a for a in row])
    out.append([st, lib.psld_last_error().decode()])
print(json.dumps(out))
"""


def test_tail_launcher_refusals():
    """Null operand, odd pointer, lda = 2, an unsupported shape and a shape the full-tile kernel takes: status 1
    (PSLD_ERR_ARG) with the entry's name in psld_last_error(), in front of the first HIP call - the child process sees no
    device, so a row that slipped through would come back as a launch error (status 2)."""
    names = ["ta", "tb", "m", "n", "k", "a", "lda", "sa", "b", "ldb", "sb", "c", "ldc", "sc", "batch", "alpha", "stream"]
    base = dict(ta=0, tb=0, m=128, n=160, k=32, a="ok", lda=32, sa=128 * 32, b="ok", ldb=160, sb=32 * 160, c="ok", ldc=160,
                sc=128 * 160, batch=2, alpha=1.0, stream="null")
    changes = [dict(a="null"), dict(b="null"), dict(c="null"), dict(batch=0),
               dict(a="odd"), dict(b="odd"), dict(lda=2), dict(ldb=162), dict(sa=130), dict(sb=2),
               dict(m=64), dict(n=96), dict(n=176), dict(k=48), dict(ta=1, tb=1),
               dict(n=256, ldb=256, ldc=256), dict(n=128),                                  # psld_bgemm_split_f32's shapes
               dict(n=96, a="odd")]
    rows = [[dict(base, **ch)[n] for n in names] for ch in changes]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(rows)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert len(got) == len(changes)
    for ch, (status, error) in zip(changes, got):
        assert status == 1, (ch, status, error)
        assert error.startswith("psld_bgemm_split_tail_f32: "), (ch, error)
        if set(ch) & {"m", "n", "k", "ta"}:
            want = dict(base, **ch)
            assert "unsupported" in error and f"m={want['m']} n={want['n']} k={want['k']}" in error, (ch, error)


def test_batched_route():
    from psld_amd import ops, score_routes as R
    ops.lib()
    assert R.batched_route(True, 0, 0, 256, 480, 256) == R.LIMB_TAIL            # P V, dQ = dS K
    assert R.batched_route(True, 1, 0, 256, 480, 256) == R.LIMB_TAIL            # dV = P^T dO, dK = dS^T Q
    assert R.batched_route(True, 0, 1, 256, 256, 480) == R.LIMB                 # Q K^T, dP = dO V^T
    for ta, tb, n, k in ((0, 1, 64, 480), (0, 0, 480, 64), (1, 0, 480, 64), (0, 1, 64, 256), (0, 0, 256, 64), (0, 0, 128, 32)):
        assert R.batched_route(True, ta, tb, 64, n, k) == R.TILE                # the 8x8 level
    for args in ((0, 0, 256, 480, 256), (1, 0, 256, 480, 256), (0, 1, 256, 256, 480), (0, 1, 64, 64, 480), (0, 0, 1024, 256, 1024)):
        assert R.batched_route(False, *args) == R.TILE
    # what the launch trace's networks ask (hw = 64; hw = 1024 at c = 256) is answered as before
    assert R.batched_route(True, 0, 1, 1024, 1024, 256) == R.LIMB and R.batched_route(True, 0, 0, 1024, 256, 1024) == R.LIMB
    assert R.batched_route(True, 0, 0, 64, 320, 64) == R.TILE and R.batched_route(True, 0, 1, 64, 64, 320) == R.TILE


def _resource_report(source):
    src = os.path.join(ROOT, "psld_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "--offload-arch=gfx950", "-std=c++17", "-I../../include", "-I.",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", source, "-o", "/dev/null"],
                       cwd=src, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        out[b.split()[0]] = (scratch, [int(v) for v in re.findall(r"[SV]GPRs Spill: (\d+)", b)])
    return out


@pytest.mark.parametrize("source,pattern,at_least", [("attention.hip", r"attn_fwd_kernelILi\d+ELi480ELi\d+EEE", 2),
                                                     ("conv_split.hip", r"bgemm_kernelILb[01]ELb[01]ELb1EEE", 3)])
def test_new_instances_have_no_scratch(source, pattern, at_least):
    """Every attn_fwd_kernel instance with C = 480 and every bgemm_kernel TAIL instance: ScratchSize 0, no SGPR or VGPR
    spill."""
    seen = {name: v for name, v in _resource_report(source).items() if re.search(pattern, name)}
    assert len(seen) >= at_least, sorted(seen)
    for name, (scratch, spills) in seen.items():
        assert scratch == 0 and len(spills) == 2 and not any(spills), (name, scratch, spills)

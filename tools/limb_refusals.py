"""What the limb kernels' entry points refuse, and what their shape predicates answer: tests/golden/limb_refusals.json.

    python -m tools.limb_refusals --write      regenerate the golden file from the library in the tree
    python -m tools.limb_refusals --replay     make the golden file's calls again, print the answers as JSON

The file was written at commit d6221a2, before the entry points of psld_amd/csrc/conv_split.hip were put on one builder
per kernel family; tests/test_limb_refusals_cpu.py replays it in a child process without a device.  A pull request that
changes a check or a kernel's shape coverage on purpose regenerates it and reviews the diff.

Rows: ``{"entry", "args", "status", "error"}``.  ``args`` follows the entry's signature in psld_amd/_lib.py: numbers for the
scalars; for a pointer "null", "ok" (a 64-byte aligned host buffer that is never dereferenced) or "odd" (the same, 4 bytes
further: misaligned); for the epilogue "null" or an object of the ``psld_epilogue_t`` fields that differ from the neutral
epilogue (alpha = out_scale = 1, the rest 0 / null).  Every row is refused with status 1 (PSLD_ERR_ARG) by a check that
precedes the entry's first HIP runtime call - ``--write`` asserts it - so the answers do not depend on the machine.

Sweep: the pure predicates over channel widths 32 .. 512 in steps of 32, square maps of 8 .. 128 and batch 1 / 16, one
character per call ("0" / "1"; the two byte / item counts as lists) in the order of ``_sweep_calls``."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "limb_refusals.json")

WIDTHS = list(range(32, 513, 32))
MAPS = [8, 16, 32, 64, 128]
BATCHES = [1, 16]


def _load_lib():
    # psld_amd/_lib.py alone (ctypes only): the replay runs in a child process of a test and should start at once
    spec = importlib.util.spec_from_file_location("_psld_lib", os.path.join(ROOT, "psld_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load_real()


# ---- launching entry points -------------------------------------------------------------------------------------------
def _variants(entry, base, changes):
    """One row per change: the base call (which passes every check in front of the first HIP call) with some arguments replaced."""
    names = list(base)
    for ch in changes:
        assert set(ch) <= set(names), (entry, ch)
        yield {"entry": entry, "args": [ch.get(n, base[n]) for n in names]}


def cases():
    rows = []
    for entry in ("psld_conv3x3_split_f32", "psld_conv3x3_limb_f32"):
        base = dict(x1="ok", c1=128, x2="null", c2=0, batch=2, h=16, w=16, wfrag="ok", cout=128, y="ok", ldy=128, epi="null",
                    ws="null", ws_bytes=0, stream="null")
        rows += _variants(entry, base, [
            dict(x1="null"), dict(wfrag="null"), dict(y="null"), dict(c2=128),                     # null; null second source
            dict(c1=48), dict(cout=96), dict(cout=160), dict(w=12), dict(h=15, w=128), dict(h=6, w=8),
            dict(batch=0), dict(c2=-32), dict(c2=48, x2="ok"), dict(h=16, w=256),                    # unsupported shapes
            dict(x1="odd"), dict(x2="odd", c2=128), dict(wfrag="odd"),                             # misaligned
            dict(x1="null", c1=48, wfrag="odd"), dict(c1=48, x1="odd"),                            # the first failing check speaks
        ])
    for entry in ("psld_conv3x3_wgrad_split_f32", "psld_conv3x3_wgrad_xlimb_f32"):
        base = dict(dy="ok", lddy=128, cout=128, x="ok", cin=128, x2="null", cin2=0, batch=2, h=16, w=16, slabs="ok",
                    cin_total=128, col0=0, nsplit=2, stream="null")
        rows += _variants(entry, base, [
            dict(dy="null"), dict(x="null"), dict(slabs="null"), dict(nsplit=0), dict(cin2=-64), dict(cin2=64),
            dict(cout=96), dict(cin=32), dict(w=12), dict(h=3, w=8), dict(batch=0), dict(cin2=32, x2="ok"),
            dict(dy="odd"), dict(x="odd"), dict(x2="odd", cin2=64), dict(lddy=130),
            dict(nsplit=7), dict(nsplit=17), dict(nsplit=7, cout=64),                               # empty slabs (16 K tiles)
            dict(nsplit=7, dy="odd"), dict(cout=96, dy="odd", nsplit=0),
        ])
    base = dict(m=128, n=128, k=64, a="ok", lda=128, b="ok", ldb=128, b2="null", ldb2=0, n2=0, slabs="ok", ldc=128, nsplit=1,
                stream="null")
    rows += _variants("psld_gemm_tn_split_f32", base, [
        dict(a="null"), dict(b="null"), dict(slabs="null"), dict(nsplit=0), dict(n2=-128), dict(n2=128, ldc=256),
        dict(m=96), dict(m=160), dict(n=160), dict(k=48), dict(k=0), dict(n2=64, b2="ok", ldb2=64, ldc=192),
        dict(a="odd"), dict(b="odd"), dict(b2="odd", n2=128, ldb2=128, ldc=256), dict(lda=130), dict(ldb=130),
        dict(b2="ok", n2=128, ldb2=130, ldc=256),
        dict(lda=124), dict(ldb=124), dict(ldc=124), dict(b2="ok", n2=128, ldb2=128, ldc=128),    # short row strides
        dict(b2="ok", n2=128, ldb2=124, ldc=256),
        dict(nsplit=3), dict(nsplit=3, lda=124), dict(m=96, a="null"),
    ])
    base = dict(m=160, n=128, k=64, a="ok", lda=160, b="ok", ldb=128, slabs="ok", ldc=128, nsplit=1, stream="null")
    rows += _variants("psld_gemm_tn_split_tail_f32", base, [
        dict(a="null"), dict(b="null"), dict(slabs="null"), dict(nsplit=0),
        dict(m=128), dict(m=96), dict(n=144), dict(k=48), dict(m=256, n=256, lda=256, ldb=256, ldc=256),
        dict(a="odd"), dict(b="odd"), dict(lda=162), dict(ldb=130),
        dict(lda=156), dict(ldb=124), dict(ldc=124),
        dict(nsplit=3), dict(nsplit=3, ldc=124), dict(m=128, b="odd"),
    ])
    for entry, n in (("psld_gemm_split_f32", 128), ("psld_gemm_split_x3_f32", 256)):
        base = dict(a1="ok", k1=128, a2="null", k2=0, m=256, bfrag="ok", n=n, y="ok", ldy=n, epi="null")
        if entry == "psld_gemm_split_f32":
            base.update(ws="null", ws_bytes=0)
        base.update(stream="null")
        rows += _variants(entry, base, [
            dict(a1="null"), dict(bfrag="null"), dict(y="null"), dict(k2=64),
            dict(k1=96), dict(k1=48), dict(n=160), dict(n=384 if n == 256 else 96), dict(m=0), dict(k2=-64), dict(k2=32, a2="ok"),
            dict(a1="odd"), dict(a2="odd", k2=128), dict(bfrag="odd"),
            dict(k1=96, a1="odd"), dict(y="null", n=160),
        ])
    base = dict(a="ok", k=160, m=256, bfrag="ok", n=160, y="ok", ldy=160, epi="null", ws="null", ws_bytes=0, stream="null")
    rows += _variants("psld_gemm_split_tail_f32", base, [
        dict(a="null"), dict(bfrag="null"), dict(y="null"),
        dict(k=128, n=128), dict(k=96), dict(n=144), dict(n=96), dict(m=0), dict(k=256, n=256, ldy=256),
        dict(a="odd"), dict(bfrag="odd"),
        dict(ldy=128), dict(ldy=159),
        dict(epi={"gn_part": "ok", "gn_hw": 64}), dict(epi={"gn_part": "ok", "gn_hw": 64}, ldy=128),
        dict(epi={"gn_part": "ok", "gn_hw": 64}, a="odd"),
    ])
    for entry in ("psld_pack_frag_batch", "psld_pack_frag_batch_x3", "psld_pack_frag_batch_tail"):
        base = dict(table="ok", entries=1, total=256, stream="null")
        rows += _variants(entry, base, [dict(table="null"), dict(entries=0), dict(total=0), dict(entries=-1, total=-1)])
    return rows


class _Caller:
    def __init__(self):
        self.mod, self.lib = _load_lib()
        self.buf = C.create_string_buffer(4096 + 128)
        self.ok = (C.addressof(self.buf) + 63) & ~63

    def _ptr(self, v):
        return {"null": None, "ok": self.ok, "odd": self.ok + 4}[v]

    def __call__(self, row):
        _, argtypes = self.mod.SIGNATURES[row["entry"]]
        assert len(argtypes) == len(row["args"]), row
        args, keep = [], []
        for t, v in zip(argtypes, row["args"]):
            if t is self.mod.EP:
                if v == "null":
                    args.append(None)
                    continue
                e = self.mod.Epilogue(alpha=1.0, out_scale=1.0, rows_per_img=1)
                for k, f in v.items():
                    setattr(e, k, self._ptr(f) if isinstance(f, str) else f)
                keep.append(e)
                args.append(C.byref(e))
            else:
                args.append(self._ptr(v) if isinstance(v, str) else v)
        st = getattr(self.lib, row["entry"])(*args)
        return st, self.lib.psld_last_error().decode()


# ---- pure predicates ----------------------------------------------------------------------------------------------------
def _sweep_calls():
    """(predicate, argument tuples) in the order of the golden file's strings / lists."""
    shapes = [(b, hw) for hw in MAPS for b in BATCHES]
    yield "psld_conv3x3_split_supported", [(c1, c2, b, hw, hw, co) for c1 in WIDTHS for c2 in (0, c1) for co in WIDTHS
                                           for b, hw in shapes]
    yield "psld_conv3x3_wgrad_split_supported", [(co, ci, b, hw, hw) for co in WIDTHS for ci in WIDTHS for b, hw in shapes]
    for name in ("psld_gemm_split_supported", "psld_gemm_split_x3_supported"):
        yield name, [(k1, k2, b * hw * hw, n) for k1 in WIDTHS for k2 in (0, k1, 32) for n in WIDTHS for b, hw in shapes]
    yield "psld_gemm_tail_supported", [(k, b * hw * hw, n) for k in WIDTHS for n in WIDTHS for b, hw in shapes]
    for name in ("psld_gemm_tn_split_supported", "psld_gemm_tn_split_tail_supported"):
        yield name, [(m, n, b * hw * hw) for m in WIDTHS for n in WIDTHS for b, hw in shapes]
    yield "psld_gemm_frag_bytes_tail", [(n, k) for n in WIDTHS for k in WIDTHS]
    # a whole tensor; the first, a middle and the last tensor of a set of three along the rows and along K
    yield "psld_pack_frag_tail_items", [(n, n0, nt and 3 * n, k, c0 * (k // 32), ct and 3 * (k // 32))
                                        for n in WIDTHS for k in WIDTHS
                                        for n0, nt in ((0, 0), (0, 1), (n, 1), (2 * n, 1))
                                        for c0, ct in ((0, 0), (0, 1), (1, 1), (2, 1))]


def sweep(lib):
    out = {}
    for name, calls in _sweep_calls():
        got = [getattr(lib, name)(*a) for a in calls]
        out[name] = "".join(str(v) for v in got) if name.endswith("_supported") else got
    return out


def replay(doc):
    call = _Caller()
    return {"rows": [list(call(r)) for r in doc["rows"]], "sweep": sweep(call.lib)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", action="store_true")
    g.add_argument("--replay", action="store_true")
    args = ap.parse_args()
    os.environ["HIP_VISIBLE_DEVICES"] = ""      # no call here is meant to reach a device
    if args.replay:
        with open(GOLDEN) as f:
            json.dump(replay(json.load(f)), sys.stdout)
        return
    call = _Caller()
    rows = cases()
    for r in rows:
        r["status"], r["error"] = call(r)
        assert r["status"] == 1 and r["error"].startswith(r["entry"] + ": "), r      # PSLD_ERR_ARG, in front of any HIP call
    doc = {"widths": WIDTHS, "maps": MAPS, "batches": BATCHES, "rows": rows, "sweep": sweep(call.lib)}
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        for k in ("widths", "maps", "batches"):
            f.write(f' "{k}": {json.dumps(doc[k])},\n')
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ],\n")
        f.write(' "sweep": {\n' + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in doc["sweep"].items()) + "\n }\n}\n")
    print(f"{GOLDEN}: {len(rows)} rows, {sum(len(c) for _, c in _sweep_calls())} predicate calls")


if __name__ == "__main__":
    main()

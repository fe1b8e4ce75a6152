"""Launch trace of the score-network executor, dry-run on the CPU: every libpsld_hip call one eval forward and one recorded
forward + backward make, in order, with its arguments - what a refactor of the executor's dispatch must leave unchanged.

    python -m tools.launch_trace                 # rows and digest per case
    python -m tools.launch_trace --write         # (re)write tests/golden/launch_trace.json
    python -m tools.launch_trace --dump CASE     # the full rows of one case, one JSON list per line (diff two commits' dumps)

A stand-in library (``_lib.set_proxy``) forwards the calls whose signature has no pointer argument - the host-side predicates
and planners - to the built library, and records every other call and answers 0.  A row is the entry point's name and its
arguments read through ``_lib.SIGNATURES``: integers and floats as they are, an ``Epilogue`` field by field, a pointer into
the network's flat parameter buffer as ``["p", element offset]``, into the flat gradient buffer as ``["g", element offset]``,
any other pointer as ``[is null, address % 16 == 0]``.  The device job tables (``ops.TableCache``) hold raw pointers and are
not part of a row; their entry and item counts are.  No GPU is needed: the tensors are CPU tensors nobody reads.

tests/test_launch_trace_cpu.py compares the cases below against the fixture."""
import argparse
import collections
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_trace.json")

class Case(collections.namedtuple("Case", "tiny batch mode pin dropout wino record_math eval_math record_f16 divisor",
                                  defaults=("bf16x6", "limb", False, None))):
    """C.tiny arguments, batch, math mode, progressive_input, dropout, set_winograd mode; then record math, eval math, record
    f16 and the loss divisor published (``ops.set_loss_divisor``) right before the recorded backward (None: none)."""


_B16 = (dict(nf=128, image_size=64), 16)
CASES = {
    "nf160_bf16x6": Case(dict(nf=160), 2, "bf16x6", "residual", 0.0, None),
    "nf128_bf16x6": Case(dict(nf=128), 2, "bf16x6", "residual", 0.0, None),
    "nf32_f32": Case(dict(nf=32), 2, "f32", "residual", 0.0, None),
    "nf160_bf16x3": Case(dict(nf=160), 2, "bf16x3", "residual", 0.0, None),
    "nf128_none_dropout_wino0": Case(dict(nf=128), 2, "bf16x6", "none", 0.1, 0),
    "nf128_wino2": Case(dict(nf=128, ch_mult=(1, 1)), 2, "bf16x6", "residual", 0.0, 2),
    # full grids: the eight-wave two-limb GEMM (>= 128 tiles of 128 x 256), unsplit and GroupNorm-fused Winograd launches
    "nf128_64px_b16_bf16x3": Case(*_B16, "bf16x3", "residual", 0.0, None),
    "nf128_64px_b16_bf16x6": Case(*_B16, "bf16x6", "residual", 0.0, None),
    # record math / eval math / record f16: two-limb weight and data gradients; every fp16 launch and packer, the data gradients
    # with the shift of the published divisor; fp16 falling back straight to three limbs; a three-limb eval forward next to an
    # fp16 recording pass; the tail routes, three-limb under every setting
    "nf128_64px_b16_rec_x3": Case(*_B16, "bf16x3", "residual", 0.0, None, "bf16x3"),
    "nf128_64px_b16_f16_rec_f16": Case(*_B16, "bf16x3", "residual", 0.0, None, "bf16x3", "f16", True, 196608),
    "nf128_64px_b16_bf16x6_eval_f16": Case(*_B16, "bf16x6", "residual", 0.0, None, "bf16x6", "f16"),
    "nf128_64px_b16_bf16x6_rec_f16": Case(*_B16, "bf16x6", "residual", 0.0, None, "bf16x3", "limb", True, 1000),
    "nf160_f16_rec_f16": Case(dict(nf=160), 2, "bf16x3", "residual", 0.0, None, "bf16x3", "f16", True, 1000),
}


class _Stream:
    cuda_stream = 0


def patches():
    """(object, attribute, value) to set while a case runs (the test applies them with monkeypatch)."""
    import torch
    from psld_amd import ops
    return [(ops, "_chk", lambda t, dtype=None: t), (torch.cuda, "current_stream", lambda *a, **k: _Stream),
            (torch.cuda, "current_device", lambda: 0)]


class _Recorder:
    """Stand-in for the loaded library (see the module docstring)."""

    def __init__(self, real):
        from psld_amd import _lib
        self._real, self._sig = real, _lib.SIGNATURES
        self._ptr, self._epi = _lib.P, _lib.EP
        self.spans = []         # (tag, first byte, bytes) of the flat parameter / gradient buffers
        self.rows = []

    def _pointer(self, v):
        v = getattr(v, "value", v) or 0
        for tag, base, nbytes in self.spans:
            if base <= v < base + nbytes:
                return [tag, (v - base) // 4]
        return [v == 0, v % 16 == 0]

    def _value(self, ty, v):
        if ty is self._epi:
            if v is None:
                return None
            return [self._value(fty, getattr(v._obj, fname)) for fname, fty in v._obj._fields_]
        if ty is self._ptr:
            return self._pointer(v)
        v = getattr(v, "value", v)
        if ty in (C.c_float, C.c_double):
            return float(v)
        assert ty in (C.c_int, C.c_longlong, C.c_ulonglong), ty
        return int(v)

    def __getattr__(self, name):
        _, types = self._sig[name]
        fn = getattr(self._real, name)
        if not any(ty is self._ptr or ty is self._epi or hasattr(ty, "contents") for ty in types):
            return fn

        def recorded(*args):
            assert len(args) == len(types), name
            self.rows.append([name] + [self._value(ty, v) for ty, v in zip(types, args)])
            return 0
        return recorded


def run_case(name, patch=setattr):
    """The rows of case ``name``: (eval forward, recorded forward + backward).  ``patch(object, attribute, value)`` sets
    ``net.overlap_wgrad`` (the caller has applied ``patches()``); the four math settings, the published loss divisor and the
    Winograd switch are restored."""
    import torch
    import psld_amd
    from psld_amd import _lib, config as cfgs, ops
    from psld_amd.registry import get_module
    from psld_amd.score_exec import _Exec
    tiny, batch, mode, pin, dropout, wino, record_math, eval_math, record_f16, divisor = CASES[name]
    psld_amd.import_modules_into_registry()
    cfg = cfgs.tiny(**tiny)
    sf = cfg.model.score_fn
    sf.progressive_input, sf.dropout = pin, dropout
    rec = _Recorder(_lib.load_real())
    saved = ops.math_mode(), ops.record_math(), ops.eval_math(), ops.record_f16(), ops.loss_divisor()
    _lib.set_proxy(rec)
    try:
        ops.set_math_mode(mode)
        ops.set_record_math(record_math)
        ops.set_eval_math(eval_math)
        ops.set_record_f16(record_f16)
        ops.set_winograd(wino)
        torch.manual_seed(0)
        net = get_module("score_fn", "ncsnpp")(cfg)
        patch(net, "overlap_wgrad", False)
        flat, grad = net.flatten_parameters(), net.flat_grad()
        rec.spans = [("p", flat.data_ptr(), 4 * flat.numel()), ("g", grad.data_ptr(), 4 * grad.numel())]
        size = cfg.data.image_size
        x, t = torch.zeros(batch, sf.in_ch, size, size), torch.zeros(batch)
        with torch.no_grad():
            net.eval()
            _Exec(net, record=False).run(x, t)
            n_eval = len(rec.rows)
            net.train()
            ex = _Exec(net, record=True)
            y = ex.run(x, t)
            net._begin_backward()
            ops.set_loss_divisor(divisor)
            ex.backward(torch.zeros_like(y))
            net._end_backward()
    finally:
        ops.set_winograd(None)
        ops.set_math_mode(saved[0])
        ops.set_record_math(saved[1])
        ops.set_eval_math(saved[2])
        ops.set_record_f16(saved[3])
        ops.set_loss_divisor(saved[4])
        _lib.set_proxy(None)
    return rec.rows[:n_eval], rec.rows[n_eval:]


def summary(ev, tr):
    """What the fixture keeps of a case."""
    rows = ev + tr
    return {"eval_rows": len(ev), "rows": len(rows), "counts": dict(sorted(collections.Counter(r[0] for r in rows).items())),
            "sha256": hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="write tests/golden/launch_trace.json")
    ap.add_argument("--dump", metavar="CASE", help="print the rows of one case")
    args = ap.parse_args()
    from unittest import mock
    with contextlib.ExitStack() as stack:
        for obj, attr, val in patches():
            stack.enter_context(mock.patch.object(obj, attr, val))
        if args.dump:
            for row in sum(run_case(args.dump), []):
                print(json.dumps(row, separators=(",", ":")))
            return
        doc = {name: summary(*run_case(name)) for name in CASES}
    for name, s in doc.items():
        print(f"{name}: eval {s['eval_rows']} train {s['rows'] - s['eval_rows']} sha256 {s['sha256'][:16]}")
    if args.write:
        with open(FIXTURE, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print("wrote", FIXTURE)


if __name__ == "__main__":
    main()

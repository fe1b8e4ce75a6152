"""One case table for the fp32 MFMA tile engine (psld_amd/csrc/tile_engine.hip), shared by tests/test_tile_engine_cpu.py
(plans, coverage, sensitivity - no GPU) and tests/test_tile_engine_gpu.py (the launches).

A case = entry point + the launch's arguments + the form code the plan query must return for them (psld_*_plan: the host code
the launch itself selects its kernel with) + seeded operands.  ``Call`` builds the argument list ONCE and hands it either to
the launch wrapper of psld_amd.ops or to its ``*_plan`` twin, so what is planned is what is launched.

Operands are exact: A / x (and dy) integers in [-4, 4], B / w (and the weight gradient's x) in [-3, 3], drawn from a seeded
generator (no symmetry); bias, row bias, residual and the previous output integers in [-8, 8]; alpha and out_scale powers of
two.  With K <= 4608 every product, every partial sum (|sum| <= 12 * 4608 < 2^24) and every epilogue step is exact in fp32 in
ANY summation order, so a launch must reproduce the fp64 reference bit for bit - no tolerance.  Outputs go into NaN-filled
buffers; everything the launch may not write must still be NaN afterwards.  Storage the launch may not read (row padding
behind an ``ld``, the float in front of an offset base) is NaN too, so a stray read that reaches a result shows.
"""
import dataclasses
import functools
import math
from typing import Optional

import torch
import torch.nn.functional as F

from psld_amd import _lib as L

GENERIC, FAST128, FAST256, FAST64, SPLITK = (L.TILE_GENERIC, L.TILE_FAST128, L.TILE_FAST256, L.TILE_FAST64,
                                             L.TILE_FAST64_SPLITK)
AV, BV = L.TILE_A_VEC, L.TILE_B_VEC
V = AV | BV
KIND_NAMES = {GENERIC: "generic", FAST128: "fast128", FAST256: "fast256", FAST64: "fast64", SPLITK: "fast64+splitK"}
NAN = float("nan")


def form_name(form):
    if form < 0:
        return "refused"
    return KIND_NAMES[form & L.TILE_KIND_MASK] + "[A:%s B:%s]" % ("float4" if form & AV else "scalar",
                                                                  "float4" if form & BV else "scalar")


# every form an entry point can reach: (layout or '', form code).  The fast kernels need float4 operands (both flags); the
# generic kernel takes each operand either way.  128 x 256 tiles need a K-contiguous B (NT GEMM, convolution), 64-row tiles a
# K-contiguous A (the same two), TT has no fast kernel.
_GENERICS = [GENERIC, GENERIC | AV, GENERIC | BV, GENERIC | V]
ALL_FORMS = {
    "gemm": {(lay, f) for lay in ("NT", "NN", "TN", "TT") for f in _GENERICS}
            | {("NT", FAST64 | V), ("NT", FAST128 | V), ("NT", FAST256 | V), ("NN", FAST128 | V), ("TN", FAST128 | V)},
    # (two float4 operands always take the fast kernel here: any K, any map)
    "tn": {("", f) for f in [GENERIC, GENERIC | AV, GENERIC | BV, FAST128 | V]},
    "conv": {("", f) for f in _GENERICS + [FAST128 | V, FAST256 | V, FAST64 | V, SPLITK | V]},
    "wgrad": {("", f) for f in _GENERICS + [FAST128 | V]},
}
SPLIT_COUNTS = set(range(2, 9))          # every K-range count the split convolution can plan


@dataclasses.dataclass(frozen=True)
class Epi:
    """Epilogue of a case: value = ((alpha acc + bias[n] + rowbias[m // rows_per_img][n] + residual[m][n]) out_scale) (+ C)."""
    alpha: float = 1.0
    bias: bool = False
    rows_per_img: int = 0          # > 0: a row bias of ceil(M / rows_per_img) rows
    residual: bool = False
    res_pad: int = 0               # ld_residual = N + res_pad; GEMM: residual_stride_batch = M * ld_residual + 4 * res_pad
    out_scale: float = 1.0
    accumulate: bool = False
    bias_off: int = 0              # the bias starts this many floats into its buffer


FULL32 = Epi(0.5, True, 32, True, 4, 2.0, True)
FULL10 = Epi(0.25, True, 10, True, 4, 2.0, True)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    entry: str                     # gemm | tn | conv | wgrad
    p: dict                        # arguments (see the builders)
    form: int                      # expected plan
    nsplit: int = 1                # conv: expected K ranges
    epi: Optional[Epi] = None
    dense: bool = False            # also the shape of this form's dense random test

    @property
    def layout(self):
        return {(0, 1): "NT", (0, 0): "NN", (1, 0): "TN", (1, 1): "TT"}[(self.p["ta"], self.p["tb"])] if self.entry == "gemm" else ""

    def __str__(self):
        return f"{self.entry}:{self.name}"


CASES = {}


def _add(entry, name, form, p, **kw):
    c = Case(name, entry, p, form, **kw)
    assert str(c) not in CASES, str(c)
    CASES[str(c)] = c


def _gemm(name, lay, M, N, K, form, batch=1, **kw):
    ta, tb = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0), "TT": (1, 1)}[lay]
    extra = {k: kw.pop(k) for k in ("epi", "dense") if k in kw}
    _add("gemm", name, form, dict(ta=ta, tb=tb, M=M, N=N, K=K, batch=batch, **kw), **extra)


# ---- psld_gemm_f32 --------------------------------------------------------------------------------------------------------
# fast64 (NT, <= 256 tiles of 128 rows, M > 64)
_gemm("nt-fast64-65x132x32", "NT", 65, 132, 32, FAST64 | V, dense=True)
_gemm("nt-fast64-65x132x96", "NT", 65, 132, 96, FAST64 | V)
_gemm("nt-fast64-batch3-strided", "NT", 65, 132, 96, FAST64 | V, batch=3, lda=100, ldb=104, ldc=136, sa_pad=8, sb_pad=4, sc_pad=12)
# fast 128-row NT: M <= 64 (the time-embedding linears), or a grid above 256 tiles
_gemm("nt-fast128-m64", "NT", 64, 128, 64, FAST128 | V)
_gemm("nt-fast128-m5", "NT", 5, 128, 64, FAST128 | V)
_gemm("nt-fast128-261tiles", "NT", 384, 384, 64, FAST128 | V, batch=29, tiles=9, dense=True)     # 9 tiles per image: grid.x % 8 = 1
# 128 x 256 tiles: N % 256 == 0 and >= 512 of them
_gemm("nt-fast256-100x256x32-b512", "NT", 100, 256, 32, FAST256 | V, batch=512, dense=True)
_gemm("nt-fast256-1152x256x32-b57", "NT", 1152, 256, 32, FAST256 | V, batch=57)
# fast NN / TN at 1, 9 and 27 tiles per image (the XCD swizzle over grid.x), tails of 4 rows and 72 columns
for _lay in ("NN", "TN"):
    _gemm(f"{_lay.lower()}-fast128-1tile", _lay, 72, 72, 32, FAST128 | V, tiles=1)
    _gemm(f"{_lay.lower()}-fast128-9tiles", _lay, 260, 328, 64, FAST128 | V, tiles=9, dense=True)
    _gemm(f"{_lay.lower()}-fast128-27tiles", _lay, 1028, 328, 32, FAST128 | V, tiles=27)
# the cut-K call of the time-embedding data gradient (score_exec.py: dtp_all Wcat with the column offset as the batch stride)
_gemm("nn-fast128-colstride-batches", "NN", 4, 64, 64, FAST128 | V, batch=8, lda=512, sa=64, sc=4 * 64)
# the generic kernel, every layout: both operands float4 (K = 36; TN: K = 16 = batch, the time-embedding weight gradients;
# TT has no fast kernel at any K), then each operand scalar in turn - by an odd ld, by K % 4, by a base one float in, by a
# batch stride that is no multiple of 4
_gemm("nt-generic-k36", "NT", 130, 72, 36, GENERIC | V, dense=True)
_gemm("nt-generic-a-odd-ld", "NT", 70, 40, 36, GENERIC | BV, lda=37, dense=True)
_gemm("nt-generic-b-offset", "NT", 70, 40, 36, GENERIC | AV, b_off=1, dense=True)
_gemm("nt-generic-k54", "NT", 130, 72, 54, GENERIC, dense=True)
_gemm("nn-generic-k36", "NN", 130, 72, 36, GENERIC | V, dense=True)
_gemm("nn-generic-a-batch-stride", "NN", 70, 40, 32, GENERIC | BV, batch=2, sa_pad=2, dense=True)
_gemm("nn-generic-b-odd-ld", "NN", 70, 40, 32, GENERIC | AV, ldb=41, dense=True)
_gemm("nn-generic-a-offset-n6", "NN", 70, 6, 36, GENERIC, a_off=1, dense=True)
_gemm("tn-generic-k16", "TN", 132, 72, 16, GENERIC | V, dense=True)
_gemm("tn-generic-m6", "TN", 6, 72, 32, GENERIC | BV, batch=8, dense=True)
_gemm("tn-generic-b-offset", "TN", 132, 40, 32, GENERIC | AV, b_off=1, dense=True)
_gemm("tn-generic-odd-lds", "TN", 132, 40, 32, GENERIC, lda=133, ldb=41, dense=True)
_gemm("tt-generic-k64", "TT", 132, 72, 64, GENERIC | V, dense=True)
_gemm("tt-generic-k36", "TT", 132, 72, 36, GENERIC | V)
_gemm("tt-generic-a-offset", "TT", 132, 40, 32, GENERIC | BV, a_off=1, dense=True)
_gemm("tt-generic-k54", "TT", 132, 40, 54, GENERIC | AV, dense=True)
_gemm("tt-generic-b-odd-ld-a-batch-stride", "TT", 132, 40, 32, GENERIC, batch=2, sa_pad=2, ldb=33, dense=True)
# the whole epilogue on each fast form, once with rows_per_img = 32 (wave-uniform row bias) and once with 10; the last 32-row
# block of the last tile lies wholly beyond M (70 in 64-row tiles, 40 / 90 in 128-row tiles)
for _tag, _e in (("rpi32", FULL32), ("rpi10", FULL10)):
    _gemm(f"nt-fast64-epilogue-{_tag}", "NT", 70, 132, 32, FAST64 | V, batch=2, epi=_e)
    _gemm(f"nt-fast128-epilogue-{_tag}", "NT", 40, 132, 32, FAST128 | V, batch=2, epi=_e)
    _gemm(f"nt-fast256-epilogue-{_tag}", "NT", 90, 256, 32, FAST256 | V, batch=512, epi=_e)
    _gemm(f"nn-fast128-epilogue-{_tag}", "NN", 40, 132, 32, FAST128 | V, batch=2, epi=_e)
    _gemm(f"tn-fast128-epilogue-{_tag}", "TN", 40, 132, 32, FAST128 | V, batch=2, epi=_e)
_gemm("nt-generic-epilogue-rpi10", "NT", 70, 40, 36, GENERIC | V, batch=2, epi=FULL10)


# ---- psld_gemm_tn_splitk_f32 ------------------------------------------------------------------------------------------------
def _tn(name, M, N, K, nsplit, form, **kw):
    extra = {k: kw.pop(k) for k in ("dense",) if k in kw}
    _add("tn", name, form, dict(M=M, N=N, K=K, nsplit=nsplit, **kw), **extra)


_tn("fast-k100-3ranges", 64, 96, 100, 3, FAST128 | V, dense=True)      # ranges of 64: [0,64) [64,100) and an empty one
_tn("fast-k64-3ranges", 132, 72, 64, 3, FAST128 | V)                   # ranges of 32: the third is empty
_tn("generic-m14", 14, 40, 100, 3, GENERIC | BV, dense=True)
_tn("generic-n6", 72, 6, 64, 3, GENERIC | AV, dense=True)
_tn("generic-odd-lds", 72, 40, 100, 2, GENERIC, lda=73, ldb=41, dense=True)


# ---- psld_conv2d_nhwc_ws_f32 --------------------------------------------------------------------------------------------------
def _conv(name, b, ih, iw, c1, c2, co, k, form, stride=1, pad=None, tstride=1, oh=None, ow=None, nsplit=1, **kw):
    kh, kw_ = k if isinstance(k, tuple) else (k, k)
    pad = (kh // 2) if pad is None else pad
    if oh is None:
        oh, ow = (ih + 2 * pad - kh) // stride + 1, (iw + 2 * pad - kw_) // stride + 1
    extra = {n: kw.pop(n) for n in ("epi", "dense") if n in kw}
    _add("conv", name, form, dict(b=b, ih=ih, iw=iw, c1=c1, c2=c2, co=co, kh=kh, kw=kw_, stride=stride, pad=pad, tstride=tstride,
                                  oh=oh, ow=ow, **kw), nsplit=nsplit, **extra)


BIAS = Epi(bias=True)
_conv("generic-scalar-6+3", 2, 8, 8, 6, 3, 32, 3, GENERIC, epi=BIAS, dense=True)
_conv("generic-scalar-x-6+2", 2, 8, 8, 6, 2, 32, 3, GENERIC | BV, dense=True)                # K = 72: only the weights are float4
_conv("generic-scalar-w-offset", 2, 8, 8, 8, 0, 32, 3, GENERIC | AV, w_off=1, dense=True)
_conv("generic-float4-c8", 2, 9, 9, 8, 0, 36, 3, GENERIC | V, epi=BIAS, dense=True)
_conv("generic-float4-36+12", 2, 8, 8, 36, 12, 32, 3, GENERIC | V)
_conv("generic-float4-transposed-stride2", 2, 4, 4, 32, 0, 32, 3, GENERIC | V, pad=2, tstride=2, oh=9, ow=9)
_conv("generic-float4-6x6taps", 2, 8, 8, 32, 0, 32, 6, GENERIC | V, pad=2)                  # 36 taps > 31
_conv("fast128-264tiles", 33, 32, 32, 32, 0, 72, 3, FAST128 | V, epi=BIAS, dense=True)
_conv("fast256-64x64-1x1", 16, 64, 64, 32, 0, 256, 1, FAST256 | V, dense=True)
_conv("fast256-64x64-3x3", 16, 64, 64, 32, 0, 256, 3, FAST256 | V, epi=BIAS)
_conv("fast256-32x128-1x1", 16, 32, 128, 32, 0, 256, 1, FAST256 | V, epi=BIAS)
_conv("fast256-32x128-3x3", 16, 32, 128, 32, 0, 256, 3, FAST256 | V)
_conv("fast64-1x9x9", 1, 9, 9, 32, 0, 32, 3, FAST64 | V, epi=BIAS, dense=True)                # M = 81: a tail, one image
_conv("fast64-2x5x13", 2, 5, 13, 32, 0, 72, 3, FAST64 | V, epi=BIAS)                          # M = 130, non-square
_conv("fast64-stride2-17to8", 2, 17, 17, 32, 0, 32, 3, FAST64 | V, stride=2, pad=0)
_conv("fast64-epilogue", 2, 5, 13, 32, 0, 72, 3, FAST64 | V, epi=dataclasses.replace(FULL10, rows_per_img=65), ldy3=True)
_conv("splitk4-5x5taps", 2, 8, 8, 32, 0, 32, 5, SPLITK | V, nsplit=4, epi=BIAS)               # 25 K-steps
# split-K at every count 2..8 (M = 128: two 8x8 images): count = min(768 / tiles64, 8, ksteps / 6); the two sources meet
# inside a run of K-steps.  Plain (bias) and once each with the whole epilogue into the middle third of rows of 3 cout floats.
_SPLITS = [(2, (2, 2), 32, 96, 1), (3, 3, 32, 32, 1), (4, 3, 64, 32, 1), (6, 3, 32, 96, 1), (7, 3, 96, 64, 1), (8, 3, 96, 96, 1),
           (8, 3, 256, 256, 1)]
for _ns, _k, _c1, _c2, _ in _SPLITS:
    _conv(f"splitk{_ns}-{_c1}+{_c2}", 2, 8, 8, _c1, _c2, 64, _k, SPLITK | V, nsplit=_ns, epi=BIAS, pad=1 if _k == 3 else 0,
          dense=(_ns == 3))
_conv("splitk3-64+0", 2, 8, 8, 64, 0, 64, 3, SPLITK | V, nsplit=3, epi=BIAS)
_conv("splitk6-128+0", 2, 8, 8, 128, 0, 64, 3, SPLITK | V, nsplit=6)
_conv("splitk5-capped-by-tiles", 130, 8, 8, 32, 96, 32, 3, SPLITK | V, nsplit=5, epi=BIAS)      # 130 tiles of 64 rows: 768 / 130 = 5
for _ns, _k, _c1, _c2, _ in _SPLITS[:-1]:
    _conv(f"splitk{_ns}-epilogue", 2, 8, 8, _c1, _c2, 64, _k, SPLITK | V, nsplit=_ns, pad=1 if _k == 3 else 0,
          epi=FULL32 if _ns % 2 else dataclasses.replace(FULL10, rows_per_img=64), ldy3=True)
_conv("splitk5-epilogue", 130, 8, 8, 32, 96, 32, 3, SPLITK | V, nsplit=5, epi=FULL32, ldy3=True)
# 49 K-steps (a 1x1 convolution of 1568 channels): 8 ranges of 7 steps would leave the eighth empty - planned as 7 x 7
# (tests/test_tile_engine_cpu.py::test_split_plan_has_no_empty_range)
_conv("splitk7-1x1-49steps", 2, 8, 8, 1568, 0, 64, 1, SPLITK | V, nsplit=7, epi=BIAS)
# a bias that is not 16-byte aligned cannot go through the float4 reduction pass: planned unsplit, still exact
_conv("fast64-unaligned-bias-unsplit", 2, 8, 8, 32, 32, 64, 3, FAST64 | V, epi=Epi(bias=True, bias_off=1))


# ---- psld_conv2d_wgrad_nhwc_f32 -------------------------------------------------------------------------------------------------
def _wgrad(name, b, ih, iw, ci, co, k, nsplit, form, stride=1, pad=None, **kw):
    pad = (k // 2) if pad is None else pad
    oh, ow = (ih + 2 * pad - k) // stride + 1, (iw + 2 * pad - k) // stride + 1
    extra = {n: kw.pop(n) for n in ("dense",) if n in kw}
    _add("wgrad", name, form, dict(b=b, ih=ih, iw=iw, ci=ci, co=co, k=k, stride=stride, pad=pad, oh=oh, ow=ow, nsplit=nsplit, **kw),
         **extra)


_wgrad("fast-4x16-empty-range", 2, 4, 16, 32, 64, 3, 3, FAST128 | V, dense=True)      # K = 128 in ranges of 64: the third is empty; 27 workgroups
_wgrad("fast-5x4x8-short-range", 5, 4, 8, 32, 64, 3, 3, FAST128 | V)                  # K = 160: 64 + 64 + 32
_wgrad("fast-stride2-9to4", 4, 9, 9, 32, 32, 3, 2, FAST128 | V, stride=2, pad=0)
_wgrad("fast-1x1", 2, 8, 8, 32, 64, 1, 2, FAST128 | V)
_wgrad("fast-col0-of-96", 2, 8, 8, 32, 64, 3, 2, FAST128 | V, cin_total=96, col0=32)
_wgrad("fast-lddy", 2, 8, 8, 32, 64, 3, 2, FAST128 | V, lddy=68)
_wgrad("fast-132x36", 2, 8, 8, 36, 132, 3, 1, FAST128 | V, lddy=136, cin_total=40, col0=4)      # 2 tiles x 9 taps = 18 workgroups
_wgrad("generic-6x6", 2, 6, 6, 32, 64, 3, 2, GENERIC | V, dense=True)
_wgrad("generic-6x6-132x36", 2, 6, 6, 36, 132, 3, 3, GENERIC | V, lddy=136)
_wgrad("generic-cout6", 2, 8, 8, 32, 6, 3, 4, GENERIC | BV, dense=True)
_wgrad("generic-cin6", 2, 8, 8, 6, 64, 3, 2, GENERIC | AV, dense=True)
_wgrad("generic-6to14-stride2", 4, 9, 9, 6, 14, 3, 2, GENERIC, stride=2, pad=0, dense=True)


def case_ids(entry=None):
    return [k for k, c in CASES.items() if entry is None or c.entry == entry]


def dense_ids():
    return [k for k, c in CASES.items() if c.dense]


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).float()


def _store(logical, ld, stride, off, tail=0):
    """``logical`` [batch][rows][cols] laid out in a NaN-filled flat buffer: element (z, i, j) at off + z stride + i ld + j."""
    z, r, c = logical.shape
    n = off + max((z - 1) * stride + (r - 1) * ld + c, 0) + tail
    flat = torch.full((n,), NAN)
    flat.as_strided((z, r, c), (stride, ld, 1), off).copy_(logical)
    return flat


def _view(flat, shape, ld, stride, off):
    return flat.as_strided(tuple(shape), (stride, ld, 1), off)


def _seed(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(str(case))) % (2 ** 31)


class Operands:
    """The CPU tensors of a case: ``t`` name -> flat fp32 storage (what the launch is handed, NaN where it may not read),
    ``logical`` name -> the dense values, ``fill`` (dense random test) chooses integers or randn."""

    def __init__(self, case, dense=False):
        self.case, self.dense = case, dense
        self.g = torch.Generator().manual_seed(_seed(case) + (7 if dense else 0))
        self.t, self.logical, self.meta = {}, {}, {}
        getattr(self, "_" + case.entry)()
        self._epilogue()

    def draw(self, shape, lim):
        return torch.randn(tuple(shape), generator=self.g) if self.dense else _ints(self.g, shape, lim)

    # -- gemm: A [batch][M][K] or [K][M]; B [batch][K][N] or [N][K]
    def _gemm(self):
        p = self.case.p
        M, N, K, z = p["M"], p["N"], p["K"], p["batch"]
        ashape, bshape = ((K, M) if p["ta"] else (M, K)), ((N, K) if p["tb"] else (K, N))
        m = self.meta
        m["lda"], m["ldb"], m["ldc"] = p.get("lda", ashape[1]), p.get("ldb", bshape[1]), p.get("ldc", N)
        m["sa"] = p.get("sa", ashape[0] * m["lda"] + p.get("sa_pad", 0))
        m["sb"] = p.get("sb", bshape[0] * m["ldb"] + p.get("sb_pad", 0))
        m["sc"] = p.get("sc", M * m["ldc"] + p.get("sc_pad", 0))
        m["a_off"], m["b_off"] = p.get("a_off", 0), p.get("b_off", 0)
        A, B = self.draw((z,) + ashape, 4), self.draw((z,) + bshape, 3)
        self.logical.update(A=A, B=B)
        self.t["A"] = _store(A, m["lda"], m["sa"], m["a_off"])
        self.t["B"] = _store(B, m["ldb"], m["sb"], m["b_off"])
        m["out_shape"], m["rows"], m["cols"] = (z, M, N), M, N

    def _tn(self):
        p = self.case.p
        M, N, K = p["M"], p["N"], p["K"]
        m = self.meta
        m["lda"], m["ldb"] = p.get("lda", M), p.get("ldb", N)
        A, B = self.draw((1, K, M), 4), self.draw((1, K, N), 3)
        self.logical.update(A=A[0], B=B[0])
        self.t["A"] = _store(A, m["lda"], 0, 0)
        self.t["B"] = _store(B, m["ldb"], 0, 0)

    def _conv(self):
        p = self.case.p
        ct = p["c1"] + p["c2"]
        x1 = self.draw((p["b"], p["ih"], p["iw"], p["c1"]), 4)
        self.logical["x1"] = self.t["x1"] = x1
        if p["c2"]:
            self.logical["x2"] = self.t["x2"] = self.draw((p["b"], p["ih"], p["iw"], p["c2"]), 4)
        w = self.draw((p["co"], p["kh"], p["kw"], ct), 3)
        if self.dense:
            w = w / math.sqrt(p["kh"] * p["kw"] * ct)
        self.logical["w"] = w
        off = p.get("w_off", 0)
        self.t["w"] = _store(w.reshape(1, 1, -1), w.numel(), 0, off)
        self.meta.update(rows=p["b"] * p["oh"] * p["ow"], cols=p["co"])

    def _wgrad(self):
        p = self.case.p
        dy = self.draw((1, p["b"] * p["oh"] * p["ow"], p["co"]), 4)
        self.logical["dy"] = dy[0]
        self.meta["lddy"] = p.get("lddy", p["co"])
        self.t["dy"] = _store(dy, self.meta["lddy"], 0, 0, tail=self.meta["lddy"] - p["co"])
        self.logical["x"] = self.t["x"] = self.draw((p["b"], p["ih"], p["iw"], p["ci"]), 3)

    def _epilogue(self):
        e, m = self.case.epi, self.meta
        if e is None or self.dense:
            return
        M, N = m["rows"], m["cols"]
        z = self.case.p.get("batch", 1)
        if e.bias:
            b = _ints(self.g, (N,), 8)
            self.logical["bias"] = b
            self.t["bias"] = _store(b.reshape(1, 1, N), N, 0, e.bias_off)
        if e.rows_per_img:
            self.logical["rowbias"] = self.t["rowbias"] = _ints(self.g, (-(-M // e.rows_per_img), N), 8)
        if e.residual:
            r = _ints(self.g, (z, M, N), 8)
            self.logical["res"] = r
            m["ldres"] = N + e.res_pad
            m["sres"] = M * m["ldres"] + 4 * e.res_pad
            self.t["res"] = _store(r, m["ldres"], m["sres"], 0)
        if e.accumulate:
            self.logical["prev"] = _ints(self.g, (z, M, N), 8)


@functools.lru_cache(maxsize=4)
def operands(key, dense=False):
    return Operands(CASES[key], dense)


# ---------------------------------------------------------------------------------------------------------------------------------
# references (fp64, plain torch on the logical values)
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_k4", "swap_sources", "transpose_taps", "shift_rowbias")


def applicable(case, mutation):
    p = case.p
    if mutation == "drop_k4":
        return True
    if mutation == "swap_sources":
        return case.entry == "conv" and p["c2"] > 0
    if mutation == "transpose_taps":
        return (case.entry == "conv" and p["kh"] == p["kw"] > 1) or (case.entry == "wgrad" and p["k"] > 1)
    return case.epi is not None and case.epi.rows_per_img > 0 and case.entry in ("gemm", "conv")


def _apply_epilogue(acc, ops_, e, mutation):
    """acc [z][M][N] fp64 -> the stored value."""
    if e is None or ops_.dense:
        return acc
    lg = ops_.logical
    x = acc * e.alpha
    if e.bias:
        x = x + lg["bias"].double()
    if e.rows_per_img:
        rb = lg["rowbias"].double()
        idx = torch.arange(acc.shape[1]) // e.rows_per_img
        if mutation == "shift_rowbias":
            idx = (idx + 1) % rb.shape[0]
        x = x + rb[idx][None]
    if e.residual:
        x = x + lg["res"].double()
    x = x * e.out_scale
    if e.accumulate:
        x = x + lg["prev"].double()
    return x


def _im2col(x, p, kh, kw, transpose_taps=False):
    """NHWC fp64 [b][ih][iw][c] -> [b oh ow][kh kw][c]: the rows of the implicit GEMM (zero outside the image; a transposed
    stride s reads input pixel (oy + ky - pad) / s where that is whole)."""
    b, ih, iw, c = x.shape
    s, pad, ts = p["stride"], p["pad"], p.get("tstride", 1)
    xn = x.permute(0, 3, 1, 2)
    if ts > 1:
        up = torch.zeros(b, c, ih * ts, iw * ts, dtype=x.dtype)
        up[:, :, ::ts, ::ts] = xn
        xn = up
    oh, ow = p["oh"], p["ow"]
    # pad far enough for every window the launch asks for, then crop to [oh][ow]
    need_h, need_w = (oh - 1) * s + kh, (ow - 1) * s + kw
    xn = F.pad(xn, (pad, max(0, need_w - pad - xn.shape[3]), pad, max(0, need_h - pad - xn.shape[2])))
    cols = F.unfold(xn, (kh, kw), stride=s)                          # [b][c kh kw][positions]
    nh, nw = (xn.shape[2] - kh) // s + 1, (xn.shape[3] - kw) // s + 1
    cols = cols.reshape(b, c, kh, kw, nh, nw)[:, :, :, :, :oh, :ow]
    if transpose_taps:
        cols = cols.transpose(2, 3)
    return cols.permute(0, 4, 5, 2, 3, 1).reshape(b * oh * ow, kh * kw, c)


def _ranges(K, nsplit):
    kper = -(-(-(-K // nsplit)) // 32) * 32
    return [(min(K, s * kper), min(K, (s + 1) * kper)) for s in range(nsplit)]


def reference(ops_, mutation=None):
    """fp64 expected values of the region the launch writes: gemm [z][M][N]; tn [nsplit][M][N]; conv [b oh ow][co];
    wgrad [nsplit][co][taps][ci]."""
    case, lg = ops_.case, ops_.logical
    p = case.p
    assert mutation is None or applicable(case, mutation)
    if case.entry == "gemm":
        A, B = lg["A"].double(), lg["B"].double()
        A = A.transpose(1, 2) if p["ta"] else A                    # [z][M][K]
        B = B.transpose(1, 2) if p["tb"] else B                    # [z][K][N]
        if mutation == "drop_k4":
            A = A[:, :, :-4]
            B = B[:, :-4]
        return _apply_epilogue(A @ B, ops_, case.epi, mutation)
    if case.entry == "tn":
        A, B = lg["A"].double(), lg["B"].double()
        if mutation == "drop_k4":
            A = A.clone()
            A[-4:] = 0
        return torch.stack([A[a:b].t() @ B[a:b] for a, b in _ranges(p["K"], p["nsplit"])])
    if case.entry == "conv":
        x = lg["x1"].double()
        if p["c2"]:
            x = torch.cat([lg["x2"].double(), x] if mutation == "swap_sources" else [x, lg["x2"].double()], dim=-1)
        cols = _im2col(x, p, p["kh"], p["kw"], mutation == "transpose_taps")
        w = lg["w"].double().reshape(p["co"], -1)
        cols = cols.reshape(cols.shape[0], -1)
        if mutation == "drop_k4":
            cols, w = cols[:, :-4], w[:, :-4]
        return _apply_epilogue((cols @ w.t())[None], ops_, case.epi, mutation)[0]
    x, dy = lg["x"].double(), lg["dy"].double()
    cols = _im2col(x, p, p["k"], p["k"], mutation == "transpose_taps")      # [K][taps][ci]
    if mutation == "drop_k4":
        dy = dy.clone()
        dy[-4:] = 0
    cols = cols.reshape(cols.shape[0], -1)
    out = [dy[a:b].t() @ cols[a:b] for a, b in _ranges(dy.shape[0], p["nsplit"])]
    return torch.stack(out).reshape(p["nsplit"], p["co"], p["k"] * p["k"], p["ci"])


def yardstick32(ops_):
    """The same contraction in fp32, accumulated sequentially in k order (one rounded product added per k, as the kernel's
    chain of one fmaf per k; not a blocked sum) - the dense test's yardstick.  Layout of ``reference``."""
    case, lg = ops_.case, ops_.logical
    p = case.p

    def chain(At, Bt):                         # At [z][M][K], Bt [z][K][N] fp32
        acc = torch.zeros(At.shape[0], At.shape[1], Bt.shape[2])
        for k in range(At.shape[2]):
            acc += At[:, :, k:k + 1] * Bt[:, k:k + 1, :]
        return acc

    if case.entry == "gemm":
        A, B = lg["A"], lg["B"]
        return chain(A.transpose(1, 2) if p["ta"] else A, B.transpose(1, 2) if p["tb"] else B)
    if case.entry == "tn":
        return torch.stack([chain(lg["A"][a:b].t()[None], lg["B"][a:b][None])[0] if b > a else
                            torch.zeros(p["M"], p["N"]) for a, b in _ranges(p["K"], p["nsplit"])])
    if case.entry == "conv":
        x = torch.cat([lg["x1"], lg["x2"]], dim=-1) if p["c2"] else lg["x1"]
        cols = _im2col(x, p, p["kh"], p["kw"]).reshape(ops_.meta["rows"], -1)
        return chain(cols[None], lg["w"].reshape(p["co"], -1).t()[None])[0]
    cols = _im2col(lg["x"], p, p["k"], p["k"])
    cols = cols.reshape(cols.shape[0], -1)
    out = [chain(lg["dy"][a:b].t()[None], cols[a:b][None])[0] if b > a else torch.zeros(p["co"], cols.shape[1])
           for a, b in _ranges(cols.shape[0], p["nsplit"])]
    return torch.stack(out).reshape(p["nsplit"], p["co"], p["k"] * p["k"], p["ci"])


# ---------------------------------------------------------------------------------------------------------------------------------
# one argument list for the launch and for its plan
# ---------------------------------------------------------------------------------------------------------------------------------
class Call:
    """The tensors of a case on ``device`` and the argument list of its launch.  ``pool`` (tests/guard.GuardPool, GPU
    only): the row bias comes from it - exactly its ceil(M / rows_per_img) rows between two bands of NaN bytes."""

    def __init__(self, ops, ops_, device="cpu", pool=None):
        self.ops, self.o, self.case = ops, ops_, ops_.case
        self.d = {k: v.to(device) for k, v in ops_.t.items()}
        if pool is not None and "rowbias" in self.d:
            self.d["rowbias"] = pool.take_like(self.d["rowbias"], "rowbias")
        self.device = device
        getattr(self, "_" + self.case.entry)()

    def _epi(self, batched):
        e, m, d = self.case.epi, self.o.meta, self.d
        if e is None or self.o.dense:
            return None
        return self.ops.epilogue(alpha=e.alpha, bias=d["bias"][e.bias_off:] if e.bias else None, rowbias=d.get("rowbias"),
                                 rows_per_img=e.rows_per_img or 1, residual=d.get("res"), ld_residual=m.get("ldres", 0),
                                 residual_stride_batch=m.get("sres", 0) if batched else 0, out_scale=e.out_scale,
                                 accumulate=e.accumulate)

    def _out(self, shape, ld, stride, off, total):
        """NaN-filled flat output of ``total`` floats holding the previous output (accumulate) in the written region."""
        out = torch.full((total,), NAN)
        if "prev" in self.o.logical:
            _view(out, shape, ld, stride, off).copy_(self.o.logical["prev"].reshape(shape))
        self.out_cpu_init = out
        self.out = out.to(self.device)
        self.region = (tuple(shape), ld, stride, off)

    def _gemm(self):
        p, m = self.case.p, self.o.meta
        z, M, N = m["out_shape"]
        self._out((z, M, N), m["ldc"], m["sc"], 0, (z - 1) * m["sc"] + M * m["ldc"])
        self.args = (p["ta"], p["tb"], M, N, p["K"], self.d["A"], m["lda"], m["sa"], self.d["B"], m["ldb"], m["sb"], self.out,
                     m["ldc"], m["sc"], z, self._epi(True), m["a_off"], m["b_off"], 0)
        self.fns = (self.ops.gemm_raw, self.ops.gemm_plan)

    def _tn(self):
        p, m = self.case.p, self.o.meta
        self._out((p["nsplit"], p["M"], p["N"]), p["N"], p["M"] * p["N"], 0, p["nsplit"] * p["M"] * p["N"])
        self.args = (p["M"], p["N"], p["K"], self.d["A"], m["lda"], self.d["B"], m["ldb"], self.out, p["nsplit"])
        self.fns = (self.ops.gemm_tn_splitk, self.ops.gemm_tn_splitk_plan)

    def _conv(self):
        p, m = self.case.p, self.o.meta
        M, co = m["rows"], p["co"]
        ldy, off = (3 * co, co) if p.get("ldy3") else (co, 0)
        self._out((1, M, co), ldy, 0, off, M * ldy)
        self.args = (self.d["x1"], self.d.get("x2"), self.d["w"][p.get("w_off", 0):], co, p["kh"], p["kw"], p["stride"], p["pad"],
                     p["tstride"], p["oh"], p["ow"], self.out[off:], self._epi(False), ldy)
        self.fns = (self.ops.conv2d_nhwc, self.ops.conv2d_plan)

    def _wgrad(self):
        p, m = self.case.p, self.o.meta
        taps, ct, col0 = p["k"] * p["k"], p.get("cin_total", p["ci"]), p.get("col0", 0)
        self._out((p["nsplit"] * p["co"] * taps, 1, p["ci"]), 0, ct, col0, p["nsplit"] * p["co"] * taps * ct)
        self.args = (self.d["dy"], p["co"], self.d["x"], p["k"], p["k"], p["stride"], p["pad"], p["oh"], p["ow"], self.out, ct, col0,
                     p["nsplit"], m["lddy"])
        self.fns = (self.ops.conv2d_wgrad_nhwc, self.ops.conv2d_wgrad_plan)

    def plan(self):
        """(form code, K ranges) the library plans for exactly the arguments ``launch`` passes."""
        r = self.fns[1](*self.args)
        return (r[0], r[1]) if isinstance(r, tuple) else (r, 1)

    def launch(self):
        self.fns[0](*self.args)
        return self.out

    def written(self, out):
        """The region the launch writes, as a view of ``out`` shaped like ``reference``'s result."""
        shape, ld, stride, off = self.region
        if self.case.entry == "wgrad":
            return _view(out, shape, stride, stride, off)        # rows of cin_total floats, columns [col0, col0 + ci)
        return _view(out, shape, ld, stride, off)

    def outside_mask(self):
        """bool [total]: the floats of the output buffer the launch must leave alone."""
        mask = torch.ones(self.out_cpu_init.numel(), dtype=torch.bool)
        self.written(mask).fill_(False)
        return mask


def explain(case, form, y, want, limit=4):
    """None when ``y`` equals ``want`` (same shape) bit for bit; else the failure message: case, form, how many elements
    differ and the first coordinates with both values."""
    bad = ~(y == want)
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()
    lines = [f"{case} [{form_name(form)}]: {len(idx)} of {y.numel()} elements differ from the fp64 reference"]
    for i in idx[:limit]:
        i = tuple(int(v) for v in i)
        lines.append(f"  at {i}: got {float(y[i])!r}, want {float(want[i])!r}")
    return "\n".join(lines)

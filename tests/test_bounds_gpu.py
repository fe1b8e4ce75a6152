"""Guard-band tests: no kernel reads or writes outside its documented buffers.

Every case calls an ``ops.*`` wrapper twice through tests/guard.py:run_guarded - on ordinary buffers and on buffers of
EXACTLY the documented size that lie between bands of 0xFF bytes (NaN as fp32 / fp64 / bf16) - and asserts that the ordinary
outputs are finite, that the guarded outputs equal them bit for bit, that no input changed and that no band byte changed.
The workspace (``ops.workspace``) has exactly the bytes the sizing function returns (no 1 MiB floor) and the outputs the
wrappers allocate themselves come from the pool as well.  The oracle is "the same call on ordinary buffers"; the wrappers
that had no direct kernel test before (em_step, sscs_*, reverse_sde_rows, lincomb, scaled_norm_sq, vp_*, copy2d,
scale_copy2d, copy_batch, im2col3x3_small, linear) also get a short fp64 reference at the tolerance of their class in
test_kernels_gpu.py (1e-12 f64 SDE math, 1e-6 elementwise fp32, 2e-6 fp32 contractions).

Limits: a read outside a buffer that never reaches a result is not seen; bands are 1 MiB (64 KiB around arena slices);
buffer starts are 256-byte aligned.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import guard as G
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_kernels_gpu import gen, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 1 << 30)
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.fixture
def guard(ops, pool, monkeypatch):
    if pool.regions:
        pool.check()
        pool.release()
    return G.Guard(ops, pool).install(monkeypatch)


def D(t):
    return t.to(DEV)


def R(*shape, seed, scale=1.0):
    return gen(*shape, seed=seed, scale=scale).to(DEV)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the harness itself
# ---------------------------------------------------------------------------------------------------------------------
def test_harness_detects_a_write_and_a_read_past_a_buffer(ops, guard):
    """One element written past a guarded view (through a wider torch view of the pool): check() fails.  A torch reduction
    over a wider view: the result turns NaN and (b) fails.  A clean op passes.  Without this the rest proves nothing."""
    pool = guard.pool
    x = R(1000, seed=1)

    def wider(t, extra):
        off = t.data_ptr() - pool.buf.data_ptr()
        return pool.buf[off:off + (t.numel() + extra) * 4].view(torch.float32)

    def clean(x, y):
        ops.axpby(x, 2.0, None, 0.0, y)
    G.run_guarded(guard, clean, dict(x=x, y=nan(1000)), ["y"])

    def writes_past(x, y):
        ops.axpby(x, 2.0, None, 0.0, y)
        if guard.active:
            wider(y, 1)[-1] = 0.0
    with pytest.raises(G.GuardViolation, match="0 bytes past the end of 'y'"):
        G.run_guarded(guard, writes_past, dict(x=x, y=nan(1000)), ["y"])

    seen = {}

    def reads_past(x, y):
        src = wider(x, 1) if guard.active else torch.cat([x, x.new_zeros(1)])
        y.copy_(src.sum().reshape(1))
        seen[guard.active] = y.clone()
    with pytest.raises(G.GuardViolation, match=r"\(b\) output 'y' differs"):
        G.run_guarded(guard, reads_past, dict(x=x, y=nan(1)), ["y"])
    assert bool(torch.isnan(seen[True]).all()) and bool(torch.isfinite(seen[False]).all())
    # the guarded workspace: exactly the bytes asked for, fresh on every call
    with guard:
        w1, w2 = ops.workspace(100, torch.device(DEV, 0)), ops.workspace(100, torch.device(DEV, 0))
    assert w1.numel() == 100 and w2.numel() == 100 and w1.data_ptr() != w2.data_ptr() and w1.data_ptr() % 256 == 0
    assert ops.workspace(100, torch.device(DEV, 0)).numel() >= 1 << 20
    pool.check()


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return reg


def spec(fn, tensors, outputs=(), check=None, min_ws=0):
    """``min_ws``: guarded ops.workspace calls the case must make (a case about a workspace proves nothing without one)."""
    return dict(fn=fn, tensors=tensors, outputs=outputs, check=check, min_ws=min_ws)


# ---- packers ---------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(128, 128), (256, 512), (160, 320)]


def _pack_cases():
    for co, ci in PACK_SHAPES:
        for kind in ("conv3x3_frag", "conv3x3_frag_dgrad", "wino_frag", "wino_frag_dgrad", "wino_frag_x3", "gemm_frag", "gemm_frag_x3"):
            direct = kind.startswith("conv3x3_frag") or kind.startswith("gemm")
            n_out = ci if kind.endswith("dgrad") else co
            if direct and n_out % 128:        # the direct limb packers take whole 128-channel tiles only
                continue

            def build(ops, co=co, ci=ci, kind=kind):
                L = ops.lib()
                if kind.startswith("gemm"):
                    b = R(co, ci, seed=2, scale=0.1)
                    x3 = kind.endswith("x3")
                    nb = ops.gemm_frag_bytes_x3(co, ci) if x3 else ops.gemm_frag_bytes(co, ci)
                    f = ops.gemm_frag_x3 if x3 else ops.gemm_frag
                    return spec(lambda b, out: f(b, co, ci, ci, 1, out), dict(b=b, out=torch.zeros(nb, dtype=torch.uint8, device=DEV)), ["out"])
                w = R(co, ci, 3, 3, seed=3, scale=0.1)
                dgrad = kind.endswith("dgrad")
                if kind.startswith("conv3x3_frag"):
                    nb, f = L.psld_conv3x3_frag_bytes(co, ci), (lambda w, out: ops.conv3x3_frag(w, dgrad, out))
                elif kind == "wino_frag_x3":
                    nb, f = ops.conv3x3_wino_frag_bytes_x3(co, ci), (lambda w, out: ops.conv3x3_wino_frag_x3(w, out))
                else:
                    nb, f = L.psld_conv3x3_wino_frag_bytes(co, ci), (lambda w, out: ops.conv3x3_wino_frag(w, dgrad, out))
                return spec(f, dict(w=w, out=torch.zeros(int(nb), dtype=torch.uint8, device=DEV)), ["out"])
            CASES[f"pack-{kind}-{co}x{ci}"] = build


_pack_cases()


def _batch_pack(kind):
    def build(ops):
        L = ops.lib()
        shapes = [(128, 128), (256, 512)] + ([(160, 320)] if "wino" in kind else [])
        x3 = kind.endswith("x3")
        ws, outs = {}, {}
        for i, (co, ci) in enumerate(shapes):
            if "wino" in kind:
                ws[f"w{i}"] = R(co, ci, 3, 3, seed=10 + i, scale=0.1)
                nb = ops.conv3x3_wino_frag_bytes_x3(co, ci) if x3 else L.psld_conv3x3_wino_frag_bytes(co, ci)
            elif x3:
                ws[f"w{i}"] = R(co, ci, seed=10 + i, scale=0.1)
                nb = ops.gemm_frag_bytes_x3(co, ci)
            else:
                ws[f"w{i}"] = R(co, ci, 3, 3, seed=10 + i, scale=0.1)
                nb = L.psld_conv3x3_frag_bytes(co, ci)
            outs[f"o{i}"] = torch.zeros(int(nb), dtype=torch.uint8, device=DEV)

        def fn(**kw):
            rows, total = [], 0
            for i, (co, ci) in enumerate(shapes):
                w, o = kw[f"w{i}"], kw[f"o{i}"]
                if "wino" in kind:
                    rows.append(ops.conv3x3_wino_frag_entry(w, False if x3 else bool(i & 1), o) + [total])
                elif x3:
                    rows.append([w.data_ptr(), o.data_ptr(), co, ci, 1, ci, 1, total])
                else:
                    rows.append(ops.conv3x3_frag_entry(w, bool(i & 1), o) + [total])
                total += co * ci // 8
            table = torch.tensor(rows, dtype=torch.int64, device=DEV)
            getattr(ops, kind)(table, len(rows), total)
        return spec(fn, {**ws, **outs}, list(outs))
    return build


for _k in ("pack_frag_batch", "pack_wino_batch", "pack_wino_batch_x3", "pack_frag_batch_x3"):
    CASES[_k] = _batch_pack(_k)


# ---- 3x3 forward -----------------------------------------------------------------------------------------------------
FWD_SHAPES = {            # b, c1, c2, co, s
    "b1_8x8": (1, 256, 0, 256, 8),                 # 64 rows: a partial M tile
    "b3_16x16": (3, 128, 0, 128, 16),
    "b1_128wide": (1, 128, 0, 128, 128),
    "two_sources_256+128": (3, 256, 128, 256, 16),
    "tail_160to160": (3, 160, 0, 160, 16),
    "tail_160to160_128wide": (1, 160, 0, 160, 128),
    "tail_320to480": (3, 320, 0, 480, 16),
    "tail_320to480_b1_8x8": (1, 320, 0, 480, 8),
}
TAILS = [k for k in FWD_SHAPES if k.startswith("tail")]
GN_OK = ["b3_16x16", "b1_128wide", "two_sources_256+128"]
SPLITS = [k for k in FWD_SHAPES if not k.startswith("tail_160")]       # (the 160 -> 160 launches fill their grids unsplit)
FWD_ENTRIES = {
    "split_f32": [k for k in FWD_SHAPES if k not in TAILS], "split_limb": [k for k in FWD_SHAPES if k not in TAILS],
    "wino": list(FWD_SHAPES), "wino_allow_split": SPLITS,
    "wino_x3": list(FWD_SHAPES), "wino_x3_allow_split": SPLITS,
    "wino_gn": GN_OK, "wino_gn_allow_split": GN_OK, "wino_gn_x3": GN_OK, "wino_gn_x3_allow_split": GN_OK,
}


def _fwd_case(entry, shape):
    b, c1, c2, co, s = FWD_SHAPES[shape]

    def build(ops):
        split = entry.endswith("allow_split")
        base = entry.replace("_allow_split", "")
        if split and ops.conv3x3_wino_ws_bytes(c1, c2, b, s, s, co) == 0:
            pytest.skip("no split on this CU count")
        if base.startswith("split"):
            assert ops.conv3x3_split_supported(c1, c2, b, s, s, co)
        elif "gn" in base:
            assert ops.conv3x3_wino_gn_supported(c1, c2, b, s, s, co)
        else:
            assert ops.conv3x3_wino_supported(c1, c2, b, s, s, co)
        x1 = R(b, s, s, c1, seed=40) * 1.5 + 0.3
        x2 = R(b, s, s, c2, seed=41) if c2 else None
        w = R(co, c1 + c2, 3, 3, seed=42, scale=0.05)
        t = dict(x1=x1, x2=x2, bias=R(co, seed=43), rowbias=R(b, co, seed=44), res=R(b, s, s, co, seed=45), y=nan(b, s, s, co))
        outs = ["y"]
        if ops.gn_part_supported(b, s * s, co):            # GroupNorm partial sums of the output: exactly gn_part_buffer
            t["part"] = ops.gn_part_buffer(b, s * s, co, DEV)
            t["part"].fill_(NAN)
            outs.append("part")
        if base == "split_limb":
            t["x1"] = ops.f32_to_limb(x1)
            t["x2"] = ops.f32_to_limb(x2) if c2 else None
        if base.startswith("split"):
            t["frag"] = ops.conv3x3_frag(w, False)
        elif "x3" in base:
            t["frag"] = ops.conv3x3_wino_frag_x3(w)
        else:
            t["frag"] = ops.conv3x3_wino_frag(w, False)
        if "gn" in base:
            t["st1"] = ops.gn_stats(x1, D(1 + 0.2 * gen(c1, seed=46)), D(0.1 * gen(c1, seed=47)))
            t["st2"] = ops.gn_stats(x2, D(1 + 0.2 * gen(c2, seed=48)), D(0.1 * gen(c2, seed=49))) if c2 else None

        def fn(x1, x2, bias, rowbias, res, y, frag, part=None, st1=None, st2=None):
            epi = ops.epilogue(bias=bias, rowbias=rowbias, rows_per_img=s * s, residual=res, ld_residual=co, out_scale=0.7,
                               gn_part=part, gn_hw=s * s)
            if base.startswith("split"):
                ops.conv3x3_split(x1, x2, frag, co, y, epi)
            elif base == "wino":
                ops.conv3x3_wino(x1, x2, frag, co, y, epi, allow_split=split)
            elif base == "wino_x3":
                ops.conv3x3_wino_x3(x1, x2, frag, co, y, epi, allow_split=split)
            elif base == "wino_gn":
                ops.conv3x3_wino_gn(x1, st1, x2, st2, True, frag, co, y, epi, allow_split=split)
            else:
                ops.conv3x3_wino_gn_x3(x1, st1, x2, st2, True, frag, co, y, epi, allow_split=split)
        # the split-chunk workspace must be taken (the case skips where this CU count does not split); ops.conv3x3_split hands
        # the direct kernels their split-K workspace (psld_conv2d_workspace_bytes) for every launch of at most 32768 rows,
        # whether or not the launch splits on this CU count - so that call does not depend on the machine
        return spec(fn, t, outs, min_ws=1 if split or base.startswith("split") else 0)
    return build


for _e, _shapes in FWD_ENTRIES.items():
    for _s in _shapes:
        CASES[f"conv3x3-{_e}-{_s}"] = _fwd_case(_e, _s)


# ---- 3x3 backward ----------------------------------------------------------------------------------------------------
def _dgrad_case(kind, b, ci, co, s, accumulate):
    def build(ops):
        gy = R(b, s, s, co, seed=62)
        w = R(co, ci, 3, 3, seed=61, scale=0.05)
        dx = R(b, s, s, ci, seed=63) if accumulate else nan(b, s, s, ci)
        if kind == "wino":
            assert ops.conv3x3_wino_supported(co, 0, b, s, s, ci)
            frag = ops.conv3x3_wino_frag(w, True)
        else:
            assert ops.conv3x3_split_supported(co, 0, b, s, s, ci)
            frag = ops.conv3x3_frag(w, True)

        def fn(gy, frag, dx):
            epi = ops.epilogue(alpha=0.5, accumulate=True) if accumulate else None
            if kind == "wino":
                ops.conv3x3_wino(gy, None, frag, ci, dx, epi, allow_split=True)
            else:
                ops.conv3x3_split(gy, None, frag, ci, dx, epi)
        return spec(fn, dict(gy=gy, frag=frag, dx=dx), ["dx"])
    return build


for _n, _a in {"wino-3x128<-128@16": ("wino", 3, 128, 128, 16, False), "wino-acc-1x256<-64@32": ("wino", 1, 256, 64, 32, True),
               "wino-tail-2x480<-480@16": ("wino", 2, 480, 480, 16, False), "wino-tail-4x160<-160@8": ("wino", 4, 160, 160, 8, True),
               "wino-tail-1x160<-320@128": ("wino", 1, 160, 320, 128, False),
               "split-2x128<-64@8": ("split", 2, 128, 64, 8, False), "split-acc-3x128<-128@16": ("split", 3, 128, 128, 16, True),
               "split-1x128<-64@64": ("split", 1, 128, 64, 64, False)}.items():
    CASES[f"dgrad-{_n}"] = _dgrad_case(*_a)


def _wgrad_split_case(b, c1, c2, co, s, limb, col0):
    def build(ops):
        assert ops.conv3x3_wgrad_split_supported(co, c1, b, s, s) and (not c2 or ops.conv3x3_wgrad_split_supported(co, c2, b, s, s))
        ktiles = b * s * s // 32
        per = -(-ktiles // min(3, ktiles))
        nsplit = -(-ktiles // per)                       # K ranges, the last one short
        cin_total = c1 + c2 + col0
        x1, x2 = R(b, s, s, c1, seed=60), (R(b, s, s, c2, seed=64) if c2 else None)
        if limb:
            x1, x2 = ops.f32_to_limb(x1), (ops.f32_to_limb(x2) if c2 else None)
        t = dict(gy=R(b, s, s, co, seed=62), x1=x1, x2=x2, slabs=torch.zeros(nsplit, co, 9, cin_total, device=DEV))

        def fn(gy, x1, x2, slabs):
            ops.conv3x3_wgrad_split(gy, co, x1, slabs, cin_total, col0, nsplit, x2)
        return spec(fn, t, ["slabs"])
    return build


for _n, _a in {"2x128->64@8": (2, 128, 0, 64, 8, False, 64), "3x128->128@16": (3, 128, 0, 128, 16, False, 0),
               "two-sources-2x128+256->128@16": (2, 128, 256, 128, 16, False, 0), "1x128->64@64": (1, 128, 0, 64, 64, False, 64),
               "xlimb-2x128->64@8": (2, 128, 0, 64, 8, True, 64), "xlimb-3x128->128@16": (3, 128, 0, 128, 16, True, 0),
               "xlimb-two-sources-2x128+256->128@16": (2, 128, 256, 128, 16, True, 0)}.items():
    CASES[f"wgrad_split-{_n}"] = _wgrad_split_case(*_a)


def _wgrad_wino_case(b, c1, c2, co, s, nsplit, accumulate):
    def build(ops):
        assert ops.conv3x3_wgrad_wino_supported(co, c1, c2, b, s, s)
        t = dict(gy=R(b, s, s, co, seed=84), x1=R(b, s, s, c1, seed=83) + 0.25, x2=(R(b, s, s, c2, seed=85) if c2 else None),
                 dw=(R(co, c1 + c2, 3, 3, seed=86) if accumulate else nan(co, c1 + c2, 3, 3)))

        def fn(gy, x1, x2, dw):                           # slabs: ops.workspace of exactly psld_conv3x3_wgrad_wino_ws_bytes
            ops.conv3x3_wgrad_wino(gy, co, x1, dw, x2=x2, nsplit=nsplit, accumulate=accumulate, alpha=0.5 if accumulate else 1.0)
        return spec(fn, t, ["dw"], min_ws=1)
    return build


for _n, _a in {"2x128->256@32": (2, 128, 0, 256, 32, None, False), "8x128->256@8-ns2": (8, 128, 0, 256, 8, 2, False),
               "x2-3x256+128->256@32-ns3": (3, 256, 128, 256, 32, 3, False), "acc-4x256->256@16-ns1": (4, 256, 0, 256, 16, 1, True),
               "x2-acc-4x128+256->256@8": (4, 128, 256, 256, 8, None, True),
               "tail-1x160->160@128": (1, 160, 0, 160, 128, None, False), "tail-4x320->480@16": (4, 320, 0, 480, 16, None, False),
               "tail-x2-1x128+160->160@64-ns3": (1, 128, 160, 160, 64, 3, True)}.items():
    CASES[f"wgrad_wino-{_n}"] = _wgrad_wino_case(*_a)


def _conv2d_wgrad_case(b, ci, co, s, k, stride, pad):
    def build(ops):
        oh = (s + 2 * pad - k) // stride + 1
        nsplit = 3
        n = co * k * k * ci
        t = dict(gy=R(b, oh, oh, co, seed=22), x=R(b, s, s, ci, seed=20), slabs=nan(nsplit, co, k * k, ci), dw=nan(co, ci, k, k))

        def fn(gy, x, slabs, dw):
            ops.conv2d_wgrad_nhwc(gy, co, x, k, k, stride, pad, oh, oh, slabs, ci, 0, nsplit)
            ops.reduce_slabs(slabs, nsplit, n, dw, layout=1, cout=co, taps=k * k, cin=ci)
        return spec(fn, t, ["slabs", "dw"])
    return build


CASES["conv2d_wgrad-3x3"] = _conv2d_wgrad_case(2, 32, 64, 8, 3, 1, 1)
CASES["conv2d_wgrad-3x3-stride2"] = _conv2d_wgrad_case(2, 32, 32, 9, 3, 2, 0)
CASES["conv2d_wgrad-head6"] = _conv2d_wgrad_case(2, 64, 6, 8, 3, 1, 1)
CASES["conv2d_wgrad-1x1"] = _conv2d_wgrad_case(2, 32, 64, 8, 1, 1, 0)


# ---- GEMMs -----------------------------------------------------------------------------------------------------------
def _gemm_case(ta, tb, M, N, K):
    def build(ops):
        A = R(*((K, M) if ta else (M, K)), seed=1)
        B = R(*((N, K) if tb else (K, N)), seed=2)

        def fn(A, B, C):
            ops.gemm_raw(ta, tb, M, N, K, A, A.shape[1], 0, B, B.shape[1], 0, C, N, 0)
        return spec(fn, dict(A=A, B=B, C=nan(M, N)), ["C"])
    return build


for _M, _N, _K in [(200, 72, 100), (6, 130, 54), (1, 1, 4)]:
    for _ta, _tb in [(0, 1), (0, 0), (1, 0), (1, 1)]:
        CASES[f"gemm_raw-{_M}x{_N}x{_K}-t{_ta}{_tb}"] = _gemm_case(_ta, _tb, _M, _N, _K)


@case("gemm_raw-batched-epilogue")
def _(ops):
    b, M, N, K = 3, 70, 96, 40
    t = dict(A=R(b, M, K, seed=3), B=R(b, N, K, seed=4), bias=R(N, seed=5), res=R(b, M, N, seed=6), rowb=R(7, N, seed=7),
             C=torch.ones(b, M, N, device=DEV))

    def fn(A, B, bias, res, rowb, C):       # rows_per_img = 10 -> 7 images per batch entry: a rowbias of exactly [7][N]
        e = ops.epilogue(alpha=0.5, bias=bias, rowbias=rowb, rows_per_img=10, residual=res, ld_residual=N,
                         residual_stride_batch=M * N, out_scale=0.7, accumulate=True)
        ops.gemm_raw(0, 1, M, N, K, A, K, M * K, B, K, N * K, C, N, M * N, b, e)
    return spec(fn, t, ["C"])


def _linear_case(M, N, K):
    def build(ops):
        t = dict(x=R(M, K, seed=8), w=R(N, K, seed=9, scale=0.3), bias=R(N, seed=10), out=nan(M, N))

        def check(p, ret):          # fp32 contraction: the tolerance of test_gemm_layouts
            ref = p["x"].double().cpu() @ p["w"].double().cpu().t() + p["bias"].double().cpu()
            assert rel_l2(p["out"], ref) < 2e-6
        return spec(lambda x, w, bias, out: ops.linear(x, w, bias, out), t, ["out"], check)
    return build


# the three element counts read as M * N * K products: 1, 3 * 5 * 7 and 100003 (a prime: 100003 rows of a 1 x 1 weight);
# (7, 13, 1099) adds a long K with a tail under a ragged tile
for _M, _N, _K in [(1, 1, 1), (3, 5, 7), (100003, 1, 1), (7, 13, 1099)]:
    CASES[f"linear-{_M}x{_N}x{_K}"] = _linear_case(_M, _N, _K)


def _gemm_split_case(m, n, k1, k2, x3, strided):
    def build(ops):
        assert (ops.gemm_split_x3_supported if x3 else ops.gemm_split_supported)(k1, k2, m, n)
        bmat = R(n, k1 + k2, seed=71, scale=0.1)
        frag = (ops.gemm_frag_x3 if x3 else ops.gemm_frag)(bmat, n, k1 + k2, k1 + k2, 1)
        ld = 3 * n if strided else n
        y = nan(m, ld)
        t = dict(a1=R(m, k1, seed=70), a2=(R(m, k2, seed=72) if k2 else None), frag=frag, bias=R(n, seed=73), res=R(m, n, seed=74), y=y)

        def fn(a1, a2, frag, bias, res, y):
            epi = ops.epilogue(bias=bias, residual=res, ld_residual=n, out_scale=0.5)
            yv = y.view(-1)[n:] if strided else y
            (ops.gemm_split_x3 if x3 else ops.gemm_split)(a1, a2, m, frag, n, yv, epi, ldy=ld)
        return spec(fn, t, {"y": (n, 2 * n) if strided else None})
    return build


for _n, _a in {"256x128k64": (256, 128, 64, 0, False, False), "640x128k96+32": (640, 128, 96, 32, False, False),
               "130x128k512-ragged": (130, 128, 512, 0, False, False), "1000x256k256-strided": (1000, 256, 256, 0, False, True),
               "x3-300x256k256": (300, 256, 256, 0, True, False), "x3-300x256k160+96": (300, 256, 160, 96, True, False),
               "x3-130x512k128-strided": (130, 512, 128, 0, True, True)}.items():
    CASES[f"gemm_split-{_n}"] = _gemm_split_case(*_a)


def _tn_split_case(m, n, k, lda, ldb, ldc, nsplit):
    def build(ops):
        assert ops.gemm_tn_split_supported(m, n, k)
        kt = k // 32
        per = -(-kt // nsplit)
        ns = -(-kt // per)

        def fn(a, bm, slabs):
            ops.gemm_tn_split(m, n, k, a, lda, bm.view(-1)[ldb - n:], ldb, slabs, ldc, ns)
        return spec(fn, dict(a=R(k, lda, seed=75), bm=R(k, ldb, seed=76), slabs=nan(ns, m, ldc)), {"slabs": n})
    return build


CASES["gemm_tn_split-256x128x2048-ld"] = _tn_split_case(256, 128, 2048, 256, 384, 128, 3)
CASES["gemm_tn_split-128x256x8192-ld"] = _tn_split_case(128, 256, 8192, 128, 256, 320, 7)
CASES["gemm_tn_split-128x128x64"] = _tn_split_case(128, 128, 64, 128, 128, 128, 1)


@case("gemm_tn_split-two-B-blocks")
def _(ops):
    m, c1, c2, k, ns = 128, 128, 256, 512, 4
    assert ops.gemm_tn_split_supported(m, c1, k)

    def fn(a, b1, b2, slabs):
        ops.gemm_tn_split(m, c1, k, a, m, b1, c1, slabs, c1 + c2, ns, b2, c2, c2)
    return spec(fn, dict(a=R(k, m, seed=77), b1=R(k, c1, seed=78), b2=R(k, c2, seed=79), slabs=nan(ns, m, c1 + c2)), ["slabs"])


@case("gemm_tn_splitk")
def _(ops):
    M, N, K = 64, 96, 1000

    def fn(A, B, slabs, out):
        ops.gemm_tn_splitk(M, N, K, A, M, B, N, slabs, 4)
        ops.reduce_slabs(slabs, 4, M * N, out)
    return spec(fn, dict(A=R(K, M, seed=30), B=R(K, N, seed=31), slabs=nan(4, M, N), out=nan(M, N)), ["slabs", "out"])


def _bgemm_case(ta, tb, m, n, k, batch, pad):
    def build(ops):
        assert ops.bgemm_split_supported(ta, tb, m, n, k)
        A = R(batch, *((k, m + pad) if ta else (m, k + pad)), seed=77)
        B = R(batch, *((n, k + pad) if tb else (k, n + pad)), seed=78)

        def fn(A, B, out):
            lda, ldb = A.shape[2], B.shape[2]
            ops.bgemm_split(ta, tb, m, n, k, A.view(-1)[pad:], lda, A.shape[1] * lda, B.view(-1)[pad:], ldb, B.shape[1] * ldb,
                            out.view(-1)[pad:], n + pad, m * (n + pad), batch, 0.25)
        return spec(fn, dict(A=A, B=B, out=nan(batch, m, n + pad)), {"out": (pad, n + pad)})
    return build


for _ta, _tb in [(0, 1), (0, 0), (1, 0)]:
    CASES[f"bgemm_split-pad64-t{_ta}{_tb}"] = _bgemm_case(_ta, _tb, 256, 256, 256, 5, 64)
CASES["bgemm_split-256x128x96"] = _bgemm_case(0, 1, 256, 128, 96, 3, 0)


def _attn_case(b, hw, c, fused, with_p):
    def build(ops):
        assert ops.attn_fwd_supported(hw, c)
        qkv = R(b, hw, 3 * c, seed=90, scale=1.5)
        t = dict(out=nan(b, hw, c), p=(nan(b, hw, hw) if with_p else None))
        if fused:
            t["qkv"] = qkv
        else:
            t.update({n: v.contiguous() for n, v in zip("qkv", qkv.split(c, dim=-1))})

        def fn(out, p, qkv=None, q=None, k=None, v=None):
            if qkv is not None:
                flat = qkv.view(-1)
                q, k, v, ld = flat, flat[c:], flat[2 * c:], 3 * c
            else:
                ld = c
            ops.attn_fwd(q, k, v, ld, b, hw, c, float(c) ** -0.5, out, p)
        return spec(fn, t, ["out", "p"] if with_p else ["out"])
    return build


for _n, _a in {"3x256x256-fused": (3, 256, 256, True, True), "2x64x256-fused": (2, 64, 256, True, False),
               "5x256x128-separate": (5, 256, 128, False, True), "1x64x128-separate": (1, 64, 128, False, False)}.items():
    CASES[f"attn_fwd-{_n}"] = _attn_case(*_a)


# ---- generic convolution and the small-channel paths ---------------------------------------------------------------
def _conv2d_case(b, c1, c2, co, s, k, stride, pad, tstride):
    def build(ops):
        if tstride > 1:        # data-gradient form: the input is the (dilated) output gradient of a stride-`tstride` convolution
            ih, oh = (s + 2 * 0 - k) // tstride + 1, s
            padk = k - 1
        else:
            ih, oh, padk = s, (s + 2 * pad - k) // stride + 1, pad
        t = dict(x1=R(b, ih, ih, c1, seed=10), x2=(R(b, ih, ih, c2, seed=13) if c2 else None),
                 w=R(co, k * k, c1 + c2, seed=11, scale=0.1), bias=R(co, seed=12), y=nan(b, oh, oh, co))

        def fn(x1, x2, w, bias, y):          # the split-K workspace: ops.workspace of exactly psld_conv2d_workspace_bytes
            ops.conv2d_nhwc(x1, x2, w, co, k, k, stride, padk, tstride, oh, oh, y, ops.epilogue(bias=bias))
        return spec(fn, t, ["y"])
    return build


CASES["conv2d_nhwc-1x1"] = _conv2d_case(3, 32, 0, 32, 16, 1, 1, 0, 1)
CASES["conv2d_nhwc-3x3-two-sources"] = _conv2d_case(2, 64, 32, 64, 8, 3, 1, 1, 1)
CASES["conv2d_nhwc-3x3-stride2"] = _conv2d_case(2, 32, 0, 32, 9, 3, 2, 0, 1)
CASES["conv2d_nhwc-3x3-transposed-stride2"] = _conv2d_case(2, 32, 0, 32, 9, 3, 1, 0, 2)
CASES["conv2d_nhwc-stem6"] = _conv2d_case(2, 6, 0, 32, 16, 3, 1, 1, 1)
CASES["conv2d_nhwc-head6"] = _conv2d_case(2, 64, 0, 6, 16, 3, 1, 1, 1)
CASES["conv2d_nhwc-K4608"] = _conv2d_case(1, 256, 256, 256, 8, 3, 1, 1, 1)


def _im2col_case(b, c, ih, stride, pad):
    def build(ops):
        oh = (ih + 2 * pad - 3) // stride + 1
        t = dict(x=R(b, ih, ih, c, seed=90), d=R(b * oh * oh, 9 * c, seed=91), dx=nan(b, ih, ih, c))

        def fn(x, d, dx):
            cols = ops.im2col3x3(x, stride, pad, oh, oh)
            ops.col2im3x3(d, (b, ih, ih, c), stride, pad, oh, oh, out=dx)
            return cols
        return spec(fn, t, ["dx"])
    return build


for _a in [(2, 8, 9, 2, 0), (1, 64, 17, 2, 0), (2, 16, 8, 1, 1)]:
    CASES["im2col_col2im-%dx%d@%d-s%d-p%d" % _a] = _im2col_case(*_a)


def _im2col_small_case(b, ih, iw, c, stride, pad, flip):
    def build(ops):
        oh, ow = (ih + 2 * pad - 3) // stride + 1, (iw + 2 * pad - 3) // stride + 1

        def check(p, ret):
            x = p["x"].cpu().permute(0, 3, 1, 2)
            ref = F.unfold(x, 3, padding=pad, stride=stride).view(b, c, 9, oh * ow)          # row = ch*9 + tap
            if flip:
                ref = ref.flip(2)
            ref = ref.permute(0, 3, 1, 2).reshape(b * oh * ow, 9 * c)
            assert torch.equal(ret.cpu()[:, :9 * c], ref) and torch.count_nonzero(ret[:, 9 * c:]) == 0
        return spec(lambda x: ops.im2col3x3_small(x, oh, ow, stride, pad, flip), dict(x=R(b, ih, iw, c, seed=92)), (), check)
    return build


CASES["im2col3x3_small-n1"] = _im2col_small_case(1, 1, 1, 1, 1, 1, False)
CASES["im2col3x3_small-n105"] = _im2col_small_case(3, 5, 7, 1, 1, 1, False)
CASES["im2col3x3_small-n105-6ch-flip"] = _im2col_small_case(3, 5, 7, 6, 1, 1, True)
CASES["im2col3x3_small-n105-stride2"] = _im2col_small_case(3, 5, 7, 6, 2, 0, False)
CASES["im2col3x3_small-n100003"] = _im2col_small_case(1, 1, 100003, 1, 1, 1, False)


@case("conv3x3_fewout-5x7")
def _(ops):
    b, c, co, h, w_ = 1, 128, 6, 5, 7
    assert ops.conv3x3_fewout_supported(c, co)
    t = dict(x=R(b, h, w_, c, seed=95), w=R(co, 3, 3, c, seed=96, scale=0.1), bias=R(co, seed=97), y=nan(b, h, w_, co))
    return spec(lambda x, w, bias, y: ops.conv3x3_fewout(x, w, bias, co, y), t, ["y"])


@case("conv3x3_fewout-3ch-16x16")
def _(ops):
    b, c, co, h = 3, 32, 3, 16
    assert ops.conv3x3_fewout_supported(c, co)
    t = dict(x=R(b, h, h, c, seed=95), w=R(co, 3, 3, c, seed=96, scale=0.1), bias=R(co, seed=97), y=nan(b, h, h, co))
    return spec(lambda x, w, bias, y: ops.conv3x3_fewout(x, w, bias, co, y), t, ["y"])


COPY2D = {1: (1, 1, 3, 5), 105: (15, 7, 9, 12), 100003: (100003, 1, 3, 2)}       # rows, cols, ld_src, ld_dst: rows * cols elements
# psld_copy2d_f32 moves float4s (16-byte aligned rows: cols and both leading dimensions multiples of 4), so an element
# count that is not a multiple of 4 cannot be one of its shapes: there the three counts are the ROW counts
COPY2D_ROWS4 = {1: (1, 4, 8, 12), 105: (105, 4, 8, 12), 100003: (100003, 4, 8, 12)}


def _copy2d_case(n, kind):
    rows, cols, lds, ldd = (COPY2D if kind == "scale" else COPY2D_ROWS4)[n]

    def build(ops):
        src = R(rows, lds, seed=100)
        dst = R(rows, ldd, seed=101) if kind == "accumulate" else nan(rows, ldd)

        def fn(src, dst):
            if kind == "scale":
                ops.scale_copy2d(src, lds, dst, ldd, rows, cols, 0.75)
            else:
                ops.copy2d(src, lds, dst, ldd, rows, cols, accumulate=kind == "accumulate")

        def check(p, ret):
            s = src[:, :cols].double().cpu()
            ref = 0.75 * s if kind == "scale" else (s + dst[:, :cols].double().cpu() if kind == "accumulate" else s)
            got = p["dst"][:, :cols].double().cpu()
            assert (got - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
        return spec(fn, dict(src=src, dst=dst), {"dst": cols}, check)
    return build


for _n in COPY2D:
    for _k in ("copy", "accumulate", "scale"):
        CASES[f"copy2d-{_k}-n{_n}"] = _copy2d_case(_n, _k)


@case("copy_batch")
def _(ops):
    counts = [1, 105, 100003]          # float4 items per entry
    t = {}
    for i, n4 in enumerate(counts):
        t[f"s{i}"], t[f"d{i}"] = R(4 * n4, seed=110 + i), nan(4 * n4)

    def fn(**kw):
        rows, first = [], 0
        for i, n4 in enumerate(counts):
            rows += [kw[f"s{i}"].data_ptr(), kw[f"d{i}"].data_ptr(), n4, first]
            first += n4
        ops.copy_batch(torch.tensor(rows, dtype=torch.int64, device=DEV), len(counts), first)

    def check(p, ret):
        for i in range(len(counts)):
            assert torch.equal(p[f"d{i}"], t[f"s{i}"])
    return spec(fn, t, [f"d{i}" for i in range(len(counts))], check)


# ---- GroupNorm -------------------------------------------------------------------------------------------------------
GN_SHAPES = [(3, 16, 128), (5, 8, 256), (7, 8, 384), (3, 8, 512), (5, 16, 512)]        # b, s, c


def _gn_inputs(ops, b, s, c):
    x = R(b, s, s, c, seed=40) * 1.5 + 0.3
    gamma, beta = D(1 + 0.2 * gen(c, seed=41)), D(0.1 * gen(c, seed=42))
    return x, gamma, beta


def _gn_fwd_case(b, s, c, kind):
    def build(ops):
        x, gamma, beta = _gn_inputs(ops, b, s, c)
        if kind == "stats":          # workspace: exactly psld_gn_workspace_bytes; the four statistics tensors from the pool
            return spec(lambda x, gamma, beta: ops.gn_stats(x, gamma, beta), dict(x=x, gamma=gamma, beta=beta))
        st = ops.gn_stats(x, gamma, beta)
        if kind == "apply":
            return spec(lambda x, st, y: ops.gn_apply(x, st, True, out=y), dict(x=x, st=st, y=nan(b, s, s, c)), ["y"])
        if kind == "apply_dropout":
            return spec(lambda x, st, seed: ops.gn_apply(x, st, True, drop_p=0.15, seed=1234, seed_dev=seed),
                        dict(x=x, st=st, seed=torch.tensor([77], dtype=torch.int64, device=DEV)))
        assert ops.lib().psld_limb_bytes(b * s * s, c) == b * s * s * c * 6
        return spec(lambda x, st: ops.gn_apply_limb(x, st, kind == "apply_limb", drop_p=0.15 if kind == "apply_limb_dropout" else 0.0,
                                                    seed=99), dict(x=x, st=st))
    return build


for _b, _s, _c in GN_SHAPES:
    for _k in ("stats", "apply", "apply_dropout", "apply_limb", "apply_limb_dropout"):
        CASES[f"gn_{_k}-{_b}x{_s}x{_s}x{_c}"] = _gn_fwd_case(_b, _s, _c, _k)


def _gn_from_part_case(b, c, co, s, groups_half):
    def build(ops):
        assert ops.gn_part_supported(b, s * s, co)
        x, w = R(b, s, s, c, seed=70), R(co, c, 3, 3, seed=71, scale=0.05)
        part = ops.gn_part_buffer(b, s * s, co, DEV)
        y = torch.empty(b, s, s, co, device=DEV)
        ops.conv3x3_split(x, None, ops.conv3x3_frag(w, False), co, y, ops.epilogue(gn_part=part, gn_hw=s * s))
        groups = ops.gn_groups(2 * co) // 2 if groups_half else None
        t = dict(part=part, gamma=D(1 + 0.1 * gen(co, seed=73)), beta=D(0.1 * gen(co, seed=74)))
        return spec(lambda part, gamma, beta: ops.gn_stats_from_part(part, (b, s, s, co), gamma, beta, groups=groups), t)
    return build


CASES["gn_stats_from_part-3x128@16"] = _gn_from_part_case(3, 64, 128, 16, False)
CASES["gn_stats_from_part-5x256@8-half-groups"] = _gn_from_part_case(5, 128, 256, 8, True)


GN_VARIANTS = ("plain", "branch", "dropout", "accumulate", "branch_accumulate", "no_act")


def _gn_bwd_case(b, s, c, variant, kernel, colsum):
    def build(ops):
        x, gamma, beta = _gn_inputs(ops, b, s, c)
        st = ops.gn_stats(x, gamma, beta)
        t = dict(dy=R(b, s, s, c, seed=61), x=x, st=st, gamma=gamma, beta=beta,
                 dx=(R(b, s, s, c, seed=65) if "accumulate" in variant else nan(b, s, s, c)),
                 add=(R(b, s, s, c, seed=64) if "branch" in variant else None),
                 dg=nan(c), db=nan(c), sums=nan(b, 2, c))
        outs = {"dx": None, "dg": None, "db": None, "sums": None}
        if colsum:
            assert ops.gn_bwd_colsum_supported(b, s * s, c)
            t["per_image"] = nan(b, c + 24)
            outs["per_image"] = (8, 8 + c)
        kw = dict(accumulate_dx="accumulate" in variant)
        if variant == "dropout":
            kw.update(drop_p=0.15, seed=1234)

        def fn(dy, x, st, gamma, beta, dx, add, dg, db, sums, per_image=None):
            initial = ops.get_gn_bwd_kernel()
            ops.set_gn_bwd_kernel(kernel)
            try:          # (the one-pass kernels these shapes take ignore the workspace: see the three-pass cases below)
                ops.gn_bwd(dy, x, st, gamma, beta, variant != "no_act", dx, dg, db, add=add, add_scale=0.5, sums=sums,
                           colsum_img=per_image.view(-1)[8:] if per_image is not None else None, ld_img=c + 24, **kw)
            finally:
                ops.set_gn_bwd_kernel(initial)
        return spec(fn, t, outs)
    return build


for _i, (_b, _s, _c) in enumerate(GN_SHAPES + [(16, 32, 256)]):
    for _j, _v in enumerate(GN_VARIANTS):
        if (_b, _s, _c) == (16, 32, 256) and _v not in ("plain", "branch_accumulate"):
            continue
        for _kern in ("auto", "one_slab"):
            CASES[f"gn_bwd-{_kern}-{_v}-{_b}x{_s}x{_s}x{_c}"] = _gn_bwd_case(_b, _s, _c, _v, _kern, False)
        CASES[f"gn_bwd-colsum-{_v}-{_b}x{_s}x{_s}x{_c}"] = _gn_bwd_case(_b, _s, _c, _v, "auto", True)


# Shapes no one-pass kernel takes (maps above 32x32; 160 / 320 channels: 5- and 10-channel groups): the three-pass form
# (partial sums, coefficients, apply), the only backward consumer of psld_gn_workspace_bytes - it carves its partial sums
# and the [b][3][c] coefficients out of a workspace of exactly that size.
GN_THREE_PASS = [(3, 64, 128), (5, 64, 256), (3, 16, 160), (7, 8, 160), (5, 16, 320)]


def _gn_bwd_three_pass_case(b, s, c, variant):
    inner = _gn_bwd_case(b, s, c, variant, "auto", False)

    def build(ops):
        assert not ops.gn_bwd_colsum_supported(b, s * s, c)           # = no one-pass plan for the shape
        assert ops.lib().psld_gn_workspace_bytes(b, s * s, c, ops.gn_groups(c)) > 0
        sp = inner(ops)
        sp["min_ws"] = 1
        return sp
    return build


for _b, _s, _c in GN_THREE_PASS:
    for _v in GN_VARIANTS:
        CASES[f"gn_bwd-three_pass-{_v}-{_b}x{_s}x{_s}x{_c}"] = _gn_bwd_three_pass_case(_b, _s, _c, _v)


def _gn_team_case(b, s, c, variant):
    def build(ops):
        initial = ops.get_gn_bwd_kernel()
        ops.set_gn_bwd_kernel("auto")
        try:
            k = ops.gn_bwd_team_rows(b, s * s, c)
        finally:
            ops.set_gn_bwd_kernel(initial)
        assert k == s * s // (128 if s * s > 1024 else 64)
        x, gamma, beta = _gn_inputs(ops, b, s, c)
        st = ops.gn_stats(x, gamma, beta)
        t = dict(dy=R(b, s, s, c, seed=81), x=x, st=st, gamma=gamma, beta=beta,
                 dx=(R(b, s, s, c, seed=85) if "accumulate" in variant else nan(b, s, s, c)),
                 add=(R(b, s, s, c, seed=84) if "branch" in variant else None), sums=nan(b * k, 2, c), rows=nan(b * k, c + 8))
        kw = dict(accumulate_dx="accumulate" in variant)
        if variant == "dropout":
            kw.update(drop_p=0.15, seed=1234)

        def fn(dy, x, st, gamma, beta, dx, add, sums, rows):
            initial = ops.get_gn_bwd_kernel()
            ops.set_gn_bwd_kernel("auto")
            try:
                ops.gn_bwd_team(dy, x, st, gamma, beta, variant != "no_act", dx, add=add, add_scale=0.5, sums=sums,
                                colsum_rows=rows, ld_rows=c + 8, **kw)
            finally:
                ops.set_gn_bwd_kernel(initial)

        def check(p, ret):
            assert ops.gn_team_errors(DEV) == 0
        return spec(fn, t, {"dx": None, "sums": None, "rows": c}, check)
    return build


for _b, _s, _c in [(5, 16, 128), (3, 32, 128), (7, 16, 512), (5, 16, 256), (2, 64, 256)]:      # (no 384: its 12-channel groups do not divide a team's 128 channels)
    for _v in GN_VARIANTS:
        CASES[f"gn_bwd_team-{_v}-{_b}x{_s}x{_s}x{_c}"] = _gn_team_case(_b, _s, _c, _v)


# ---- reductions ----------------------------------------------------------------------------------------------------
@case("colsum-3x50x70")
def _(ops):         # workspace: exactly psld_colsum_workspace_bytes
    return spec(lambda m, cs: ops.colsum(m, 70, 3, 50, 70, cs), dict(m=R(150, 70, seed=65), cs=nan(3, 70)), ["cs"])


@case("colsum-ld-5x64x128of384")
def _(ops):
    return spec(lambda m, cs: ops.colsum(m.view(-1)[256:], 384, 5, 64, 128, cs),
                dict(m=R(5, 64, 384, seed=66), cs=nan(5, 128)), ["cs"])


def _bias_grad_case(per_image):
    def build(ops):
        b, hw, c, ld = 5, 64, 128, 384
        t = dict(x=R(b, hw, ld, seed=83), out=nan(c), per=(nan(b, c + 8) if per_image else None))

        def fn(x, out, per):
            ops.bias_grad(x.view(-1)[128:], ld, b, hw, c, out, 0.5, per, c + 8 if per is not None else 0)
        return spec(fn, t, {"out": None, "per": c} if per_image else ["out"])
    return build


CASES["bias_grad-per-image"] = _bias_grad_case(True)
CASES["bias_grad"] = _bias_grad_case(False)


@case("bias_grad_seg")
def _(ops):
    b, hw, c = 6, 64, 256
    t = dict(d=R(b, hw, 3 * c, seed=310), o0=nan(c), o1=nan(c), o2=nan(c))
    return spec(lambda d, o0, o1, o2: ops.bias_grad_seg(d, 3 * c, b, hw, [o0, o1, o2], c, 0.5), t, ["o0", "o1", "o2"])


def _param_reduce2_case(rows, ld, c, two):
    def build(ops):
        t = dict(a=R(rows, ld, seed=120), da=nan(c), db=(nan(c) if two else None))

        def fn(a, da, db):
            ops.param_reduce2(a, a.view(-1)[ld - c:] if two else None, rows, ld, c, da, db, 0.5)
        return spec(fn, t, ["da", "db"] if two else ["da"])
    return build


CASES["param_reduce2-5x2cx128"] = _param_reduce2_case(5, 256, 128, True)
CASES["param_reduce2-7x70of94"] = _param_reduce2_case(7, 94, 70, False)
CASES["param_reduce2-3x1"] = _param_reduce2_case(3, 1, 1, False)


@case("param_reduce_batch")
def _(ops):
    """Jobs as gn_backward / bias_from park them; ``nbytes`` as flush_params computes it (sum of 4 (rows + 1) c)."""
    b, c = 5, 384
    t = dict(sums=R(b, 2, c, seed=121), per=R(b, c + 24, seed=122), small=R(3, 70, seed=123),
             db=nan(c), dg=nan(c), t1=nan(c), t2=nan(c), s1=nan(70))

    def fn(sums, per, small, db, dg, t1, t2, s1):
        jobs = [ops.param_job(sums, b, 2 * c, c, db), ops.param_job(sums, b, 2 * c, c, dg, src_off=c),
                ops.param_job(per, b, c + 24, c, t1, t2, 0.5, src_off=8), ops.param_job(small, 3, 70, 70, s1)]
        rows, blocks = [], 0
        for j in jobs:
            rows += list(j) + [blocks]
            blocks += (j[3] + 63) // 64
        ops.param_reduce_batch(torch.tensor(rows, dtype=torch.int64, device=DEV), len(jobs), blocks,
                               sum(4 * (j[1] + 1) * j[3] for j in jobs))
    return spec(fn, t, ["db", "dg", "t1", "t2", "s1"])


SLAB_SHAPES = [(64, 9, 64, 6, 1, 0.7), (128, 1, 128, 3, 0, 1.0), (32, 1, 36, 1, 0, 0.5), (16, 9, 512, 5, 1, 1.0), (8, 9, 36, 2, 1, 1.0),
               (130, 1, 96, 4, 1, 1.0)]


def _reduce_slabs_case(co, taps, ci, ns, layout, alpha):
    def build(ops):
        n = co * taps * ci
        return spec(lambda slabs, out: ops.reduce_slabs(slabs, ns, n, out, layout=layout, cout=co, taps=taps, cin=ci, alpha=alpha),
                    dict(slabs=R(ns, n, seed=300), out=nan(n)), ["out"])
    return build


for _a in SLAB_SHAPES:
    CASES["reduce_slabs-%dx%dx%d-ns%d-layout%d" % _a[:5]] = _reduce_slabs_case(*_a)


@case("reduce_slabs_batch")
def _(ops):
    t = {}
    for i, (co, taps, ci, ns, layout, alpha) in enumerate(SLAB_SHAPES):
        t[f"s{i}"], t[f"o{i}"] = R(ns, co * taps * ci, seed=300 + i), nan(co * taps * ci)
    cq, nsq = 64, 5
    t["wide"] = R(nsq, cq, 3 * cq, seed=330)          # three column blocks of one [c][3c] slab set (layout 2)
    for kb in range(3):
        t[f"q{kb}"] = nan(cq * cq)

    def fn(**kw):
        jobs = []
        for i, (co, taps, ci, ns, layout, alpha) in enumerate(SLAB_SHAPES):
            jobs.append(ops.slab_job(kw[f"s{i}"], ns, co * taps * ci, kw[f"o{i}"], layout, taps, ci, alpha))
        for kb in range(3):
            jobs.append(ops.slab_job(kw["wide"].view(-1)[kb * cq:], nsq, cq * cq, kw[f"q{kb}"], 2, cq, 3 * cq, 0.5))
        rows, units = [], 0
        for j in jobs:
            u = ops.slab_units(j[2], j[4], j[5], j[6])
            assert u > 0
            rows += list(j) + [units, u]
            units += u
        ops.reduce_slabs_batch(torch.tensor(rows, dtype=torch.int64, device=DEV), len(jobs), units,
                               sum(4 * j[2] * (j[1] + 1) for j in jobs))
    return spec(fn, t, [k for k in t if k[0] in "oq"])


# ---- resampling and pointwise ----------------------------------------------------------------------------------------
FIR_K = np.array([[1.0, 2.0, -1.0], [0.5, 3.0, 0.25], [-2.0, 1.5, 4.0], [0.1, 0.2, 0.3]], dtype=np.float32)


def _upfirdn_case(up, down, pad, layout, bwd):
    def build(ops):
        b, c, h, w_ = 2, 8, 9, 7
        oh, ow = ops.upfirdn2d_out_size(h, w_, 4, 3, up, down, pad)
        shape = (b, c, oh, ow) if bwd else (b, c, h, w_)
        x = R(*shape, seed=50)
        if layout == 1:
            x = x.permute(0, 2, 3, 1).contiguous()
        if bwd:
            return spec(lambda x: ops.upfirdn2d_bwd_raw(x, FIR_K, up, down, pad, (h, w_), layout), dict(x=x))
        return spec(lambda x: ops.upfirdn2d_raw(x, FIR_K, up, down, pad, layout), dict(x=x))
    return build


for _up, _down, _pad in [(2, 1, (2, 1)), (1, 2, (1, 1)), (1, 1, (2, 2)), (3, 2, (0, 3))]:
    for _l in (0, 1):
        for _bwd in (False, True):
            CASES[f"upfirdn2d{'_bwd' if _bwd else ''}-up{_up}-down{_down}-pad{_pad[0]}{_pad[1]}-layout{_l}"] = \
                _upfirdn_case(_up, _down, _pad, _l, _bwd)


# A 4 x 3 kernel only reaches the generic NHWC form.  With 4 x 4 taps x2 up takes the kernel that writes 2 x 2 outputs per
# thread from a 3 x 3 / 2 x 2 neighbourhood (four pad-parity instantiations, `ok ? load : 0` at the borders) and x2 down
# the one-output kernel with compile-time taps; the gradient of either runs on the other.  Pads are (x0, x1, y0, y1).
FIR_K4 = np.array([[1, 2, -1, .75], [.5, 3, .25, -1.25], [-2, 1.5, 4, .6], [.1, .2, .3, -.4]], dtype=np.float32)


def _upfirdn4_case(up, down, pads, shape, bwd, accumulate):
    def build(ops):
        b, c, h, w_ = shape
        oh, ow = ops.upfirdn2d_out_size(h, w_, 4, 4, up, down, pads)
        assert oh > 0 and ow > 0
        x = R(b, oh, ow, c, seed=50) if bwd else R(b, h, w_, c, seed=50)
        out = (R(b, h, w_, c, seed=51) if bwd else R(b, oh, ow, c, seed=51)) if accumulate else None
        if bwd:
            return spec(lambda x, out: ops.upfirdn2d_bwd_raw(x, FIR_K4, up, down, pads, (h, w_), 1, out=out, accumulate=accumulate),
                        dict(x=x, out=out), ["out"] if accumulate else [])
        return spec(lambda x, out: ops.upfirdn2d_raw(x, FIR_K4, up, down, pads, 1, out=out, accumulate=accumulate),
                    dict(x=x, out=out), ["out"] if accumulate else [])
    return build


for _up, _down, _pads, _shape, _acc in (
        [(2, 1, _p, (2, 8, 5, 7), False) for _p in [(2, 1, 2, 1), (1, 2, 1, 2), (2, 1, 1, 2), (1, 2, 2, 1),      # the four parities
                                                    (2, 2, 2, 2), (-1, 3, 2, -1)]] +                             # odd output; crop
        [(1, 2, _p, (2, 8, 9, 7), False) for _p in [(1, 1, 1, 1), (2, 1, 1, 2)]] +
        [(2, 1, (2, 1, 2, 1), (2, 8, 5, 7), True), (2, 1, (1, 2, 1, 2), (1, 132, 3, 3), False)]):
    for _bwd in (False, True):
        CASES["upfirdn2d%s-4x4-up%d-down%d-pad%d_%d_%d_%d-%dx%dx%dx%d%s" % (("_bwd" if _bwd else "", _up, _down) + _pads + _shape +
                                                                         ("-accumulate" if _acc else "",))] = \
            _upfirdn4_case(_up, _down, _pads, _shape, _bwd, _acc)


@case("fused_bias_act")
def _(ops):
    return spec(lambda x, b: ops.fused_bias_act(x, b), dict(x=R(2, 5, 4, 4, seed=52), b=R(5, seed=53)))


@case("fused_bias_act-grad")
def _(ops):
    return spec(lambda gy, ref: ops.fused_bias_act(gy, None, refer=ref, grad=1), dict(gy=R(3, 5, 7, 1, seed=54), ref=R(3, 5, 7, 1, seed=55)))


for _n in (1, 105, 1003, 100003):
    CASES[f"axpby-n{_n}"] = (lambda n: lambda ops: spec(lambda a, b, out: ops.axpby(a, 0.5, b, -2.0, out, accumulate=True),
                                                        dict(a=R(n, seed=62), b=R(n, seed=63), out=torch.ones(n, device=DEV)), ["out"]))(_n)
    CASES[f"silu-n{_n}"] = (lambda n: lambda ops: spec(lambda x: ops.silu(x), dict(x=R(n, seed=64, scale=3.0))))(_n)
    CASES[f"silu_bwd-n{_n}"] = (lambda n: lambda ops: spec(lambda x, dy: ops.silu_bwd(x, dy), dict(x=R(n, seed=64, scale=3.0), dy=R(n, seed=65))))(_n)


def _softmax_case(rows, L):
    def build(ops):
        s = R(rows, L, seed=66, scale=4.0)
        y = torch.softmax(s, -1)

        def fn(s, y, gy, out, dx):
            ops.softmax_rows(s, out, rows, L)
            ops.softmax_rows_bwd(y, gy, dx, rows, L)
        return spec(fn, dict(s=s, y=y, gy=R(rows, L, seed=67), out=nan(rows, L), dx=nan(rows, L)), ["out", "dx"])
    return build


for _rows, _L in [(37, 100), (5, 129), (3, 1000), (37, 256), (1, 1)]:
    CASES[f"softmax_rows-{_rows}x{_L}"] = _softmax_case(_rows, _L)


@case("time_embed-log")
def _(ops):
    return spec(lambda t, W: ops.time_embed(t, W, True), dict(t=D(torch.rand(5, generator=torch.Generator().manual_seed(1))), W=R(128, seed=190)))


@case("time_embed-positional")
def _(ops):
    freq = torch.exp(torch.arange(16, dtype=torch.float32) * -(math.log(10000) / 15))
    return spec(lambda t, W: ops.time_embed(t, W, False), dict(t=D(torch.tensor([3.0, 999.0, 17.0])), W=D(freq)))


for _shape in [(3, 6, 5, 7), (2, 70, 9, 9), (1, 1, 1, 1)]:
    CASES["nchw_to_nhwc-%dx%dx%dx%d" % _shape] = (lambda sh: lambda ops: spec(lambda x: ops.nchw_to_nhwc(x), dict(x=R(*sh, seed=60))))(_shape)
    CASES["nhwc_to_nchw-%dx%dx%dx%d" % _shape] = (lambda sh: lambda ops: spec(lambda x: ops.nhwc_to_nchw(x), dict(x=R(*sh, seed=61))))(_shape)

for _shape in [(2, 4, 8, 96), (1, 1, 1, 32)]:
    CASES["f32_to_limb-%dx%dx%dx%d" % _shape] = (lambda sh: lambda ops: spec(lambda x: ops.f32_to_limb(x), dict(x=R(*sh, seed=3))))(_shape)
    CASES["limb_to_f32-%dx%dx%dx%d" % _shape] = (lambda sh: lambda ops: spec(lambda x: ops.limb_to_f32(x), dict(x=ops.f32_to_limb(R(*sh, seed=3)))))(_shape)


# ---- SDE, loss and optimiser: element counts 1, 3*5*7 and 100003 --------------------------------------------------
COUNTS = {1: (1, 1, 1), 105: (3, 5, 7), 100003: (1, 1, 100003)}          # n = b * c * hw of the [b, 2c, hw, 1] state


def _sde_params():
    from psld_amd._lib import SdeParams
    p = SdeParams()
    p.beta_0, p.beta_1, p.nu, p.gamma = 8.0, 8.0, 4.01, 0.01
    p.m_inv = (0.01 - 4.01) ** 2 / 4
    p.numerical_eps = 1e-9
    p.decomp_lower = 1
    return p


def _em_coeffs(score_mode=0, pf=0, dt=0.01):
    from psld_amd._lib import EmCoeffs
    k = EmCoeffs()
    k.beta, k.m_inv, k.gamma, k.nu, k.m = 8.0, 4.0, 0.01, 4.01, 0.25
    k.c11, k.c12, k.c21, k.c22 = 1.25, -0.5, 0.125, 2.0
    k.dt, k.score_mode, k.probability_flow = dt, score_mode, pf
    return k


def _state(n, seed):
    b, c, hw = COUNTS[n]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 2 * c, hw, 1, generator=g, dtype=torch.float64).to(DEV)


def _rev_terms_ref(k, x, eps):
    """reverse_terms of csrc/sde.hip in torch on the CPU: the score in fp32 with fp32 coefficients, the rest in fp64."""
    x, eps = x.cpu(), eps.cpu()
    c = x.shape[1] // 2
    xv, mv = x[:, :c], x[:, c:]
    if k.score_mode == 0:
        ex, em = eps[:, :c], eps[:, c:]
    else:
        ex = em = eps
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    if k.score_mode == 1:
        sx, sm = torch.zeros_like(ex), -f32(k.c22) * em
    elif k.score_mode == 2:
        sx, sm = -f32(k.c11) * ex, torch.zeros_like(em)
    else:
        sx, sm = -f32(k.c11) * ex - f32(k.c12) * em, -f32(k.c21) * ex - f32(k.c22) * em
    fx, fm = 0.5 * k.beta * (k.m_inv * mv - k.gamma * xv), 0.5 * k.beta * (-k.nu * mv - xv)
    gx, gm = math.sqrt(k.beta * k.gamma), math.sqrt(k.beta * k.m * k.nu)
    return xv, mv, sx, sm, fx, fm, gx, gm


def _close64(got, ref, tol=1e-12):
    got, ref = got.double().cpu(), ref.double()
    assert (got - ref).abs().max().item() <= tol * max(ref.abs().max().item(), 1e-300), (got - ref).abs().max().item()


def _em_step_case(n, score_mode, with_z):
    def build(ops):
        b, c, hw = COUNTS[n]
        k = _em_coeffs(score_mode)
        x0 = _state(n, 1)
        eps = R(b, 2 * c if score_mode == 0 else c, hw, 1, seed=2)
        t = dict(x=x0, eps=eps, z=(_state(n, 3) if with_z else None), xf=nan(b, 2 * c, hw, 1))

        def check(p, ret):
            xv, mv, sx, sm, fx, fm, gx, gm = _rev_terms_ref(k, x0, eps)
            nx, nm = xv + (-fx + gx * gx * sx.double()) * k.dt, mv + (-fm + gm * gm * sm.double()) * k.dt
            if with_z:
                z = t["z"].cpu()
                nx, nm = nx + gx * math.sqrt(k.dt) * z[:, :c], nm + gm * math.sqrt(k.dt) * z[:, c:]
            ref = torch.cat([nx, nm], 1)
            _close64(p["x"], ref)
            assert torch.equal(p["xf"].cpu(), p["x"].cpu().float())
        return spec(lambda x, eps, z, xf: ops.em_step(x, eps, z, k, xf), t, ["x", "xf"], check)
    return build


def _reverse_sde_case(n, pf):
    def build(ops):
        b, c, hw = COUNTS[n]
        k = _em_coeffs(0, pf, dt=0.0)
        return spec(lambda x, eps: ops.reverse_sde(x, eps, k), dict(x=_state(n, 1), eps=R(b, 2 * c, hw, 1, seed=2)))
    return build


def _reverse_rows_case(n, forward_only):
    def build(ops):
        from oracle import psld_oracle as O
        b, c, hw = COUNTS[n]
        p, sde = _sde_params(), O.PSLDOracle()
        x0 = _state(n, 1)
        eps = None if forward_only else R(b, 2 * c, hw, 1, seed=2)
        tr = D(torch.rand(b, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 0.9 + 0.05)
        t = dict(x=x0, eps=eps, tr=tr, flag=torch.zeros(1, dtype=torch.int32, device=DEV))

        def check(pl, ret):
            f, g = ret
            assert int(pl["flag"].item()) == 0
            for i in range(b):
                ti = tr[i:i + 1].cpu()
                k = _em_coeffs(0, 0, 0.0)
                k.beta = float(sde.beta_t(ti))
                if forward_only:
                    xv, mv, _, _, fx, fm, gx, gm = _rev_terms_ref(k, x0[i:i + 1], torch.zeros(1, 2 * c, hw, 1))
                    ref = torch.cat([fx, fm], 1)
                else:
                    k.c11, k.c12, k.c21, k.c22 = (float(v.float()) for v in sde.inv_coeff(sde.cov(0.0, sde.mm_0, ti)))
                    xv, mv, sx, sm, fx, fm, gx, gm = _rev_terms_ref(k, x0[i:i + 1], eps[i:i + 1])
                    ref = torch.cat([-fx + gx * gx * sx.double(), -fm + gm * gm * sm.double()], 1)
                _close64(f[i:i + 1], ref)
                _close64(g[i:i + 1, :c], torch.full((1, c, hw, 1), gx, dtype=torch.float64))
                _close64(g[i:i + 1, c:], torch.full((1, c, hw, 1), gm, dtype=torch.float64))
        return spec(lambda x, eps, tr, flag: ops.reverse_sde_rows(x, eps, tr, p, 0.0, sde.mm_0, 0, False, flag), t, ["flag"], check)
    return build


def _sscs_analytic_case(n):
    def build(ops):
        from psld_amd._lib import SscsCoeffs
        b, c, hw = COUNTS[n]
        k = SscsCoeffs()
        k.a_xx, k.a_xm, k.a_mx, k.a_mm, k.c11, k.c12, k.c21, k.c22 = 0.9, 0.3, -0.2, 0.8, 0.1, 0.0, 0.05, 0.2
        x0, z = _state(n, 1), _state(n, 3)

        def check(p, ret):
            xv, mv, zx, zm = x0.cpu()[:, :c], x0.cpu()[:, c:], z.cpu()[:, :c], z.cpu()[:, c:]
            ref = torch.cat([(k.a_xx * xv + k.a_xm * mv) + (k.c11 * zx + k.c12 * zm), (k.a_mx * xv + k.a_mm * mv) + (k.c21 * zx + k.c22 * zm)], 1)
            _close64(p["x"], ref)
            assert torch.equal(p["xf"].cpu(), p["x"].cpu().float())
        return spec(lambda x, z, xf: ops.sscs_analytic(x, z, k, xf), dict(x=x0, z=z, xf=nan(b, 2 * c, hw, 1)), ["x", "xf"], check)
    return build


def _sscs_score_case(n, score_mode):
    def build(ops):
        b, c, hw = COUNTS[n]
        k = _em_coeffs(score_mode)
        x0, eps = _state(n, 1), R(b, 2 * c if score_mode == 0 else c, hw, 1, seed=2)

        def check(p, ret):
            xv, mv, sx, sm, *_ = _rev_terms_ref(k, x0, eps)
            ref = torch.cat([xv + k.dt * k.gamma * k.beta * (sx.double() + xv), mv + k.dt * k.m * k.nu * k.beta * (sm.double() + k.m_inv * mv)], 1)
            _close64(p["x"], ref)
        return spec(lambda x, eps: ops.sscs_score_step(x, eps, k), dict(x=x0, eps=eps), ["x"], check)
    return build


def _lincomb_case(n, with_base):
    def build(ops):
        vs = [_state(n, 10 + j).view(-1) for j in range(3)]
        coefs = [0.5, -1.25, 2.0]
        base = _state(n, 20).view(-1) if with_base else None
        t = dict(out=nan(vs[0].numel(), dtype=torch.float64), base=base, v0=vs[0], v1=vs[1], v2=vs[2], o32=nan(vs[0].numel()))

        def check(p, ret):
            ref = (base.cpu() if with_base else 0.0) + sum(cf * v.cpu() for cf, v in zip(coefs, vs))
            _close64(p["out"], ref)
            assert torch.equal(p["o32"].cpu(), p["out"].cpu().float())
        return spec(lambda out, base, v0, v1, v2, o32: ops.lincomb(out, base, [v0, v1, v2], coefs, o32), t, ["out", "o32"], check)
    return build


def _scaled_norm_case(n):
    def build(ops):
        vs = [_state(n, 10 + j).view(-1) for j in range(2)]
        coefs = [0.5, -1.25]
        pp, q = _state(n, 21).view(-1), _state(n, 22).view(-1)
        t = dict(v0=vs[0], v1=vs[1], p=pp, q=q, out=nan(1, dtype=torch.float64))

        def check(pl, ret):      # workspace: exactly psld_reduce_workspace_bytes
            e = sum(cf * v.cpu() for cf, v in zip(coefs, vs))
            ref = ((e / (1e-5 + 1e-3 * torch.maximum(pp.cpu().abs(), q.cpu().abs()))) ** 2).sum()
            _close64(pl["out"], ref.reshape(1))
        return spec(lambda v0, v1, p, q, out: ops.scaled_norm_sq([v0, v1], coefs, p, q, 1e-5, 1e-3, out), t, ["out"], check)
    return build


def _vp_lmc(t, b0, b1):
    return -0.25 * t * t * (b1 - b0) - 0.5 * t * b0


def _vp_perturb_case(n, want_f32, want_f64):
    def build(ops):
        b, c, hw = COUNTS[n]
        x0, eps = R(b, c, hw, 1, seed=30), R(b, c, hw, 1, seed=31)
        tt = D(torch.rand(b, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 0.9 + 0.05)

        def check(p, ret):
            lmc = _vp_lmc(tt.cpu(), 0.1, 20.0).view(-1, 1, 1, 1)
            ref = torch.exp(lmc) * x0.double().cpu() + eps.double().cpu() * torch.sqrt(1.0 - torch.exp(2.0 * lmc))
            z, u = ret
            if want_f64:
                _close64(u, ref)
            if want_f32:
                _close64(z, ref, 1e-6)
        return spec(lambda x0, eps, t: ops.vp_perturb(x0, eps, t, 0.1, 20.0, want_f32, want_f64), dict(x0=x0, eps=eps, t=tt), (), check)
    return build


def _vp_reverse_case(n, update, pf):
    def build(ops):
        beta, sd, dt = 7.5, 0.8, 0.01
        x0 = _state(n, 1)
        eps = R(*x0.shape, seed=2)
        z = _state(n, 3) if update and not pf else None
        t = dict(x=x0, eps=eps, z=z, xf=(nan(*x0.shape) if update else None))

        def check(p, ret):
            score = -eps.double().cpu() / sd
            if pf:
                score = 0.5 * score
            fb = 0.5 * beta * x0.cpu() + beta * score
            if not update:
                _close64(ret, fb)
                return
            nx = x0.cpu() + fb * dt
            if z is not None:
                nx = nx + math.sqrt(beta) * math.sqrt(dt) * z.cpu()
            _close64(p["x"], nx)
            assert torch.equal(p["xf"].cpu(), p["x"].cpu().float())
        return spec(lambda x, eps, z, xf: ops.vp_reverse(x, eps, z, beta, sd, dt, pf, update, xf), t, ["x", "xf"] if update else (), check)
    return build


def _vp_loss_case(n, mode, mean):
    def build(ops):
        b, c, hw = COUNTS[n]
        e, ep = R(b, c, hw, 1, seed=32), R(b, c, hw, 1, seed=33)
        tt = D(torch.rand(b, generator=torch.Generator().manual_seed(6), dtype=torch.float64) * 0.9 + 0.05) if mode == 2 else None

        def check(p, ret):          # workspace: exactly psld_reduce_workspace_bytes
            loss, grad = ret
            e64, ep64 = e.double().cpu().requires_grad_(False), ep.double().cpu().requires_grad_(True)
            if mode == 1:
                per = (e64 - ep64).abs()
            else:
                t_ = tt.cpu().view(-1, 1, 1, 1)
                sd = torch.sqrt(1.0 - torch.exp(2.0 * _vp_lmc(t_, 0.1, 20.0)))
                per = ((-ep64 / sd) - (-e64 / sd)) ** 2 * (0.1 + t_ * (20.0 - 0.1))
            ref = per.mean() if mean else per.sum()
            ref.backward()
            _close64(loss.reshape(1), ref.detach().reshape(1), 1e-12 if mode == 2 else 1e-6)
            _close64(grad, ep64.grad, 1e-6)
        return spec(lambda e, ep, t: ops.vp_score_loss(e, ep, t, 0.1, 20.0, mode, mean, True), dict(e=e, ep=ep, t=tt), (), check)
    return build


def _perturb_case(n, with_m0, f32, f64, mu):
    def build(ops):
        from oracle import psld_oracle as O
        b, c, hw = COUNTS[n]
        p = _sde_params()
        tt = D(torch.rand(b, generator=torch.Generator().manual_seed(7), dtype=torch.float64) * 0.9 + 0.05)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        co = ops.perturb_coeffs(tt, p, 0.0, 0.0 if with_m0 else O.PSLDOracle().mm_0, flag)
        t = dict(x0=R(b, c, hw, 1, seed=34), m0=(R(b, c, hw, 1, seed=35) if with_m0 else None), eps=R(b, 2 * c, hw, 1, seed=36), co=co)
        return spec(lambda x0, m0, eps, co: ops.perturb(x0, m0, eps, co, p, f32, f64, mu), t)
    return build


@case("perturb_coeffs")
def _(ops):
    p = _sde_params()
    t = dict(t=D(torch.rand(7, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 0.9 + 0.05),
             flag=torch.zeros(1, dtype=torch.int32, device=DEV))
    return spec(lambda t, flag: ops.perturb_coeffs(t, p, 0.0, 0.01, flag), t, ["flag"])


for _n in COUNTS:
    for _f32, _f64, _mu in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
                            (False, True, True), (True, True, True)]:
        CASES[f"perturb-n{_n}-z{int(_f32)}u{int(_f64)}mu{int(_mu)}"] = _perturb_case(_n, False, _f32, _f64, _mu)
    CASES[f"perturb-n{_n}-m0"] = _perturb_case(_n, True, True, True, True)
    for _f32, _f64 in [(True, False), (False, True), (True, True)]:
        CASES[f"vp_perturb-n{_n}-z{int(_f32)}u{int(_f64)}"] = _vp_perturb_case(_n, _f32, _f64)
    for _mode, _z in [(0, True), (0, False), (1, True), (2, True)]:
        CASES[f"em_step-n{_n}-mode{_mode}-z{int(_z)}"] = _em_step_case(_n, _mode, _z)
    for _pf in (0, 1):
        CASES[f"reverse_sde-n{_n}-pf{_pf}"] = _reverse_sde_case(_n, _pf)
    CASES[f"reverse_sde_rows-n{_n}"] = _reverse_rows_case(_n, False)
    CASES[f"reverse_sde_rows-n{_n}-forward"] = _reverse_rows_case(_n, True)
    CASES[f"sscs_analytic-n{_n}"] = _sscs_analytic_case(_n)
    for _mode in (0, 1, 2):
        CASES[f"sscs_score_step-n{_n}-mode{_mode}"] = _sscs_score_case(_n, _mode)
    CASES[f"vp_reverse-n{_n}-fbar"] = _vp_reverse_case(_n, False, False)
    CASES[f"vp_reverse-n{_n}-fbar-pf"] = _vp_reverse_case(_n, False, True)
    CASES[f"vp_reverse-n{_n}-update"] = _vp_reverse_case(_n, True, False)
    CASES[f"vp_reverse-n{_n}-update-pf"] = _vp_reverse_case(_n, True, True)
    CASES[f"lincomb-n{_n}"] = _lincomb_case(_n, False)
    CASES[f"lincomb-n{_n}-base"] = _lincomb_case(_n, True)
    CASES[f"scaled_norm_sq-n{_n}"] = _scaled_norm_case(_n)
    for _mode in (1, 2):
        for _mean in (True, False):
            CASES[f"vp_score_loss-n{_n}-mode{_mode}-{'mean' if _mean else 'sum'}"] = _vp_loss_case(_n, _mode, _mean)

    def _guide(ops, n=_n):
        x = _state(n, 1)
        return spec(lambda x, g, xf: ops.guide(x, g, 0.25, -1.5, xf), dict(x=x, g=R(*x.shape, seed=91), xf=nan(*x.shape)), ["x", "xf"])
    CASES[f"guide-n{_n}"] = _guide

    def _mask(ops, n=_n):
        b, c, hw = COUNTS[n]
        x = _state(n, 1)
        mask = (R(b, c, hw, 1, seed=87) > 0).float()
        return spec(lambda x, u, mask, xf: ops.mask_combine(x, u, mask, xf), dict(x=x, u=_state(n, 2), mask=mask, xf=nan(*x.shape)), ["x", "xf"])
    CASES[f"mask_combine-n{_n}"] = _mask

    def _sqerr(ops, n=_n):         # workspace: exactly psld_reduce_workspace_bytes
        return spec(lambda a, b: ops.sqerr_loss(a, b, True, True), dict(a=R(n, seed=70), b=R(n, seed=71)))
    CASES[f"sqerr_loss-n{_n}"] = _sqerr
    CASES[f"sqerr_loss-n{_n}-sum-nograd"] = (lambda n: lambda ops: spec(lambda a, b: ops.sqerr_loss(a, b, False, False)[0],
                                                                     dict(a=R(n, seed=70), b=R(n, seed=71))))(_n)

    def _gnorm(ops, n=_n):
        return spec(lambda g, out: ops.grad_norm(g, out), dict(g=R(n, seed=81, scale=0.01), out=nan(1, dtype=torch.float64)), ["out"])
    CASES[f"grad_norm-n{_n}"] = _gnorm

    def _adam(ops, n=_n):
        p = R(n, seed=80)
        t = dict(p=p, g=R(n, seed=81, scale=0.01), m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV), ema=p.clone(),
                 norm=torch.full((1,), 3.0, dtype=torch.float64, device=DEV))
        return spec(lambda p, g, m, v, ema, norm: ops.adam_ema(p, g, m, v, ema, norm, 1.0, 2e-4, 0.9, 0.999, 1e-8, 0.0, 1, 0.9999),
                    t, ["p", "m", "v", "ema"])
    CASES[f"adam_ema-n{_n}"] = _adam

    def _adam_clip(ops, n=_n):
        p = R(n, seed=80)
        t = dict(p=p, g=R(n, seed=81, scale=0.01), m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV),
                 norm=torch.full((1,), 3.0, dtype=torch.float64, device=DEV))
        return spec(lambda p, g, m, v, norm: ops.adam_ema(p, g, m, v, None, norm, 1.0, 2e-4, 0.9, 0.999, 1e-8, 0.01, 3, 0.0,
                                                         write_clipped_grad=True), t, ["p", "g", "m", "v"])
    CASES[f"adam_ema-n{_n}-clipped-grad"] = _adam_clip
    CASES[f"ema-n{_n}"] = (lambda n: lambda ops: spec(lambda t, s: ops.ema(t, s, 0.99), dict(t=R(n, seed=82), s=R(n, seed=83)), ["t"]))(_n)
    CASES[f"f64_to_f32-n{_n}"] = (lambda n: lambda ops: spec(lambda x: ops.f64_to_f32(x), dict(x=_state(n, 1))))(_n)
    CASES[f"f32_to_f64-n{_n}"] = (lambda n: lambda ops: spec(lambda x: ops.f32_to_f64(x), dict(x=R(n, seed=84))))(_n)

    def _to_u8(ops, n=_n):
        return spec(lambda x: ops.samples_to_uint8(x, is_augmented=True), dict(x=_state(n, 1) * 0.8))
    CASES[f"samples_to_uint8-n{_n}"] = _to_u8
    CASES[f"samples_to_uint8-n{_n}-raw"] = (lambda n: lambda ops: spec(lambda x: ops.samples_to_uint8(x, is_augmented=False, denorm=False),
                                                                      dict(x=_state(n, 1) * 0.8)))(_n)

    def _from_u8(ops, n=_n):
        b, c, hw = COUNTS[n]
        g = torch.Generator().manual_seed(90)
        img = D(torch.randint(0, 256, (b, hw, 1, c), generator=g, dtype=torch.uint8))
        flip = D(torch.randint(0, 2, (b,), generator=g, dtype=torch.uint8))
        return spec(lambda img, flip: ops.uint8_to_images(img, flip=flip), dict(img=img, flip=flip))
    CASES[f"uint8_to_images-n{_n}"] = _from_u8


def _xent_case(rows, n):
    def build(ops):
        y = D(torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(89)))
        return spec(lambda z, y: ops.softmax_xent(z, y, 1.0 / rows, 1.0 / rows), dict(z=R(rows, n, seed=88, scale=3.0), y=y))
    return build


for _rows, _n in [(37, 10), (1, 1), (105, 1000), (3, 100003)]:
    CASES[f"softmax_xent-{_rows}x{_n}"] = _xent_case(_rows, _n)


@pytest.mark.parametrize("name", list(CASES))
def test_bounds(ops, guard, name):
    s = CASES[name](ops)
    torch.cuda.synchronize()
    plain, ret = G.run_guarded(guard, s["fn"], s["tensors"], s["outputs"])
    assert guard.workspace_calls >= s["min_ws"], f"{guard.workspace_calls} guarded workspace calls, expected {s['min_ws']}"
    if s["check"] is not None:
        s["check"](plain, ret)


# ---------------------------------------------------------------------------------------------------------------------
# whole training step: forward, backward, deferred flushes, fused Adam - on guarded arenas and workspaces
# ---------------------------------------------------------------------------------------------------------------------
# batch, pool bytes.  Measured peaks on an MI355X (256 CUs), 1 MiB bands included: tiny / tiny_ablation 0.23 GB, c10_sota
# 7.94 GB (753 workspace calls of up to 33.5 MB: the Winograd-domain weight gradients' slabs), afhq160 2.85 GB
STEP_NETS = {"tiny": (5, 512 << 20), "tiny_ablation": (5, 512 << 20), "c10_sota": (3, 10 << 30), "afhq160": (1, 4 << 30)}
STEP_VARIANTS = [("default policy", None, None, True), ("default policy, reductions per layer", None, None, False),
                 ("winograd wherever supported", 2, 2, True), ("winograd wherever supported, reductions per layer", 2, 2, False)]


def _step_net(name):
    if name == "afhq160":
        from tests.test_afhq160_gpu import _build
        net, cfg, _ = _build(train=True, dropout=0.0)
    else:
        from tests.test_model_gpu import _build
        net, cfg, _ = _build(name, train=True)
        cfg.model.score_fn.dropout = 0.0
    return net, cfg


def _train_step(ops, net, crit, data, start, wino, wgrad, defer):
    """One step from the parameters ``start``: (loss, network output, flat gradient, parameters after fused Adam)."""
    from psld_amd.optim import FusedAdam
    x0, eps, t = data
    with torch.no_grad():
        net.flatten_parameters().copy_(start)
    for p in net.parameters():
        p.grad = None
    net.defer_param_grads = defer
    ops.set_winograd(wino)
    ops.set_wgrad_winograd(wgrad)
    outs = []
    hook = net.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone()))
    try:
        torch.manual_seed(11)
        opt = FusedAdam(net, lr=1e-3, grad_clip=1.0)
        loss = crit(x0, t, net, eps=eps)
        loss.backward()
        grad = net.flat_grad().clone()
        opt.step()
        torch.cuda.synchronize()
    finally:
        hook.remove()
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
        net.defer_param_grads = True
    return loss.detach().clone(), outs[0], grad, net.flatten_parameters().clone()


@pytest.mark.parametrize("name", list(STEP_NETS))
def test_training_step_on_guarded_arenas_and_workspaces(ops, monkeypatch, name):
    """ops.Arena -> GuardedArena (exact slices, 64 KiB bands) and ops.workspace -> exact bytes from a pool (1 MiB bands),
    patched before the guarded network's first step: no band is touched, and loss, output, every parameter gradient and the
    parameters after the fused Adam step equal those of the same step without the patches, bit for bit - under the default
    policy and with every supported 3x3 convolution / weight gradient in Winograd form, with the parameter-gradient reductions
    deferred (slab and parameter arenas) and per layer (slabs in the workspace)."""
    import copy

    from psld_amd.registry import get_module
    from tests.synth import synth_inputs
    batch, pool_bytes = STEP_NETS[name]
    net, cfg = _step_net(name)
    size = cfg.data.image_size
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    data = tuple(D(v) for v in synth_inputs(batch, 3, size, seed=5))
    start = net.flatten_parameters().clone()
    plain = [_train_step(ops, net, crit, data, start, w, wg, d) for _, w, wg, d in STEP_VARIANTS]
    for loss, out, grad, _ in plain:
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())

    Arena = G.make_guarded_arena(ops)
    pool = G.GuardPool(DEV, pool_bytes)
    guard = G.Guard(ops, pool).install(monkeypatch, outputs=False)
    monkeypatch.setattr(ops, "Arena", Arena)
    twin = copy.deepcopy(net)            # executor state starts afresh: its arenas are created under the patch
    del net
    peak = 0
    for (tag, w, wg, d), want in zip(STEP_VARIANTS, plain):
        with guard:
            got = _train_step(ops, twin, crit, data, start, w, wg, d)
        pool.check()
        peak = max(peak, pool.peak)
        calls, guard.workspace_calls = guard.workspace_calls, 0
        assert calls > 0 and calls == len(pool.regions), f"{name}, {tag}: {calls} guarded workspace calls"
        pool.release()
        for what, a, b in zip(("loss", "output", "gradient", "parameters after the step"), got, want):
            assert torch.equal(a, b), f"{name}, {tag}: {what} differs between ordinary and guarded scratch"
        print(f"{name}, {tag}: {calls} workspace calls, pool peak {peak} bytes")
    arenas = {"parameter arena": twin._param_arena(), "slab arena": twin._slab_arena()}
    for what, a in arenas.items():
        assert isinstance(a, Arena) and a.total_slices > 0, what
        bad = a.violations()
        print(f"{name}: {what}: {a.total_slices} slices, peak {a.peak} bytes (bands included)")
        assert bad == 0, f"{name}: {bad} band bytes of the {what} changed"


def test_inference_forward_under_bf16x3_on_guarded_workspaces(ops, monkeypatch):
    """A non-recording forward of c10_sota in math mode 'bf16x3' with every supported convolution on the two-limb Winograd
    kernels and GroupNorm fused into their staging: bitwise the forward on ordinary workspaces, no band touched - and the
    two-limb launches with a split-chunk workspace were really taken."""
    import copy

    from tests.test_model_gpu import _build
    net, _, _ = _build("c10_sota")
    gg = torch.Generator().manual_seed(5)
    x, t = D(torch.randn(3, 6, 32, 32, generator=gg)), D(torch.rand(3, generator=gg) * 0.9 + 0.05)
    old = ops.math_mode()
    try:
        ops.set_math_mode("bf16x3")
        ops.set_winograd(2)
        ops.set_fused_gn(2)
        with torch.no_grad():
            want = net(x, t)
        pool = G.GuardPool(DEV, 2 << 30)            # measured peak on an MI355X: 1.41 GB (173 workspace calls)
        guard = G.Guard(ops, pool).install(monkeypatch, outputs=False)
        Arena = G.make_guarded_arena(ops)
        monkeypatch.setattr(ops, "Arena", Arena)
        taken = {}
        for fname in ("conv3x3_wino_x3", "conv3x3_wino_gn_x3", "gemm_split_x3", "conv3x3_wino", "conv3x3_wino_gn"):
            def counted(*a, _f=getattr(ops, fname), _n=fname, **kw):
                taken[_n] = taken.get(_n, 0) + 1
                return _f(*a, **kw)
            monkeypatch.setattr(ops, fname, counted)
        twin = copy.deepcopy(net)
        with guard, torch.no_grad():
            got = twin(x, t)
        torch.cuda.synchronize()
    finally:
        ops.set_math_mode(old)
        ops.set_winograd(None)
        ops.set_fused_gn(None)
    pool.check()
    print(f"bf16x3 forward: {guard.workspace_calls} workspace calls, pool peak {pool.peak} bytes, launches {taken}")
    assert guard.workspace_calls > 0 and guard.workspace_calls == len(pool.regions)
    assert taken.get("conv3x3_wino_x3", 0) > 0 and taken.get("conv3x3_wino_gn_x3", 0) > 0, taken
    assert not taken.get("conv3x3_wino") and not taken.get("conv3x3_wino_gn"), taken       # no three-limb forward left
    for a in Arena.instances:                      # (a non-recording forward parks nothing; whatever it took stayed in bounds)
        assert a.violations() == 0
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)

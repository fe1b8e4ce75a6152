"""Eval math 'f16' on the GPU: the one-product fp16 packers, Winograd forward and pointwise forward kernels against the CPU
reference of the arithmetic (tests/f16_ref.py, fp64 accumulation: products of fp16 values are exact in fp32, so the kernels
differ from it in fp32 summation order only - the project's 3e-6 kernel gate), the clamp, where the kernels read and write
(tests/guard.py), the networks and samplers under the setting against the reference goldens (bound: 1.25 x the CPU figure of
tests/golden/f16_meta.json - NOT the 1e-4 parity contract, which this mode is outside of by design), and that nothing else
moved.  Every test restores the process's settings."""
import contextlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from psld_amd import config as C
from tests import f16_ref as H
from tests import guard as G
from tests.conftest import GOLDEN
from tests.synth import synth_inputs, synth_state_dict
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy
GATE = 3e-6


@contextlib.contextmanager
def settings(mode, eval_math="limb", winograd=None, fused_gn=None):
    from psld_amd import ops as o
    old, old_eval = o.math_mode(), o.eval_math()
    try:
        o.set_math_mode(mode)
        o.set_eval_math(eval_math)
        o.set_winograd(winograd)
        o.set_fused_gn(fused_gn)
        yield
    finally:
        o.set_winograd(None)
        o.set_fused_gn(None)
        o.set_math_mode(old)
        o.set_eval_math(old_eval)


def _meta():
    with open(os.path.join(GOLDEN, "f16_meta.json")) as fh:
        return json.load(fh)


# ---------------------------------------------------------------------------------------------------------------------
# Winograd forward, one fp16 product
# ---------------------------------------------------------------------------------------------------------------------
WINO = [            # c1, c2, B, H, W, cout
    (128, 0, 2, 8, 8, 128),            # two images per region
    (128, 0, 1, 16, 16, 128),
    (128, 128, 1, 32, 32, 256),        # two sources
    (128, 0, 1, 64, 64, 128),          # 4 x 32 blocks
    (32, 0, 1, 128, 128, 128),
    (160, 0, 1, 16, 16, 160),          # channel tail
    (320, 160, 1, 8, 8, 320),          # channel tail
    (256, 0, 2, 8, 8, 256, True),      # allow_split: split-chunk path + reduction
]


@pytest.mark.parametrize("cfg", WINO, ids=lambda c: "{}+{}x{}x{}x{}->{}".format(*c[:6]) + ("-split" if len(c) > 6 else ""))
def test_conv3x3_wino_f16_forward(ops, cfg):
    """Plain launch and full epilogue against the fp16 reference within 3e-6, each repeated bit for bit; against a true fp64
    convolution the kernel lies within [0.5, 2] x the reference's own error (a silent fall-back to limbs would be far below)."""
    c1, c2, b, h, w_, co = cfg[:6]
    split = len(cfg) > 6
    assert ops.conv3x3_wino_supported(c1, c2, b, h, w_, co)
    if split:
        assert ops.conv3x3_wino_ws_bytes(c1, c2, b, h, w_, co) > 0, "the split-chunk path is what this case is about"
    x = gen(b, c1 + c2, h, w_, seed=40)
    w = gen(co, c1 + c2, 3, 3, seed=41, scale=0.05)
    bias, res, temb = gen(co, seed=42), gen(b, co, h, w_, seed=43), gen(b, co, seed=44)
    emu = H.f16_conv3x3(x, w)
    conv64 = F.conv2d(x.double(), w.double(), padding=1)
    x1 = _nhwc(x[:, :c1]).to(DEV)
    x2 = _nhwc(x[:, c1:]).to(DEV) if c2 else None
    uf = ops.conv3x3_wino_frag_f16(w.to(DEV))
    assert uf.numel() == ops.conv3x3_wino_frag_bytes_f16(co, c1 + c2)
    nan = torch.full((b, h, w_, co), float("nan"), device=DEV)

    def run(e, init=nan):
        y = init.clone()
        ops.conv3x3_wino_f16(x1, x2, uf, co, y, e, allow_split=split)
        return y
    y = run(None)
    e_emu, e_64, emu_64 = rel_l2(y.permute(0, 3, 1, 2), emu), rel_l2(y.permute(0, 3, 1, 2), conv64), rel_l2(emu, conv64)
    print(f"wino f16 {cfg}: vs fp16 reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e})")
    assert e_emu <= GATE
    assert 0.5 * emu_64 <= e_64 <= 2 * emu_64
    assert torch.equal(y, run(None))
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=h * w_, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)
    ref = (emu + bias.double()[None, :, None, None] + temb.double()[:, :, None, None] + res.double()) * 0.7
    y = run(epi)
    err = rel_l2(y.permute(0, 3, 1, 2), ref)
    print(f"wino f16 {cfg} full epilogue: {err:.2e}")
    assert err <= GATE and torch.equal(y, run(epi))
    prev = gen(b, h, w_, co, seed=49).to(DEV)
    acc = run(ops.epilogue(alpha=0.5, accumulate=True), prev)
    assert rel_l2(acc.permute(0, 3, 1, 2), emu * 0.5 + prev.permute(0, 3, 1, 2).cpu().double()) <= GATE


@pytest.mark.parametrize("c1,c2,b,s,co", [(128, 0, 1, 32, 128), (128, 128, 1, 32, 256)])
def test_conv3x3_wino_gn_f16_is_apply_plus_convolution(ops, c1, c2, b, s, co):
    """GroupNorm + SiLU inside the staging: bit for bit the apply pass + the f16 convolution, and the reference on that input."""
    assert ops.conv3x3_wino_gn_supported(c1, c2, b, s, s, co)
    xs = gen(b, c1 + c2, s, s, seed=40) * 1.5 + 0.3
    w = gen(co, c1 + c2, 3, 3, seed=41, scale=0.05)
    bias = gen(co, seed=42)
    uf = ops.conv3x3_wino_frag_f16(w.to(DEV))
    xs1 = _nhwc(xs[:, :c1]).to(DEV)
    xs2 = _nhwc(xs[:, c1:]).to(DEV) if c2 else None
    st1 = ops.gn_stats(xs1, (gen(c1, seed=74) * 0.2 + 1.0).to(DEV), (gen(c1, seed=75) * 0.1).to(DEV))
    st2 = ops.gn_stats(xs2, (gen(c2, seed=76) * 0.2 + 1.0).to(DEV), (gen(c2, seed=77) * 0.1).to(DEV)) if c2 else None
    a1 = ops.gn_apply(xs1, st1, True)
    a2 = ops.gn_apply(xs2, st2, True) if c2 else None
    e = ops.epilogue(bias=bias.to(DEV))
    nan = torch.full((b, s, s, co), float("nan"), device=DEV)
    y_un, y_f, y_f2 = nan.clone(), nan.clone(), nan.clone()
    ops.conv3x3_wino_f16(a1, a2, uf, co, y_un, e, allow_split=True)
    ops.conv3x3_wino_gn_f16(xs1, st1, xs2, st2, True, uf, co, y_f, e, allow_split=True)
    ops.conv3x3_wino_gn_f16(xs1, st1, xs2, st2, True, uf, co, y_f2, e, allow_split=True)
    assert torch.equal(y_f, y_un) and torch.equal(y_f, y_f2)
    act = torch.cat([a1] + ([a2] if c2 else []), -1).permute(0, 3, 1, 2).cpu()
    err = rel_l2(y_f.permute(0, 3, 1, 2), H.f16_conv3x3(act, w) + bias.double()[None, :, None, None])
    print(f"wino f16 {c1}+{c2}->{co}@{s} fused GroupNorm + SiLU: {err:.2e}")
    assert err <= GATE


# ---------------------------------------------------------------------------------------------------------------------
# pointwise forward, one fp16 product
# ---------------------------------------------------------------------------------------------------------------------
M_PW = 16 * 32 * 32         # the smallest M at which the executor takes the eight-wave form for n = 256 (128 tiles of 128 x 256)


@pytest.mark.parametrize("k1,k2,n", [(256, 0, 256), (512, 0, 256), (256, 256, 256), (256, 0, 768)])
def test_gemm_split_f16_forward(ops, k1, k2, n):
    m = M_PW
    assert ops.gemm_split_f16_supported(k1, k2, m, n) and ops.gemm_split_f16_wanted(k1, k2, m, n)
    assert not ops.gemm_split_f16_wanted(k1, k2, m // 2, 256)
    a = gen(m, k1 + k2, seed=50)
    bm = gen(n, k1 + k2, seed=51, scale=0.05)               # [n][k]
    bias, res = gen(n, seed=52), gen(m, n, seed=53)
    emu, ref64 = H.f16_matmul(a, bm), a.double() @ bm.double().t()
    a1 = a[:, :k1].contiguous().to(DEV)
    a2 = a[:, k1:].contiguous().to(DEV) if k2 else None
    bd = bm.to(DEV)
    fr = ops.gemm_frag_f16(bd, n, k1 + k2, k1 + k2, 1)
    assert fr.numel() == ops.gemm_frag_bytes_f16(n, k1 + k2) == n * (k1 + k2) * 2
    nan = torch.full((m, n), float("nan"), device=DEV)

    def run(e, init=nan):
        y = init.clone()
        ops.gemm_split_f16(a1, a2, m, fr, n, y, e)
        return y
    y = run(None)
    e_emu, e_64, emu_64 = rel_l2(y, emu), rel_l2(y, ref64), rel_l2(emu, ref64)
    print(f"gemm f16 {k1}+{k2}->{n} m={m}: vs fp16 reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e})")
    assert e_emu <= GATE
    assert 0.5 * emu_64 <= e_64 <= 2 * emu_64
    assert torch.equal(y, run(None))
    epi = ops.epilogue(bias=bias.to(DEV), residual=res.to(DEV), ld_residual=n, out_scale=0.7)
    y = run(epi)
    assert rel_l2(y, (emu + bias.double() + res.double()) * 0.7) <= GATE and torch.equal(y, run(epi))
    # a refreshed weight: the batched packer into the same buffer writes what a fresh pack of the new values writes
    bd.mul_(1.25).add_(0.01)
    row = [bd.data_ptr(), fr.data_ptr(), n, k1 + k2, 1, k1 + k2, 1, 0]
    ops.pack_frag_batch_f16(torch.tensor([row], dtype=torch.int64, device=DEV), 1, n * (k1 + k2) // 8)
    assert torch.equal(fr, ops.gemm_frag_f16(bd, n, k1 + k2, k1 + k2, 1))


def test_wino_packer_batch_equals_single(ops):
    co, ci = 160, 320
    w, w2 = gen(co, ci, 3, 3, seed=11, scale=0.05).to(DEV), gen(co, ci, 3, 3, seed=12, scale=0.05).to(DEV)
    f1 = ops.conv3x3_wino_frag_f16(w)
    outs = [torch.zeros_like(f1), torch.zeros_like(f1)]
    rows, total = [], 0
    for wt, out in zip((w, w2), outs):
        rows.append(ops.conv3x3_wino_frag_entry(wt, False, out) + [total])
        total += co * ci // 8
    ops.pack_wino_batch_f16(torch.tensor(rows, dtype=torch.int64, device=DEV), 2, total)
    pay = co * ci * 32
    assert torch.equal(outs[0][:pay], f1[:pay]) and torch.equal(outs[1][:pay], ops.conv3x3_wino_frag_f16(w2)[:pay])
    # the fragments are fp16 roundings of U = G g G^T: every value is one the reference's rounding produces
    from tests.x3_ref import wino_u
    got = f1[:pay].view(torch.float16).float().cpu()
    want = H.round_f16(wino_u(w.cpu()))
    assert torch.equal(got.sort().values, want.reshape(-1).sort().values)


# ---------------------------------------------------------------------------------------------------------------------
# range
# ---------------------------------------------------------------------------------------------------------------------
def test_range_clamp_and_tiny_weights(ops):
    """Inputs holding +-1e6 and +-70000 among normal values: finite outputs, equal to the clamping reference (the transformed
    values V are what is clamped); weights scaled by 2^-30 (transformed values below fp16's smallest subnormal where the
    reference flushes them too)."""
    b, c, s, co = 1, 128, 16, 128
    x = gen(b, c, s, s, seed=60)
    x[0, 3, 4, 5], x[0, 7, 8, 9], x[0, 100, 0, 0], x[0, 31, 15, 15] = 1e6, -1e6, 70000.0, -70000.0
    w = gen(co, c, 3, 3, seed=61, scale=0.05)
    xd = _nhwc(x).to(DEV)
    # x 2^-12: transformed weights in fp16's subnormal range (kept, not flushed); x 2^-30: below 2^-25, zero in the reference too
    for tag, wt in (("normal weights", w), ("weights x 2^-12", w * 2.0 ** -12), ("weights x 2^-30", w * 2.0 ** -30)):
        emu = H.f16_conv3x3(x, wt)
        y = torch.full((b, s, s, co), float("nan"), device=DEV)
        ops.conv3x3_wino_f16(xd, None, ops.conv3x3_wino_frag_f16(wt.to(DEV)), co, y)
        assert bool(torch.isfinite(y).all()), tag
        if float(emu.abs().max()) == 0.0:
            assert float(y.abs().max()) == 0.0, tag
        else:
            err = rel_l2(y.permute(0, 3, 1, 2), emu)
            print(f"range, {tag}: vs the clamping reference {err:.2e}")
            assert err <= GATE, tag
    # pointwise: rows beyond +-65504 are clamped, not turned into infinities
    m, k, n = 128 * 128, 256, 256
    a = gen(m, k, seed=62)
    a[5, 7], a[100, 200], a[4000, 1], a[9000, 255] = 1e6, -1e6, 70000.0, -70000.0
    bm = gen(n, k, seed=63, scale=0.05)
    y = torch.full((m, n), float("nan"), device=DEV)
    ops.gemm_split_f16(a.to(DEV), None, m, ops.gemm_frag_f16(bm.to(DEV), n, k, k, 1), n, y)
    assert bool(torch.isfinite(y).all()) and rel_l2(y, H.f16_matmul(a, bm)) <= GATE


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 256 << 20)
    yield p
    del p
    torch.cuda.empty_cache()


def _R(*shape, seed, scale=1.0):
    return gen(*shape, seed=seed, scale=scale).to(DEV)


def _guard_cases(ops):
    nanf = lambda *s: torch.full(s, float("nan"), device=DEV)       # noqa: E731
    for co, ci in ((128, 128), (160, 320)):
        yield f"pack-wino-{co}x{ci}", (lambda w, out: ops.conv3x3_wino_frag_f16(w, out)), \
            dict(w=_R(co, ci, 3, 3, seed=1, scale=0.05), out=torch.zeros(ops.conv3x3_wino_frag_bytes_f16(co, ci), dtype=torch.uint8, device=DEV)), ["out"], 0
    for n, k in ((256, 256), (768, 256)):
        yield f"pack-gemm-{n}x{k}", (lambda b, out, n=n, k=k: ops.gemm_frag_f16(b, n, k, k, 1, out)), \
            dict(b=_R(n, k, seed=2, scale=0.05), out=torch.zeros(ops.gemm_frag_bytes_f16(n, k), dtype=torch.uint8, device=DEV)), ["out"], 0

    def batch_wino(w0, w1, o0, o1):
        rows = [ops.conv3x3_wino_frag_entry(w0, False, o0) + [0], ops.conv3x3_wino_frag_entry(w1, False, o1) + [128 * 128 // 8]]
        ops.pack_wino_batch_f16(torch.tensor(rows, dtype=torch.int64, device=DEV), 2, 2 * 128 * 128 // 8)
    nb = ops.conv3x3_wino_frag_bytes_f16(128, 128)
    yield "pack-wino-batch", batch_wino, dict(w0=_R(128, 128, 3, 3, seed=3, scale=0.05), w1=_R(128, 128, 3, 3, seed=4, scale=0.05),
                                              o0=torch.zeros(nb, dtype=torch.uint8, device=DEV),
                                              o1=torch.zeros(nb, dtype=torch.uint8, device=DEV)), ["o0", "o1"], 0

    def batch_gemm(b0, b1, o0, o1):
        rows = [[b0.data_ptr(), o0.data_ptr(), 256, 256, 1, 256, 1, 0], [b1.data_ptr(), o1.data_ptr(), 256, 256, 1, 256, 1, 256 * 256 // 8]]
        ops.pack_frag_batch_f16(torch.tensor(rows, dtype=torch.int64, device=DEV), 2, 2 * 256 * 256 // 8)
    nb = ops.gemm_frag_bytes_f16(256, 256)
    yield "pack-gemm-batch", batch_gemm, dict(b0=_R(256, 256, seed=5, scale=0.05), b1=_R(256, 256, seed=6, scale=0.05),
                                              o0=torch.zeros(nb, dtype=torch.uint8, device=DEV),
                                              o1=torch.zeros(nb, dtype=torch.uint8, device=DEV)), ["o0", "o1"], 0
    for cfg in WINO:
        c1, c2, b, h, w_, co = cfg[:6]
        split = len(cfg) > 6
        wt = _R(co, c1 + c2, 3, 3, seed=42, scale=0.05)
        t = dict(x1=_R(b, h, w_, c1, seed=40), x2=_R(b, h, w_, c2, seed=41) if c2 else None, bias=_R(co, seed=43),
                 rowbias=_R(b, co, seed=44), res=_R(b, h, w_, co, seed=45), y=nanf(b, h, w_, co), frag=ops.conv3x3_wino_frag_f16(wt))

        def fn(x1, x2, bias, rowbias, res, y, frag, co=co, hw=h * w_, split=split):
            epi = ops.epilogue(bias=bias, rowbias=rowbias, rows_per_img=hw, residual=res, ld_residual=co, out_scale=0.7)
            ops.conv3x3_wino_f16(x1, x2, frag, co, y, epi, allow_split=split)
        yield "wino-{}+{}x{}x{}x{}->{}".format(*cfg[:6]) + ("-split" if split else ""), fn, t, ["y"], int(split)
    for c1, c2, b, s, co in ((128, 0, 1, 32, 128), (128, 128, 1, 32, 256)):
        x1, x2 = _R(b, s, s, c1, seed=40) * 1.5 + 0.3, (_R(b, s, s, c2, seed=41) if c2 else None)
        t = dict(x1=x1, x2=x2, bias=_R(co, seed=43), y=nanf(b, s, s, co),
                 frag=ops.conv3x3_wino_frag_f16(_R(co, c1 + c2, 3, 3, seed=42, scale=0.05)),
                 st1=ops.gn_stats(x1, (1 + 0.2 * gen(c1, seed=46)).to(DEV), (0.1 * gen(c1, seed=47)).to(DEV)),
                 st2=ops.gn_stats(x2, (1 + 0.2 * gen(c2, seed=48)).to(DEV), (0.1 * gen(c2, seed=49)).to(DEV)) if c2 else None)

        def fng(x1, x2, bias, y, frag, st1, st2, co=co):
            ops.conv3x3_wino_gn_f16(x1, st1, x2, st2, True, frag, co, y, ops.epilogue(bias=bias), allow_split=True)
        yield f"wino-gn-{c1}+{c2}->{co}@{s}", fng, t, ["y"], 0
    for k1, k2, n in ((256, 0, 256), (256, 256, 256), (256, 0, 768)):
        m = M_PW - 64               # a partial last row tile
        t = dict(a1=_R(m, k1, seed=50), a2=_R(m, k2, seed=51) if k2 else None, bias=_R(n, seed=52), y=nanf(m, n),
                 frag=ops.gemm_frag_f16(_R(n, k1 + k2, seed=53, scale=0.05), n, k1 + k2, k1 + k2, 1))

        def fnp(a1, a2, bias, y, frag, m=m, n=n):
            ops.gemm_split_f16(a1, a2, m, frag, n, y, ops.epilogue(bias=bias))
        yield f"gemm-{k1}+{k2}->{n}", fnp, t, ["y"], 0


def test_guard_bands_of_every_f16_launch_and_packer(ops, pool, monkeypatch):
    """Every new launch and packer on exact-size buffers between pattern bands (tests/guard.py, as tests/test_bounds_gpu.py):
    results equal the run on ordinary buffers bit for bit, inputs unchanged, no band touched."""
    guard = G.Guard(ops, pool).install(monkeypatch)
    n = 0
    for name, fn, tensors, outs, min_ws in _guard_cases(ops):
        try:
            G.run_guarded(guard, fn, tensors, outs)
        except G.GuardViolation as e:
            raise AssertionError(f"{name}: {e}") from e
        assert guard.workspace_calls >= min_ws, name
        n += 1
    assert n == 2 + 2 + 2 + len(WINO) + 2 + 3


# ---------------------------------------------------------------------------------------------------------------------
# networks and samplers
# ---------------------------------------------------------------------------------------------------------------------
LIMB2 = ("conv3x3_wino_x3", "conv3x3_wino_gn_x3", "gemm_split_x3")
F16 = ("conv3x3_wino_f16", "conv3x3_wino_gn_f16", "gemm_split_f16")
LIMB3 = ("conv3x3_wino", "conv3x3_wino_gn", "gemm_split")


def _record(monkeypatch, log, phase=lambda: None):
    from psld_amd import ops as o
    for name in LIMB3 + LIMB2 + F16:
        def rec(*a, _fn=getattr(o, name), _name=name, **k):
            log.append((_name, phase()))
            return _fn(*a, **k)
        monkeypatch.setattr(o, name, rec)


def _net(name):
    if name in ("c10_sota", "celeba64", "tiny"):
        from tests.test_model_gpu import _build
        return _build(name)[0], f"net_{name}.npz"
    if name == "afhqv2_128":
        from tests.test_afhq_gpu import _build
        return _build()[0], "net_afhq128.npz"
    from tests.test_afhq160_gpu import _build
    return _build()[0], "net_afhq160.npz"


@pytest.mark.parametrize("name", ["c10_sota", "celeba64", "afhqv2_128", "afhqv2_128_inpaint"])
def test_network_forward_under_f16(golden, monkeypatch, name):
    """Eval forward against the reference golden under PSLD_MATH=f16's settings with every supported 3x3 convolution on the
    fp16 Winograd kernel: within 1.25 x the CPU oracle's figure for the same arithmetic (attention and the small launches stay
    on limbs here, so at or below it; 25 % for rounding decisions that flip with the summation order)."""
    net, gname = _net(name)
    g = golden(gname)
    x, t = T(g["x"]).to(DEV), T(g["t"]).to(DEV)
    log = []
    _record(monkeypatch, log)
    with settings("bf16x3", "f16", winograd=2, fused_gn=2), torch.no_grad():
        y = net(x, t)
        yb = net(x, t)
    monkeypatch.undo()
    err, bound = rel_l2(y, T(g["y"])), 1.25 * _meta()[name]["f16"]
    print(f"{name}: eval math f16 {err:.3e} vs the reference golden (CPU oracle, same arithmetic: {_meta()[name]['f16']:.3e})")
    assert torch.equal(y, yb)
    names = [n for n, _ in log]
    assert "conv3x3_wino_f16" in names or "conv3x3_wino_gn_f16" in names
    assert not [n for n in names if n in ("conv3x3_wino", "conv3x3_wino_gn", "conv3x3_wino_x3", "conv3x3_wino_gn_x3")], sorted(set(names))
    assert err <= bound


@pytest.mark.parametrize("stride", ["uniform", "quadratic"])
def test_em_sampler_under_f16(golden, stride):
    from psld_amd.registry import get_module
    from tests.test_fullsize_gpu import _sampler
    from tests.test_model_gpu import _build
    net, cfg, _ = _build("c10_sota")
    g = golden("em_c10_sota.npz")
    noise = T(g[f"noise_{stride}"]).to(DEV)
    sde, sampler, _ = _sampler(cfg, net, noise)
    cfg.evaluation.n_discrete_steps = 4
    cfg.evaluation.stride_type = stride
    wr = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=net, sampler_cls=None)
    ts = wr.sampling_times(DEV)
    with settings("bf16x3", "f16", winograd=2, fused_gn=2):
        x = sampler.sample(T(g[f"batch_{stride}"]).to(DEV), ts, wr.n_discrete_steps, denoise=True, eps=cfg.evaluation.eval_eps)
    err, rec = rel_l2(x, T(g[f"x_{stride}"])), _meta()[f"em_{stride}"]["f16"]
    print(f"EM on C10-SOTA under eval math f16 ({stride}): rel-L2 vs reference = {err:.3e} (CPU oracle: {rec:.3e})")
    assert x.dtype == torch.float64 and err <= 1.25 * rec


def test_inpainting_sampler_under_f16(monkeypatch):
    """3 ip_em_sde steps of afhqv2_128_inpaint at B = 2, synthetic weights: runs on fp16 launches and stays finite."""
    from psld_amd.registry import get_module
    from tests.test_afhq160_gpu import _build
    net, cfg, _ = _build()
    sde = get_module("sde", "psld")(cfg)
    gg = torch.Generator().manual_seed(3)
    x0 = torch.rand(2, 3, 128, 128, generator=gg) * 2 - 1
    mask = torch.ones(2, 3, 128, 128)
    mask[:, :, 32:96, 32:96] = 0
    ts = torch.linspace(0, 1.0 - cfg.evaluation.eval_eps, 4, dtype=torch.float64).to(DEV)
    sampler = get_module("samplers", "ip_em_sde")(cfg, sde, net)
    dg = torch.Generator().manual_seed(17)
    sampler.draw_fn = lambda shape, dtype, device: torch.randn(*shape, generator=dg, dtype=torch.float64).to(device=device, dtype=dtype)
    log = []
    _record(monkeypatch, log)
    with settings("bf16x3", "f16"):
        out = sampler.sample((x0.to(DEV), mask.to(DEV)), ts, 3, denoise=True, eps=cfg.evaluation.eval_eps)
    monkeypatch.undo()
    names = [n for n, _ in log]
    assert bool(torch.isfinite(out).all())
    assert [n for n in names if n in F16] and not [n for n in names if n in ("conv3x3_wino", "conv3x3_wino_gn")]


def test_class_conditional_sampler_under_f16(golden, monkeypatch):
    """3 cc_em_sde steps of the tiny configuration: finite; the classifier's recording guidance pass takes no fp16 launch."""
    from psld_amd.registry import get_module
    from tests.test_model_gpu import _build, _build_clf
    g = golden("clf_tiny.npz")
    clf, ccfg, meta = _build_clf()
    net, dcfg, _ = _build("tiny")
    root = C.with_clf(dcfg, ccfg)
    root.clf.evaluation.clf_temp = meta["clf_temp"]
    root.clf.evaluation.label_to_sample = int(T(g["label_cc5"])) if T(g["label_cc5"]).dim() == 0 else T(g["label_cc5"])
    sde = get_module("sde", "psld")(dcfg)
    sampler = get_module("samplers", "cc_em_sde")(root, sde, net, clf)
    noise = T(g["noise_cc5"]).to(DEV)
    sampler.noise_fn = lambda i, x: noise[i]
    phase = ["score"]
    guidance = sampler._guidance

    def in_clf(x32, t):
        phase[0] = "clf"
        try:
            return guidance(x32, t)
        finally:
            phase[0] = "score"
    sampler._guidance = in_clf
    log = []
    _record(monkeypatch, log, lambda: phase[0])
    with settings("bf16x3", "f16", winograd=2):
        x = sampler.sample(T(g["batch_cc5"]).to(DEV), T(g["ts_cc5"]).to(DEV)[:4], 3, denoise=True, eps=dcfg.evaluation.eval_eps)
    monkeypatch.undo()
    assert x.dtype == torch.float64 and bool(torch.isfinite(x).all())
    assert not [n for n, p in log if p == "clf" and n in F16]


# ---------------------------------------------------------------------------------------------------------------------
# nothing else moved
# ---------------------------------------------------------------------------------------------------------------------
def _tiny128():
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    cfg = C.tiny(nf=128, ch_mult=(1, 1))
    net = get_module("score_fn", "ncsnpp")(cfg)
    net.load_state_dict(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7))
    return net.to(DEV), cfg


def test_limb_modes_are_bitwise_the_same_around_a_visit_to_f16():
    net, _ = _tiny128()
    net.eval()
    x0, _, t = synth_inputs(4, 3, 16, seed=3)
    x = torch.cat([x0, torch.zeros_like(x0)], 1).to(DEV)
    t = t.float().to(DEV)
    out = {}
    for tag in ("before", "after"):
        for mode in ("bf16x6", "bf16x3"):
            with settings(mode, "limb", winograd=2, fused_gn=2), torch.no_grad():
                out[tag, mode] = net(x, t)
        if tag == "before":
            with settings("bf16x3", "f16", winograd=2, fused_gn=2), torch.no_grad():
                out["f16"] = net(x, t)
    for mode in ("bf16x6", "bf16x3"):
        assert torch.equal(out["before", mode], out["after", mode]), mode
    assert not torch.equal(out["f16"], out["before", "bf16x3"])
    d = rel_l2(out["f16"], out["before", "bf16x6"])
    print(f"tiny 128-channel network: f16 vs bf16x6 {d:.3e}")
    assert 1e-5 < d < 1e-2


def test_recording_pass_under_f16_is_the_bf16x3_pass(monkeypatch):
    """Forward + backward of a training-mode network under PSLD_MATH=f16's settings: outputs and every parameter gradient
    bitwise those of 'bf16x3', and no fp16 launch."""
    from psld_amd.registry import get_module
    res, log = {}, []
    for ev in ("limb", "f16"):
        with settings("bf16x3", ev, winograd=2):
            net, cfg = _tiny128()
            net.train()
            cfg.model.score_fn.dropout = 0.0
            sde = get_module("sde", "psld")(cfg)
            crit = get_module("losses", "psld_score_loss")(cfg, sde)
            x0, eps, t = synth_inputs(4, 3, 16, seed=3)
            if ev == "f16":
                _record(monkeypatch, log)
            loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
            loss.backward()
            res[ev] = (loss.detach().clone(), net.flat_grad().clone())
            monkeypatch.undo()
    names = [n for n, _ in log]
    assert names and not [n for n in names if n in F16], sorted(set(names))
    assert torch.equal(res["limb"][0], res["f16"][0]) and torch.equal(res["limb"][1], res["f16"][1])


def test_captured_graph_is_keyed_by_eval_math():
    net, _ = _tiny128()
    net.eval()
    x0, _, t = synth_inputs(4, 3, 16, seed=3)
    x = torch.cat([x0, torch.zeros_like(x0)], 1).to(DEV)
    t = t.float().to(DEV)
    try:
        with settings("bf16x3", "limb", winograd=2, fused_gn=2), torch.no_grad():
            e3 = net(x, t)
            net.enable_graphs(True)
            g3 = net(x, t)
        with settings("bf16x3", "f16", winograd=2, fused_gn=2), torch.no_grad():
            g16 = net(x, t)
            g16b = net(x, t)
        with settings("bf16x3", "limb", winograd=2, fused_gn=2), torch.no_grad():
            g3b = net(x, t)
        net.enable_graphs(False)
        with settings("bf16x3", "f16", winograd=2, fused_gn=2), torch.no_grad():
            e16 = net(x, t)
    finally:
        net.enable_graphs(False)
    assert torch.equal(e3, g3) and torch.equal(g3, g3b)
    assert torch.equal(e16, g16) and torch.equal(g16, g16b)
    assert not torch.equal(g3, g16)


def test_dispatch_at_b16(monkeypatch):
    """C10-SOTA at B = 16 under the default policy and PSLD_MATH=f16's settings: a non-recording forward issues no two-limb
    launch where an fp16 form exists (Winograd forward, wide pointwise)."""
    from psld_amd import ops as o
    from tests.test_model_gpu import _build
    net, _, _ = _build("c10_sota")
    gg = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(16, 6, 32, 32, device=DEV, generator=gg)
    t = torch.rand(16, device=DEV, generator=gg) * 0.9 + 0.05
    log = []
    _record(monkeypatch, log)
    with settings("bf16x3", "f16"), torch.no_grad():
        y = net(x, t)
    monkeypatch.undo()
    names = [n for n, _ in log]
    print("B=16 launches under f16:", {n: names.count(n) for n in set(names)})
    assert bool(torch.isfinite(y).all())
    assert "gemm_split_f16" in names and ("conv3x3_wino_f16" in names or "conv3x3_wino_gn_f16" in names)
    assert not [n for n in names if n in LIMB2 + ("conv3x3_wino", "conv3x3_wino_gn")], sorted(set(names))
    assert o.eval_math() == "limb"

"""The ends of wino_conv8s_kernel (conv_wino.hip): set-up without runtime divisions (shifts, proven multiply-shifts, host
constants), the peeled last channel chunk and the in-place epilogue with 32-bit offsets from scalar bases.

Every launch runs through tests/guard.py:run_guarded - once on ordinary buffers, once on exact-size buffers between 0xFF
bands: outputs prefilled with NaN must come out finite and bit-equal in both runs, no input and no band byte may change -
and is compared with an fp64 torch convolution at the gates of tests/test_kernels_gpu.py (rel-L2 < 3e-6; 5e-6 for the
GroupNorm-fused staging) or, for two limbs, with tests/x3_ref.py at the gate of tests/test_math_x3_gpu.py (3e-6).

Shapes are the smallest that reach each path: one, two and three chunks per workgroup (the peeled chunk is the first one at
c_in = 32), two sources with the last chunk in the second, every region geometry (4 / 2 / 1 images per region with absent
images in the last one, 16x16, 32x32, 4 x 32 blocks of 64- and 128-wide maps, a non-square map whose regions per image are
no power of two), whole and cut-short channel tiles, a split-chunk launch and a data-gradient fragment set."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import guard as G
from tests import x3_ref as X
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 1 << 28)
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.fixture
def guard(ops, pool, monkeypatch):
    if pool.regions:
        pool.check()
        pool.release()
    return G.Guard(ops, pool).install(monkeypatch)


def nan(*shape):
    return torch.full(shape, NAN, device=DEV)


# b, c1, c2, co, h, w
SHAPES = {
    "4x8_b3_32to128": (3, 32, 0, 128, 4, 8),            # one chunk; four images per region, one of them absent
    "8x8_b3_64to128": (3, 64, 0, 128, 8, 8),            # two chunks; two images per region, the last region half empty
    "16x16_b2_96to256": (2, 96, 0, 256, 16, 16),        # three chunks, two channel tiles
    "16x16_b2_32+32to160": (2, 32, 32, 160, 16, 16),    # the last chunk lies in source 2; the last channel tile cut short
    "32x32_b1_32to128": (1, 32, 0, 128, 32, 32),
    "64x64_b1_64to128": (1, 64, 0, 128, 64, 64),        # 4 x 32 blocks, two per row band
    "4x128_b1_32to160": (1, 32, 0, 160, 4, 128),        # a 128-wide map: four blocks per row band, cut-short tile
    "12x32_b2_32to128": (2, 32, 0, 128, 12, 32),        # three regions per image: the division that stays on the scalar unit
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the fp64 convolution of a shape: computed once, shared by the tests, never written."""
    b, c1, c2, co, h, w_ = SHAPES[name]
    x = gen(b, c1 + c2, h, w_, seed=40)
    w = gen(co, c1 + c2, 3, 3, seed=41, scale=0.1)
    return dict(x=x, w=w, conv=F.conv2d(x.double(), w.double(), padding=1), bias=gen(co, seed=42),
                res=gen(b, co, h, w_, seed=43), temb=gen(b, co, seed=44), temb2=gen(2 * b, co, seed=45),
                prev=gen(b, co, h, w_, seed=46))


def _forms(c, b, co, h, w_):
    """name -> (epilogue keywords naming tensors of the call, leading dimension of y, initial y, fp64 reference)"""
    conv, bias, res, temb, prev = c["conv"], c["bias"].double()[None, :, None, None], c["res"].double(), c["temb"].double(), c["prev"]
    half = c["temb2"].double().view(b, 2, co).permute(0, 2, 1)[:, :, :, None].repeat_interleave(h // 2, 2)     # [b][co][h][1]
    return {
        "plain": (dict(), co, None, conv),
        "bias": (dict(bias="bias"), co, None, conv + bias),
        "rowbias": (dict(rowbias="temb", rows_per_img=h * w_), co, None, conv + temb[:, :, None, None]),
        # a row bias of another granularity (one row per half image): the kernel's division path
        "rowbias_half": (dict(rowbias="temb2", rows_per_img=h * w_ // 2), co, None, conv + half),
        "residual_wide": (dict(residual="res_wide", ld_residual=co + 32), co, None, conv + res),
        "accumulate": (dict(alpha=0.5, accumulate=True), co, prev, 0.5 * conv + prev.double()),
        "scales": (dict(bias="bias", alpha=1.5, out_scale=0.7), co, None, (1.5 * conv + bias) * 0.7),
        "full_wide_y": (dict(bias="bias", rowbias="temb", rows_per_img=h * w_, residual="res_wide", ld_residual=co + 32,
                             out_scale=0.7), co + 32, None, (conv + bias + temb[:, :, None, None] + res) * 0.7),
    }


@pytest.mark.parametrize("name", list(SHAPES))
def test_wino_epilogue_forms(ops, guard, name):
    """Three limbs, every epilogue form, against fp64 torch: rel-L2 < 3e-6 (the gate of test_conv3x3_wino_forward)."""
    b, c1, c2, co, h, w_ = SHAPES[name]
    assert ops.conv3x3_wino_supported(c1, c2, b, h, w_, co)
    c = _case(name)
    x1 = _nhwc(c["x"][:, :c1]).to(DEV)
    x2 = _nhwc(c["x"][:, c1:]).to(DEV) if c2 else None
    res_wide = gen(b, h, w_, co + 32, seed=47)
    res_wide[..., :co] = _nhwc(c["res"])
    base = dict(x1=x1, x2=x2, frag=ops.conv3x3_wino_frag(c["w"].to(DEV), False), bias=c["bias"].to(DEV), temb=c["temb"].to(DEV),
                temb2=c["temb2"].to(DEV), res_wide=res_wide.to(DEV))
    errs = {}
    for form, (kw, ldy, init, ref) in _forms(c, b, co, h, w_).items():
        y0 = nan(b, h, w_, ldy) if init is None else _nhwc(init).to(DEV)

        def fn(x1, x2, frag, bias, temb, temb2, res_wide, y):
            t = dict(bias=bias, temb=temb, temb2=temb2, res_wide=res_wide)
            epi = ops.epilogue(**{k: (t[v] if isinstance(v, str) else v) for k, v in kw.items()})
            ops.conv3x3_wino(x1, x2, frag, co, y, epi, ldy=ldy)
        plain, _ = G.run_guarded(guard, fn, dict(base, y=y0), {"y": co} if ldy > co else ["y"])
        errs[form] = rel_l2(plain["y"][..., :co].permute(0, 3, 1, 2), ref)
        print(f"wino ends {name} {form}: {errs[form]:.2e}")
    assert all(e < 3e-6 for e in errs.values()), errs


@pytest.mark.parametrize("name,fine", [("8x8_b3_64to128", 4), ("16x16_b2_96to256", 8), ("32x32_b1_32to128", 4)])
def test_wino_epilogue_gn_partial_sums(ops, guard, name, fine):
    """GroupNorm partial sums of the output in both granularities (4 channels for a 128-channel output, else 8), checked as
    test_gn_partials_from_wino_epilogue does: statistics from the partial sums against a statistics pass over the output."""
    b, c1, c2, co, h, w_ = SHAPES[name]
    c = _case(name)
    assert ops.gn_part_supported(b, h * w_, co)
    part = ops.gn_part_buffer(b, h * w_, co, DEV)
    part.fill_(NAN)
    assert part.fine_width == fine
    t = dict(x1=_nhwc(c["x"]).to(DEV), frag=ops.conv3x3_wino_frag(c["w"].to(DEV), False), bias=c["bias"].to(DEV),
             y=nan(b, h, w_, co), part=part)

    def fn(x1, frag, bias, y, part):
        ops.conv3x3_wino(x1, None, frag, co, y, ops.epilogue(bias=bias, gn_part=part, gn_hw=h * w_))
    plain, _ = G.run_guarded(guard, fn, t, ["y", "part"])
    y, part = plain["y"], plain["part"]
    assert rel_l2(y.permute(0, 3, 1, 2), c["conv"] + c["bias"].double()[None, :, None, None]) < 3e-6
    gamma, beta = (1 + 0.1 * gen(co, seed=73)).to(DEV), (0.1 * gen(co, seed=74)).to(DEV)
    for groups in (co // fine, co // 8, co // 16):
        st = ops.gn_stats_from_part(part, y.shape, gamma, beta, groups=groups)
        ref = ops.gn_stats(y, gamma, beta, groups=groups)
        assert rel_l2(st.mean, ref.mean) < 1e-5 and rel_l2(st.rstd, ref.rstd) < 1e-5


@pytest.mark.parametrize("name", ["16x16_b2_96to256", "32x32_b1_32to128", "64x64_b1_64to128"])
def test_wino_ends_fused_groupnorm(ops, guard, name):
    """The GroupNorm-fused staging (GNF instantiation): bitwise the apply pass + convolution, and within 5e-6 of fp64
    GroupNorm + SiLU + convolution (the gate of test_conv3x3_wino_fused_groupnorm)."""
    b, c1, c2, co, h, w_ = SHAPES[name]
    assert ops.conv3x3_wino_gn_supported(c1, c2, b, h, w_, co)
    c = _case(name)
    xs = c["x"] * 1.5 + 0.3
    x1 = _nhwc(xs).to(DEV)
    g1, b1 = (gen(c1, seed=74) * 0.2 + 1.0).to(DEV), (gen(c1, seed=75) * 0.1).to(DEV)
    st1 = ops.gn_stats(x1, g1, b1)
    frag = ops.conv3x3_wino_frag(c["w"].to(DEV), False)
    t = dict(x1=x1, st1=st1, frag=frag, bias=c["bias"].to(DEV), res=_nhwc(c["res"]).to(DEV), y=nan(b, h, w_, co))

    def fn(x1, st1, frag, bias, res, y):
        ops.conv3x3_wino_gn(x1, st1, None, None, True, frag, co, y, ops.epilogue(bias=bias, residual=res, ld_residual=co, out_scale=0.7))
    plain, _ = G.run_guarded(guard, fn, t, ["y"])
    y_un = nan(b, h, w_, co)
    ops.conv3x3_wino(ops.gn_apply(x1, st1, True), None, frag, co, y_un,
                     ops.epilogue(bias=t["bias"], residual=t["res"], ld_residual=co, out_scale=0.7))
    assert torch.equal(plain["y"], y_un)
    a = F.silu(F.group_norm(xs.double(), ops.gn_groups(c1), g1.double().cpu(), b1.double().cpu(), eps=1e-6))
    ref = (F.conv2d(a, c["w"].double(), c["bias"].double(), padding=1) + c["res"].double()) * 0.7
    err = rel_l2(plain["y"].permute(0, 3, 1, 2), ref)
    print(f"wino ends fused GroupNorm {name}: {err:.2e}")
    assert err < 5e-6


@pytest.mark.parametrize("name", ["4x8_b3_32to128", "16x16_b2_32+32to160", "64x64_b1_64to128"])
def test_wino_ends_two_limbs(ops, guard, name):
    """The two-limb instantiations (whole and cut-short tiles; one chunk, and the last chunk in source 2) against the two-limb
    reference of tests/x3_ref.py within 3e-6 (the gate of test_conv3x3_wino_x3_forward), full epilogue."""
    b, c1, c2, co, h, w_ = SHAPES[name]
    c = _case(name)
    x1 = _nhwc(c["x"][:, :c1]).to(DEV)
    x2 = _nhwc(c["x"][:, c1:]).to(DEV) if c2 else None
    t = dict(x1=x1, x2=x2, frag=ops.conv3x3_wino_frag_x3(c["w"].to(DEV)), bias=c["bias"].to(DEV), temb=c["temb"].to(DEV),
             res=_nhwc(c["res"]).to(DEV), y=nan(b, h, w_, co))

    def fn(x1, x2, frag, bias, temb, res, y):
        ops.conv3x3_wino_x3(x1, x2, frag, co, y, ops.epilogue(bias=bias, rowbias=temb, rows_per_img=h * w_, residual=res,
                                                              ld_residual=co, out_scale=0.7))
    plain, _ = G.run_guarded(guard, fn, t, ["y"])
    emu = X.two_limb_conv3x3(c["x"], c["w"])
    ref = (emu + c["bias"].double()[None, :, None, None] + c["temb"].double()[:, :, None, None] + c["res"].double()) * 0.7
    err = rel_l2(plain["y"].permute(0, 3, 1, 2), ref)
    print(f"wino ends two limbs {name}: {err:.2e}")
    assert err <= 3e-6


def test_wino_ends_split_chunk_launch(ops, guard):
    """B = 2, 8x8, c_in = 128: one pixel tile, so the four chunks split over workgroups of two chunks each (plain partial
    outputs, the epilogue in the reduction pass); full epilogue against fp64 within 3e-6."""
    b, ci, co, s = 2, 128, 128, 8
    assert ops.conv3x3_wino_ws_bytes(ci, 0, b, s, s, co) > 0
    x, w = gen(b, ci, s, s, seed=40), gen(co, ci, 3, 3, seed=41, scale=0.1)
    bias, res, temb = gen(co, seed=42), gen(b, co, s, s, seed=43), gen(b, co, seed=44)
    ref = (F.conv2d(x.double(), w.double(), bias.double(), padding=1) + temb.double()[:, :, None, None] + res.double()) * 0.7
    t = dict(x1=_nhwc(x).to(DEV), frag=ops.conv3x3_wino_frag(w.to(DEV), False), bias=bias.to(DEV), temb=temb.to(DEV),
             res=_nhwc(res).to(DEV), y=nan(b, s, s, co))

    def fn(x1, frag, bias, temb, res, y):
        ops.conv3x3_wino(x1, None, frag, co, y, ops.epilogue(bias=bias, rowbias=temb, rows_per_img=s * s, residual=res,
                                                             ld_residual=co, out_scale=0.7), allow_split=True)
    plain, _ = G.run_guarded(guard, fn, t, ["y"])
    assert guard.workspace_calls >= 1
    err = rel_l2(plain["y"].permute(0, 3, 1, 2), ref)
    print(f"wino ends split chunks: {err:.2e}")
    assert err < 3e-6


def test_wino_ends_data_gradient(ops, guard):
    """A data-gradient fragment set (rotated, role-swapped filter): dx of a 128 -> 64 convolution at 8x8, plain and with the
    backward tape's alpha / accumulate epilogue, against autograd in fp64 within 3e-6 (the gate of test_conv3x3_wino_dgrad)."""
    b, ci, co, s = 3, 128, 64, 8
    x = gen(b, ci, s, s, seed=60).requires_grad_(True)
    w = gen(co, ci, 3, 3, seed=61, scale=0.1).requires_grad_(True)
    y = F.conv2d(x.double(), w.double(), padding=1)
    gy = gen(*y.shape, seed=62)
    y.backward(gy.double())
    assert ops.conv3x3_wino_supported(co, 0, b, s, s, ci)
    prev = gen(b, s, s, ci, seed=63)
    t = dict(gy=_nhwc(gy).to(DEV), frag=ops.conv3x3_wino_frag(w.detach().to(DEV), True), dx=nan(b, s, s, ci), acc=prev.to(DEV))

    def fn(gy, frag, dx, acc):
        ops.conv3x3_wino(gy, None, frag, ci, dx)
        ops.conv3x3_wino(gy, None, frag, ci, acc, ops.epilogue(alpha=0.5, accumulate=True))
    plain, _ = G.run_guarded(guard, fn, t, ["dx", "acc"])
    e1 = rel_l2(plain["dx"].permute(0, 3, 1, 2), x.grad)
    e2 = rel_l2(plain["acc"].permute(0, 3, 1, 2), 0.5 * x.grad + prev.permute(0, 3, 1, 2).double())
    print(f"wino ends data gradient: {e1:.2e} accumulate {e2:.2e}")
    assert e1 < 3e-6 and e2 < 3e-6

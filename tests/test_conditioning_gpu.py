"""GroupNorm, softmax and attention kernels on ill-conditioned inputs (tests/cond_ref.py): groups whose mean is up to 1000
spreads away from zero, spreads of 1e-3 and 1e3, a constant group; peaked, flat and large softmax rows.  Every figure is
taken against an fp64 reference of the fp32 tensor the kernel actually read, and judged either by the project's own
statistics tolerances (rstd 2e-6 relative, mean 2e-6 |mu| + 1e-7, at EVERY ratio and scale) or against what plain torch
fp32 manages on the same input (YARD_FACTOR x its error + a floor).  Each test prints its figures before it asserts.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import cond_ref as R
from tests import f16_ref as H
from tests import x3_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
SWEEP_IDS = [f"r{r}-s{s:g}" for r, s in R.SWEEP]
APPLY_RATIOS = (0, 30, 1000)

# Largest quotient (kernel error / fp32 yardstick error) measured on the MI355X over all cases of a family, with fp64
# statistics sums; the cap is YARD_FACTOR = 4 (+ the floor).  In brackets: the same with the fp32 sums these tests replaced.
#   gn_apply, gn_apply_limb, max-abs of y ........ 1.05 (ratio 0; 1.00 at 30 and 1000)          [2.67 at 30, 102 at 1000]
#   conv3x3_wino_gn f32, rel-L2 .................. 4.00 at ratio 0, where kernel 1.9e-7 / yardstick 4.8e-8 and the 5e-6
#                                                  tolerance decides; below 1.1 at 30 and 1000                [26 at 1000]
#   conv3x3_wino_gn_x3 / _f16, rel-L2 ............ 0.98 / 1.00                                 [26 / 6.4 at 1000]
#   GroupNorm backward dx / dgamma / dbeta ....... 0.94 / 0.89 / 0.79, every kernel kind      [24 / 9.2 / 7.8 at 1000]
#   attn_fwd out / p, rel-L2 ..................... 1.47 / 1.46 (1 x 256 x 256, spread 30); three kernels 1.41 / 1.42
#     dominant key: p quotient 1.00; out 2.3e-10 against a yardstick of 5e-17 - the ATTN_FLOOR decides, no quotient
# Statistics with fp64 sums, worst over every producer and sweep point: rstd 6.0e-8 relative (cap 2e-6), mean 3 % of its cap,
# scale 1.2e-7, shift 37 % of its cap.  softmax_rows: forward rel-L2 9.8e-8, backward 3.7e-8 (fp32 row sum: 0.30).
APPLY_FLOOR = 1e-7
BWD_FLOOR = 1e-6
ATTN_FLOOR = 3e-6           # today's tolerance of test_fused_attention_forward
WINO_GN_TOL = {"f32": 5e-6, "x3": 3e-6, "f16": 3e-6}      # test_conv3x3_wino_fused_groupnorm / test_math_x3_gpu / test_math_f16_gpu


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def affine(c, seed):
    return 1 + 0.2 * gen(c, seed=seed), 0.1 * gen(c, seed=seed + 1)


def check_stats(tag, st, ref, beta):
    """mean, rstd, scale, shift of a GNStats against the fp64 reference of the tensor the GroupNorm reads."""
    dev = ref.mean.device
    e_rstd, e_mean = R.stats_errors(st.mean, st.rstd, ref)
    scale_rel, shift_cap = R.affine_caps(ref, beta)
    e_scale = ((st.scale.double().to(dev) - ref.scale).abs() / ref.scale.abs()).max().item()
    e_shift = ((st.shift.double().to(dev) - ref.shift).abs() / shift_cap).max().item()
    print(f"{tag}: rstd rel {e_rstd:.2e} (cap {R.RSTD_REL:.0e}), mean err/cap {e_mean:.2e}, scale rel {e_scale:.2e} "
          f"(cap {scale_rel:.2e}), shift err/cap {e_shift:.2e}")
    assert e_rstd < R.RSTD_REL and e_mean < 1.0 and e_scale < scale_rel and e_shift < 1.0, tag


# ---------------------------------------------------------------------------------------------------------------------
# statistics: one test per producer
# ---------------------------------------------------------------------------------------------------------------------
# (b, h, c, groups): 32 channels; five channels per group (the other branch of gn_partial_kernel); 384; one half of a
# 256-channel concatenation (its share of the groups, via groups=)
STATS_SHAPES = [(2, 8, 32, None), (2, 16, 160, None), (1, 8, 384, None), (2, 8, 128, 16)]


@pytest.mark.parametrize("ratio,scale", R.SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("b,h,c,groups", STATS_SHAPES)
def test_gn_stats_on_offset_groups(ops, b, h, c, groups, ratio, scale):
    g = groups or ops.gn_groups(c)
    x = R.offset_groups(b, c, h, h, g, ratio, scale, seed=11)
    gamma, beta = affine(c, 12)
    st = ops.gn_stats(R.nhwc(x).to(DEV), gamma.to(DEV), beta.to(DEV), groups=groups)
    check_stats(f"gn_stats {b}x{h}x{h}x{c}/{g} ratio {ratio} scale {scale:g}", st, R.gn_ref64(x, g, gamma, beta, want_y=False), beta)


@pytest.mark.parametrize("b,h,c,groups", [(2, 8, 32, None), (2, 8, 128, 16)])
def test_gn_stats_on_a_constant_group(ops, b, h, c, groups):
    """One (image, group) exactly constant and non-zero, the rest of the image at ratio 1: the variance is clamped at 0
    (rstd = eps^-1/2 exactly as rounded to fp32) or rstd lies within 2e-6 of eps^-1/2; every other group as usual."""
    g = groups or ops.gn_groups(c)
    x = R.set_constant_group(R.offset_groups(b, c, h, h, g, 1, 1.0, seed=13), g, 1, 3, 2.5)
    gamma, beta = affine(c, 14)
    st = ops.gn_stats(R.nhwc(x).to(DEV), gamma.to(DEV), beta.to(DEV), groups=groups)
    want = R.EPS ** -0.5
    got = st.rstd[1, 3].item()
    print(f"constant group {c}/{g}: rstd {got!r} against eps^-1/2 = {want!r}, mean {st.mean[1, 3].item()!r}")
    assert got == torch.tensor(want).float().item() or abs(got - want) < 2e-6 * want
    assert st.mean[1, 3].item() == 2.5
    check_stats(f"constant group {c}/{g}", st, R.gn_ref64(x, g, gamma, beta, want_y=False), beta)


@pytest.mark.parametrize("ratio,scale", R.SWEEP, ids=SWEEP_IDS)
def test_gn_stats_at_the_longest_run_per_thread(ops, ratio, scale):
    """make_map gives a thread at most 64 pixels per chunk, and 64 only when 32 chunks of 256 / (c/4) pixel lanes still
    leave that many: b * hw * c = 2^26 (128 x 32 x 32 x 512).  Input and fp64 reference are formed on the device."""
    b, hw, c, g = 128, 1024, 512, 32
    gd = torch.Generator(device=DEV).manual_seed(15)
    off = R.group_offsets(b, g, ratio, seed=15).float().to(DEV).repeat_interleave(c // g, dim=1)
    x = ((torch.randn(b, hw, c, generator=gd, device=DEV) + off[:, None, :]) * scale).view(b, 32, 32, c)
    gamma, beta = affine(c, 16)
    st = ops.gn_stats(x, gamma.to(DEV), beta.to(DEV))
    ref = R.gn_ref64(x, g, gamma, beta, channels_last=True, want_y=False)
    check_stats(f"gn_stats 128x32x32x512 ratio {ratio} scale {scale:g}", st, ref, beta)


def _offset_epilogue(ops, b, hw, co, ratio, spread, seed):
    """bias [co] and residual [b, hw, co] that add group_offsets(...) * spread to a [b, hw, co] output: the bias carries
    image 0's offsets, the residual the difference of every image to image 0."""
    g = ops.gn_groups(co)
    o = (R.group_offsets(b, g, ratio, seed) * spread).repeat_interleave(co // g, dim=1).float()        # [b, co]
    res = (o - o[:1])[:, None, :].expand(b, hw, co).contiguous()
    return o[0].contiguous().to(DEV), res.to(DEV)


def _epilogue_stats_case(ops, tag, run, b, hw, co, ratio, seed=20):
    """``run(y, epi)`` launches the producer.  First without offsets to measure the output's spread, then with bias and
    residual set to ratio x that spread per (image, group) and the partial sums asked for; the statistics are checked
    against fp64 moments of the fp32 output read back from the device - the tensor the GroupNorm reads."""
    assert ops.gn_part_supported(b, hw, co)
    y = torch.empty(b, hw, co, device=DEV)
    run(y, None)
    spread = y.double().std().item()
    bias, res = _offset_epilogue(ops, b, hw, co, ratio, spread, seed)
    part = ops.gn_part_buffer(b, hw, co, DEV)
    part.fill_(float("nan"))
    y.fill_(float("nan"))
    run(y, ops.epilogue(bias=bias, residual=res, ld_residual=co, gn_part=part, gn_hw=hw))
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(y).all())
    y_plain = torch.empty_like(y)
    run(y_plain, ops.epilogue(bias=bias, residual=res, ld_residual=co))
    assert torch.equal(y, y_plain)
    gamma, beta = affine(co, seed + 1)
    h = int(round(hw ** 0.5))
    for groups in (None, ops.gn_groups(2 * co) // 2):            # own GroupNorm / as one half of a concatenation
        g = groups or ops.gn_groups(co)
        st = ops.gn_stats_from_part(part, (b, h, h, co), gamma.to(DEV), beta.to(DEV), groups=groups)
        ref = R.gn_ref64(y.view(b, h, h, co), g, gamma, beta, channels_last=True, want_y=False)
        check_stats(f"{tag} /{g} ratio {ratio}", st, ref, beta)


def _conv_inputs(b, c, co, h, scale, seed):
    x = gen(b, h, h, c, seed=seed).to(DEV)
    w = (gen(co, c, 3, 3, seed=seed + 1, scale=0.1) * scale).to(DEV)
    return x, w


@pytest.mark.parametrize("ratio,scale", R.SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("b,c,co,h", [(6, 128, 256, 16), (8, 128, 128, 8)])         # eight- / four-channel sums
def test_gn_partials_of_the_limb_conv_epilogue_on_offset_groups(ops, b, c, co, h, ratio, scale):
    """The direct limb 3x3 kernel's own epilogue (conv_split.hip): launched WITHOUT a workspace, so that these small grids do
    not take the split-K route (ops.conv3x3_split always offers one; that route is the split-launch test below)."""
    x, w = _conv_inputs(b, c, co, h, scale, 30)
    wf = ops.conv3x3_frag(w, False)

    def run(y, epi):
        ops.conv3x3_split(x, None, wf, co, y.view(b, h, h, co), epi, workspace=False)
    _epilogue_stats_case(ops, f"limb conv epilogue {b}x{c}->{co}@{h} scale {scale:g}", run, b, h * h, co, ratio)


@pytest.mark.parametrize("ratio,scale", R.SWEEP, ids=SWEEP_IDS)
def test_gn_partials_of_the_pointwise_epilogue_on_offset_groups(ops, ratio, scale):
    b, h, c, co = 6, 16, 128, 256
    m = b * h * h
    x = gen(m, c, seed=32).to(DEV)
    gf = ops.gemm_frag((gen(co, c, seed=33, scale=0.1) * scale).to(DEV), co, c, c, 1)

    def run(y, epi):            # no workspace: the kernel's own epilogue, not the split-K reduction
        ops.gemm_split(x, None, m, gf, co, y, epi, workspace=False)
    _epilogue_stats_case(ops, f"pointwise epilogue {m}x{c}->{co} scale {scale:g}", run, b, h * h, co, ratio)


# The Winograd kernel's gn_part branch is taken by every launch without a workspace whose output has whole 128-channel
# tiles and maps of a multiple of 64 pixels (wino_conv's argument check); the batch does not enter.  So: the issue's 64-wide
# map (4 x 32 pixel blocks, four-channel sums) as it is, its 32 x 32 case at batch 3 instead of 24, and an 8 x 8 map, where a
# tile block is one of the two images of a region and an odd batch leaves the last region half empty (img < B).
@pytest.mark.parametrize("ratio,scale", R.SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("b,c,co,h", [(6, 32, 128, 64), (3, 128, 256, 32), (3, 128, 256, 8)])
def test_gn_partials_of_the_winograd_epilogue_on_offset_groups(ops, b, c, co, h, ratio, scale):
    assert ops.conv3x3_wino_supported(c, 0, b, h, h, co)
    x, w = _conv_inputs(b, c, co, h, scale, 34)
    uf = ops.conv3x3_wino_frag(w, False)

    def run(y, epi):
        ops.conv3x3_wino(x, None, uf, co, y.view(b, h, h, co), epi)         # allow_split=False: no workspace
    _epilogue_stats_case(ops, f"winograd epilogue {b}x{c}->{co}@{h} scale {scale:g}", run, b, h * h, co, ratio)


@pytest.mark.parametrize("ratio,scale", R.SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("b,c,co,h", [(8, 128, 128, 8), (3, 512, 256, 8)])
def test_gn_partials_of_split_launches_on_offset_groups(ops, b, c, co, h, ratio, scale):
    """The shapes of test_gn_partials_from_split_launches: grids that split K and finish through
    conv_reduce_epilogue_gn_kernel - direct limb kernel, Winograd form with allow_split, pointwise form."""
    x, w = _conv_inputs(b, c, co, h, scale, 36)
    wf = ops.conv3x3_frag(w, False)
    m = b * h * h

    def took_the_split_route(launch):
        """The split route leaves its partial outputs at the start of the stream's workspace: poison it, launch, look."""
        ws = ops.workspace(64 << 20, x.device)[:2 * m * co * 4].view(torch.float32)      # (grow-only: the launch gets this buffer)
        ws.fill_(float("nan"))
        launch()
        return bool(torch.isfinite(ws).all())
    y0 = torch.empty(b, h, h, co, device=DEV)
    assert took_the_split_route(lambda: ops.conv3x3_split(x, None, wf, co, y0, None))
    assert not took_the_split_route(lambda: ops.conv3x3_split(x, None, wf, co, y0, None, workspace=False))
    _epilogue_stats_case(ops, f"split launch, direct {b}x{c}->{co}@{h} scale {scale:g}",
                         lambda y, epi: ops.conv3x3_split(x, None, wf, co, y.view(b, h, h, co), epi), b, h * h, co, ratio)
    if ops.conv3x3_wino_supported(c, 0, b, h, h, co) and ops.conv3x3_wino_ws_bytes(c, 0, b, h, h, co) > 0:
        uf = ops.conv3x3_wino_frag(w, False)
        _epilogue_stats_case(ops, f"split launch, winograd {b}x{c}->{co}@{h} scale {scale:g}",
                             lambda y, epi: ops.conv3x3_wino(x, None, uf, co, y.view(b, h, h, co), epi, allow_split=True),
                             b, h * h, co, ratio)
    gf = ops.gemm_frag((gen(co, c, seed=38, scale=0.1) * scale).to(DEV), co, c, c, 1)
    assert took_the_split_route(lambda: ops.gemm_split(x.view(m, c), None, m, gf, co, y0.view(m, co), None))
    _epilogue_stats_case(ops, f"split launch, pointwise {m}x{c}->{co} scale {scale:g}",
                         lambda y, epi: ops.gemm_split(x.view(m, c), None, m, gf, co, y.view(m, co), epi), b, h * h, co, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# apply and its consumers
# ---------------------------------------------------------------------------------------------------------------------
def _yard(tag, err, yard, floor):
    cap = R.YARD_FACTOR * yard + floor
    print(f"{tag}: kernel {err:.3e}, fp32 yardstick {yard:.3e}, quotient {err / max(yard, 1e-300):.2f}, cap {cap:.3e}")
    return err <= cap


@pytest.fixture(scope="module")
def apply_case():
    """128 channels @ 32 x 32, b = 1, per ratio: input, affine, fp64 reference and fp32 yardstick (shared, never written)."""
    out = {}
    for ratio in APPLY_RATIOS:
        x = R.offset_groups(1, 128, 32, 32, 32, ratio, 1.0, seed=40)
        gamma, beta = affine(128, 41)
        out[ratio] = (x, gamma, beta, R.gn_ref64(x, 32, gamma, beta), R.gn_yard32(x, 32, gamma, beta))
    return out


@pytest.mark.parametrize("ratio", APPLY_RATIOS)
@pytest.mark.parametrize("act", [False, True])
def test_gn_apply_on_offset_groups(ops, apply_case, ratio, act):
    x, gamma, beta, ref, yard = apply_case[ratio]
    xd = R.nhwc(x).to(DEV)
    st = ops.gn_stats(xd, gamma.to(DEV), beta.to(DEV))
    want = F.silu(ref.y) if act else ref.y
    y32 = F.silu(yard.y) if act else yard.y
    e_yard = (y32.double() - want).abs().max().item()
    ok = True
    for name, y in (("gn_apply", ops.gn_apply(xd, st, act)), ("gn_apply_limb", ops.limb_to_f32(ops.gn_apply_limb(xd, st, act)))):
        err = (y.permute(0, 3, 1, 2).double().cpu() - want).abs().max().item()
        ok &= _yard(f"{name} act={act} ratio {ratio}", err, e_yard, APPLY_FLOOR)
    assert ok


@pytest.mark.parametrize("ratio", APPLY_RATIOS)
@pytest.mark.parametrize("mode", ["f32", "x3", "f16"])
def test_conv3x3_wino_gn_on_offset_groups(ops, apply_case, mode, ratio):
    """GroupNorm + SiLU inside the Winograd staging, 128 -> 128 @ 32 x 32: against 'apply in fp64, then the mode's own
    reference' (fp64 convolution / tests/x3_ref.py / tests/f16_ref.py).  The yardstick is the same reference behind torch's
    fp32 GroupNorm + SiLU; the bound is the larger of the mode's tolerance at ratio 0 and YARD_FACTOR x the yardstick."""
    x, gamma, beta, ref, yard = apply_case[ratio]
    co = 128
    assert ops.conv3x3_wino_gn_supported(128, 0, 1, 32, 32, co)
    w = gen(co, 128, 3, 3, seed=42, scale=0.05)
    bias = gen(co, seed=43)
    xd = R.nhwc(x).to(DEV)
    st = ops.gn_stats(xd, gamma.to(DEV), beta.to(DEV))
    y = torch.full((1, 32, 32, co), float("nan"), device=DEV)
    e = ops.epilogue(bias=bias.to(DEV))
    if mode == "f32":
        ops.conv3x3_wino_gn(xd, st, None, None, True, ops.conv3x3_wino_frag(w.to(DEV), False), co, y, e)
        conv = lambda a: F.conv2d(a.double(), w.double(), padding=1)
    elif mode == "x3":
        ops.conv3x3_wino_gn_x3(xd, st, None, None, True, ops.conv3x3_wino_frag_x3(w.to(DEV)), co, y, e)
        conv = lambda a: X.two_limb_conv3x3(a.float(), w)
    else:
        ops.conv3x3_wino_gn_f16(xd, st, None, None, True, ops.conv3x3_wino_frag_f16(w.to(DEV)), co, y, e)
        conv = lambda a: H.f16_conv3x3(a.float(), w)
    want = conv(F.silu(ref.y)) + bias.double()[None, :, None, None]
    y32 = conv(F.silu(yard.y)) + bias.double()[None, :, None, None]
    err, e_yard = R.rel_l2(y.permute(0, 3, 1, 2), want), R.rel_l2(y32, want)
    cap = max(WINO_GN_TOL[mode], R.YARD_FACTOR * e_yard)
    print(f"conv3x3_wino_gn {mode} ratio {ratio}: kernel {err:.3e}, fp32 yardstick {e_yard:.3e}, "
          f"quotient {err / max(e_yard, 1e-300):.2f}, cap {cap:.3e}")
    assert err <= cap


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", APPLY_RATIOS)
@pytest.mark.parametrize("kind,b,s,c", [("auto", 5, 16, 128), ("one_slab", 5, 16, 128), ("colsum", 3, 8, 256),
                                        ("colsum", 2, 4, 512), ("team", 5, 16, 128)])
def test_gn_backward_on_offset_groups(ops, kind, b, s, c, ratio):
    """dx, dgamma, dbeta of SiLU(GroupNorm(x)) with the statistics of ops.gn_stats on the same offset input, against fp64
    autograd; the yardstick is fp32 autograd of F.group_norm + F.silu."""
    g = ops.gn_groups(c)
    x = R.offset_groups(b, c, s, s, g, ratio, 1.0, seed=50)
    gamma, beta = affine(c, 51)
    dy = gen(b, c, s, s, seed=53)

    def autograd(dt):
        xr, gr, br = (t.to(dt).requires_grad_(True) for t in (x, gamma, beta))
        F.silu(F.group_norm(xr, g, gr, br, R.EPS)).backward(dy.to(dt))
        return xr.grad, gr.grad, br.grad
    want, yard = autograd(torch.float64), autograd(torch.float32)
    xd, dyd, gd, bd = R.nhwc(x).to(DEV), R.nhwc(dy).to(DEV), gamma.to(DEV), beta.to(DEV)
    st = ops.gn_stats(xd, gd, bd)
    dx = torch.full_like(xd, float("nan"))
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    initial = ops.get_gn_bwd_kernel()
    try:
        ops.set_gn_bwd_kernel("one_slab" if kind == "one_slab" else "auto")
        if kind == "team":
            k = ops.gn_bwd_team_rows(b, s * s, c)
            assert k > 0
            sums = ops.gn_bwd_team(dyd, xd, st, gd, bd, True, dx)
            ops.param_reduce2(sums, sums.view(-1)[c:], b * k, 2 * c, c, db, dg)
            assert ops.gn_team_errors(xd.device) == 0
        elif kind == "colsum":
            assert ops.gn_bwd_colsum_supported(b, s * s, c)
            cols = torch.full((b, c), float("nan"), device=DEV)
            ops.gn_bwd(dyd, xd, st, gd, bd, True, dx, dg, db, colsum_img=cols, ld_img=c)
            mag = dx.double().abs().sum(dim=(1, 2)).clamp_min(1e-30)
            assert ((cols.double() - dx.double().sum(dim=(1, 2))).abs() / mag).max().item() < 2e-6
        else:
            ops.gn_bwd(dyd, xd, st, gd, bd, True, dx, dg, db)
    finally:
        ops.set_gn_bwd_kernel(initial)
    ok = True
    for name, got, w64, y32 in zip(("dx", "dgamma", "dbeta"), (dx.permute(0, 3, 1, 2), dg, db), want, yard):
        ok &= _yard(f"gn_bwd {kind} {b}x{s}x{s}x{c} ratio {ratio} {name}", R.rel_l2(got, w64), R.rel_l2(y32, w64), BWD_FLOOR)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# softmax rows, attention, cross entropy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,param", R.SOFTMAX_KINDS, ids=[f"{k}-{p:g}" for k, p in R.SOFTMAX_KINDS])
@pytest.mark.parametrize("L", [64, 100, 256, 1024])        # the register kernels and the generic one
def test_softmax_rows_on_peaked_flat_and_large_rows(ops, L, kind, param):
    rows = 37
    x = R.softmax_rows(kind, param, rows, L, seed=60)
    want = R.softmax_ref64(x)
    xd = x.to(DEV)
    y = torch.full((rows, L), float("nan"), device=DEV)
    ops.softmax_rows(xd, y, rows, L)
    assert bool(torch.isfinite(y).all())
    yc = y.double().cpu()
    e_sum, err = (yc.sum(-1) - 1).abs().max().item(), R.rel_l2(yc, want)
    dy = gen(rows, L, seed=61)
    dx = torch.full((rows, L), float("nan"), device=DEV)
    ops.softmax_rows_bwd(y, dy.to(DEV), dx, rows, L)
    assert bool(torch.isfinite(dx).all())
    e_bwd = R.rel_l2(dx, R.softmax_bwd_ref64(y.cpu(), dy))
    print(f"softmax_rows {kind} {param:g} L={L}: row sums off by {e_sum:.2e}, rel-L2 {err:.2e}, backward rel-L2 {e_bwd:.2e}")
    assert e_sum < 1e-6 and err < 1e-6 and e_bwd < 1e-5
    if kind == "const":
        e_flat = ((yc - 1.0 / L).abs().max() * L).item()
        print(f"  repeated value {param:g}: worst relative distance from 1/L {e_flat:.2e}")
        assert e_flat < 1e-7
    if kind == "dominant":
        assert yc.max(-1).values.min().item() >= 1 - 1e-6
    if kind == "two_max":
        top = y.topk(2, dim=-1).values
        assert torch.equal(top[:, 0], top[:, 1])


def _attn_inputs(b, hw, c, case):
    q, k, v = gen(b, hw, c, seed=70), gen(b, hw, c, seed=71), gen(b, hw, c, seed=72)
    if case == "dominant":          # k rows = q rows times a constant: the diagonal logit |q_i|^2 * 4 / sqrt(c) towers over the rest
        return q, 4.0 * q, v
    s = float(case) ** 0.5          # logits scale * q.k have spread sigma_q * sigma_k = case
    return q * s, k * s, v


@pytest.mark.parametrize("case", [1, 30, 300, "dominant"])
@pytest.mark.parametrize("b,hw,c", [(2, 64, 128), (1, 256, 256)])
def test_attention_on_peaked_rows(ops, b, hw, c, case):
    assert ops.attn_fwd_supported(hw, c)
    q, k, v = _attn_inputs(b, hw, c, case)
    scale = float(c) ** -0.5

    def ref(dt):
        p = torch.softmax(torch.einsum("bic,bjc->bij", q.to(dt), k.to(dt)) * scale, dim=-1)
        return torch.einsum("bij,bjc->bic", p, v.to(dt)), p
    (o64, p64), (o32, p32) = ref(torch.float64), ref(torch.float32)
    yo, yp = R.rel_l2(o32, o64), R.rel_l2(p32, p64)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out = torch.full((b, hw, c), float("nan"), device=DEV)
    p = torch.full((b, hw, hw), float("nan"), device=DEV)
    ops.attn_fwd(qd, kd, vd, c, b, hw, c, scale, out, p)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(p).all())
    tag = f"attn_fwd {b}x{hw}x{c} {case}"
    ok = _yard(f"{tag} out", R.rel_l2(out, o64), yo, ATTN_FLOOR) & _yard(f"{tag} p", R.rel_l2(p, p64), yp, ATTN_FLOOR)
    if case == "dominant":
        assert p.double().cpu().max(-1).values.min().item() >= 1 - 1e-6
    if ops.bgemm_split_supported(0, 1, hw, hw, c):          # the three-kernel path: limb GEMM, softmax rows, limb GEMM
        p3 = torch.empty((b, hw, hw), device=DEV)
        ops.bgemm_split(0, 1, hw, hw, c, qd, c, hw * c, kd, c, hw * c, p3, hw, hw * hw, b, scale)
        ops.softmax_rows(p3, p3, b * hw, hw)
        o3 = torch.empty((b, hw, c), device=DEV)
        ops.bgemm_split(0, 0, hw, c, hw, p3, hw, hw * hw, vd, c, hw * c, o3, c, hw * c, b)
        ok &= _yard(f"{tag} three kernels out", R.rel_l2(o3, o64), yo, ATTN_FLOOR)
        ok &= _yard(f"{tag} three kernels p", R.rel_l2(p3, p64), yp, ATTN_FLOOR)
    assert ok


@pytest.mark.parametrize("mult", [1.0, 1e3])
def test_softmax_xent_on_large_logits(ops, mult):
    """Loss and gradient against fp64 log_softmax.  Bounds: the gradient as test_softmax_xent_and_guide (rel-L2 1e-6); the
    loss 1e-6 relative to max(1, |loss|) - it is stored in fp32, whose rounding alone is 6e-8 |loss|."""
    rows, n = 37, 10
    z = gen(rows, n, seed=80) * mult
    y = torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(81))
    loss, grad, _ = ops.softmax_xent(z.to(DEV), y.to(DEV), 1.0 / rows, 1.0 / rows)
    zr = z.double().requires_grad_()
    ref = -(torch.log_softmax(zr, dim=-1)[torch.arange(rows), y]).mean()
    ref.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    e_loss, e_grad = abs(loss.item() - ref.item()) / max(1.0, abs(ref.item())), R.rel_l2(grad, zr.grad)
    print(f"softmax_xent logits x {mult:g}: loss {loss.item()!r} against {ref.item()!r} (rel {e_loss:.2e}), gradient rel-L2 {e_grad:.2e}")
    assert e_loss < 1e-6 and e_grad < 1e-6

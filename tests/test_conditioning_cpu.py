"""The generators and references of tests/cond_ref.py checked on the CPU: the offset inputs have the mean/std they are
asked for, the fp32 yardstick (torch.var_mean, Welford-style) itself stays inside the statistics caps at every sweep
point - so a kernel that misses them is worse than plain fp32, not up against the format -, and the softmax references
are proper distributions."""
import pytest
import torch

from tests import cond_ref as R

# (b, c, h, groups): the small statistics shapes of the GPU tests (32 channels in 8 groups, five channels per group, 384)
SHAPES = [(2, 32, 8, 8), (2, 160, 16, 32), (1, 384, 8, 32)]


@pytest.mark.parametrize("ratio,scale", R.SWEEP)
@pytest.mark.parametrize("b,c,h,groups", SHAPES)
def test_offset_groups_have_the_requested_mean_over_std(b, c, h, groups, ratio, scale):
    x = R.offset_groups(b, c, h, h, groups, ratio, scale, seed=3)
    assert x.dtype == torch.float32 and x.shape == (b, c, h, h)
    mu, var = R.group_moments64(x, groups)
    want = R.group_offsets(b, groups, ratio, seed=3)
    std = var.sqrt()
    assert ((std / scale - 1).abs() < 0.05).all()
    assert ((mu / std - want).abs() <= 0.05 * want.abs() + 1e-6).all()
    if ratio:
        assert (want.abs() >= 0.5 * ratio).all() and (want.abs() <= ratio).all()
        assert len(set(torch.sign(want).flatten().tolist())) == 2           # both signs occur


def test_ratio_zero_is_zero_mean_unit_spread():
    x = R.offset_groups(2, 32, 8, 8, 8, 0, 1.0, seed=1)
    assert abs(x.mean().item()) < 1e-6 and abs(x.std().item() - 1) < 1e-3


def test_constant_group():
    x = R.set_constant_group(R.offset_groups(2, 32, 8, 8, 8, 1, 1.0, seed=2), 8, 1, 3, 2.5)
    ref = R.gn_ref64(x, 8, torch.ones(32), torch.zeros(32))
    assert ref.rstd[1, 3].item() == pytest.approx(R.EPS ** -0.5, rel=1e-12) and ref.mean[1, 3].item() == 2.5
    assert (ref.y[1, 12:16] == 0).all()
    others = torch.ones(2, 8, dtype=torch.bool)
    others[1, 3] = False
    assert (ref.rstd[others] < 2).all()


@pytest.mark.parametrize("ratio,scale", R.SWEEP)
@pytest.mark.parametrize("b,c,h,groups", SHAPES)
def test_fp32_yardstick_stays_inside_the_statistics_caps(b, c, h, groups, ratio, scale):
    x = R.offset_groups(b, c, h, h, groups, ratio, scale, seed=4)
    gamma = 1 + 0.2 * torch.randn(c, generator=torch.Generator().manual_seed(5))
    beta = 0.1 * torch.randn(c, generator=torch.Generator().manual_seed(6))
    ref = R.gn_ref64(x, groups, gamma, beta)
    yard = R.gn_yard32(x, groups, gamma, beta)
    e_rstd, e_mean = R.stats_errors(yard.mean, yard.rstd, ref)
    assert e_rstd < R.RSTD_REL and e_mean < 1.0, (e_rstd, e_mean)
    # the reference is self-consistent: y == x * scale + shift
    cpg = c // groups
    y2 = x.double() * ref.scale[:, :, None, None] + ref.shift[:, :, None, None]
    assert (y2 - ref.y).abs().max().item() < 1e-9 * max(1.0, float(ratio))
    assert ref.scale.shape == (b, c) and cpg * groups == c


@pytest.mark.parametrize("kind,param", R.SOFTMAX_KINDS)
@pytest.mark.parametrize("L", [64, 100, 256, 1024])
def test_softmax_references_are_distributions(kind, param, L):
    x = R.softmax_rows(kind, param, 37, L, seed=8)
    assert x.dtype == torch.float32 and x.shape == (37, L) and bool(torch.isfinite(x).all())
    p = R.softmax_ref64(x)
    assert bool(torch.isfinite(p).all()) and (p.sum(-1) - 1).abs().max().item() < 1e-12
    top = p.topk(2, dim=-1).values
    if kind == "const":
        assert torch.equal(p, torch.full_like(p, 1.0 / L))
    if kind == "dominant":
        assert (top[:, 0] >= 1 - 1e-6).all()
    if kind == "two_max":
        assert torch.equal(top[:, 0], top[:, 1]) and (top[:, 0] > 0.3).all()
    dx = R.softmax_bwd_ref64(p.float(), torch.randn(37, L, generator=torch.Generator().manual_seed(9)))
    assert bool(torch.isfinite(dx).all()) and dx.sum(-1).abs().max().item() < 1e-6

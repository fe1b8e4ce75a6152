"""Ill-conditioned inputs and high-precision references for the GroupNorm / softmax conditioning tests
(tests/test_conditioning_cpu.py, tests/test_conditioning_gpu.py).

GroupNorm: activations whose (image, group) mean is far from zero compared with their spread - the case in which a
variance formed as E[x^2] - E[x]^2 from fp32 sums loses (mean/std)^2 * 2^-24 of its value.  Softmax: peaked, flat and
large rows.  Every reference is computed in fp64 from the fp32 input AS STORED (quantising the input is never counted
as error); the yardstick is plain torch in fp32 on the same input, never a kernel of this project.
"""
import torch
import torch.nn.functional as F

EPS = 1e-6                                   # nn.GroupNorm(eps=1e-6) of the reference network
RATIOS = (0, 1, 10, 30, 100, 1000)           # |mean| / std of a group, before the per-group factor in [0.5, 1]
SWEEP = tuple((r, 1.0) for r in RATIOS) + ((10, 1e-3), (10, 1e3))       # (ratio, scale)
F32_EPS = 2.0 ** -24                         # unit roundoff of fp32

# caps of the statistics tests: the project's own tolerances of test_gn_partials_from_conv_epilogue, per (image, group)
RSTD_REL = 2e-6
MEAN_REL, MEAN_ABS = 2e-6, 1e-7
# apply / backward / block / attention: K x the fp32 yardstick's own error + a floor
YARD_FACTOR = 4.0


def group_offsets(b, groups, ratio, seed):
    """[b, groups] fp64: the signed mean/std of every (image, group): +-ratio times a factor in [0.5, 1]."""
    g = torch.Generator().manual_seed(seed + 7919)
    sign = torch.randint(0, 2, (b, groups), generator=g).double() * 2 - 1
    fac = 0.5 + 0.5 * torch.rand(b, groups, generator=g, dtype=torch.float64)
    return sign * fac * float(ratio)


def offset_groups(b, c, h, w, groups, ratio, scale, seed):
    """NCHW fp32.  Within each (image, group): spread ``scale`` (exactly, before the rounding to fp32) and mean
    group_offsets(...) * scale - so the groups of one image, and one group across images, sit at different offsets.
    ratio = 0: zero-mean unit-spread data, what the rest of the suite feeds."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, groups, (c // groups) * h * w, generator=g, dtype=torch.float64)
    z = z - z.mean(-1, keepdim=True)
    z = z / z.pow(2).mean(-1, keepdim=True).sqrt()
    x = (z + group_offsets(b, groups, ratio, seed)[:, :, None]) * float(scale)
    return x.view(b, c, h, w).float()


def set_constant_group(x, groups, image, group, value):
    """One (image, group) of an NCHW tensor exactly constant (variance 0: rstd = eps^-1/2), in place."""
    cpg = x.shape[1] // groups
    x[image, group * cpg:(group + 1) * cpg] = value
    return x


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def group_moments64(x, groups, channels_last=False):
    """(mean, biased variance) per (image, group) in fp64, two-pass, of an NCHW (or NHWC) tensor on any device."""
    xd = x.double()
    b = xd.shape[0]
    if channels_last:
        c = xd.shape[-1]
        xd = xd.reshape(b, -1, groups, c // groups)
        mu = xd.mean(dim=(1, 3))
        var = (xd - mu[:, None, :, None]).pow(2).mean(dim=(1, 3))
    else:
        xd = xd.reshape(b, groups, -1)
        mu = xd.mean(-1)
        var = (xd - mu[:, :, None]).pow(2).mean(-1)
    return mu, var


class GNRef:
    """mean, rstd [b, groups]; scale, shift [b, c] (y = x * scale + shift); y NCHW (None when not asked for); fp64."""

    def __init__(self, mean, rstd, scale, shift, y):
        self.mean, self.rstd, self.scale, self.shift, self.y = mean, rstd, scale, shift, y


def gn_ref64(x, groups, gamma, beta, eps=EPS, channels_last=False, want_y=True):
    mu, var = group_moments64(x, groups, channels_last)
    rstd = (var + eps).rsqrt()
    c = gamma.numel()
    cpg = c // groups
    ga, be = gamma.double().to(x.device), beta.double().to(x.device)
    scale = rstd.repeat_interleave(cpg, dim=1) * ga
    shift = be - mu.repeat_interleave(cpg, dim=1) * scale
    y = None
    if want_y:
        assert not channels_last
        y = F.group_norm(x.double(), groups, ga, be, eps)
    return GNRef(mu, rstd, scale, shift, y)


def gn_yard32(x, groups, gamma, beta, eps=EPS, want_y=True):
    """The fp32 yardstick: torch.var_mean and F.group_norm in fp32 on the same NCHW input."""
    b = x.shape[0]
    var, mu = torch.var_mean(x.float().reshape(b, groups, -1), dim=-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    y = F.group_norm(x.float(), groups, gamma.float(), beta.float(), eps) if want_y else None
    return GNRef(mu, rstd, None, None, y)


def stats_errors(mean, rstd, ref):
    """(worst rstd relative error, worst |mean - mu64| / (MEAN_REL |mu64| + MEAN_ABS)) over the (image, group)s."""
    mean, rstd = mean.double().to(ref.mean.device), rstd.double().to(ref.rstd.device)
    e_rstd = ((rstd - ref.rstd).abs() / ref.rstd).max().item()
    e_mean = ((mean - ref.mean).abs() / (MEAN_REL * ref.mean.abs() + MEAN_ABS)).max().item()
    return e_rstd, e_mean


def affine_caps(ref, beta):
    """Caps of the folded affine (scale = rstd gamma, shift = beta - mean scale, both stored in fp32), derived from the
    caps of mean and rstd and the format: scale carries rstd's error and one rounding; shift carries the mean's cap times
    |scale|, scale's relative error times |mean scale|, and the roundings of the product, the difference and beta."""
    scale_rel = RSTD_REL + 2 * F32_EPS
    ms = (ref.mean.repeat_interleave(ref.scale.shape[1] // ref.mean.shape[1], dim=1) * ref.scale).abs()
    mean_cap = (MEAN_REL * ref.mean.abs() + MEAN_ABS).repeat_interleave(ref.scale.shape[1] // ref.mean.shape[1], dim=1)
    shift_cap = ref.scale.abs() * mean_cap + ms * (scale_rel + 4 * F32_EPS) + 2 * F32_EPS * beta.double().abs().to(ms.device)
    return scale_rel, shift_cap


# ---- softmax rows -----------------------------------------------------------------------------------------------------
SOFTMAX_KINDS = (("gauss", 1.0), ("gauss", 30.0), ("gauss", 1e3), ("gauss", 1e4),
                 ("const", 0.0), ("const", 1e4), ("const", -1e4), ("const", 1e30),
                 ("dominant", 100.0), ("two_max", 5.0))


def softmax_rows(kind, param, rows, L, seed=0):
    """[rows, L] fp32 logits, no -inf (the network never masks).  gauss: N(0, 1) * param; const: every entry param;
    dominant: one entry per row ``param`` above the largest of a Gaussian rest; two_max: two entries per row, equal to
    each other, ``param`` above the largest of the rest."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, L, generator=g)
    if kind == "gauss":
        return z * param
    if kind == "const":
        return torch.full((rows, L), param, dtype=torch.float32)
    top = z.max(dim=1).values + param
    r = torch.arange(rows)
    j = torch.randint(0, L, (rows,), generator=g)
    z[r, j] = top
    if kind == "two_max":
        z[r, (j + 1 + torch.randint(0, L - 1, (rows,), generator=g)) % L] = top
    elif kind != "dominant":
        raise ValueError(kind)
    return z


def softmax_ref64(x):
    return torch.softmax(x.double(), dim=-1)


def softmax_bwd_ref64(y, dy):
    """dx of y = softmax(x) for the fp32 y and dy as stored."""
    y, dy = y.double(), dy.double()
    return y * (dy - (y * dy).sum(-1, keepdim=True))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()

"""The super-resolution operator of measurement-guided sampling, host side (psld_amd.guidance, DESIGN section 13,
"Super-resolution") against the independent float64 restatement tests/sr_ref.py: the kernels, the operator pair, the
eigenvalues of A A^T, the exactness of the guided score on Gaussian data against dense linear algebra, the convergence of the
few-step samplers under it, and what the front, the wrapper and the command line accept and refuse.  No GPU: nothing here
launches a kernel.

Bounds.
  * kernels, the operator pair, Lambda: both sides are float64 sums of at most H W <= 1024 terms of magnitude <= max|x| with
    weights that sum to <= 1 in modulus; 1e-13 of the sums involved (the gate of tests/test_deconv_cpu.py), 1e-12 against
    torch's anti-aliased bicubic as the issue sets it.
  * exactness: the 1e-9 of DESIGN section 13, relative to the largest entry (measured <= 7.6e-13 over all cases).
  * convergence: deterministic float64; each entry gated at twice the value measured on the CPU with the reference loops of
    tests/ (MEASURED below; DESIGN section 13 holds the table), and every doubling of the step count must lower the error.
"""
import numpy as np
import pytest
import torch

import psld_amd
from psld_amd import cli
from psld_amd import config as C
from psld_amd.guidance import apply_adjoint, apply_operator, check_task, sr_kernel, sr_spectrum
from psld_amd.registry import get_module
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests import restore_ref as F
from tests import sr_ref as Q
from tests.test_deconv_cpu import _gauss, _rel

KERNELS = ["bicubic", "gauss:1.0", "block"]


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_bicubic_kernel(s):
    """4 s taps per axis that sum to 1 and match the closed form; the product's torus kernel is their outer product as a
    correlation; away from the two outermost low-resolution rows and columns (torch clamps, this operator wraps) A x is
    torch's anti-aliased bicubic downsample."""
    offs, wts = Q.taps("bicubic", s)
    assert len(offs) == 4 * s and offs[0] == -3 * s // 2 and offs[-1] == 5 * s // 2 - 1
    assert abs(sum(wts) - 1.0) <= 1e-15
    raw = [Q.cubic((o - (s - 1) / 2) / s) for o in offs]
    assert all(abs(w - r / sum(raw)) <= 1e-16 for w, r in zip(wts, raw))
    assert wts == wts[::-1] or max(abs(a - b) for a, b in zip(wts, wts[::-1])) <= 1e-16       # symmetric about the block's middle
    # Keys' cubic: 1 at 0, 0 at the other integers, -0.5 the slope parameter
    assert Q.cubic(0) == 1.0 and Q.cubic(1) == 0.0 and Q.cubic(2) == 0.0 and Q.cubic(0.5) == 0.5625 and Q.cubic(1.5) == -0.0625
    k = sr_kernel("bicubic", s, 32, 32)
    assert k.shape == (32, 32) and k.dtype == np.float64 and abs(k.sum() - 1.0) <= 1e-14
    np.testing.assert_allclose(k, Q.kernel("bicubic", s, 32, 32), rtol=0, atol=1e-16)
    np.testing.assert_array_equal(sr_kernel(None, s, 32, 32), k)              # the default
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 3, 32, 32)))
    got = apply_operator(x, f"sr{s}")
    want = torch.nn.functional.interpolate(x, scale_factor=1 / s, mode="bicubic", antialias=True, align_corners=False)
    assert got.shape == want.shape == (2, 3, 32 // s, 32 // s) and got.dtype == torch.float64
    err = (got - want)[..., 2:-2, 2:-2].abs().max().item()
    print(f"bicubic s = {s}: interior against torch's anti-aliased bicubic {err:.1e}")
    assert err <= 1e-12
    assert (got - want).abs().max().item() > 1e-3                               # the border differs: periodic against clamped
    # on the smallest torus the 4 s taps wrap onto themselves and still sum to 1
    assert abs(sr_kernel("bicubic", s, 4 * s, 2 * s).sum() - 1.0) <= 1e-14


@pytest.mark.parametrize("s", [2, 4])
def test_block_kernel_is_the_pool_operator_over_s(s):
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 3, 16, 32)))
    got, pool = apply_operator(x, f"sr{s}", psf="block"), apply_operator(x, f"pool{s}")
    assert got.shape == pool.shape
    np.testing.assert_allclose(got.numpy(), pool.numpy() / s, rtol=0, atol=1e-13 * x.abs().max().item())
    k = sr_kernel("block", s, 16, 32)
    assert np.count_nonzero(k) == s * s and abs(k.sum() - 1.0) <= 1e-15
    np.testing.assert_array_equal(k, Q.kernel("block", s, 16, 32))


def test_parse_psf_kernels_sample_the_top_left_pixel():
    """gauss / box / motion / arrays are centred on the sampled pixel (s i, s j): the kernel is parse_psf's."""
    from psld_amd.guidance import parse_psf
    for spec in ("gauss:1.0", "box:3", "motion:5", np.arange(9.0).reshape(3, 3)):
        np.testing.assert_array_equal(sr_kernel(spec, 2, 8, 16), parse_psf(spec, 8, 16))
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 1, 8, 8)))
    ident = apply_operator(x, "sr2", psf=np.array([[1.0]]))
    np.testing.assert_allclose(ident.numpy(), x.numpy()[..., ::2, ::2], rtol=0, atol=1e-15)


# ---- the operator pair and the eigenvalues -------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", KERNELS + ["motion:3"])
@pytest.mark.parametrize("shape,s", [((1, 1, 8, 8), 2), ((2, 3, 8, 16), 4), ((2, 3, 16, 8), 2), ((2, 3, 32, 32), 4)])
def test_operator_pair(shape, s, spec):
    """<A x, r> = <x, A^T r>; apply_operator / apply_adjoint on CPU tensors against the reference, and the reference against
    the dense matrix built from the definition."""
    rng = np.random.default_rng(3)
    h, w = shape[2:]
    low = shape[:2] + (h // s, w // s)
    x, r = rng.standard_normal(shape), rng.standard_normal(low)
    k = Q.kernel(spec, s, h, w)
    ax, atr = Q.forward(x, k, s), Q.adjoint(r, k, s)
    assert ax.shape == low and atr.shape == shape
    assert abs((ax * r).sum() - (x * atr).sum()) <= 1e-13 * (np.abs(ax * r).sum() + np.abs(x * atr).sum())
    if h * w <= 128:
        a = Q.dense(k, s)
        np.testing.assert_allclose(a @ x[0, 0].reshape(-1), ax[0, 0].reshape(-1), rtol=0, atol=1e-13 * np.abs(x).max())
        np.testing.assert_allclose(a.T @ r[0, 0].reshape(-1), atr[0, 0].reshape(-1), rtol=0, atol=1e-13 * np.abs(r).max())
    got_f = apply_operator(torch.from_numpy(x), f"sr{s}", psf=spec)
    got_a = apply_adjoint(torch.from_numpy(r), f"sr{s}", psf=spec)
    assert got_f.dtype == got_a.dtype == torch.float64 and got_f.shape == low and got_a.shape == shape
    np.testing.assert_allclose(got_f.numpy(), ax, rtol=0, atol=1e-13 * np.abs(x).max())
    np.testing.assert_allclose(got_a.numpy(), atr, rtol=0, atol=1e-13 * np.abs(r).max())
    assert apply_operator(torch.from_numpy(x).float(), f"sr{s}", psf=spec).dtype == torch.float32


@pytest.mark.parametrize("spec", KERNELS)
@pytest.mark.parametrize("h,w,s", [(8, 8, 2), (8, 16, 4), (16, 8, 2), (16, 16, 4)])
def test_lambda_is_the_spectrum_of_a_at(h, w, s, spec):
    """A A^T = F'^-1 diag(Lambda) F' with the H/s x W/s DFT: off-diagonal 0, the diagonal Lambda, and Lambda the sorted
    eigenvalues of the dense matrix; the product's half is that Lambda's."""
    k = Q.kernel(spec, s, h, w)
    a = Q.dense(k, s)
    aat = a @ a.T
    hl, wl = h // s, w // s
    lm = Q.lam(np.fft.fft2(k), s)
    f1, f2 = np.fft.fft(np.eye(hl)), np.fft.fft(np.eye(wl))
    fm = np.kron(f1, f2)
    d = fm @ aat @ np.conj(fm.T) / (hl * wl)
    scale = np.abs(aat).sum(axis=1).max()
    assert np.abs(d - np.diag(np.diag(d))).max() <= 1e-13 * scale
    assert np.abs(np.diag(d) - lm.reshape(-1)).max() <= 1e-13 * scale
    np.testing.assert_allclose(np.sort(np.linalg.eigvalsh(aat)), np.sort(lm.reshape(-1)), rtol=0, atol=1e-13 * scale)
    hh, half = sr_spectrum(spec, s, h, w)
    assert hh.shape == (h, w // 2 + 1) and hh.dtype == np.complex128 and half.shape == (hl, wl // 2 + 1) and half.dtype == np.float64
    np.testing.assert_allclose(half, lm[:, :wl // 2 + 1], rtol=0, atol=1e-14)
    np.testing.assert_allclose(Q.symmetric(half, wl), lm, rtol=0, atol=1e-14)     # real and symmetric: the half holds it all
    np.testing.assert_allclose(hh, np.fft.fft2(k)[:, :w // 2 + 1], rtol=0, atol=1e-14)
    if spec == "bicubic":                                                        # the issue's table
        lo, hi = {2: (0.055, 0.25), 4: (0.0147, 0.0625)}[s]
        big = Q.lam(np.fft.fft2(Q.kernel(spec, s, 32, 32)), s)
        assert abs(big.max() - hi) <= 1e-12 and abs(big.min() - lo) <= 1e-3


# ---- exactness on Gaussian data ---------------------------------------------------------------------------------------------
EXACT = [((1, 1, 8, 8), 2), ((1, 1, 8, 16), 2), ((1, 1, 16, 16), 4)]


@pytest.mark.parametrize("spec", KERNELS)
@pytest.mark.parametrize("shape,s", EXACT, ids=[f"{sh[2]}x{sh[3]}-s{s}" for sh, s in EXACT])
@pytest.mark.parametrize("sigma_y", [0.05, 0.5])
@pytest.mark.parametrize("v0", [1.0, 0.25])
@pytest.mark.parametrize("kind", ["psld", "vpsde"])
def test_guided_eps_is_the_posterior_score_on_gaussian_data(kind, v0, sigma_y, shape, s, spec):
    """eps' from the reference measure / combine with the closed-form Jacobian equals -L^T grad log p(u_t | y) by dense linear
    algebra with the matrix of A built from the definition, at t = 0.01, 0.1, 0.5 and 0.999."""
    gauss = _gauss(kind, v0)
    rng = np.random.default_rng(11)
    h, w = shape[2:]
    k = Q.kernel(spec, s, h, w)
    a_mat = Q.dense(k, s)
    low = (1, 1, h // s, w // s)
    worst = 0.0
    for t in (0.01, 0.1, 0.5, 0.999):
        ct = 2 if gauss.augmented else 1
        u = rng.standard_normal((1, ct) + shape[2:])
        y = rng.standard_normal(low)
        got = Q.guided_eps(gauss, u, t, y, k, s, sigma_y)
        want = F.exact_guided_eps(gauss, u, t, a_mat, y.reshape(-1), sigma_y)
        plain = gauss.eps(u, t)
        worst = max(worst, _rel(got, want))
        assert _rel(got, want) <= 1e-9, t
        assert _rel(plain, want) > 1e4 * 1e-9, t
    print(f"{kind} sr{s} {spec} {shape[2:]} v0={v0} sigma_y={sigma_y}: guided eps against the posterior score, worst relative error {worst:.1e}")


def test_a_frequency_that_measures_nothing_contributes_nothing():
    """sigma_y = 0 and a hand-made h^ that vanishes on every alias of the low-resolution frequencies (1, 0), (3, 0), (0, 1) and
    (0, 3): Lambda is exactly 0 there, the weight is 0, and every value is finite; where Lambda > 0 the weight is 1 / Lambda."""
    rng = np.random.default_rng(2)
    h = w = 8
    s = 2
    k = Q.kernel("bicubic", s, h, w)
    hh = np.fft.fft2(k)
    for m1, m2 in ((1, 0), (0, 1)):
        for a in range(s):
            for b in range(s):
                hh[m1 + a * 4, m2 + b * 4] = 0.0
                hh[(-(m1 + a * 4)) % h, (-(m2 + b * 4)) % w] = 0.0
    lm = Q.lam(hh, s)
    zero = lm == 0.0
    assert zero.sum() == 4 and zero[1, 0] and zero[3, 0] and zero[0, 1] and zero[0, 3]
    f = Q.solve_weight(lm, 0.0, 0.3)
    assert np.isfinite(f).all() and (f[zero] == 0.0).all()
    np.testing.assert_allclose(f[~zero] * lm[~zero], 1.0, rtol=1e-15)
    q = F.Coeffs([1.0, 0.0], [0.5, 0.0], [0.4, 0.0, 0.0], 1.0, False, [1.0, 0.0], 0.3)
    u, e, y = rng.standard_normal((1, 1, h, w)), rng.standard_normal((1, 1, h, w)), rng.standard_normal((1, 1, 4, 4))
    g = Q.measure(u, e, y, k, s, q, 0.0, 0.3, hh=hh, lm=lm)[0]
    assert np.isfinite(g).all()
    # the residual's components at those frequencies do not reach g: adding them to y changes nothing
    wave = np.real(np.fft.ifft2(np.where(zero, 1.0, 0.0)))[None, None]
    g2 = Q.measure(u, e, y + 3.0 * wave, k, s, q, 0.0, 0.3, hh=hh, lm=lm)[0]
    assert np.abs(g2 - g).max() <= 1e-13 * np.abs(g).max()


# ---- convergence of the few-step samplers under the guided eps ---------------------------------------------------------------
STEPS = (8, 16, 32, 64, 128)
# max over the image's pixels of |std of x - exact|, measured on the CPU (deterministic float64) with the reference loops
MEASURED = {
    "ei_sde": (2.993e-01, 1.824e-01, 1.022e-01, 5.434e-02, 2.806e-02),
    "ei_ode1": (3.759e-01, 2.296e-01, 1.294e-01, 6.919e-02, 3.585e-02),
    "ei_ode2": (3.243e-01, 1.421e-01, 4.807e-02, 1.373e-02, 3.625e-03),
}


def propagate(gauss, shape, k, s, y, sigma_y, n, sampler, m0, p0):
    """(mean, covariance) of u_N for u_0 ~ N(m0, p0) under the reference sampler loops driven by the guided Gaussian eps,
    which is affine in u: the loops are run on 0 and on the unit states (and, for ei_sde, the unit noises), which gives the
    affine map exactly; pixel-major flat states.  The deterministic samplers are run whole (ei_ode at order 2 is a multistep
    method): u_N = G u_0 + h.  ei_sde has no memory, so its loop is run one step at a time, u_{i+1} = G_i u_i + h_i + K_i z_i,
    and the moments are carried through the steps: 2 d + 1 states per step instead of (n + 1) d + 1 for the whole run."""
    ref, ts = gauss.ref, R.grid(n, "quadratic")
    ct, d = 2 * shape[1], 2 * int(np.prod(shape))
    basis = np.stack([F.from_pixel_major(e, shape, True)[0] for e in np.eye(d)])
    flat = lambda out: np.stack([F.to_pixel_major(o[None], True) for o in R.from_pairs(out)])

    def eps_fn(u, t, tau):
        un = R.from_pairs(u)
        return R.to_pairs(Q.guided_eps(gauss, un, t, np.repeat(y, un.shape[0], axis=0), k, s, sigma_y))

    if sampler != "ei_sde":
        u0 = np.zeros((1 + d, ct) + shape[2:])
        u0[1:] = basis
        f = flat(R.sample(ref.coeffs(ts, int(sampler[-1])), ts, R.to_pairs(u0), eps_fn))
        g = (f[1:] - f[0]).T
        return g @ m0 + f[0], g @ p0 @ g.T
    steps = [(phi, c, S.chol2(pp)) for phi, _, c, pp in S.coeffs(ref, ts, 1.0)]
    u0, z = np.zeros((1 + 2 * d, ct) + shape[2:]), np.zeros((1 + 2 * d, ct) + shape[2:])
    u0[1:1 + d], z[1 + d:] = basis, basis
    m, p = m0, p0
    for i in range(n):
        f = flat(S.sample(steps[i:i + 1], ts[i:i + 2], R.to_pairs(u0), eps_fn, lambda _, u: R.to_pairs(z)))
        g, kk = (f[1:1 + d] - f[0]).T, (f[1 + d:] - f[0]).T
        m, p = g @ m + f[0], g @ p @ g.T + kk @ kk.T
    return m, p


def convergence_errors(sampler):
    v0, sigma_y, shape, s = 1.0, 0.1, (1, 1, 8, 8), 2
    gauss = _gauss("psld", v0)
    rng = np.random.default_rng(5)
    k = Q.kernel("bicubic", s, 8, 8)
    x0 = rng.standard_normal(shape) * np.sqrt(v0)
    y = Q.forward(x0, k, s) + sigma_y * rng.standard_normal((1, 1, 4, 4))
    a_mat = Q.dense(k, s)
    post = F.posterior_x0(a_mat, y.reshape(-1), sigma_y, v0)
    m0, p0 = F.posterior_state(gauss, R.T, *post)
    me, pe = F.posterior_state(gauss, 1e-3, *post)
    errs, mean_errs = [], []
    for n in STEPS:
        m, p = propagate(gauss, shape, k, s, y, sigma_y, n, sampler, m0, p0)
        mean_errs.append(np.abs(m[::2] - me[::2]).max())
        errs.append(np.abs(np.sqrt(np.diag(p)[::2]) - np.sqrt(np.diag(pe)[::2])).max())
    return errs, mean_errs


@pytest.mark.parametrize("sampler", ["ei_sde", "ei_ode1", "ei_ode2"])
def test_samplers_converge_to_the_posterior(sampler):
    """From the exact u_T | y through 8 .. 128 quadratic steps to t = 1e-3 on an 8 x 8 image measured at 4 x 4 through the
    bicubic kernel: mean and covariance of the affine-Gaussian map propagated exactly (no Monte Carlo); the x marginal
    against the closed-form u_t | y.  v0 = 1, sigma_y = 0.1."""
    errs, mean_errs = convergence_errors(sampler)
    print(f"sr2 {sampler}: |std - exact| over {STEPS} steps: " + " ".join(f"{e:.3e}" for e in errs))
    print(f"sr2 {sampler}: |mean - exact| over {STEPS} steps: " + " ".join(f"{e:.3e}" for e in mean_errs))
    for e, w in zip(errs, MEASURED[sampler]):
        assert e <= 2 * w
    assert all(b < a for a, b in zip(errs, errs[1:]))
    # the score of a Gaussian vanishes at its mean, so the mean is carried exactly up to rounding: at most 128 steps, each a
    # few hundred float64 operations on O(1) values.  The weights: kappa |h^|^2 (s2 + r2) / (s2 + r2 Lambda) with |h^|^2 <= s^2
    # Lambda is at most s^2 / r2 for scale 1, and r2 >= 1e-3 v0 on this grid (t >= 1e-3): < 1e4 (measured <= 4e-13)
    assert max(mean_errs) <= 128 * 300 * 1e4 * 2.0 ** -53


# ---- the front, the wrapper and the command line --------------------------------------------------------------------------
def test_check_task_and_kernel_refusals(tmp_path):
    assert check_task("sr4", None) == "sr4" and check_task("sr2", "bicubic") == "sr2" and check_task("sr2") == "sr2"
    assert check_task("sr4", "gauss:1.5") == "sr4" and check_task("deconv", "gauss:1.5") == "deconv"
    with pytest.raises(ValueError, match="PSF"):
        check_task("gray", "bicubic")
    with pytest.raises(ValueError, match="PSF"):
        check_task("pool4", "block")
    with pytest.raises(ValueError, match="PSF"):
        check_task("deconv", None)
    with pytest.raises(ValueError, match="task"):
        check_task("blur", "bicubic")
    with pytest.raises(ValueError, match="task"):
        check_task("sr3", None)
    # bicubic and block belong to sr alone: parse_psf, and with it deconv, keeps refusing them
    from psld_amd.guidance import parse_psf
    for name in ("bicubic", "block"):
        with pytest.raises(ValueError, match="not gauss"):
            parse_psf(name, 8, 8)
        with pytest.raises(ValueError, match="not gauss"):
            apply_operator(torch.zeros(1, 3, 8, 8), "deconv", psf=name)
    for bad, what in (("box:4", "odd"), ("gauss:0", "S must be > 0"), ("disc:3", "not gauss"), ("box:9", "larger"),
                      (np.ones((2, 3)), "odd")):
        with pytest.raises(ValueError, match=what):
            sr_kernel(bad, 2, 8, 8)
    for s, h, w in ((3, 12, 12), (1, 8, 8), (8, 16, 16), (2, 7, 8), (4, 8, 10)):
        with pytest.raises(ValueError, match="factors 2 and 4"):
            sr_kernel("bicubic", s, h, w)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        apply_operator(torch.zeros(3, 8, 8), "sr2")


def test_posterior_score_fn_checks_its_arguments_for_sr():
    """Every refusal comes from the argument checks, before anything touches a device."""
    from psld_amd.guidance import CFGScoreFn, PosteriorScoreFn
    cfg = C.tiny()
    psld_amd.import_modules_into_registry()
    sde = get_module("sde", "psld")(cfg)
    plain = lambda x, t: x
    fn = PosteriorScoreFn(plain, sde, "sr4", 0.1)
    assert fn.operator == "sr4" and fn.psf == "bicubic" and fn.k == 4 and fn.eval() is fn
    assert PosteriorScoreFn(plain, sde, "sr2", 0.1, psf="gauss:1.5").psf == "gauss:1.5"
    with pytest.raises(ValueError, match="odd"):
        PosteriorScoreFn(plain, sde, "sr2", 0.1, psf="box:4")
    with pytest.raises(ValueError, match="PSF"):
        PosteriorScoreFn(plain, sde, "pool4", 0.1, psf="bicubic")
    with pytest.raises(ValueError, match="sigma_y"):
        PosteriorScoreFn(plain, sde, "sr4", -0.1)
    net = get_module("score_fn", "ncsnpp")(C.tiny())
    net.label_classes = 3
    with pytest.raises(ValueError, match="CFGScoreFn"):
        PosteriorScoreFn(CFGScoreFn(net, 1), sde, "sr4", 0.1)
    x, t = torch.zeros(2, 6, 16, 16), torch.full((2,), 0.5)
    with pytest.raises(RuntimeError, match="set_measurement"):
        fn(x, t)
    with pytest.raises(ValueError, match="mask"):
        fn.set_measurement(torch.zeros(2, 3, 4, 4), mask=torch.ones(2, 3, 4, 4))
    fn.set_measurement(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="device tensors"):                     # CPU tensors: no fallback
        fn(x, t)
    off = PosteriorScoreFn(plain, sde, "sr4", 0.1, scale=0.0)
    assert off(x, t) is x                                                        # scale 0: the plain call, nothing else


def test_wrapper_reads_the_sr_task():
    import copy
    from psld_amd.guidance import PosteriorScoreFn
    psld_amd.import_modules_into_registry()
    em = get_module("samplers", "ei_sde")

    def front(restore):
        cfg = C.tiny()
        cfg.evaluation.restore = restore
        net = get_module("score_fn", "ncsnpp")(cfg)
        sde = get_module("sde", "psld")(cfg)
        return get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=copy.deepcopy(net), sampler_cls=em).sampler.score_fn

    fn = front({"task": "sr2", "sigma_y": 0.2})
    assert isinstance(fn, PosteriorScoreFn) and fn.operator == "sr2" and fn.k == 2 and fn.psf == "bicubic" and fn.sigma_y == 0.2
    fn = front({"task": "sr4", "psf": "block"})
    assert fn.operator == "sr4" and fn.psf == "block"
    with pytest.raises(ValueError, match="PSF"):
        front({"task": "gray", "psf": "bicubic"})


def test_parser_knows_the_sr_tasks():
    parse = lambda argv: cli.build_parser().parse_known_args(argv)
    args, rest = parse(["restore", "--config", "tiny", "--task", "sr4", "--sigma-y", "0.05"])
    assert (args.cmd, args.task, args.psf, args.sigma_y) == ("restore", "sr4", None, 0.05) and rest == []
    args, _ = parse(["restore", "--task", "sr2", "--psf", "block"])
    assert (args.task, args.psf) == ("sr2", "block")
    for bad in ("blur", "sr3", "sr8", "sr"):
        with pytest.raises(SystemExit):
            parse(["restore", "--task", bad])
    text = cli.build_parser()._subparsers._group_actions[0].choices["restore"].format_help()
    assert "sr2" in text and "sr4" in text and "bicubic" in text and "top-left" in text and "periodic" in text


def test_presets_do_not_carry_a_restore_key():
    for name in ("c10_sota", "celeba64_sota", "afhqv2_128", "afhqv2_128_inpaint", "c10_ablation", "c10_vpsde", "yaml_default",
                 "tiny", "tiny_vpsde"):
        ev = getattr(C, name)().evaluation
        assert "restore" not in ev and "psf" not in ev and "sr" not in str(sorted(ev.keys()))

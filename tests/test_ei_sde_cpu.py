"""Host side of the ``ei_sde`` sampler (psld_amd.ei.plan_sde) against the independent float64 reference
tests/ei_sde_ref.py: the two closed-form ends of the lambda family, the numerically integrated middle, the VP-SDE scalars,
exactness in distribution on point-mass data, the two-point mixture, and what the plan, the sampler and the export refuse.
No GPU.  Measured values: profiles/r18/ei_sde.md.

Which covariance: ``numerical_eps = 0`` only in test_lam_one_is_the_gaussian_posterior (where the identity is exact); every
other test keeps the product's 1e-9 on Sigma's diagonal, on both sides of the comparison."""
import math
import time

import numpy as np
import pytest

from psld_amd import config as C
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests.test_ei_cpu import PARAMS, _psld, _ref

GRIDS = [("quadratic", 10), ("quadratic", 20), ("uniform", 50)]
LONG = ("uniform", 1000)                       # once, on the first parameter set
CASES = [(nu, ga, st, n) for nu, ga in PARAMS for st, n in GRIDS] + [PARAMS[0] + LONG]
LAMS = [0.3, 0.7, 2.0]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _vp(beta_min=0.1, beta_max=20.0):
    from psld_amd.vpsde import VPSDE
    cfg = C.yaml_default()
    cfg.model.sde.beta_min, cfg.model.sde.beta_max = beta_min, beta_max
    return VPSDE(cfg), R.RefVP(beta_min, beta_max)


# ---- the two ends ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu,gamma,stride,n", CASES)
def test_lam_zero_is_ei_ode_order_one(nu, gamma, stride, n):
    """phi and c of plan(sde, ts, 1) to 1e-12 of the largest entry (they are the same numbers), s = 0."""
    from psld_amd import ei
    sde, ts = _psld(nu, gamma), R.grid(n, stride)
    got, want = ei.plan_sde(sde, ts, 0.0), ei.plan(sde, ts, 1)
    assert len(got) == len(want) == n
    for k, w in zip(got, want):
        assert k.augmented and k.phi.shape == k.c.shape == k.s.shape == (2, 2)
        assert _rel(k.phi, w.phi) <= 1e-12 and _rel(k.c, w.c[0]) <= 1e-12
        assert not k.s.any()
        assert (k.t, k.t_next) == (w.t, w.t_next)


LAM1_GATE = 2.1e-10


@pytest.mark.parametrize("decomp", ["lower", "upper"])
def test_lam_one_is_the_gaussian_posterior(decomp):
    """lam = 1 with numerical_eps = 0: Psi^ = Sigma_s Phi(t, s)^T Sigma_t^-1 and S S^T = Sigma_s - Psi^ Phi(t, s) Sigma_s, and
    C = (Psi^ - Phi) L_t with the factor of the SDE's own host scalars, for either decomp_mode.  Measured, relative to the
    largest entry of each matrix, over the three parameter sets and the four grids: Psi^ 2.03e-11, S S^T 1.15e-11, C 2.3e-12
    (the RK4 sub-steps of the plan; the prototype's 3e-13 came from 4000 sub-steps per step).  The gate is 10x the largest."""
    from psld_amd import ei
    worst = [0.0, 0.0, 0.0]
    for nu, gamma, stride, n in CASES:
        sde, ref = _psld(nu, gamma, numerical_eps=0.0, decomp=decomp), _ref(nu, gamma, numerical_eps=0.0)
        for k in ei.plan_sde(sde, R.grid(n, stride), 1.0):
            psi, p = S.posterior(ref, k.t, k.t_next)
            lt = np.linalg.inv(np.array(sde._inv_coeff_host(sde._cov_host(0.0, sde.mm_0, k.t))).reshape(2, 2)).T
            assert (lt[0, 1] == 0.0) if decomp == "lower" else (lt[1, 0] == 0.0)
            errs = (_rel(k.psi, psi), _rel(k.s @ k.s.T, p), _rel(k.c, (psi - ref.flow(k.t_next, k.t)) @ lt))
            worst = [max(a, b) for a, b in zip(worst, errs)]
    print(f"lam = 1 against the posterior ({decomp}): Psi^ {worst[0]:.2e}, S S^T {worst[1]:.2e}, C {worst[2]:.2e}")
    assert max(worst) <= LAM1_GATE


# ---- the middle of the family --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("nu,gamma,stride,n", CASES)
def test_plan_matches_reference(nu, gamma, stride, n, lam):
    """Psi^, C and S S^T within 1e-7 of the largest entry of each matrix of the DOP853 reference (rtol 1e-12), on every step;
    measured 1.8e-10 at the worst (S S^T at lam = 0.3, where P is the difference of two matrices up to 22x larger).  On every
    step also: Psi^ Sigma_t Psi^T + S S^T = Sigma_s to 1e-13 of the largest entry (the plan forms P as that difference, so what is
    left is rounding: Sigma's closed form as NumPy and as math evaluate it, ~10 products and sums, the factorisation); P's
    smallest eigenvalue >= 0 (measured >= 2e-3 of its largest entry); S lower-triangular with a positive diagonal."""
    from psld_amd import ei
    sde, ref = _psld(nu, gamma), _ref(nu, gamma)
    ts = R.grid(n, stride)
    got, want = ei.plan_sde(sde, ts, lam), S.coeffs(ref, ts, lam)
    assert len(got) == n
    worst = [0.0, 0.0, 0.0]
    for k, (phi, psi, c, p) in zip(got, want):
        assert k.augmented and k.lam == lam
        np.testing.assert_allclose(k.phi, phi, rtol=1e-12, atol=1e-15)
        errs = (_rel(k.psi, psi), _rel(k.c, c), _rel(k.s @ k.s.T, p))
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert max(errs) <= 1e-7, (k.t, errs)
        sig_s, carried = ref.sigma(k.t_next), k.psi @ ref.sigma(k.t) @ k.psi.T
        assert np.abs(carried + k.s @ k.s.T - sig_s).max() <= 1e-13 * max(np.abs(sig_s).max(), np.abs(carried).max())
        assert np.linalg.eigvalsh(sig_s - carried).min() >= 0.0
        assert k.s[0, 1] == 0.0 and k.s[0, 0] > 0.0 and k.s[1, 1] > 0.0
    print(f"plan_sde vs reference nu={nu} gamma={gamma} {stride} {n} lam={lam}: Psi^ {worst[0]:.2e}, C {worst[1]:.2e}, "
          f"S S^T {worst[2]:.2e}")


@pytest.mark.parametrize("stride,n", GRIDS + [LONG])
def test_vpsde_closed_forms(stride, n):
    """psi^, c and s^2 of the issue's three closed forms at 1e-10 relative on beta 0.1 / 20; lam = 1 also against
    s^2 = sigma_s^2 / sigma_t^2 (1 - alpha_t^2 / alpha_s^2); lam = 0 is DDIM's c_0 with s = 0."""
    from psld_amd import ei
    sde, ref = _vp()
    ts = R.grid(n, stride)
    worst = 0.0
    for lam in (0.0, 0.3, 0.7, 1.0, 2.0):
        for k in ei.plan_sde(sde, ts, lam):
            phi, psi, c, s2 = S.vp_step(ref, k.t, k.t_next, lam)
            assert not k.augmented and all(isinstance(v, float) for v in (k.phi, k.c, k.s))
            assert abs(k.phi - phi) <= 1e-14 * phi
            if lam == 0.0:
                assert k.s == 0.0
                errs = [abs(k.c - (ref.sigma(k.t_next) - phi * ref.sigma(k.t))) / abs(c)]
            else:
                errs = [abs(k.psi - psi) / psi, abs(k.c - c) / abs(c), abs(k.s ** 2 - s2) / s2]
            if lam == 1.0:
                a_t, a_s = math.exp(ref.log_alpha(k.t)), math.exp(ref.log_alpha(k.t_next))
                gap = -math.expm1(2 * (ref.log_alpha(k.t) - ref.log_alpha(k.t_next)))          # 1 - alpha_t^2 / alpha_s^2
                s2_post = ref.sigma(k.t_next) ** 2 / ref.sigma(k.t) ** 2 * gap
                assert a_t < a_s
                errs.append(abs(k.s ** 2 - s2_post) / s2_post)
            worst = max(worst, *errs)
    print(f"VP-SDE closed forms {stride} {n}: worst {worst:.2e}")
    assert worst <= 1e-10


# ---- the method itself ---------------------------------------------------------------------------------------------------
def _steps(plan):
    return [(k.phi, k.c, k.s) for k in plan]


def _noise(rng):
    return lambda n, u: rng.standard_normal(u.shape)


@pytest.mark.parametrize("lam", [0.5, 1.0])
def test_exact_in_distribution_on_a_point_mass(lam):
    """Point-mass data with its own x_0 in [-1, 1] per pixel, u_T drawn from N(mu_T, Sigma_T), 5 quadratic steps of the
    reference loop on the product's plan: L_{t_end}^-1 (u - mu_{t_end}) is standard normal whatever the step size.
    n = 200 000 pairs, fixed seed: |mean| <= 5 / sqrt(n) per component, |cov - I| <= 5 sqrt(2 / n) per entry (standard errors
    1 / sqrt(n) and at most sqrt(2 / n); the prototype stayed within 2.7 of them on two seeds)."""
    from psld_amd import ei
    n = 200_000
    ref = _ref(4.01, 0.01)
    rng = np.random.default_rng(20)
    x0 = rng.uniform(-1.0, 1.0, n)
    mu = lambda t: x0[:, None] * (ref.flow(t, 0.0) @ np.array([1.0, 0.0]))
    u0 = mu(R.T) + rng.standard_normal((n, 2)) @ ref.chol(R.T).T
    ts = R.grid(5, "quadratic")
    u = S.sample(_steps(ei.plan_sde(_psld(4.01, 0.01), ts, lam)), ts, u0, lambda u, t, tau: S.point_mass_eps(ref, u, t, x0),
                 _noise(rng))
    t_end = R.T - ts[-1]
    w = (u - mu(t_end)) @ ref.chol_inv(t_end).T
    mean, cov = w.mean(axis=0), (w.T @ w) / n
    print(f"point mass, 5 quadratic steps, lam = {lam}: |mean| {np.abs(mean).max() * math.sqrt(n):.2f} standard errors, "
          f"|cov - I| {np.abs(cov - np.eye(2)).max() / math.sqrt(2 / n):.2f}")
    assert np.abs(mean).max() <= 5 / math.sqrt(n)
    assert np.abs(cov - np.eye(2)).max() <= 5 * math.sqrt(2 / n)


def mixture_start(ref, n, rng):
    """n pairs of the mixture's marginal at t = T: +-mu_T + L_T z."""
    sign = rng.integers(0, 2, n) * 2.0 - 1.0
    return sign[:, None] * (ref.flow(R.T, 0.0) @ np.array([1.0, 0.0])) + rng.standard_normal((n, 2)) @ ref.chol(R.T).T


def mixture_figures(ref, x):
    """(share of samples with | |x| - 1 | < 0.05, median of | |x| - 1 |, its exact value 0.6745 sqrt(Sigma_xx(1e-3)))."""
    d = np.abs(np.abs(x) - 1.0)
    return (d < 0.05).mean(), np.median(d), 0.6745 * math.sqrt(ref.sigma(1e-3)[0, 0])


@pytest.mark.parametrize("lam", [0.5, 1.0])
def test_reference_sampler_on_the_mixture(lam):
    """Data +-1 per pixel with the exact score, 10 quadratic steps, 20 000 samples: at least 99 % within 0.05 of +-1
    (prototype 0.998 / 0.999; Euler-Maruyama on the same grid 0.26) and the median of | |x| - 1 | within 10 % of the end
    time's own spread 0.6745 sqrt(Sigma_xx(1e-3)) = 0.00615."""
    from psld_amd import ei
    ref = _ref(4.01, 0.01)
    rng = np.random.default_rng(21)
    ts = R.grid(10, "quadratic")
    u = S.sample(_steps(ei.plan_sde(_psld(4.01, 0.01), ts, lam)), ts, mixture_start(ref, 20_000, rng),
                 lambda u, t, tau: ref.mixture_eps(u, t), _noise(rng))
    share, med, want = mixture_figures(ref, u[:, 0])
    print(f"mixture, 10 quadratic steps, lam = {lam}: share within 0.05 {share:.4f}, median {med:.5f} (exact {want:.5f})")
    assert share >= 0.99
    assert abs(med - want) <= 0.1 * want


# ---- refusals, registry, cache, struct, export ---------------------------------------------------------------------------
@pytest.mark.parametrize("nu,gamma,mode", [(4.0, 0.0, "score_m"), (0.0, 4.0, "score_x")])
@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_half_eps_modes_are_refused(nu, gamma, mode, lam):
    from psld_amd import ei
    sde = _psld(nu, gamma)
    assert sde.mode == mode
    with pytest.raises(ValueError, match=mode):
        ei.plan_sde(sde, R.grid(5, "quadratic"), lam)


def _sampler_cls():
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    return get_module("samplers", "ei_sde")


@pytest.mark.parametrize("lam", [-0.1, float("nan"), float("inf"), "1", True])
def test_bad_lam_is_refused(lam):
    from psld_amd import ei
    with pytest.raises(ValueError, match="lam"):
        ei.plan_sde(_psld(4.01, 0.01), R.grid(5, "quadratic"), lam)
    cfg = C.yaml_default()
    cfg.evaluation.sampler.lam = lam
    with pytest.raises(ValueError, match="lam"):
        _sampler_cls()(cfg, _psld(4.01, 0.01), None)


def test_bad_grids_are_refused():
    from psld_amd import ei
    for sde in (_psld(4.01, 0.01), _vp()[0]):
        for ts in ([0.0], [0.0, 0.5, 0.5], [0.0, 0.5, 0.4], [0.0, 1.0]):
            for lam in (0.0, 1.0):
                with pytest.raises(ValueError, match="grid"):
                    ei.plan_sde(sde, ts, lam)


def test_registry_key_default_lam_and_corrector():
    cls = _sampler_cls()
    cfg = C.yaml_default()
    s = cls(cfg, _psld(4.01, 0.01), None)
    assert s.lam == 1.0 and isinstance(s.lam, float) and s.noise_fn is None
    for lam in (0, 0.5, 2):
        cfg.evaluation.sampler.lam = lam
        assert cls(cfg, _psld(4.01, 0.01), None).lam == lam
    with pytest.raises(ValueError, match="corrector"):
        cls(cfg, _psld(4.01, 0.01), None, corrector_fn=lambda x, t, dt: (x, x))


def test_plan_is_cached_and_cheap():
    """Cached per (SDE parameters, grid, lam), beside ei_ode's plans; a 1000-step plan at lam = 0.5 stays a sub-second host
    job (measured 0.11 .. 0.44 s on the uniform grid: 174 RK4 sub-steps for all steps in lock-step; printed, not gated)."""
    from psld_amd import ei
    sde = _psld(4.01, 0.01)
    ts = R.grid(1000, "uniform")
    ei._CACHE.clear()
    t0 = time.perf_counter()
    a = ei.plan_sde(sde, ts, 0.5)
    dt = time.perf_counter() - t0
    print(f"1000-step plan at lam = 0.5: {dt * 1e3:.1f} ms")
    assert len(a) == 1000
    assert ei.plan_sde(_psld(4.01, 0.01), ts, 0.5) is a
    assert ei.plan_sde(sde, ts, 0.25) is not a
    assert ei.plan_sde(_psld(4.02, 0.02), ts, 0.5) is not a
    assert ei.plan_sde(sde, R.grid(999, "uniform"), 0.5) is not a
    assert ei.plan(sde, ts, 1) is not a and ei.plan_sde(sde, ts, 0.5) is a


def test_coefficient_struct_layout():
    """EiSdeCoeffs.struct(): row-major 2x2 matrices in float64 with s[0][1] = 0; the VP-SDE scalars in entry 0; the C layout
    of psld_ei_sde_coeffs_t (three double[4], one int, padded to 8)."""
    import ctypes
    from psld_amd import _lib, ei
    k = ei.plan_sde(_psld(4.01, 0.01), R.grid(5, "quadratic"), 0.5)[1]
    s = k.struct()
    assert isinstance(s, _lib.EiSdeCoeffs) and k.struct() is s
    assert s.augmented == 1
    assert list(s.phi) == list(k.phi.reshape(-1)) and list(s.c) == list(k.c.reshape(-1)) and list(s.s) == list(k.s.reshape(-1))
    assert s.s[1] == 0.0 and s.s[0] > 0.0 and s.s[3] > 0.0
    v = ei.plan_sde(_vp()[0], R.grid(5, "quadratic"), 0.5)[1].struct()
    kv = ei.plan_sde(_vp()[0], R.grid(5, "quadratic"), 0.5)[1]
    assert v.augmented == 0 and (v.phi[0], v.c[0], v.s[0]) == (kv.phi, kv.c, kv.s)
    assert list(v.phi)[1:] == list(v.c)[1:] == list(v.s)[1:] == [0.0] * 3
    t = _lib.EiSdeCoeffs
    assert (t.phi.offset, t.c.offset, t.s.offset, t.augmented.offset, ctypes.sizeof(t)) == (0, 32, 64, 96, 104)


def test_export_validates_its_arguments_on_the_host():
    """psld_ei_sde_step_f64 is exported and refuses NULL pointers (z may be NULL), empty shapes and an ``augmented`` other
    than 0 / 1 before any launch (no GPU here)."""
    import ctypes
    from psld_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 14 == lib.psld_version()
    k = _lib.EiSdeCoeffs()
    k.augmented = 1
    buf = (ctypes.c_double * 8)()
    x = ctypes.addressof(buf)
    bad = [(None, x, 1, 1, 1), (x, None, 1, 1, 1), (x, x, 0, 1, 1), (x, x, 1, 0, 1), (x, x, 1, 1, 0)]
    for z in (x, None):
        for xx, ee, b, c, hw in bad:
            assert lib.psld_ei_sde_step_f64(xx, ee, z, ctypes.byref(k), b, c, hw, None, None) != 0
            assert b"psld_ei_sde_step_f64" in lib.psld_last_error()
        assert lib.psld_ei_sde_step_f64(x, x, z, None, 1, 1, 1, None, None) != 0
        for aug in (2, -1):
            k.augmented = aug
            assert lib.psld_ei_sde_step_f64(x, x, z, ctypes.byref(k), 1, 1, 1, None, None) != 0
            assert b"psld_ei_sde_step_f64" in lib.psld_last_error()
        k.augmented = 1

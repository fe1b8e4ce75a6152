"""The deconv operator of measurement-guided sampling, host side (psld_amd.guidance, DESIGN section 13, "Deconvolution")
against the independent float64 restatement tests/deconv_ref.py: the PSF parser, the operator pair, the exactness of the
guided score on Gaussian data against dense linear algebra with the circulant matrix, the convergence of the few-step
samplers under it, and what the front, the wrapper and the command line accept and refuse.  No GPU: nothing here launches
a kernel.

Bounds.
  * PSFs and the operator pair: both sides are float64 (numpy.fft there, torch.fft here) of sums of at most H W <= 1024 terms
    of magnitude <= max|x|; 1e-13 of the sums involved, the gate of tests/test_restore_cpu.py.
  * exactness: the 1e-9 of DESIGN section 13, relative to the largest entry (measured <= 9.1e-13 over all cases).  box:3 is
    larger than the 2 x 8 image and refused there, so that one pairing does not exist.
  * convergence: deterministic float64; each entry gated at twice the value measured on the CPU with the reference loops of
    tests/ (MEASURED below; DESIGN section 13 holds the table), and every doubling of the step count must lower the error.
"""
import numpy as np
import pytest
import torch

import psld_amd
from psld_amd import cli
from psld_amd import config as C
from psld_amd.registry import get_module
from tests import deconv_ref as D
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests import restore_ref as F
from tests.test_ei_cpu import PARAMS, _ref

PSFS = ["gauss:0.8", "gauss:1.5", "gauss:2.0", "box:3"]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _gauss(kind, v0):
    return F.GaussPSLD(_ref(*PARAMS[0]), v0) if kind == "psld" else F.GaussVP(R.RefVP(), v0)


# ---- the PSF parser ----------------------------------------------------------------------------------------------------------
def test_psf_parser_forms(tmp_path):
    from psld_amd.guidance import parse_psf, psf_spectrum
    for spec in ("gauss:0.8", "gauss:1.5", "box:3", "box:5", "motion:7", "motion:1"):
        for h, w in ((8, 8), (8, 16), (32, 32)):
            k = parse_psf(spec, h, w)
            assert k.shape == (h, w) and k.dtype == np.float64
            assert abs(k.sum() - 1.0) <= 1e-14
            np.testing.assert_allclose(k, D.psf(spec, h, w), rtol=0, atol=1e-15)
            assert k[0, 0] == k.max()                                        # centred: the middle tap is at the origin
            np.testing.assert_array_equal(k, np.roll(k[::-1, ::-1], (1, 1), (0, 1)))     # symmetric about it
            hh = psf_spectrum(spec, h, w)
            assert hh.shape == (h, w // 2 + 1) and hh.dtype == np.complex128
            np.testing.assert_allclose(hh, np.fft.fft2(D.psf(spec, h, w))[:, :w // 2 + 1], rtol=0, atol=1e-14)
    k = parse_psf("motion:5", 8, 8)
    assert np.count_nonzero(k) == 5 and np.count_nonzero(k[0]) == 5          # horizontal
    assert np.count_nonzero(parse_psf("box:3", 8, 8)) == 9
    # an array / a file is used as given (not normalised), the middle tap at the origin
    taps = np.arange(15, dtype=np.float32).reshape(3, 5)
    np.save(tmp_path / "k.npy", taps)
    for src in (taps, str(tmp_path / "k.npy")):
        k = parse_psf(src, 8, 8)
        assert k[0, 0] == taps[1, 2] and k[7, 6] == taps[0, 0] and k[1, 2] == taps[2, 4] and k.sum() == taps.sum()
        np.testing.assert_array_equal(k, D.psf(taps, 8, 8))


def test_psf_parser_refusals(tmp_path):
    from psld_amd.guidance import apply_operator, check_task, parse_psf
    for bad, what in (("box:4", "odd"), ("motion:2", "odd"), ("box:2.5", "odd"), ("gauss:0", "S must be > 0"),
                      ("gauss:-1", "S must be > 0"), ("gauss:nan", "S must be > 0"), ("box:9", "larger"),
                      ("motion:17", "larger"), ("disc:3", "not gauss"), ("gauss", "not gauss"), ("box:x", "not gauss"),
                      (np.ones((2, 3)), "odd"), (np.ones((3, 4)), "odd"), (np.ones(3), "odd"), (np.ones((9, 1)), "larger")):
        with pytest.raises(ValueError, match=what):
            parse_psf(bad, 8, 16)
    assert parse_psf("motion:15", 8, 16).shape == (8, 16)                     # as wide as fits
    with pytest.raises(ValueError, match="larger"):
        parse_psf("motion:15", 16, 8)
    np.save(tmp_path / "even.npy", np.ones((4, 3)))
    with pytest.raises(ValueError, match="odd"):
        parse_psf(str(tmp_path / "even.npy"), 8, 8)
    # a PSF goes with deconv and with no other task
    with pytest.raises(ValueError, match="PSF"):
        check_task("deconv", None)
    with pytest.raises(ValueError, match="PSF"):
        check_task("gray", "gauss:1.5")
    assert check_task("deconv", "gauss:1.5") == "deconv" and check_task("deconv") == "deconv" and check_task("pool2", None) == "pool2"
    with pytest.raises(ValueError, match="PSF"):
        apply_operator(torch.zeros(1, 3, 8, 8), "deconv")
    with pytest.raises(ValueError, match="PSF"):
        apply_operator(torch.zeros(1, 3, 8, 8), "pool2", psf="box:3")
    with pytest.raises(ValueError, match="task"):
        check_task("blur", "gauss:1.5")


# ---- the operator pair -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", PSFS + ["motion:3"])
@pytest.mark.parametrize("shape", [(1, 1, 4, 4), (2, 3, 8, 16), (2, 3, 32, 32)])
def test_operator_pair(shape, spec):
    """<A x, r> = <x, A^T r>; the product's apply_operator / apply_adjoint on CPU tensors against the reference."""
    from psld_amd.guidance import apply_adjoint, apply_operator
    rng = np.random.default_rng(3)
    x, r = rng.standard_normal(shape), rng.standard_normal(shape)
    k = D.psf(spec, *shape[2:])
    ax, atr = D.forward(x, k), D.adjoint(r, k)
    assert abs((ax * r).sum() - (x * atr).sum()) <= 1e-13 * (np.abs(ax * r).sum() + np.abs(x * atr).sum())
    # against the definition at one pixel: (A x)[n] = sum_m k[m] x[n - m]
    h, w = shape[2:]
    direct = sum(k[i, j] * x[0, 0, (1 - i) % h, (2 - j) % w] for i in range(h) for j in range(w))
    assert abs(direct - ax[0, 0, 1, 2]) <= 1e-13 * np.abs(x).max()
    got_f = apply_operator(torch.from_numpy(x), "deconv", psf=spec)
    got_a = apply_adjoint(torch.from_numpy(r), "deconv", psf=spec)
    assert got_f.dtype == got_a.dtype == torch.float64 and got_f.shape == shape
    np.testing.assert_allclose(got_f.numpy(), ax, rtol=0, atol=1e-13 * np.abs(x).max())
    np.testing.assert_allclose(got_a.numpy(), atr, rtol=0, atol=1e-13 * np.abs(r).max())


# ---- exactness on Gaussian data ---------------------------------------------------------------------------------------------
# every PSF on every image it fits: a 3 x 3 box is larger than the 2 x 8 image (and refused there, test_psf_parser_refusals)
EXACT = [(shape, spec) for shape in ((1, 1, 4, 4), (1, 1, 2, 8), (1, 1, 8, 8)) for spec in PSFS
         if not (spec == "box:3" and shape[2] < 3)]


@pytest.mark.parametrize("shape,spec", EXACT, ids=[f"{s[2]}x{s[3]}-{p}" for s, p in EXACT])
@pytest.mark.parametrize("sigma_y", [0.05, 0.5])
@pytest.mark.parametrize("v0", [1.0, 0.25])
@pytest.mark.parametrize("kind", ["psld", "vpsde"])
def test_guided_eps_is_the_posterior_score_on_gaussian_data(kind, v0, sigma_y, shape, spec):
    """eps' from the reference measure / combine with the closed-form Jacobian equals -L^T grad log p(u_t | y) by dense linear
    algebra with the circulant matrix of the blur, at t = 0.01, 0.1, 0.5 and 0.999."""
    gauss = _gauss(kind, v0)
    rng = np.random.default_rng(11)
    k = D.psf(spec, *shape[2:])
    a_mat = D.operator_matrix(shape, k)
    assert np.abs(a_mat @ a_mat.T - np.eye(a_mat.shape[0])).max() > 0.1      # no orthonormal rows: the new ground
    worst = 0.0
    for t in (0.01, 0.1, 0.5, 0.999):
        ct = shape[1] * (2 if gauss.augmented else 1)
        u = rng.standard_normal((1, ct) + shape[2:])
        y = rng.standard_normal(shape)
        got = D.guided_eps(gauss, u, t, y, k, sigma_y)
        want = F.exact_guided_eps(gauss, u, t, a_mat, y.reshape(-1), sigma_y)
        plain = gauss.eps(u, t)
        worst = max(worst, _rel(got, want))
        assert _rel(got, want) <= 1e-9, t
        assert _rel(plain, want) > 1e4 * 1e-9, t
    print(f"{kind} deconv {spec} {shape[2:]} v0={v0} sigma_y={sigma_y}: guided eps against the posterior score, worst relative error {worst:.1e}")


def test_a_frequency_that_measures_nothing_contributes_nothing():
    """sigma_y = 0 and h^ = 0 (the taps (1/2, 0, 1/2) on a side of 4: h^ = cos(2 pi k2 / 4), exactly 0 at k2 = 1 and 3): the
    weight is 0 there; and for |h^| = 1 (the identity PSF) g = A^T (y - A x0^) = y - x0^."""
    rng = np.random.default_rng(2)
    q = F.Coeffs([1.0, 0.0], [0.5, 0.0], [0.4, 0.0, 0.0], 1.0, False, [1.0, 0.0], 0.3)
    u, e, y = rng.standard_normal((1, 1, 4, 4)), rng.standard_normal((1, 1, 4, 4)), rng.standard_normal((1, 1, 4, 4))
    k = D.psf(np.array([[0.5, 0.0, 0.5]]), 4, 4)
    hh, mm = D.weight(k, 0.0, 0.3)
    assert np.isfinite(mm).all()
    zero = np.abs(hh) == 0.0
    assert zero.sum() == 8 and (mm[zero] == 0.0).all() and (np.abs(mm[~zero]) == 1.0).all()
    g = D.measure(u, e, y, k, q, 0.0, 0.3)[0]
    assert np.isfinite(g).all()
    ident = D.psf(np.array([[1.0]]), 4, 4)
    g1 = D.measure(u, e, y, ident, q, 0.01, 0.3)[0]
    np.testing.assert_allclose(g1, y - F.x0_hat(u, e, q)[0], rtol=0, atol=1e-14)


# ---- convergence of the few-step samplers under the guided eps ---------------------------------------------------------------
STEPS = (8, 16, 32, 64, 128)
# max over the image's pixels of |std of x - exact|, measured on the CPU (deterministic float64) with the reference loops
MEASURED = {
    "ei_sde": (2.517e-01, 1.541e-01, 8.667e-02, 4.619e-02, 2.388e-02),
    "ei_ode1": (3.110e-01, 1.896e-01, 1.068e-01, 5.707e-02, 2.956e-02),
    "ei_ode2": (2.672e-01, 1.170e-01, 3.962e-02, 1.133e-02, 2.992e-03),
}


def affine_run(gauss, shape, k, y, sigma_y, n, sampler):
    """tests/test_restore_cpu.affine_run for the deconv operator: (G, h, K) with u_N = G u_0 + h + K z for the reference
    sampler loops driven by the guided Gaussian eps, which is affine in u.  Pixel-major flat states."""
    ref, ts = gauss.ref, R.grid(n, "quadratic")
    ct, d = 2 * shape[1], 2 * int(np.prod(shape))
    basis = np.stack([F.from_pixel_major(e, shape, True)[0] for e in np.eye(d)])

    def eps_fn(u, t, tau):
        un = R.from_pairs(u)
        return R.to_pairs(D.guided_eps(gauss, un, t, np.repeat(y, un.shape[0], axis=0), k, sigma_y))

    runs = 1 + d + (n * d if sampler == "ei_sde" else 0)
    u0 = np.zeros((runs, ct) + shape[2:])
    u0[1:1 + d] = basis
    if sampler == "ei_sde":
        steps = [(phi, c, S.chol2(p)) for phi, _, c, p in S.coeffs(ref, ts, 1.0)]

        def noise(i, u):
            z = np.zeros_like(u0)
            z[1 + d + i * d:1 + d + (i + 1) * d] = basis
            return R.to_pairs(z)

        out = R.from_pairs(S.sample(steps, ts, R.to_pairs(u0), eps_fn, noise))
    else:
        out = R.from_pairs(R.sample(ref.coeffs(ts, int(sampler[-1])), ts, R.to_pairs(u0), eps_fn))
    flat = np.stack([F.to_pixel_major(o[None], True) for o in out])
    return (flat[1:1 + d] - flat[0]).T, flat[0], (flat[1 + d:] - flat[0]).T


def convergence_errors(sampler):
    v0, sigma_y, shape = 1.0, 0.1, (1, 1, 4, 4)
    gauss = _gauss("psld", v0)
    rng = np.random.default_rng(5)
    k = D.psf("gauss:1.0", 4, 4)
    x0 = rng.standard_normal(shape) * np.sqrt(v0)
    y = D.forward(x0, k) + sigma_y * rng.standard_normal(shape)
    a_mat = D.operator_matrix(shape, k)
    post = F.posterior_x0(a_mat, y.reshape(-1), sigma_y, v0)
    m0, p0 = F.posterior_state(gauss, R.T, *post)
    me, pe = F.posterior_state(gauss, 1e-3, *post)
    errs, mean_errs = [], []
    for n in STEPS:
        g, h, kk = affine_run(gauss, shape, k, y, sigma_y, n, sampler)
        m, p = g @ m0 + h, g @ p0 @ g.T + kk @ kk.T
        mean_errs.append(np.abs(m[::2] - me[::2]).max())
        errs.append(np.abs(np.sqrt(np.diag(p)[::2]) - np.sqrt(np.diag(pe)[::2])).max())
    return errs, mean_errs


@pytest.mark.parametrize("sampler", ["ei_sde", "ei_ode1", "ei_ode2"])
def test_samplers_converge_to_the_posterior(sampler):
    """From the exact u_T | y through 8 .. 128 quadratic steps to t = 1e-3 on a 4 x 4 image blurred by gauss:1.0: mean and
    covariance of the affine-Gaussian map propagated exactly (no Monte Carlo); the x marginal against the closed-form
    u_t | y.  v0 = 1, sigma_y = 0.1."""
    errs, mean_errs = convergence_errors(sampler)
    print(f"deconv {sampler}: |std - exact| over {STEPS} steps: " + " ".join(f"{e:.3e}" for e in errs))
    print(f"deconv {sampler}: |mean - exact| over {STEPS} steps: " + " ".join(f"{e:.3e}" for e in mean_errs))
    for e, w in zip(errs, MEASURED[sampler]):
        assert e <= 2 * w
    assert all(b < a for a, b in zip(errs, errs[1:]))
    # the score of a Gaussian vanishes at its mean, so the mean is carried exactly up to rounding: at most 128 steps, each
    # a few hundred float64 operations on O(1) values with weights |m^| <= 1 / (2 sigma_y sqrt(r2)) < 1e3 (measured <= 5.1e-13)
    assert max(mean_errs) <= 128 * 300 * 1e3 * 2.0 ** -53


# ---- the front, the wrapper and the command line --------------------------------------------------------------------------
def test_posterior_score_fn_checks_its_arguments_for_deconv():
    """Every refusal comes from the argument checks, before anything touches a device."""
    from psld_amd.guidance import PosteriorScoreFn, posterior_coeffs
    cfg = C.tiny()
    psld_amd.import_modules_into_registry()
    sde = get_module("sde", "psld")(cfg)
    plain = lambda x, t: x
    with pytest.raises(ValueError, match="PSF"):
        PosteriorScoreFn(plain, sde, "deconv", 0.1)                          # deconv without a PSF
    with pytest.raises(ValueError, match="PSF"):
        PosteriorScoreFn(plain, sde, "mask", 0.1, psf="gauss:1.5")           # a PSF without deconv
    with pytest.raises(ValueError, match="odd"):
        PosteriorScoreFn(plain, sde, "deconv", 0.1, psf="box:4")
    with pytest.raises(ValueError, match="S must be > 0"):
        PosteriorScoreFn(plain, sde, "deconv", 0.1, psf="gauss:0")
    with pytest.raises(ValueError, match="sigma_y"):
        PosteriorScoreFn(plain, sde, "deconv", -0.1, psf="gauss:1.5")
    fn = PosteriorScoreFn(plain, sde, "deconv", 0.1, psf="gauss:1.5")
    assert fn.operator == "deconv" and fn.psf == "gauss:1.5" and fn.eval() is fn
    x, t = torch.zeros(2, 6, 8, 8), torch.full((2,), 0.5)
    with pytest.raises(RuntimeError, match="set_measurement"):
        fn(x, t)
    with pytest.raises(ValueError, match="mask"):
        fn.set_measurement(torch.zeros(2, 3, 8, 8), mask=torch.ones(2, 3, 8, 8))
    for bad in ((2, 3, 4, 4), (2, 1, 8, 8), (2, 6, 8, 8), (1, 3, 8, 8)):        # not the image's shape
        fn.set_measurement(torch.zeros(bad))
        with pytest.raises(ValueError, match="measurement of shape"):
            fn(x, t)
    off = PosteriorScoreFn(plain, sde, "deconv", 0.1, scale=0.0, psf="gauss:1.5")
    assert off(x, t) is x                                                      # scale 0: the plain call, nothing else
    # the coefficients expose r_t^2 and sigma_y^2 beside the struct, whose layout is unchanged
    import ctypes
    q = posterior_coeffs(sde, 0.5, 0.1, 1.3, 0.5)
    assert ctypes.sizeof(q) == 72 and q.sigma_y2 == 0.1 ** 2
    assert abs(q.kappa - 1.3 / (q.sigma_y2 + q.r2)) <= 1e-15 * q.kappa
    want = F.psld_coeffs(R.RefPSLD.from_config(cfg), 0.5, 0.1, 1.3, 0.5)
    assert abs(q.r2 - want.r2) <= 1e-12 * want.r2


def test_wrapper_reads_the_psf():
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

    fn = front({"task": "deconv", "psf": "box:3", "sigma_y": 0.2})
    assert isinstance(fn, PosteriorScoreFn) and fn.operator == "deconv" and fn.psf == "box:3" and fn.sigma_y == 0.2
    assert front({"task": "pool2"}).psf is None
    with pytest.raises(ValueError, match="PSF"):
        front({"task": "deconv"})
    with pytest.raises(ValueError, match="PSF"):
        front({"task": "gray", "psf": "box:3"})


def test_parser_knows_the_deconv_task():
    parse = lambda argv: cli.build_parser().parse_known_args(argv)
    args, rest = parse(["restore", "--config", "tiny", "--task", "deconv", "--psf", "gauss:1.5", "--sigma-y", "0.05"])
    assert (args.cmd, args.task, args.psf, args.sigma_y) == ("restore", "deconv", "gauss:1.5", 0.05) and rest == []
    args, _ = parse(["restore", "--task", "pool2"])
    assert args.psf is None
    with pytest.raises(SystemExit):
        parse(["restore", "--task", "blur", "--psf", "gauss:1.5"])           # the name of the task is deconv
    for cmd in ("sample", "inpaint", "bpd"):                                  # the other commands do not know the argument
        args, rest = parse([cmd, "--psf", "box:3"])
        assert not hasattr(args, "psf") and rest == ["--psf", "box:3"]
    text = cli.build_parser()._subparsers._group_actions[0].choices["restore"].format_help()
    assert "deconv" in text and "periodic" in text and "gauss:S" in text


def test_presets_do_not_carry_a_psf():
    for name in ("c10_sota", "celeba64_sota", "afhqv2_128", "afhqv2_128_inpaint", "c10_ablation", "c10_vpsde", "yaml_default",
                 "tiny", "tiny_vpsde"):
        ev = getattr(C, name)().evaluation
        assert "restore" not in ev and "psf" not in ev and "psf" not in str(sorted(ev.keys()))

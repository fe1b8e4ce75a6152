"""Measurement-guided (posterior) sampling, host side (psld_amd.guidance.PosteriorScoreFn) against the
independent float64 restatement tests/restore_ref.py: the coefficients, the three operators, the exactness of the guided
score on Gaussian data, the convergence of the few-step samplers under it, and what the front, the wrapper and the command
line refuse.  No GPU: nothing here launches a kernel.

Bounds.
  * coefficients: both sides are float64 closed forms that differ in the order of a handful of operations; 1e-12 relative,
    the gate of the closed-form coefficients in tests/test_ei_sde_cpu.py (measured <= 4.2e-16).
  * operators: A A^T = I and <A x, r> = <x, A^T r> to 1e-13 of the sums involved (at most 16 float64 terms per entry).
  * exactness: the issue's 1e-9 relative to the largest entry (measured < 1e-11 in every case).
  * convergence: deterministic float64; each entry gated at twice the value measured on the CPU (DESIGN section 13 holds the
    table), and every doubling of the step count must lower the error.
"""
import argparse
import copy

import numpy as np
import pytest
import torch

import psld_amd
from psld_amd import cli
from psld_amd import config as C
from psld_amd.registry import get_module
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests import restore_ref as F
from tests.test_ei_cpu import PARAMS, _psld, _ref
from tests.test_ei_sde_cpu import _vp

TIMES = [1e-3, 0.01, 0.1, 0.5, 0.999]
# (B, C, H, W), tasks: the shapes of the kernel tests
SHAPES = [((1, 1, 2, 2), ("mask", "pool2")), ((2, 3, 4, 4), ("mask", "gray", "pool2", "pool4")),
          ((3, 3, 6, 10), ("mask", "gray", "pool2")), ((5, 1, 7, 1), ("mask",)),
          ((2, 3, 32, 32), ("mask", "gray", "pool2", "pool4")), ((1, 3, 4, 4), ("pool4",)), ((2, 3, 8, 12), ("pool4",))]
OP_CASES = [(shape, task) for shape, tasks in SHAPES for task in tasks]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ---- coefficients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v0,sigma_y,scale", [(1.0, 0.05, 1.0), (0.25, 0.5, 1.7)])
@pytest.mark.parametrize("nu,gamma", PARAMS)
def test_psld_coefficients_match_the_reference(nu, gamma, v0, sigma_y, scale):
    from psld_amd.guidance import posterior_coeffs
    sde, ref = _psld(nu, gamma), _ref(nu, gamma)
    worst = 0.0
    for t in TIMES:
        q, w = posterior_coeffs(sde, t, sigma_y, scale, v0), F.psld_coeffs(ref, t, sigma_y, scale, v0)
        assert q.augmented == 1
        pairs = list(zip(q.q_u, w.q_u)) + list(zip(q.q_e, w.q_e)) + list(zip(q.l, w.l)) + [(q.kappa, w.kappa)]
        errs = [abs(a - b) / abs(b) for a, b in pairs]
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-12, (t, errs)
        # the first column of predict_x_from_eps's matrix is the flow from time 0
        b = sde.b_t(t)
        sf = np.exp((nu + gamma) / 4 * b)
        assert _rel([((nu - gamma) / 4 * b + 1) / sf, -0.5 * b / sf], w.a) <= 1e-12
    print(f"PSLD nu={nu} v0={v0} sigma_y={sigma_y}: worst relative coefficient difference {worst:.1e}")


def test_vpsde_coefficients_match_the_reference():
    from psld_amd.guidance import posterior_coeffs
    sde, ref = _vp()
    for v0, sigma_y, scale in ((1.0, 0.05, 1.0), (0.25, 0.5, 1.7)):
        for t in TIMES:
            q, w = posterior_coeffs(sde, t, sigma_y, scale, v0), F.vp_coeffs(ref, t, sigma_y, scale, v0)
            assert q.augmented == 0
            for a, b in ((q.q_u[0], w.q_u[0]), (q.q_e[0], w.q_e[0]), (q.l[0], w.l[0]), (q.kappa, w.kappa)):
                assert abs(a - b) <= 1e-12 * abs(b), t


def test_coefficients_refuse_what_they_cannot_serve():
    from psld_amd.guidance import posterior_coeffs
    sde = _psld(*PARAMS[0])
    with pytest.raises(ValueError, match="sigma_y"):
        posterior_coeffs(sde, 0.5, 0.0, 1.0, 0.0)                       # sigma_y^2 + r_t^2 = 0
    with pytest.raises(ValueError, match="sigma_y"):
        posterior_coeffs(sde, 0.5, 0.1, 1.0, -1.0)                      # a negative prior variance: the sum is negative
    with pytest.raises(ValueError, match="score_xm"):
        posterior_coeffs(_psld(4.0, 0.0), 0.5, 0.1)                     # score_m: half of eps is missing
    with pytest.raises(ValueError, match="lower"):
        posterior_coeffs(_psld(*PARAMS[0], decomp="upper"), 0.5, 0.1)
    with pytest.raises(TypeError):
        posterior_coeffs(object(), 0.5, 0.1)
    assert posterior_coeffs(sde, 0.5, 0.0, 1.0, 1.0).kappa > 0         # a noise-free measurement is fine


# ---- operators -----------------------------------------------------------------------------------------------------------
def _mask(shape, seed):
    m = (np.random.default_rng(seed).uniform(size=shape) < 0.6).astype(np.float64)
    m.reshape(-1)[0], m.reshape(-1)[-1] = 1.0, 0.0
    return m


@pytest.mark.parametrize("shape,task", OP_CASES)
def test_operators_have_orthonormal_rows_and_true_adjoints(shape, task):
    """Reference and product (torch) operators: A A^T r = r on the range, <A x, r> = <x, A^T r>, product == reference."""
    from psld_amd.guidance import apply_adjoint, apply_operator
    rng = np.random.default_rng(3)
    mask = _mask(shape, 4) if task == "mask" else None
    x, r = rng.standard_normal(shape), rng.standard_normal(F.measurement_shape(shape, task))
    if mask is not None:
        r = r * mask                                                      # the range of a mask: the kept pixels
    ax, atr = F.forward(x, task, mask), F.adjoint(r, task, mask)
    assert ax.shape == r.shape and atr.shape == x.shape
    assert np.abs(F.forward(atr, task, mask) - r).max() <= 1e-13 * np.abs(r).max()
    assert abs((ax * r).sum() - (x * atr).sum()) <= 1e-13 * (np.abs(ax * r).sum() + np.abs(x * atr).sum())
    tm = None if mask is None else torch.from_numpy(mask)
    np.testing.assert_allclose(apply_operator(torch.from_numpy(x), task, tm).numpy(), ax, rtol=0, atol=1e-13 * np.abs(x).max() * 16)
    np.testing.assert_allclose(apply_adjoint(torch.from_numpy(r), task, tm).numpy(), atr, rtol=0, atol=1e-13 * np.abs(r).max())


def test_operators_refuse_shapes_that_do_not_fit():
    from psld_amd import ops
    from psld_amd.guidance import apply_operator, check_task
    x = torch.zeros(1, 2, 6, 6)
    with pytest.raises(ValueError, match="3 image channels"):
        apply_operator(x, "gray")
    with pytest.raises(ValueError, match="multiple"):
        apply_operator(x, "pool4")
    with pytest.raises(ValueError, match="mask"):
        apply_operator(x, "mask")
    with pytest.raises(ValueError, match="task"):
        check_task("blur")
    assert ops.restore_measurement_shape((2, 6, 8, 8), 2, 4, 1) == (2, 3, 2, 2)
    assert ops.restore_measurement_shape((2, 3, 8, 8), 1, 1, 0) == (2, 1, 8, 8)
    with pytest.raises(ValueError, match="even"):
        ops.restore_measurement_shape((2, 3, 8, 8), 0, 1, 1)
    with pytest.raises(ValueError, match="block size"):
        ops.restore_measurement_shape((2, 6, 9, 9), 2, 3, 1)
    with pytest.raises(ValueError, match="operator code"):
        ops.restore_measurement_shape((2, 6, 8, 8), 3, 1, 1)


# ---- exactness on Gaussian data ----------------------------------------------------------------------------------------------
# tiny images: a mask with an observed and an unobserved pixel, one grey pixel, one 2 x 2 block
EXACT = [("mask", (1, 1, 1, 2), np.array([1.0, 0.0]).reshape(1, 1, 1, 2)), ("gray", (1, 3, 1, 1), None), ("pool2", (1, 1, 2, 2), None)]


def _gauss(kind, v0):
    return F.GaussPSLD(_ref(*PARAMS[0]), v0) if kind == "psld" else F.GaussVP(R.RefVP(), v0)


@pytest.mark.parametrize("task,shape,mask", EXACT, ids=[e[0] for e in EXACT])
@pytest.mark.parametrize("sigma_y", [0.05, 0.5])
@pytest.mark.parametrize("v0", [1.0, 0.25])
@pytest.mark.parametrize("kind", ["psld", "vpsde"])
def test_guided_eps_is_the_posterior_score_on_gaussian_data(kind, v0, sigma_y, task, shape, mask):
    """eps' from measure / combine with the closed-form Jacobian equals -L^T grad log p(u_t | y), u_t | y ~ N(a m_y, a a^T
    V_y + Sigma_t) over the pixels the operator couples (dense linear algebra), at t = 0.01, 0.1, 0.5 and 0.999."""
    gauss = _gauss(kind, v0)
    rng = np.random.default_rng(11)
    a_mat, keep = F.operator_matrix(shape, task, mask)
    assert np.abs(a_mat @ a_mat.T - np.eye(a_mat.shape[0])).max() <= 1e-15
    worst = 0.0
    for t in (0.01, 0.1, 0.5, 0.999):
        ct = shape[1] * (2 if gauss.augmented else 1)
        u = rng.standard_normal((1, ct) + shape[2:])
        y = rng.standard_normal(F.measurement_shape(shape, task))
        y = y if mask is None else y * mask
        got = F.guided_eps(gauss, u, t, y, mask, task, sigma_y)
        want = F.exact_guided_eps(gauss, u, t, a_mat, y.reshape(-1)[keep], sigma_y)
        plain = gauss.eps(u, t)
        worst = max(worst, _rel(got, want))
        assert _rel(got, want) <= 1e-9, t
        assert _rel(plain, want) > 1e4 * 1e-9, t                         # (the guidance is far above the gate: 4e-4 at t = 0.999, where |a| = 3e-3)
    print(f"{kind} {task} v0={v0} sigma_y={sigma_y}: guided eps against the posterior score, worst relative error {worst:.1e}")


# ---- convergence of the few-step samplers under the guided eps ---------------------------------------------------------------
STEPS = (8, 16, 32, 64, 128)
# max over the image's pixels of |std of x - exact|, measured on the CPU (deterministic float64); the means agree to 1e-14
# because the score of a Gaussian vanishes at its mean
MEASURED = {
    ("mask", "ei_sde"): (3.407e-01, 2.072e-01, 1.160e-01, 6.166e-02, 3.183e-02),
    ("mask", "ei_ode1"): (4.294e-01, 2.623e-01, 1.479e-01, 7.908e-02, 4.097e-02),
    ("mask", "ei_ode2"): (3.707e-01, 1.624e-01, 5.490e-02, 1.568e-02, 4.138e-03),
    ("gray", "ei_sde"): (2.793e-01, 1.699e-01, 9.515e-02, 5.059e-02, 2.612e-02),
    ("gray", "ei_ode1"): (3.515e-01, 2.146e-01, 1.210e-01, 6.470e-02, 3.352e-02),
    ("gray", "ei_ode2"): (3.034e-01, 1.329e-01, 4.494e-02, 1.284e-02, 3.389e-03),
}


def affine_run(gauss, task, shape, mask, y, sigma_y, n, sampler):
    """(G, h, K) with u_N = G u_0 + h + K z for the reference sampler loops (tests/ei_sde_ref.sample at lam = 1,
    tests/ei_ref.sample at order 1 / 2) driven by the guided Gaussian eps, which is affine in u: the loops run on a batch of
    start points - zero, the unit vectors - and, for the stochastic loop, on unit noise at one step and one entry at a time.
    Pixel-major flat states; z stacks the noise of all steps."""
    ref, ts = gauss.ref, R.grid(n, "quadratic")
    ct, d = 2 * shape[1], 2 * int(np.prod(shape))
    basis = np.stack([F.from_pixel_major(e, shape, True)[0] for e in np.eye(d)])

    def eps_fn(u, t, tau):
        un = R.from_pairs(u)
        yy = np.repeat(y, un.shape[0], axis=0)
        mm = None if mask is None else np.repeat(mask, un.shape[0], axis=0)
        return R.to_pairs(F.guided_eps(gauss, un, t, yy, mm, task, sigma_y))

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


@pytest.mark.parametrize("sampler", ["ei_sde", "ei_ode1", "ei_ode2"])
@pytest.mark.parametrize("task,shape,mask", EXACT[:2], ids=["mask", "gray"])
def test_samplers_converge_to_the_posterior(task, shape, mask, sampler):
    """From the exact u_T | y through 8 .. 128 quadratic steps to t = 1e-3: mean and covariance of the affine-Gaussian map
    propagated exactly (no Monte Carlo); the x marginal against the closed-form u_t | y.  v0 = 1, sigma_y = 0.1."""
    v0, sigma_y = 1.0, 0.1
    gauss = _gauss("psld", v0)
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal(shape) * np.sqrt(v0)
    y = F.forward(x0, task, mask) + sigma_y * rng.standard_normal(F.measurement_shape(shape, task))
    y = y if mask is None else y * mask
    a_mat, keep = F.operator_matrix(shape, task, mask)
    post = F.posterior_x0(a_mat, y.reshape(-1)[keep], sigma_y, v0)
    m0, p0 = F.posterior_state(gauss, R.T, *post)
    me, pe = F.posterior_state(gauss, 1e-3, *post)
    errs = []
    for n in STEPS:
        g, h, k = affine_run(gauss, task, shape, mask, y, sigma_y, n, sampler)
        m, p = g @ m0 + h, g @ p0 @ g.T + k @ k.T
        assert np.abs(m[::2] - me[::2]).max() <= 1e-12 * max(1.0, np.abs(me).max())
        errs.append(np.abs(np.sqrt(np.diag(p)[::2]) - np.sqrt(np.diag(pe)[::2])).max())
    print(f"{task} {sampler}: |std - exact| over {STEPS} steps: " + " ".join(f"{e:.3e}" for e in errs))
    for e, w in zip(errs, MEASURED[(task, sampler)]):
        assert e <= 2 * w
    assert all(b < a for a, b in zip(errs, errs[1:]))
    order = 2 if sampler == "ei_ode2" else 1
    assert errs[-2] / errs[-1] >= 0.85 * 2 ** order                      # asymptotic: first / second order


# ---- the front, the wrapper and the command line --------------------------------------------------------------------------
def _net(cfg):
    psld_amd.import_modules_into_registry()
    return get_module("score_fn", "ncsnpp")(cfg)


def test_posterior_score_fn_checks_its_arguments():
    """Every refusal comes from the argument checks, before anything touches a device."""
    from psld_amd.guidance import CFGScoreFn, PosteriorScoreFn
    cfg = C.tiny()
    sde = get_module("sde", "psld")(cfg)
    plain = lambda x, t: x
    cond = C.tiny()
    cond.model.score_fn.label_classes = 3
    with pytest.raises(ValueError, match="labels are out of scope"):
        PosteriorScoreFn(CFGScoreFn(_net(cond), 1, 2.0), sde, "mask", 0.1)
    with pytest.raises(ValueError, match="task"):
        PosteriorScoreFn(plain, sde, "blur", 0.1)
    with pytest.raises(ValueError, match="sigma_y"):
        PosteriorScoreFn(plain, sde, "mask", 0.0, prior_var=0.0)
    with pytest.raises(ValueError, match="sigma_y"):
        PosteriorScoreFn(plain, sde, "mask", -0.1)
    fn = PosteriorScoreFn(plain, sde, "pool2", 0.1)
    assert fn.training is False and fn.eval() is fn
    x, t = torch.zeros(2, 6, 8, 8), torch.full((2,), 0.5)
    with pytest.raises(RuntimeError, match="set_measurement"):
        fn(x, t)
    with pytest.raises(ValueError, match="mask"):
        fn.set_measurement(torch.zeros(2, 3, 4, 4), mask=torch.ones(2, 3, 4, 4))      # a mask with another operator
    fn.set_measurement(torch.zeros(2, 3, 8, 8))                                       # not the pooled shape
    with pytest.raises(ValueError, match="measurement of shape"):
        fn(x, t)
    fn.set_measurement(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="ONE time"):
        fn(x, torch.tensor([0.5, 0.25]))
    mk = PosteriorScoreFn(plain, sde, "mask", 0.1)
    with pytest.raises(ValueError, match="mask"):
        mk.set_measurement(torch.zeros(2, 3, 8, 8))                                   # the mask operator without a mask
    with pytest.raises(ValueError, match="mask of shape"):
        mk.set_measurement(torch.zeros(2, 3, 8, 8), mask=torch.ones(2, 3, 8, 4))
    gray = PosteriorScoreFn(plain, sde, "gray", 0.1).set_measurement(torch.zeros(2, 1, 8, 8))
    with pytest.raises(ValueError, match="3 image channels"):
        gray(torch.zeros(2, 4, 8, 8), t)
    # scale 0 is the plain call: no measurement needed, nothing else computed
    off = PosteriorScoreFn(plain, sde, "gray", 0.1, scale=0.0)
    assert off(x, t) is x


def test_presets_do_not_carry_the_keys():
    for name in ("c10_sota", "celeba64_sota", "afhqv2_128", "c10_vpsde", "yaml_default", "tiny", "tiny_vpsde"):
        ev = getattr(C, name)().evaluation
        assert "restore" not in ev and "save_momentum" not in ev


def test_wrapper_wraps_the_sampling_network_only_when_asked():
    from psld_amd.guidance import PosteriorScoreFn
    psld_amd.import_modules_into_registry()
    em = get_module("samplers", "ei_sde")
    for restore in (None, {"sigma_y": 0.1}, {"task": "pool2", "sigma_y": 0.2, "scale": 1.5, "prior_var": 0.25}, {"task": "gray"}):
        cfg = C.tiny()
        if restore is not None:
            cfg.evaluation.restore = restore
        net = _net(cfg)
        ema = copy.deepcopy(net)
        sde = get_module("sde", "psld")(cfg)
        fn = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, sampler_cls=em).sampler.score_fn
        if restore is None or "task" not in restore:
            assert fn is ema
        else:
            assert isinstance(fn, PosteriorScoreFn) and fn.net is ema and fn.sde is sde and fn.operator == restore["task"]
            assert (fn.sigma_y, fn.scale, fn.prior_var) == (restore.get("sigma_y", 0.0), restore.get("scale", 1.0),
                                                          restore.get("prior_var", 1.0))
    cfg = C.tiny()
    cfg.model.score_fn.label_classes = 3
    cfg.evaluation.label_to_sample = 1
    cfg.evaluation.restore = {"task": "gray"}
    net = _net(cfg)
    with pytest.raises(ValueError, match="labels are out of scope"):
        get_module("pl_modules", "sde_wrapper")(cfg, get_module("sde", "psld")(cfg), net, ema_score_fn=net, sampler_cls=em)


def test_parser_knows_the_restore_command():
    parse = lambda argv: cli.build_parser().parse_known_args(argv)
    args, rest = parse(["restore", "--config", "tiny", "--task", "pool4", "--sigma-y", "0.05", "--guidance-scale", "2",
                        "evaluation.sampler.name=ei_sde"])
    assert (args.cmd, args.task, args.sigma_y, args.guidance_scale) == ("restore", "pool4", 0.05, 2.0)
    assert rest == ["evaluation.sampler.name=ei_sde"]
    args, _ = parse(["restore", "--task", "mask"])
    assert (args.sigma_y, args.guidance_scale, args.mask, args.math) == (0.0, 1.0, "synthetic", None)
    with pytest.raises(SystemExit):
        parse(["restore"])                                                 # --task is required
    with pytest.raises(SystemExit):
        parse(["restore", "--task", "blur"])
    for cmd in ("sample", "inpaint", "bpd"):                                # the other commands do not know the arguments
        args, rest = parse([cmd, "--task", "gray"])
        assert not hasattr(args, "task") and rest == ["--task", "gray"]
    assert "RECORDING" in cli.build_parser()._subparsers._group_actions[0].choices["restore"].format_help()


def test_vjp_input_takes_a_callable_cotangent():
    """The signature and the docstring carry the two-phase form (the device behaviour: tests/test_restore_gpu.py)."""
    import inspect
    from psld_amd.score_fn import NCSNpp
    assert list(inspect.signature(NCSNpp.vjp_input).parameters)[:4] == ["self", "x", "time_cond", "w"]
    assert "w_fn(out)" in NCSNpp.vjp_input.__doc__


def test_image_writer_writes_the_momentum_half_when_asked(tmp_path):
    """SimpleImageWriter(save_momentum=True): momentum/<name>.npy, float32 [B, C, H, W], the raw second half of the state; off by
    default and for a state without a momentum half."""
    import os
    from psld_amd.callbacks import SimpleImageWriter
    pred = torch.randn(2, 6, 4, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for flag, augmented in ((False, True), (True, True), (True, False)):
        out = str(tmp_path / f"{flag}_{augmented}")
        wr = SimpleImageWriter(out, sample_prefix="gpu", save_mode="np", is_norm=False, is_augmented=augmented, save_momentum=flag)
        wr.write_on_batch_end(None, argparse.Namespace(global_rank=0), pred, None, None, 3)
        assert sorted(os.listdir(out)) == (["images", "momentum"] if flag and augmented else ["images"])
        assert len(os.listdir(os.path.join(out, "images"))) == 2
        if flag and augmented:
            m = np.load(os.path.join(out, "momentum", "output_gpu_0_3.npy"))
            assert m.dtype == np.float32 and np.array_equal(m, pred[:, 3:].float().numpy())

"""The ``ei_sde`` sampler on the GPU: the fused update kernel against torch float64 (values, guard bands, alignment forms,
refusals), the sampler with exact device score functions (point mass against the float64 reference loop fed the same noise;
the two-point mixture), lam = 0 against ``ei_ode``, the launch and draw counts, the tiny networks against the reference loop
(tests/ei_sde_ref.py) driven by the CPU oracle network, classifier-free guidance, the math modes and the command.

Bounds.
  * kernel: every element is a sum of at most 6 float64 products (2 of the state, 2 of eps, up to 2 of the noise); products
    and sums round once each, in either order of summation -> |err| <= 16 * 2^-53 * sum|terms|.  The float32 copy is the
    rounding of the float64 result: torch.equal with x.float().  Without noise: ops.ei_step's bits.
  * sampler against the reference loop with the same noise: the project's 1e-4 rel-L2 gate.
  * mixture: the issue's two conditions (share within 0.05 of +-1 >= 0.99; median within 10 % of the exact spread).
  Measured values: profiles/r18/ei_sde.md.

Named to sort after tests/test_fullsize_gpu.py, with scipy imported only inside the functions of the reference modules: see
the header of tests/test_sampler_ei_gpu.py."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests import guard as G
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_ei_sde_cpu import mixture_figures, mixture_start
from tests.test_sampler_ei_gpu import GRID_PASS, SHAPES, U64, _MixtureScore, _net, _rand, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
assert SHAPES == [(1, 1, 1), (2, 3, 16), (3, 3, 25), (5, 1, 7), (2, 3, 1024), (5, 1, 209717), (1, 1, 4 * GRID_PASS + 8)]


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as o
    o.lib()
    return o


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


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _coeffs(augmented, seed):
    """Random coefficients of the sizes the plan produces (|Phi| <= 1, |C| up to ~50, |S| <= 1, S lower-triangular), as the
    stochastic struct and as ei_ode's with one eps buffer."""
    from psld_amd._lib import EiCoeffs, EiSdeCoeffs
    rng = np.random.default_rng(seed)
    phi, c, s = rng.uniform(-1, 1, 4), rng.uniform(-50, 50, 4), rng.uniform(-1, 1, 4)
    s[1] = 0.0
    k, d = EiSdeCoeffs(), EiCoeffs()
    k.augmented = d.augmented = augmented
    d.n_hist = 1
    for i in range(4):
        k.phi[i] = d.phi[i] = phi[i]
        k.c[i] = d.c[0][i] = c[i]
        k.s[i] = s[i]
    return k, d, phi, c, s


def _kernel_ref(x, eps, z, phi, c, s, augmented):
    """(new state, sum of |terms|) in torch float64."""
    e = eps.double()
    if not augmented:
        terms = [phi[0] * x, c[0] * e] + ([s[0] * z] if z is not None else [])
        return sum(terms), sum(t.abs() for t in terms)
    h = x.shape[1] // 2
    rows = []
    for r in (0, 1):
        terms = [phi[2 * r] * x[:, :h], phi[2 * r + 1] * x[:, h:], c[2 * r] * e[:, :h], c[2 * r + 1] * e[:, h:]]
        if z is not None:
            terms += [s[2 * r] * z[:, :h]] + ([s[3] * z[:, h:]] if r else [])
        rows.append((sum(terms), sum(t.abs() for t in terms)))
    return torch.cat([rows[0][0], rows[1][0]], 1), torch.cat([rows[0][1], rows[1][1]], 1)


@pytest.mark.parametrize("b,c,hw", SHAPES)
@pytest.mark.parametrize("augmented", [1, 0])
@pytest.mark.parametrize("noise", [True, False])
def test_ei_sde_step_kernel(ops, guard, noise, augmented, b, c, hw):
    """ops.ei_sde_step on guarded buffers and on ordinary ones: same bits, no band touched, inputs unchanged; values within
    16 * 2^-53 * sum|terms| of torch float64; the float32 copy is x.float() bit for bit; without noise the result is
    ops.ei_step's with one eps buffer, bit for bit."""
    ct = 2 * c if augmented else c
    k, d, phi, cm, sm = _coeffs(augmented, seed=3 + 10 * augmented)
    x0 = _rand(b, ct, hw, 1, seed=1, dtype=torch.float64).to(DEV)
    eps = _rand(b, ct, hw, 1, seed=2).to(DEV)
    z = _rand(b, ct, hw, 1, seed=5, dtype=torch.float64).to(DEV) if noise else None
    xf0 = torch.full((b, ct, hw, 1), float("nan"), device=DEV)
    tensors = dict(x=x0, xf=xf0, e=eps, **({"z": z} if noise else {}))

    def fn(x, xf, e, z=None):
        ops.ei_sde_step(x, e, z, k, xf)

    plain, _ = G.run_guarded(guard, fn, tensors, outputs=["x", "xf"])
    want, mag = _kernel_ref(x0, eps, z, phi, cm, sm, augmented)
    err = (plain["x"] - want).abs()
    assert bool((err <= 16 * U64 * mag).all()), (err / mag).max().item() / U64
    assert torch.equal(plain["xf"], plain["x"].float())
    x1 = x0.clone()                                                             # without the float32 copy: the same result
    ops.ei_sde_step(x1, eps, z, k, None)
    assert torch.equal(x1, plain["x"])
    x2, xf2 = x0.clone(), torch.empty_like(xf0)
    ops.ei_step(x2, [eps], d, xf2)
    if noise:
        assert not torch.equal(x2, plain["x"])
    else:
        assert torch.equal(x2, plain["x"]) and torch.equal(xf2, plain["xf"])


@pytest.mark.parametrize("augmented", [1, 0])
def test_ei_sde_step_kernel_on_misaligned_buffers(ops, augmented):
    """Buffers that start 4 (float32) / 8 (float64) bytes past a 16-byte boundary take the element-wise form: same values as
    the 16-byte form on aligned copies, bit for bit.  x, eps, z and the float32 copy in turn."""
    b, c, hw = 2, 3, 1024
    ct = 2 * c if augmented else c
    n = b * ct * hw
    k = _coeffs(augmented, seed=7)[0]
    x0 = _rand(b, ct, hw, 1, seed=1, dtype=torch.float64).to(DEV)
    eps = _rand(b, ct, hw, 1, seed=2).to(DEV)
    z = _rand(b, ct, hw, 1, seed=5, dtype=torch.float64).to(DEV)
    xa, xfa = x0.clone(), torch.empty_like(eps)
    ops.ei_sde_step(xa, eps, z, k, xfa)
    off = lambda t: torch.zeros(n + 1, device=DEV, dtype=t.dtype)[1:].view(t.shape).copy_(t)
    for which in ("x", "eps", "z", "xf"):
        xm = off(x0) if which == "x" else x0.clone()
        em = off(eps) if which == "eps" else eps
        zm = off(z) if which == "z" else z
        xfm = off(xfa) if which == "xf" else torch.empty_like(xfa)
        for name, t in (("x", xm), ("eps", em), ("z", zm), ("xf", xfm)):
            assert (t.data_ptr() % 16 != 0) == (which == name), (which, name)
        ops.ei_sde_step(xm, em, zm, k, xfm)
        assert torch.equal(xm, xa) and torch.equal(xfm, xfa), which


def test_ei_sde_step_refuses_bad_arguments(ops):
    """ValueError from the wrapper, before any launch: the state is unchanged."""
    from psld_amd._lib import EiSdeCoeffs
    x = torch.ones(1, 2, 4, 1, device=DEV, dtype=torch.float64)
    e = torch.ones(1, 2, 4, 1, device=DEV)
    z = torch.ones(1, 2, 4, 1, device=DEV, dtype=torch.float64)
    k = EiSdeCoeffs()
    k.augmented = 1
    half = lambda t: t[:, :1].contiguous()
    with pytest.raises(ValueError, match="eps"):
        ops.ei_sde_step(x, half(e), z, k)                                    # eps of another shape
    with pytest.raises(ValueError, match="noise"):
        ops.ei_sde_step(x, e, half(z), k)                                    # noise of another shape
    with pytest.raises(ValueError, match="float32 copy"):
        ops.ei_sde_step(x, e, z, k, half(e))                                 # float32 copy of another shape
    with pytest.raises(ValueError, match="even"):
        ops.ei_sde_step(half(x), half(e), half(z), k)                        # augmented state with an odd channel count
    for aug in (2, -1):
        k.augmented = aug
        with pytest.raises(ValueError, match="augmented"):
            ops.ei_sde_step(x, e, z, k)
    assert bool((x == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the sampler with exact score functions on the device
# ---------------------------------------------------------------------------------------------------------------------
def _sampler(cfg, sde, fn, lam, name="ei_sde"):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    cfg = copy.deepcopy(cfg)
    cfg.evaluation.sampler = C.Config({"name": name, "lam": lam, "order": 1})
    return get_module("samplers", name)(cfg, sde, fn)


def _seeded_noise(step, x):
    """The test hook's noise: float64 standard normals from a CPU generator seeded by the step."""
    g = torch.Generator().manual_seed(1000 + step)
    return torch.randn(x.shape, generator=g, dtype=torch.float64).to(x.device)


class _PointMassScore:
    """The exact eps of point-mass data x_0 (one value per pixel) as a device ``score_fn``: float64 torch ops on the float32
    state, coefficients of the (float32) time from the reference on the host, result rounded to float32."""

    def __init__(self, ref, x0):
        self.ref, self.x0, self.calls = ref, x0, 0

    def __call__(self, x32, t32):
        self.calls += 1
        ref, t = self.ref, float(t32[0])
        mu = ref.flow(t, 0.0) @ np.array([1.0, 0.0])
        li = ref.chol_inv(t)
        h = x32.shape[1] // 2
        dx, dm = x32[:, :h].double() - self.x0 * mu[0], x32[:, h:].double() - self.x0 * mu[1]
        return torch.cat([li[0, 0] * dx + li[0, 1] * dm, li[1, 0] * dx + li[1, 1] * dm], 1).float()


@pytest.fixture(scope="module")
def point_mass():
    from psld_amd.sde import PSLD
    cfg = C.yaml_default()
    ref = R.RefPSLD.from_config(cfg)
    rng = np.random.default_rng(30)
    x0 = rng.uniform(-1.0, 1.0, (2, 3, 4, 4))
    pairs = x0[..., None] * (ref.flow(R.T, 0.0) @ np.array([1.0, 0.0])) + rng.standard_normal((2, 3, 4, 4, 2)) @ ref.chol(R.T).T
    return cfg, PSLD(cfg), ref, x0, pairs


@pytest.mark.parametrize("lam", [0.5, 1.0])
def test_sampler_on_a_point_mass(point_mass, lam):
    """6 quadratic steps with seeded noise against the float64 reference loop (its own DOP853 coefficients, the same noise,
    eps of the float32 state at the float32 time rounded to float32, as the device function gives it): 1e-4 rel-L2."""
    cfg, sde, ref, x0, pairs = point_mass
    ts = R.grid(6, "quadratic")
    steps = [(phi, c, S.chol2(p)) for phi, _, c, p in S.coeffs(ref, ts, lam)]

    def eps_fn(u, t, tau):
        u32 = u.astype(np.float32).astype(np.float64)
        return S.point_mass_eps(ref, u32, float(np.float32(t)), x0).astype(np.float32)

    noise = lambda n, u: R.to_pairs(_seeded_noise(n, torch.empty(2, 6, 4, 4)).numpy())
    want = R.from_pairs(S.sample(steps, ts, pairs, eps_fn, noise))
    fn = _PointMassScore(ref, torch.from_numpy(x0).to(DEV))
    s = _sampler(cfg, sde, fn, lam)
    s.noise_fn = _seeded_noise
    x = s.sample(torch.from_numpy(R.from_pairs(pairs)).to(DEV), torch.from_numpy(ts).to(DEV), 6, denoise=False)
    assert x.dtype == torch.float64 and x.shape == (2, 6, 4, 4) and s.nfe == 6 == fn.calls
    err = rel_l2(x, torch.from_numpy(want))
    quiet = R.from_pairs(S.sample(steps, ts, pairs, eps_fn, None))
    print(f"ei_sde on a point mass, 6 quadratic steps, lam = {lam}: rel-L2 vs reference loop = {err:.3e} "
          f"(the noise moves the state by {rel_l2(torch.from_numpy(quiet), torch.from_numpy(want)):.2e})")
    assert err < 1e-4
    assert rel_l2(torch.from_numpy(quiet), torch.from_numpy(want)) > 100 * 1e-4          # (the noise is not below the gate)


def test_lam_zero_is_ei_ode_order_one(point_mass):
    """Same bits as ei_ode at order 1, with and without the denoising step, and sample() leaves the device's RNG state as
    it was."""
    cfg, sde, ref, x0, pairs = point_mass
    fn = _PointMassScore(ref, torch.from_numpy(x0).to(DEV))
    ts = torch.from_numpy(R.grid(6, "quadratic")).to(DEV)
    u0 = torch.from_numpy(R.from_pairs(pairs)).to(DEV)
    for denoise in (False, True):
        want = _sampler(cfg, sde, fn, 0.0, name="ei_ode").sample(u0, ts, 6, denoise=denoise)
        torch.cuda.synchronize()
        before = torch.cuda.get_rng_state()
        s = _sampler(cfg, sde, fn, 0.0)
        got = s.sample(u0, ts, 6, denoise=denoise)
        torch.cuda.synchronize()
        assert torch.equal(torch.cuda.get_rng_state(), before)
        assert torch.equal(got, want) and s.nfe == 6 + int(denoise)


@pytest.mark.parametrize("denoise", [False, True])
def test_one_draw_and_one_launch_per_step(point_mass, ops, monkeypatch, denoise):
    """lam > 0: exactly one torch.randn_like (on the float64 state) and one ops.ei_sde_step per step; the denoising step adds
    a network call and neither a draw nor an ei_sde_step."""
    cfg, sde, ref, x0, pairs = point_mass
    fn = _PointMassScore(ref, torch.from_numpy(x0).to(DEV))
    draws, launches = [], []
    randn_like, step = torch.randn_like, ops.ei_sde_step

    def counting_randn_like(t, *a, **kw):
        draws.append((t.dtype, tuple(t.shape)))
        return randn_like(t, *a, **kw)

    def counting_step(x, e, z, k, xf=None):
        launches.append(z is not None)
        return step(x, e, z, k, xf)

    monkeypatch.setattr(torch, "randn_like", counting_randn_like)
    monkeypatch.setattr(ops, "ei_sde_step", counting_step)
    s = _sampler(cfg, sde, fn, 0.5)
    x = s.sample(torch.from_numpy(R.from_pairs(pairs)).to(DEV), torch.from_numpy(R.grid(7, "quadratic")).to(DEV), 7,
                 denoise=denoise)
    assert bool(torch.isfinite(x).all())
    assert draws == [(torch.float64, (2, 6, 4, 4))] * 7 and launches == [True] * 7
    assert s.nfe == fn.calls == 7 + int(denoise)


def test_sampler_on_the_mixture():
    """10 quadratic steps at lam = 1 on 20 000 pairs of the two-point mixture with the device's own noise: the two
    conditions of the CPU test (there 0.999 and a median of 0.00618 against 0.00615)."""
    from psld_amd.sde import PSLD
    cfg = C.yaml_default()
    ref = R.RefPSLD.from_config(cfg)
    pairs = mixture_start(ref, 20_000, np.random.default_rng(31)).reshape(8, 1, 50, 50, 2)
    fn = _MixtureScore(ref)
    s = _sampler(cfg, PSLD(cfg), fn, 1.0)
    torch.manual_seed(32)
    x = s.sample(torch.from_numpy(R.from_pairs(pairs)).to(DEV), torch.from_numpy(R.grid(10, "quadratic")).to(DEV), 10,
                 denoise=False)
    assert x.shape == (8, 2, 50, 50) and s.nfe == 10 == fn.calls
    share, med, want = mixture_figures(ref, x[:, 0].cpu().numpy().reshape(-1))
    print(f"ei_sde on the mixture, 10 quadratic steps, lam = 1: share within 0.05 {share:.4f}, median {med:.5f} "
          f"(exact {want:.5f})")
    assert share >= 0.99
    assert abs(med - want) <= 0.1 * want


# ---------------------------------------------------------------------------------------------------------------------
# tiny networks: the sampler against the float64 reference loop driven by the CPU oracle network
# ---------------------------------------------------------------------------------------------------------------------
_REF_RUNS = {}


def _reference_run(name, lam, denoise):
    """ei_sde_ref's loop on its own coefficients with the seeded noise, eps from the oracle network on the float32 state and
    float32 time; the denoising step is the oracle's reverse_sde(probability_flow=True) Euler step of size eval_eps."""
    _, cfg, sd = _net(name)
    vp = name == "vpsde"
    ts = R.grid(6, "quadratic")
    batch = torch.randn(2, 3 if vp else 6, 16, 16, generator=torch.Generator().manual_seed(91))
    net_fn = lambda u32, t32: O.ncsnpp_forward(sd, cfg, u32, t32)
    if (name, lam) not in _REF_RUNS:
        def eps_fn(u, t, tau):
            u32 = torch.from_numpy(u if vp else R.from_pairs(u)).float()
            with torch.no_grad():
                e = net_fn(u32, torch.full((2,), float(np.float32(t)))).double().numpy()
            return e if vp else R.to_pairs(e)

        def noise(n, u):
            z = _seeded_noise(n, batch).numpy()
            return z if vp else R.to_pairs(z)

        if vp:
            steps = S.vp_coeffs(R.RefVP(cfg.model.sde.beta_min, cfg.model.sde.beta_max), ts, lam)
            u = S.sample(steps, ts, batch.double().numpy(), eps_fn, noise, augmented=False)
        else:
            steps = [(phi, c, S.chol2(p)) for phi, _, c, p in S.coeffs(R.RefPSLD.from_config(cfg), ts, lam)]
            u = R.from_pairs(S.sample(steps, ts, R.to_pairs(batch.double().numpy()), eps_fn, noise))
        u = torch.from_numpy(u)
        osde = (O.VPSDEOracle(cfg.model.sde.beta_min, cfg.model.sde.beta_max) if vp else O.PSLDOracle.from_config(cfg))
        with torch.no_grad():
            f = osde.reverse_sde(u, torch.full((2,), 1.0 - 1e-3, dtype=torch.float64), net_fn, probability_flow=True)[0]
        _REF_RUNS[(name, lam)] = (u, u + f * 1e-3)
    return batch, ts, _REF_RUNS[(name, lam)][1 if denoise else 0]


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("name", ["psld", "vpsde"])
def test_sampler_with_tiny_networks(name, denoise):
    """6 quadratic steps at lam = 0.5 with seeded noise against the reference loop + oracle network: the project's 1e-4
    rel-L2 gate.  The result must also be nearer to its own reference than to that of the other denoise setting."""
    from psld_amd.registry import get_module
    net, cfg, _ = _net(name)
    sde = get_module("sde", cfg.model.sde.name)(cfg)
    batch, ts, want = _reference_run(name, 0.5, denoise)
    s = _sampler(cfg, sde, net, 0.5)
    s.noise_fn = _seeded_noise
    x = s.sample(batch.to(DEV), torch.from_numpy(ts).to(DEV), 6, denoise=denoise, eps=1e-3)
    assert x.dtype == torch.float64 and x.shape == want.shape and s.nfe == 6 + int(denoise)
    err = rel_l2(x, want)
    print(f"ei_sde {name} lam 0.5 denoise {denoise}: rel-L2 vs reference + oracle = {err:.3e}")
    assert err < 1e-4
    assert rel_l2(x, _reference_run(name, 0.5, not denoise)[2]) > 10 * err


def test_sampler_under_every_eval_math_mode(ops):
    """The arithmetic of the evaluation forward changes the network's output only: the sampler runs under each mode and
    returns a finite float64 state that differs from the default run's exactly where the mode differs (same noise)."""
    from psld_amd.registry import get_module
    net, cfg, _ = _net("psld128")
    sde = get_module("sde", "psld")(cfg)
    ts = torch.from_numpy(R.grid(4, "quadratic")).to(DEV)
    batch = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(92))

    def run():
        s = _sampler(cfg, sde, net, 0.5)
        s.noise_fn = _seeded_noise
        return s.sample(batch.to(DEV), ts, 4, denoise=True)

    before = ops.math_mode(), ops.eval_math()
    try:
        ops.set_winograd(2)
        base = run()
        for math, ev in (("f32", "limb"), ("bf16x6", "limb"), ("bf16x3", "limb"), ("bf16x6", "f16")):
            ops.set_math_mode(math)
            ops.set_eval_math(ev)
            x = run()
            assert x.dtype == torch.float64 and bool(torch.isfinite(x).all())
            d = rel_l2(x, base)
            print(f"ei_sde math {math} / eval math {ev}: rel-L2 vs default = {d:.3e}")
            assert (d == 0.0) == ((math, ev) == before), "the mode did not reach the network"
    finally:
        ops.set_winograd(None)
        ops.set_math_mode(before[0])
        ops.set_eval_math(before[1])


def test_sampler_under_cfg():
    """CFGScoreFn (one doubled-batch forward + combine kernel) against the two-pass torch callable under ei_sde, 3 quadratic
    steps + denoising with the same noise: under 1e-4, as under ei_ode."""
    from psld_amd.guidance import CFGScoreFn
    from psld_amd.registry import get_module
    from tests.test_cfg_gpu import _net as cond_net, _two_pass
    net, cfg, *_ = cond_net(32)
    sde = get_module("sde", "psld")(cfg)
    batch = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(63)).to(DEV)
    ts = torch.from_numpy(R.grid(3, "quadratic")).to(DEV)
    y = torch.tensor([1, 2], device=DEV)
    outs = []
    for fn in (CFGScoreFn(net, y, 1.5), _two_pass(net, y, 1.5), CFGScoreFn(net, y, 0.0)):
        s = _sampler(cfg, sde, fn, 0.5)
        s.noise_fn = _seeded_noise
        outs.append(s.sample(batch, ts, 3, denoise=True, eps=1e-3))
    e = rel_l2(outs[0], outs[1])
    print(f"ei_sde: 3 steps under CFGScoreFn against the two-pass callable: rel-L2 {e:.3e}")
    assert outs[0].dtype == torch.float64 and bool(torch.isfinite(outs[0]).all()) and e < 1e-4
    assert rel_l2(outs[2], outs[1]) > 1e-4                                  # (guidance changes the trajectory)


@pytest.mark.parametrize("config,channels", [("tiny", 3), ("tiny_vpsde", 3)])
def test_cli_sample_with_ei_sde(tmp_path, config, channels):
    from psld_amd import cli
    out = str(tmp_path / config)
    args = ["sample", "--config", config, "evaluation.n_samples=2", "evaluation.batch_size=2", "evaluation.n_discrete_steps=6",
            "evaluation.stride_type=quadratic", "evaluation.sampler.name=ei_sde", "evaluation.sampler.lam=0.5",
            "evaluation.save_mode=np"]
    torch.manual_seed(5)                                                    # no checkpoint: the command draws its weights
    cli.main(args + [f"evaluation.save_path={out}"])
    files = sorted(os.listdir(os.path.join(out, "images")))
    assert files == ["output_gpu_0_0.npy"]
    a = np.load(os.path.join(out, "images", files[0]))
    assert a.dtype == np.uint8 and a.shape == (2, 16, 16, channels)
    torch.manual_seed(5)                                                    # same weights; the command seeds its own noise
    cli.main(args + [f"evaluation.save_path={out}_again"])
    np.testing.assert_array_equal(a, np.load(os.path.join(out + "_again", "images", files[0])))
    with pytest.raises(ValueError, match="lam"):
        cli.main(args + [f"evaluation.save_path={out}_bad", "evaluation.sampler.lam=-1"])

"""The ``ei_ode`` sampler on the GPU: the fused update kernel against torch float64 (values and guard bands), the sampler
on the two-point mixture with a device score function (the accuracy claim of DESIGN section 11, next to what Euler steps of
the probability flow reach on the same grid), the sampler with the tiny networks against the float64 reference loop
(tests/ei_ref.py) driven by the CPU oracle network, classifier-free guidance, and the command.

Bounds.
  * kernel: every element is a sum of at most 8 float64 products (2 of the state, 2 per eps tensor); products and sums round
    once each, in either order of summation -> |err| <= 16 * 2^-53 * sum|terms|.  The float32 copy is the rounding of the
    float64 result: torch.equal with x.float().
  * mixture: the issue's own bounds (0.05 at 20 quadratic steps, 0.1 at 10), measured 7.8e-3 / 4.0e-2 on the CPU in float64.
  * tiny networks against reference + oracle: the project's 1e-4 rel-L2 gate.  Measured values: profiles/r17/ei_ode.md.

The module's name sorts it after tests/test_fullsize_gpu.py on purpose, and tests/ei_ref.py imports scipy only inside the
functions that use it.  The co-residency test there holds a foreign kernel resident for 400 ms beside a launch-bound pass and
fails when the pass outlasts it; on the same tree it passed with this module left out and failed with it collected - ahead of
that test or behind it - while the module still loaded scipy at import (supposed cause: scipy's thread pools in the process
slow the launching thread)."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import ei_ref as R
from tests import guard as G
from tests.synth import synth_state_dict
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U64 = 2.0 ** -53
GRID_PASS = 4096 * 256          # work items of one pass of the streaming kernels' grid (csrc/sde.hip: grid_for)
# (B, c, hw): one element; whole 16-byte groups; odd planes (element-wise form); the VP-SDE tail of 3; several blocks; more
# element-wise items than one pass of the grid; more 4-element groups than one pass of the grid
SHAPES = [(1, 1, 1), (2, 3, 16), (3, 3, 25), (5, 1, 7), (2, 3, 1024), (5, 1, 209717), (1, 1, 4 * GRID_PASS + 8)]


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


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rand(*shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(dtype)


def _coeffs(n_hist, augmented, seed):
    """Random coefficients of the sizes the plan produces (|Phi| <= 1, |C| up to ~50)."""
    from psld_amd._lib import EiCoeffs
    rng = np.random.default_rng(seed)
    k = EiCoeffs()
    k.n_hist, k.augmented = n_hist, augmented
    phi, c = rng.uniform(-1, 1, 4), rng.uniform(-50, 50, (3, 4))
    for i in range(4):
        k.phi[i] = phi[i]
        for j in range(3):
            k.c[j][i] = c[j, i]
    return k, phi, c


def _kernel_ref(x, eps, phi, c, augmented):
    """(new state, sum of |terms|) in torch float64."""
    es = [e.double() for e in eps]
    if not augmented:
        terms = [phi[0] * x] + [c[j][0] * e for j, e in enumerate(es)]
        return sum(terms), sum(t.abs() for t in terms)
    h = x.shape[1] // 2
    xs, ms = x[:, :h], x[:, h:]
    rows = []
    for r in (0, 1):
        terms = [phi[2 * r] * xs, phi[2 * r + 1] * ms]
        for j, e in enumerate(es):
            terms += [c[j][2 * r] * e[:, :h], c[j][2 * r + 1] * e[:, h:]]
        rows.append((sum(terms), sum(t.abs() for t in terms)))
    return torch.cat([rows[0][0], rows[1][0]], 1), torch.cat([rows[0][1], rows[1][1]], 1)


@pytest.mark.parametrize("b,c,hw", SHAPES)
@pytest.mark.parametrize("augmented", [1, 0])
@pytest.mark.parametrize("n_hist", [1, 2, 3])
def test_ei_step_kernel(ops, guard, n_hist, augmented, b, c, hw):
    """ops.ei_step on guarded buffers and on ordinary ones: same bits, no band touched, inputs unchanged; values within
    16 * 2^-53 * sum|terms| of torch float64; the float32 copy is x.float() bit for bit."""
    ct = 2 * c if augmented else c
    k, phi, cm = _coeffs(n_hist, augmented, seed=n_hist + 10 * augmented)
    x0 = _rand(b, ct, hw, 1, seed=1, dtype=torch.float64).to(DEV)
    eps = [_rand(b, ct, hw, 1, seed=2 + j).to(DEV) for j in range(n_hist)]
    xf0 = torch.full((b, ct, hw, 1), float("nan"), device=DEV)
    tensors = dict(x=x0, xf=xf0, **{f"e{j}": e for j, e in enumerate(eps)})

    def fn(x, xf, **es):
        ops.ei_step(x, [es[f"e{j}"] for j in range(n_hist)], k, xf)

    plain, _ = G.run_guarded(guard, fn, tensors, outputs=["x", "xf"])
    want, mag = _kernel_ref(x0, eps, phi, cm, augmented)
    err = (plain["x"] - want).abs()
    assert bool((err <= 16 * U64 * mag).all()), (err / mag).max().item() / U64
    assert torch.equal(plain["xf"], plain["x"].float())
    # without the float32 copy: the same float64 result
    x1 = x0.clone()
    ops.ei_step(x1, eps, k, None)
    assert torch.equal(x1, plain["x"])


@pytest.mark.parametrize("augmented", [1, 0])
def test_ei_step_kernel_on_misaligned_buffers(ops, augmented):
    """Buffers that start 4 (float32) / 8 (float64) bytes past a 16-byte boundary take the element-wise form: same values as
    the 16-byte form on aligned copies, bit for bit."""
    b, c, hw = 2, 3, 1024
    ct = 2 * c if augmented else c
    n = b * ct * hw
    k, phi, cm = _coeffs(3, augmented, seed=7)
    x0 = _rand(b, ct, hw, 1, seed=1, dtype=torch.float64).to(DEV)
    eps = [_rand(b, ct, hw, 1, seed=2 + j).to(DEV) for j in range(3)]
    xa, xfa = x0.clone(), torch.empty_like(eps[0])
    ops.ei_step(xa, eps, k, xfa)
    off = lambda t: torch.zeros(n + 1, device=DEV, dtype=t.dtype)[1:].view(t.shape).copy_(t)
    for which in ("x", "eps", "xf"):
        xm = off(x0) if which == "x" else x0.clone()
        em = [off(e) if which == "eps" and j == 1 else e for j, e in enumerate(eps)]
        xfm = off(xfa) if which == "xf" else torch.empty_like(xfa)
        assert (xm.data_ptr() % 16 != 0) == (which == "x") and (xfm.data_ptr() % 16 != 0) == (which == "xf")
        ops.ei_step(xm, em, k, xfm)
        assert torch.equal(xm, xa) and torch.equal(xfm, xfa), which


def test_ei_step_refuses_bad_arguments(ops):
    from psld_amd._lib import EiCoeffs
    x = torch.zeros(1, 2, 4, 1, device=DEV, dtype=torch.float64)
    e = torch.zeros(1, 2, 4, 1, device=DEV)
    k = EiCoeffs()
    k.n_hist, k.augmented = 1, 1
    with pytest.raises(ValueError):
        ops.ei_step(x, [e, e], k)                                            # history length against n_hist
    with pytest.raises(ValueError):
        ops.ei_step(x, [e[:, :1].contiguous()], k)                           # eps of another shape
    with pytest.raises(ValueError):
        ops.ei_step(x[:, :1].contiguous(), [e[:, :1].contiguous()], k)       # augmented state with an odd channel count
    for n_hist, aug in ((0, 1), (4, 1), (1, 2)):
        k.n_hist, k.augmented = n_hist, aug
        with pytest.raises((RuntimeError, ValueError), match="psld_ei_step_f64|ei_step"):
            ops.ei_step(x, [e] * n_hist, k)


# ---------------------------------------------------------------------------------------------------------------------
# the method on the device: 96 start points of the two-point mixture
# ---------------------------------------------------------------------------------------------------------------------
def _sampler(cfg, sde, fn, order):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    cfg = copy.deepcopy(cfg)
    cfg.evaluation.sampler = C.Config({"name": "ei_ode", "order": order})
    return get_module("samplers", "ei_ode")(cfg, sde, fn)


class _MixtureScore:
    """The mixture's exact eps as a device ``score_fn``: float64 torch ops on the float32 state, coefficients of the (float32)
    time from the reference on the host, result rounded to float32 like a network's output."""

    def __init__(self, ref):
        self.ref, self.calls = ref, 0

    def __call__(self, x32, t32):
        self.calls += 1
        ref, t = self.ref, float(t32[0])
        mu = ref.flow(t, 0.0) @ np.array([1.0, 0.0])
        w = np.linalg.inv(ref.sigma(t)) @ mu
        li = ref.chol_inv(t)
        h = x32.shape[1] // 2
        x, m = x32[:, :h].double(), x32[:, h:].double()
        g = torch.tanh(w[0] * x + w[1] * m)
        dx, dm = x - g * mu[0], m - g * mu[1]
        return torch.cat([li[0, 0] * dx + li[0, 1] * dm, li[1, 0] * dx + li[1, 1] * dm], 1).float()


@pytest.fixture(scope="module")
def mixture():
    from psld_amd.sde import PSLD
    cfg = C.yaml_default()
    ref = R.RefPSLD.from_config(cfg)
    u0 = R.start_points(ref.m)
    exact = R.from_pairs(ref.solve_mixture(R.to_pairs(u0).reshape(-1, 2), 1e-3).reshape(2, 3, 4, 4, 2))
    return cfg, PSLD(cfg), ref, torch.from_numpy(u0).to(DEV), torch.from_numpy(exact).to(DEV)


@pytest.mark.parametrize("n,order,bound", [(20, 1, 0.05), (20, 2, 0.05), (20, 3, 0.05), (10, 1, 0.1), (10, 2, 0.1)])
def test_sampler_on_the_mixture(mixture, n, order, bound):
    cfg, sde, ref, u0, exact = mixture
    fn = _MixtureScore(ref)
    s = _sampler(cfg, sde, fn, order)
    ts = torch.from_numpy(R.grid(n, "quadratic")).to(DEV)
    x = s.sample(u0, ts, n, denoise=False)
    assert x.dtype == torch.float64 and x.shape == u0.shape and s.nfe == n == fn.calls
    err = (x[:, :3] - exact[:, :3]).abs().max().item()
    print(f"ei_ode on the mixture, quadratic {n} steps, order {order}: max |x - exact| = {err:.3e}")
    assert err <= bound


def test_euler_probability_flow_steps_on_the_mixture(mixture, ops):
    """What the existing kernels reach on the same 20-step grid: Euler steps of the probability flow (em_step with
    probability_flow coefficients, no noise) leave fewer than 25 % of the samples within 0.05 (measured 5 % on the CPU)."""
    cfg, sde, ref, u0, exact = mixture
    fn = _MixtureScore(ref)
    tl = R.grid(20, "quadratic").tolist()
    x64 = u0.clone()
    x32 = x64.float()
    for i in range(20):
        t_rev = sde.T - tl[i]
        t32 = torch.full((2,), float(np.float32(t_rev)), device=DEV)
        ops.em_step(x64, fn(x32, t32).contiguous(), None, sde.em_coeffs(t_rev, tl[i + 1] - tl[i], probability_flow=True), x32)
    err = (x64[:, :3] - exact[:, :3]).abs()
    frac = (err <= 0.05).double().mean().item()
    print(f"Euler on the probability flow, quadratic 20 steps: {100 * frac:.1f} % within 0.05, max error {err.max().item():.2f}")
    assert frac < 0.25


# ---------------------------------------------------------------------------------------------------------------------
# tiny networks: the sampler against the float64 reference loop driven by the CPU oracle network
# ---------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name):
    if name not in _NETS:
        import psld_amd
        from psld_amd.registry import get_module
        psld_amd.import_modules_into_registry()
        cfg = {"vpsde": C.tiny_vpsde, "psld": C.tiny, "psld128": lambda: C.tiny(nf=128, ch_mult=(1, 1))}[name]()
        net = get_module("score_fn", "ncsnpp")(cfg)
        sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7)
        net.load_state_dict(sd, strict=True)
        _NETS[name] = net.to(DEV).eval(), cfg, sd
    return _NETS[name]


_REF_RUNS = {}


def _reference_run(name, order, denoise):
    """ei_ref's loop on ei_ref's own coefficients, eps from the oracle network on the float32 state and float32 time; the
    denoising step is the oracle's reverse_sde(probability_flow=True) Euler step of size eval_eps, as bb_ode's."""
    key = (name, order)
    _, cfg, sd = _net(name)
    vp = name == "vpsde"
    ts = R.grid(6, "quadratic")
    g = torch.Generator().manual_seed(91)
    batch = torch.randn(2, 3 if vp else 6, 16, 16, generator=g)
    net_fn = lambda u32, t32: O.ncsnpp_forward(sd, cfg, u32, t32)
    if key not in _REF_RUNS:
        def eps_fn(u, t, tau):
            u32 = torch.from_numpy(u if vp else R.from_pairs(u)).float()
            with torch.no_grad():
                e = net_fn(u32, torch.full((2,), float(np.float32(t)))).double().numpy()
            return e if vp else R.to_pairs(e)
        if vp:
            ref = R.RefVP(cfg.model.sde.beta_min, cfg.model.sde.beta_max)
            u = R.sample(ref.coeffs(ts, order), ts, batch.double().numpy(), eps_fn, augmented=False)
        else:
            ref = R.RefPSLD.from_config(cfg)
            u = R.from_pairs(R.sample(ref.coeffs(ts, order), ts, R.to_pairs(batch.double().numpy()), eps_fn))
        u = torch.from_numpy(u)
        osde = (O.VPSDEOracle(cfg.model.sde.beta_min, cfg.model.sde.beta_max) if vp else O.PSLDOracle.from_config(cfg))
        with torch.no_grad():
            f = osde.reverse_sde(u, torch.full((2,), 1.0 - 1e-3, dtype=torch.float64), net_fn, probability_flow=True)[0]
        _REF_RUNS[key] = (u, u + f * 1e-3)
    return batch, ts, _REF_RUNS[key][1 if denoise else 0]


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("name", ["psld", "vpsde"])
def test_sampler_with_tiny_networks(name, order, denoise):
    """6 quadratic steps against the reference loop + oracle network: the project's 1e-4 rel-L2 gate (the coefficients reach
    |C| ~ 50 on so short a grid and the synthetic weights give eps of ~1e4: the state is the accumulated C eps terms).
    Measured 3.5e-7 .. 3.6e-7 in all twelve cases.  The references of different orders lie 8e-4 .. 8e-3 apart and the
    denoising step moves the state by 9e-3 (PSLD) / 7e-5 (VP-SDE, below the gate): the result must also be nearer to its
    own reference than to those of the other orders and of the other denoise setting."""
    from psld_amd.registry import get_module
    net, cfg, _ = _net(name)
    sde = get_module("sde", cfg.model.sde.name)(cfg)
    batch, ts, want = _reference_run(name, order, denoise)
    s = _sampler(cfg, sde, net, order)
    x = s.sample(batch.to(DEV), torch.from_numpy(ts).to(DEV), 6, denoise=denoise, eps=1e-3)
    assert x.dtype == torch.float64 and x.shape == want.shape and s.nfe == 6 + int(denoise)
    err = rel_l2(x, want)
    print(f"ei_ode {name} order {order} denoise {denoise}: rel-L2 vs reference + oracle = {err:.3e}")
    assert err < 1e-4
    others = [_reference_run(name, o, d)[2] for o in (1, 2, 3) for d in (False, True) if (o, d) != (order, denoise)]
    assert all(rel_l2(x, w) > 10 * err for w in others)


def test_sampler_copies_a_reused_output_buffer():
    """A score function that writes every result into one buffer: the kept eps tensors are copies, same samples."""
    from psld_amd.registry import get_module
    net, cfg, _ = _net("psld")
    sde = get_module("sde", "psld")(cfg)
    batch, ts, _ = _reference_run("psld", 3, False)
    ts = torch.from_numpy(ts).to(DEV)
    out = torch.empty(2, 6, 16, 16, device=DEV)

    def reusing(x32, t32):
        return out.copy_(net(x32, t32))

    with torch.no_grad():
        a = _sampler(cfg, sde, net, 3).sample(batch.to(DEV), ts, 6, denoise=False)
        b = _sampler(cfg, sde, reusing, 3).sample(batch.to(DEV), ts, 6, denoise=False)
    assert torch.equal(a, b)


def test_sampler_under_every_eval_math_mode(ops):
    """The arithmetic of the evaluation forward (fp32 MFMA, two-limb bf16, fp16 products) changes the network's output only:
    the sampler runs under each and returns a finite float64 state (the distances to the default run are printed).  On a
    128-channel network with its 3x3 convolutions forced onto the Winograd limb kernels, which the modes switch."""
    from psld_amd.registry import get_module
    net, cfg, _ = _net("psld128")
    sde = get_module("sde", "psld")(cfg)
    ts = torch.from_numpy(R.grid(6, "quadratic")).to(DEV)
    batch = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(92))
    before = ops.math_mode(), ops.eval_math()
    try:
        ops.set_winograd(2)             # the Winograd launches at this small batch too: the ones the two-limb / fp16 modes switch
        base = _sampler(cfg, sde, net, 2).sample(batch.to(DEV), ts, 6, denoise=True)
        for math, ev in (("f32", "limb"), ("bf16x6", "limb"), ("bf16x3", "limb"), ("bf16x6", "f16")):
            ops.set_math_mode(math)
            ops.set_eval_math(ev)
            x = _sampler(cfg, sde, net, 2).sample(batch.to(DEV), ts, 6, denoise=True)
            assert x.dtype == torch.float64 and bool(torch.isfinite(x).all())
            d = rel_l2(x, base)
            print(f"ei_ode math {math} / eval math {ev}: rel-L2 vs default = {d:.3e}")
            assert (d == 0.0) == ((math, ev) == before), "the mode did not reach the network"
    finally:
        ops.set_winograd(None)
        ops.set_math_mode(before[0])
        ops.set_eval_math(before[1])


def test_sampler_under_cfg():
    """CFGScoreFn (one doubled-batch forward + combine kernel) against the two-pass torch callable under ei_ode, 3 quadratic
    steps + denoising: the combine's 4 * 2^-24 per element, amplified by |C| <= ~150 over the steps, stays under 1e-4."""
    from psld_amd.guidance import CFGScoreFn
    from psld_amd.registry import get_module
    from tests.test_cfg_gpu import _net as cond_net, _two_pass
    net, cfg, *_ = cond_net(32)
    sde = get_module("sde", "psld")(cfg)
    batch = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(63)).to(DEV)
    ts = torch.from_numpy(R.grid(3, "quadratic")).to(DEV)
    y = torch.tensor([1, 2], device=DEV)
    outs = [_sampler(cfg, sde, fn, 2).sample(batch, ts, 3, denoise=True, eps=1e-3)
            for fn in (CFGScoreFn(net, y, 1.5), _two_pass(net, y, 1.5), CFGScoreFn(net, y, 0.0))]
    e = rel_l2(outs[0], outs[1])
    print(f"ei_ode: 3 steps under CFGScoreFn against the two-pass callable: rel-L2 {e:.3e}")
    assert outs[0].dtype == torch.float64 and bool(torch.isfinite(outs[0]).all()) and e < 1e-4
    assert rel_l2(outs[2], outs[1]) > 1e-4                                  # (guidance changes the trajectory)


@pytest.mark.parametrize("config,channels", [("tiny", 3), ("tiny_vpsde", 3)])
def test_cli_sample_with_ei_ode(tmp_path, config, channels):
    from psld_amd import cli
    out = str(tmp_path / config)
    args = ["sample", "--config", config, "evaluation.n_samples=2", "evaluation.batch_size=2", "evaluation.n_discrete_steps=6",
            "evaluation.stride_type=quadratic", "evaluation.sampler.name=ei_ode", "evaluation.sampler.order=3",
            "evaluation.save_mode=np"]
    cli.main(args + [f"evaluation.save_path={out}"])
    files = sorted(os.listdir(os.path.join(out, "images")))
    assert files == ["output_gpu_0_0.npy"]
    a = np.load(os.path.join(out, "images", files[0]))
    assert a.dtype == np.uint8 and a.shape == (2, 16, 16, channels)
    cli.main(args + [f"evaluation.save_path={out}_again"])                  # deterministic given the seed
    np.testing.assert_array_equal(a, np.load(os.path.join(out + "_again", "images", files[0])))
    cli.main(args[:-1] + [f"evaluation.save_path={out}_img"])               # the default writer: one image file per sample
    assert len(os.listdir(os.path.join(out + "_img", "images"))) >= 1
    if config == "tiny":
        with pytest.raises(ValueError, match="order"):
            cli.main(args + [f"evaluation.save_path={out}_bad", "evaluation.sampler.order=4"])
        with pytest.raises(ValueError, match="score_m"):
            cli.main(args + [f"evaluation.save_path={out}_half", "model.sde.gamma=0.0", "model.sde.nu=4.0",
                             "model.score_fn.out_ch=3"])

"""Probability-flow likelihood on the GPU (psld_amd/likelihood.py, NCSNpp.vjp_input, the four kernels of csrc/sde.hip):

* the kernels against NumPy in float64 (odd tails, one wave, several workgroups per sample), bitwise repeatability,
  independence of a sample's value from its batch, guard bands;
* ``vjp_input`` against the full backward: bitwise ``dx`` and ``y``, the flat gradient buffer untouched;
* one right-hand-side evaluation against the oracle (autograd through ``oracle.reverse_sde(probability_flow=True)``);
* an analytic end-to-end check with the stationary Gaussian's score (no network, no oracle);
* the integrated ``log_prob`` against scipy's ``solve_ivp(RK45)`` on the augmented state with the oracle network;
* ``bpd``: its fields against ``log_prob_terms`` and the closed forms."""
import math

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import guard as G
from tests.synth import synth_state_dict
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 3, 25), (3, 3, 256), (2, 3, 1024)]       # (B, C, H*W): odd tails, one wave, several workgroups per sample


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rand(*shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _em_coeffs(score_mode=0):
    from psld_amd._lib import EmCoeffs
    k = EmCoeffs()
    k.beta, k.m_inv, k.gamma, k.nu, k.m = 8.0, 4.0, 0.01, 4.01, 0.25
    k.c11, k.c12, k.c21, k.c22 = 1.25, -0.5, 0.125, 2.0
    k.dt, k.score_mode, k.probability_flow = 0.0, score_mode, 0
    return k


# ---------------------------------------------------------------------------------------------------------------------
# kernels against NumPy float64
# ---------------------------------------------------------------------------------------------------------------------
def test_rademacher(ops):
    n, k = 100003, 4099
    whole = ops.rademacher(torch.empty(n, device=DEV), seed=1234, offset=7)
    v = whole.cpu().numpy()
    assert set(np.unique(v).tolist()) == {-1.0, 1.0}
    assert abs(v.mean()) <= 5.0 / math.sqrt(n), v.mean()
    # two launches over the halves of the range (the second on an unaligned pointer: the scalar kernel): the same values
    parts = torch.empty(n, device=DEV)
    ops.rademacher(parts[:k], seed=1234, offset=7)
    ops.rademacher(parts[k:], seed=1234, offset=7 + k)
    assert torch.equal(whole, parts)
    assert torch.equal(whole, ops.rademacher(torch.empty(n, device=DEV), seed=1234, offset=7))
    other = ops.rademacher(torch.empty(n, device=DEV), seed=1235, offset=7)
    assert 0.4 < (other != whole).float().mean().item() < 0.6
    # consecutive offsets are not correlated either
    assert abs(float((v[:-1] * v[1:]).mean())) <= 5.0 / math.sqrt(n)


def _gauss_ref(u, var_x, var_m, c_m):
    u = u.cpu().numpy().astype(np.float64)
    b, ct = u.shape[:2]
    out = []
    for i in range(b):
        x, m = u[i, :ct - c_m].ravel(), u[i, ct - c_m:].ravel()
        lp = -0.5 * math.fsum(x * x) / var_x - 0.5 * x.size * math.log(2 * math.pi * var_x)
        if m.size:
            lp += -0.5 * math.fsum(m * m) / var_m - 0.5 * m.size * math.log(2 * math.pi * var_m)
        out.append(lp)
    return np.array(out)


@pytest.mark.parametrize("b,c,hw", SHAPES)
@pytest.mark.parametrize("vp", [False, True])
def test_gauss_logp(ops, b, c, hw, vp):
    ct, c_m = (c, 0) if vp else (2 * c, c)
    u = _rand(3, ct, hw, 1, seed=5, dtype=torch.float64)[:b].contiguous().to(DEV)        # sample 0 is the same in every batch
    got = ops.gauss_logp(u, 1.0 if vp else 1.5, 0.25, c_m)
    ref = _gauss_ref(u, 1.0 if vp else 1.5, 0.25, c_m)
    assert got.dtype == torch.float64 and got.shape == (b,)
    err = np.abs(got.cpu().numpy() - ref) / np.abs(ref)
    assert err.max() <= 1e-13, err
    assert torch.equal(got, ops.gauss_logp(u, 1.0 if vp else 1.5, 0.25, c_m))
    one = ops.gauss_logp(u[:1].contiguous(), 1.0 if vp else 1.5, 0.25, c_m)
    assert torch.equal(one[0], got[0])


def test_prior_logp(ops):
    from psld_amd.sde import PSLD
    from psld_amd.vpsde import VPSDE
    sde = PSLD(C.tiny())
    z = sde.prior_sampling((3, 3, 8, 8), device=DEV)
    lp = sde.prior_logp(z)
    assert lp.dtype == torch.float64 and lp.shape == (3,)
    ref = _gauss_ref(z.double(), 1.0, sde.m, 3)
    assert np.abs(lp.cpu().numpy() - ref).max() <= 1e-13 * np.abs(ref).max()
    vp = VPSDE(C.tiny_vpsde())
    zv = vp.prior_sampling((3, 3, 8, 8), device=DEV)
    ref = _gauss_ref(zv.double(), 1.0, 1.0, 0)
    assert np.abs(vp.prior_logp(zv).cpu().numpy() - ref).max() <= 1e-13 * np.abs(ref).max()


def _pf_ref(k, vp_std, u, eps, vjp, z):
    """reverse_terms / vp_reverse_kernel of csrc/sde.hip on the CPU (score in fp32 with fp32 coefficients, the rest in fp64),
    sign flipped to forward time; the divergence estimate with an exactly rounded sum."""
    u, eps, vjp, z = u.cpu(), eps.cpu(), vjp.cpu(), z.cpu()
    b = u.shape[0]
    if vp_std > 0:
        g = math.sqrt(k.beta)
        score = 0.5 * (-eps.double() / vp_std)
        f = -(-(-0.5 * k.beta * u) + (g * g) * score)
        per = u[0].numel()
        div_lin = -0.5 * k.beta * per
    else:
        c = u.shape[1] // 2
        xv, mv = u[:, :c], u[:, c:]
        ex, em = (eps[:, :c], eps[:, c:]) if k.score_mode == 0 else (eps, eps)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        if k.score_mode == 1:
            sx, sm = torch.zeros_like(ex), -f32(k.c22) * em
        elif k.score_mode == 2:
            sx, sm = -f32(k.c11) * ex, torch.zeros_like(em)
        else:
            sx, sm = -f32(k.c11) * ex - f32(k.c12) * em, -f32(k.c21) * ex - f32(k.c22) * em
        sx, sm = f32(0.5) * sx, f32(0.5) * sm
        fx, fm = 0.5 * k.beta * (k.m_inv * mv - k.gamma * xv), 0.5 * k.beta * (-k.nu * mv - xv)
        gx, gm = math.sqrt(k.beta * k.gamma), math.sqrt(k.beta * k.m * k.nu)
        f = -torch.cat([-fx + (gx * gx) * sx.double(), -fm + (gm * gm) * sm.double()], 1)
        per = xv[0].numel()
        div_lin = -0.5 * k.beta * (k.gamma + k.nu) * per
    prod = (z.double() * vjp.double()).numpy()
    div = np.array([div_lin + math.fsum(prod[i].ravel()) for i in range(b)])
    return f.numpy().ravel(), div


def _pf_inputs(b, c, hw, mode):
    """(k, vp_std, u, eps, vjp, z) for score mode 0 / 1 / 2 or 'vp'; sample 0 is the same in every batch."""
    vp = mode == "vp"
    ct = c if vp else 2 * c
    k = _em_coeffs(0 if vp else mode)
    u = _rand(3, ct, hw, 1, seed=1, dtype=torch.float64)[:b].contiguous().to(DEV)
    eps = _rand(3, ct if (vp or mode == 0) else c, hw, 1, seed=2)[:b].contiguous().to(DEV)
    vjp = _rand(3, ct, hw, 1, seed=3)[:b].contiguous().to(DEV)
    z = _rand(3, ct, hw, 1, seed=4).sign()[:b].contiguous().to(DEV)
    return k, (0.75 if vp else 0.0), u, eps, vjp, z


@pytest.mark.parametrize("b,c,hw", SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, "vp"])
def test_pf_div_rhs(ops, b, c, hw, mode):
    k, vp_std, u, eps, vjp, z = _pf_inputs(b, c, hw, mode)
    got = ops.pf_div_rhs(u, eps, vjp, z, k, vp_std)
    n = u.numel()
    assert got.dtype == torch.float64 and got.shape == (n + b,)
    f_ref, div_ref = _pf_ref(k, vp_std, u, eps, vjp, z)
    g = got.cpu().numpy()
    assert np.abs(g[:n] - f_ref).max() <= 1e-13 * np.abs(f_ref).max()
    err = np.abs(g[n:] - div_ref) / np.abs(div_ref)
    assert err.max() <= 1e-13, err
    assert torch.equal(got, ops.pf_div_rhs(u, eps, vjp, z, k, vp_std))
    one = ops.pf_div_rhs(u[:1].contiguous(), eps[:1].contiguous(), vjp[:1].contiguous(), z[:1].contiguous(), k, vp_std)
    per = n // b
    assert torch.equal(one[:per], got[:per]) and torch.equal(one[per], got[n])


@pytest.mark.parametrize("b,c,hw", SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, "vp"])
def test_pf_cotangent(ops, b, c, hw, mode):
    k, vp_std, u, _, _, z = _pf_inputs(b, c, hw, mode)
    w = ops.pf_cotangent(z, k, vp_std)
    zz = z.cpu().double()
    hx, hm = 0.5 * k.beta * k.gamma, 0.5 * k.beta * k.m * k.nu
    if mode == "vp":
        ref = (0.5 * k.beta / vp_std) * zz
    elif mode == 1:
        ref = (hm * k.c22) * zz[:, c:]
    elif mode == 2:
        ref = (hx * k.c11) * zz[:, :c]
    else:
        zx, zm = zz[:, :c], zz[:, c:]
        ref = torch.cat([hx * k.c11 * zx + hm * k.c21 * zm, hx * k.c12 * zx + hm * k.c22 * zm], 1)
    assert w.dtype == torch.float32 and w.shape == ref.shape
    # float64 products rounded to float32 once: at most one float32 ulp from the rounded reference
    assert (w.cpu().double() - ref).abs().max().item() <= 2.0 ** -23 * ref.abs().max().item()


@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 64 << 20)
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.mark.parametrize("b,c,hw", [(3, 5, 7), (2, 3, 256)])
def test_guard_bands(ops, pool, monkeypatch, b, c, hw):
    """No read or write outside the documented buffers (tests/guard.py): the four kernels, PSLD and VP forms, with exactly
    psld_pf_workspace_bytes of workspace."""
    if pool.regions:
        pool.check()
        pool.release()
    guard = G.Guard(ops, pool).install(monkeypatch)
    n = 2 * b * c * hw
    G.run_guarded(guard, lambda out: ops.rademacher(out, 5, 11), dict(out=torch.zeros(n + 1, device=DEV)), ["out"])
    for mode in (0, 1, 2, "vp"):
        k, vp_std, u, eps, vjp, z = _pf_inputs(b, c, hw, mode)
        G.run_guarded(guard, lambda z: ops.pf_cotangent(z, k, vp_std), dict(z=z))
        G.run_guarded(guard, lambda u, eps, vjp, z: ops.pf_div_rhs(u, eps, vjp, z, k, vp_std), dict(u=u, eps=eps, vjp=vjp, z=z))
        assert guard.workspace_calls == 1
        G.run_guarded(guard, lambda u: ops.gauss_logp(u, 1.0, 0.25, 0 if mode == "vp" else c), dict(u=u))
        assert guard.workspace_calls == 1
    pool.check()


# ---------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(name):
    """(network in eval mode on the device, config, CPU state dict) of a tiny configuration, built once."""
    if name in _NETS:
        return _NETS[name]
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    if name == "clf":
        cfg = C.tiny_clf()
        net = get_module("clf_fn", "ncsnpp_clf")(cfg)
    else:
        if name == "vpsde":
            cfg = C.tiny_vpsde()
        elif name == "nf128_score_m":
            cfg = C.tiny(nf=128)
            cfg.model.score_fn.out_ch = 3
            cfg.model.sde.gamma, cfg.model.sde.nu = 0.0, 4.0
        else:
            cfg = C.tiny(nf=int(name[2:]))
        net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7)
    net.load_state_dict(sd)
    _NETS[name] = net.to(DEV).eval(), cfg, sd
    return _NETS[name]


@pytest.mark.parametrize("name", ["nf128", "nf160", "nf32", "clf"])
def test_vjp_input_is_the_full_backwards_dx(name):
    net, cfg, _ = _net(name)
    x, t = _rand(2, 6, 16, 16, seed=11).to(DEV), torch.tensor([0.3, 0.8], device=DEV)
    with torch.no_grad():
        out_shape = net(x, t).shape
    w = _rand(*out_shape, seed=12).to(DEV)
    fg = net.flat_grad()
    fg.copy_(torch.arange(fg.numel(), device=DEV, dtype=torch.float32) * 0.25 - 3.0)
    before = fg.clone()
    grads_before = [p.grad for p in net.parameters()]
    y, dx = net.vjp_input(x, t, w)
    assert net.flat_grad().data_ptr() == fg.data_ptr()
    assert torch.equal(fg, before), "vjp_input wrote into the flat gradient buffer"
    assert all(a is b for a, b in zip(grads_before, [p.grad for p in net.parameters()]))
    assert dx.shape == x.shape and dx.dtype == torch.float32 and not dx.requires_grad and not y.requires_grad
    xr = x.clone().requires_grad_()
    y_full = net(xr, t)
    y_full.backward(w)
    assert torch.equal(y, y_full.detach()), "y is not the recorded forward's output"
    assert torch.equal(dx, xr.grad), f"dx differs from the full backward's: rel-L2 {rel_l2(dx, xr.grad):.3e}"
    assert not torch.equal(fg, before)          # (the full backward does write the buffer: the check above can fail)
    assert float(dx.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# one right-hand side against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_sde(cfg):
    s = cfg.model.sde
    return O.VPSDEOracle(s.beta_min, s.beta_max) if s.name == "vpsde" else O.PSLDOracle.from_config(cfg)


def _oracle_rhs(osde, cfg, sd, u32, t32, z, vp):
    """(F, vjp, div) at the float32 state / time: F = -f_bar of the oracle's probability-flow reverse_sde (forward time),
    vjp = d(F . z)/d(network input) by autograd through it, div = div_lin + z . vjp per sample."""
    b = u32.shape[0]
    u_net = u32.clone().requires_grad_()
    tau = torch.full((b,), 1.0 - float(t32), dtype=torch.float64)               # reverse_sde evaluates at T - tau = t32
    f_bar, _ = osde.reverse_sde(u32, tau, lambda x, tt: O.ncsnpp_forward(sd, cfg, u_net, tt), probability_flow=True)
    f = -f_bar
    (vjp,) = torch.autograd.grad((f * z.double()).sum(), u_net)
    beta = float(osde.beta_t(float(t32)))
    per = u32[0].numel() // (1 if vp else 2)
    div_lin = -0.5 * beta * per * (1.0 if vp else (osde.gamma + osde.nu))
    div = div_lin + (z.double() * vjp.double()).flatten(1).sum(1)
    return f.detach(), vjp.detach(), div.detach()


def _sde_of(cfg):
    from psld_amd.registry import get_module
    return get_module("sde", cfg.model.sde.name)(cfg)


@pytest.mark.parametrize("when", ["eps", "0.3", "T-eps"])
@pytest.mark.parametrize("name", ["nf128", "nf128_score_m", "vpsde"])
def test_rhs_against_the_oracle(ops, name, when):
    """Drift rel-L2 < 1e-5, vjp rel-L2 < 1e-4 (the project's parity gate), per-sample divergence estimate within
    1e-4 |z| |vjp_oracle| (Cauchy-Schwarz on the gate; not a relative error of the estimate, which cancels heavily).

    Measured on an MI355X:

        network          t        drift rel-L2   vjp rel-L2
        nf128 (full)     1e-3     4.97e-7        1.21e-6
        nf128 (full)     0.3      1.82e-7        1.31e-6
        nf128 (full)     0.999    1.77e-7        1.18e-6
        nf128 (score_m)  1e-3     6.59e-7        1.20e-6
        nf128 (score_m)  0.3      1.78e-7        1.29e-6
        nf128 (score_m)  0.999    1.60e-7        1.29e-6
        vpsde            1e-3     6.54e-7        1.62e-6
        vpsde            0.3      4.73e-7        1.67e-6
        vpsde            0.999    4.12e-7        1.66e-6

    With the device's logf in the Fourier time embedding the two PSLD cases at t = eps stood at 1.69e-5 and 2.20e-5 (vjp
    3.99e-5, 3.81e-5): logf was one fp32 ulp from the nearest float there, 2 pi W log t reaches hundreds of radians, and the
    drift at t = eps is the network output times L_t^-T (~3e4).  The kernel now rounds log t correctly (csrc/pointwise.hip)."""
    from psld_amd.likelihood import PFLikelihood
    net, cfg, sd = _net(name)
    vp = name == "vpsde"
    sde, osde = _sde_of(cfg), _oracle_sde(cfg)
    lik = PFLikelihood(cfg, sde, net)
    ct = 3 if vp else 6
    u32 = _rand(2, ct, 16, 16, seed=21)
    z = ops.rademacher(torch.empty(2, ct, 16, 16, device=DEV), seed=3)
    z_cpu = z.cpu()
    eps0 = cfg.evaluation.eval_eps
    t = {"eps": eps0, "0.3": 0.3, "T-eps": 1.0 - eps0}[when]
    t32 = np.float32(t)
    out, _, vjp = lik.rhs_terms(u32.to(DEV), float(t), z)
    f_ref, vjp_ref, div_ref = _oracle_rhs(osde, cfg, sd, u32, t32, z_cpu, vp)
    n = u32.numel()
    e_f, e_v = rel_l2(out[:n], f_ref.flatten()), rel_l2(vjp, vjp_ref)
    d = (out[n:].cpu() - div_ref).abs()
    bound = 1e-4 * z_cpu.double().flatten(1).norm(dim=1) * vjp_ref.double().flatten(1).norm(dim=1)
    print(f"rhs {name} t={t}: drift rel-L2 {e_f:.3e}, vjp rel-L2 {e_v:.3e}, |d div| {d.tolist()} (bound {bound.tolist()}), "
          f"div {div_ref.tolist()}")
    assert e_v < 1e-4
    assert bool((d <= bound).all())
    assert e_f < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# analytic end to end: the stationary Gaussian
# ---------------------------------------------------------------------------------------------------------------------
def test_stationary_gaussian_psld(ops):
    """u ~ N(0, diag(I, M I)) is stationary under PSLD; with its score s = -(x, m / M), handed over as eps = -L_t^T s, the
    probability-flow drift is the rotation (1/2 beta M^-1 m, -1/2 beta x): int div F = 0 and log p_eps = the prior's density."""
    from psld_amd.likelihood import PFLikelihood
    cfg = C.tiny()
    sde = _sde_of(cfg)
    assert sde.mode == "score_xm"
    m_var = float(sde.m)

    def score_fn(x, t):
        tt = torch.tensor([float(t[0])], dtype=torch.float64)
        osde = O.PSLDOracle.from_config(cfg)
        l11, l12, l21, l22 = (float(v) for v in osde.coeff(osde.cov(0.0, osde.mm_0, tt)))
        sx, sm = -x[:, :3], -x[:, 3:] / m_var
        return torch.cat([-(l11 * sx + l21 * sm), -(l12 * sx + l22 * sm)], dim=1)

    rtol = 1e-5
    lik = PFLikelihood(cfg, sde, score_fn, rtol=rtol, atol=rtol)
    u0 = torch.cat([_rand(3, 3, 8, 8, seed=31), _rand(3, 3, 8, 8, seed=32) * math.sqrt(m_var)], 1).to(DEV)
    prior0 = sde.prior_logp(u0)
    prior, integral, nfe = lik.log_prob_terms(u0, seed=1)
    logp = prior + integral
    d = u0[0].numel() // 2
    print(f"stationary PSLD: logp {logp.tolist()} prior(u0) {prior0.tolist()} int div {integral.tolist()} nfe {nfe}")
    assert bool(((logp - prior0).abs() <= 10 * rtol * prior0.abs()).all())
    assert bool((integral.abs() <= 10 * rtol * d).all())
    lp2, nfe2 = lik.log_prob(u0, seed=1)
    assert torch.equal(lp2, logp) and nfe2 == nfe


def test_stationary_gaussian_vp(ops):
    """x ~ N(0, I) is stationary under the VP-SDE: eps = sigma_t x."""
    from psld_amd.likelihood import PFLikelihood
    cfg = C.tiny_vpsde()
    sde = _sde_of(cfg)
    rtol = 1e-5
    lik = PFLikelihood(cfg, sde, lambda x, t: x * float(sde._std(float(t[0]))), rtol=rtol, atol=rtol)
    u0 = _rand(3, 3, 8, 8, seed=33).to(DEV)
    prior0 = sde.prior_logp(u0)
    prior, integral, nfe = lik.log_prob_terms(u0, seed=2)
    print(f"stationary VP: logp {(prior + integral).tolist()} prior(u0) {prior0.tolist()} int div {integral.tolist()} nfe {nfe}")
    assert bool(((prior + integral - prior0).abs() <= 10 * rtol * prior0.abs()).all())
    assert bool((integral.abs() <= 10 * rtol * u0[0].numel()).all())


# ---------------------------------------------------------------------------------------------------------------------
# log_prob against scipy on the oracle network
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_log_prob_against_scipy(ops, tol):
    """Measured on an MI355X (with the device's logf in the time embedding; see test_rhs_against_the_oracle): tol 1e-3: logp (-13803.84, -13471.78) against (-13803.94, -13471.77), NFE 452 = 452; tol 1e-5:
    (-13767.53, -13481.54) against (-13767.74, -13481.33), NFE 2990 against 2996.  The synthetic weights make the score
    term large near t = eps (an untrained eps scaled by L_t^-T), hence the step counts - and the run time of the 1e-5 case,
    most of it the oracle's ~3000 forward + backward passes on the CPU."""
    from scipy.integrate import solve_ivp

    from psld_amd.likelihood import PFLikelihood
    net, cfg, sd = _net("nf32")
    sde, osde = _sde_of(cfg), _oracle_sde(cfg)
    shape = (2, 6, 16, 16)
    u0 = torch.cat([_rand(2, 3, 16, 16, seed=41) * 0.5, _rand(2, 3, 16, 16, seed=42) * math.sqrt(sde.mm_0)], 1)
    z = ops.rademacher(torch.empty(shape, device=DEV), seed=9)
    z_cpu = z.cpu()
    lik = PFLikelihood(cfg, sde, net, rtol=tol, atol=tol)
    logp, nfe = lik.log_prob(u0.to(DEV), probes=z)
    n = u0.numel()
    calls = [0]

    def func(t, y):
        calls[0] += 1
        u32 = torch.tensor(y[:n]).to(torch.float32).view(shape)
        f, _, div = _oracle_rhs(osde, cfg, sd, u32, np.float32(t), z_cpu, False)
        return np.concatenate([f.numpy().ravel(), div.numpy()])

    y0 = np.concatenate([u0.double().numpy().ravel(), np.zeros(2)])
    sol = solve_ivp(func, [cfg.evaluation.eval_eps, 1.0], y0, method="RK45", rtol=tol, atol=tol)
    u_t = torch.tensor(sol.y[:n, -1]).view(shape)
    ref = _gauss_ref(u_t, 1.0, osde.m, 3) + sol.y[n:, -1]
    got = logp.cpu().numpy()
    print(f"log_prob tol={tol}: {got.tolist()} (scipy + oracle {ref.tolist()}), NFE {nfe} (oracle {calls[0]})")
    assert np.all(np.abs(got - ref) <= 10 * tol * np.maximum(1.0, np.abs(ref)))
    assert abs(nfe - calls[0]) <= 6            # one rejected step: a float32-noise flip of one accept decision is no failure


# ---------------------------------------------------------------------------------------------------------------------
# bits per dimension
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nf32", "vpsde"])
def test_bpd(ops, name):
    from psld_amd.likelihood import LEVELS_NORM, PFLikelihood
    net, cfg, _ = _net(name)
    sde = _sde_of(cfg)
    vp = name == "vpsde"
    lik = PFLikelihood(cfg, sde, net, rtol=1e-2, atol=1e-2)       # (consistency of the fields: a loose solve is enough)
    x0 = (torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(51)) * 2 - 1).to(DEV)
    d = 3 * 16 * 16
    if vp:
        z = ops.rademacher(torch.empty(2, 3, 16, 16, device=DEV), seed=4)
        out = lik.bpd(x0, probes=z)
        prior, integral, nfe = lik.log_prob_terms(x0, probes=z)
        entropy = 0.0
    else:
        z = ops.rademacher(torch.empty(2, 6, 16, 16, device=DEV), seed=4)
        momenta = (math.sqrt(sde.mm_0) * _rand(2, 2, 3, 16, 16, seed=52)).to(DEV)
        out = lik.bpd(x0, n_momentum=2, probes=z, momenta=momenta)
        terms = [lik.log_prob_terms(torch.cat([x0, m0], 1), probes=z) for m0 in momenta]
        prior, integral = (terms[0][0] + terms[1][0]) / 2, (terms[0][1] + terms[1][1]) / 2
        nfe = terms[0][2] + terms[1][2]
        entropy = 0.5 * d * math.log(2 * math.pi * math.e * sde.mm_0)
    assert set(out) >= {"bpd", "logp", "nfe", "prior", "integral", "entropy", "offset"}
    assert out["nfe"] == nfe and out["entropy"] == pytest.approx(entropy, rel=1e-14) and out["offset"] == math.log2(LEVELS_NORM)
    assert torch.allclose(out["prior"], prior, rtol=1e-9, atol=0) and torch.allclose(out["integral"], integral, rtol=1e-9, atol=1e-9)
    logp = prior + integral + entropy
    assert torch.allclose(out["logp"], logp, rtol=1e-9, atol=0)
    assert torch.allclose(out["bpd"], -logp / (d * math.log(2.0)) + math.log2(127.5), rtol=1e-9, atol=0)
    assert out["bpd"].shape == (2,) and out["bpd"].dtype == torch.float64 and bool(torch.isfinite(out["bpd"]).all())
    print(f"bpd {name}: {out['bpd'].tolist()} nfe {out['nfe']}")


def test_bpd_command(capsys):
    """``python -m psld_amd.cli bpd`` in-process on the tiny preset: synthetic images, the freshly initialised EMA network,
    a loose solve - one JSON line with the documented fields."""
    import json

    from psld_amd import cli
    cli.main(["bpd", "--config", "tiny", "--synthetic-size", "4", "--max-images", "3", "--rtol", "1e-2", "--atol", "1e-2",
              "--n-momentum", "2", "evaluation.batch_size=2"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert set(out) == {"bpd", "bpd_stderr", "n_images", "mean_nfe"}
    assert out["n_images"] == 3 and math.isfinite(out["bpd"]) and out["bpd_stderr"] >= 0 and out["mean_nfe"] > 0

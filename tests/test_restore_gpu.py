"""Measurement-guided (posterior) sampling on the GPU: the two kernels against the float64 restatement
tests/restore_ref.py (values, guard bands, alignment forms, refusals), the two-phase ``NCSNpp.vjp_input``, ``PosteriorScoreFn``
on the tiny networks against the CPU oracle network differentiated by torch autograd, guided runs of three samplers with the
analytic Gaussian eps against CPU float64 loops fed the same noise, and the ``restore`` command.

Bounds.
  * kernels: an output element is the float32 rounding (relative 2^-24) of a float64 expression of n <= 4 p + 8 products and
    sums, p the pixels the operator couples (1 mask, 3 gray, k^2 pool); each rounds once, in either order of summation ->
    |err| <= 2^-24 |want| + (4 p + 8) 2^-53 sum|terms|.  The cotangent is formed from the unrounded g.
  * PosteriorScoreFn against oracle + autograd, and the samplers against the CPU loops: the project's 1e-4 rel-L2 gate.
  Measured values: profiles/r19/restore.md.

scipy is imported only inside the functions of the reference modules (see the header of tests/test_sampler_ei_gpu.py)."""
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
from tests import restore_ref as F
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_restore_cpu import OP_CASES
from tests.test_sampler_ei_gpu import U64, _net, _rand, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
OPS = {"mask": (0, 1), "gray": (1, 1), "pool2": (2, 2), "pool4": (2, 4)}
COUPLED = {"mask": 1, "gray": 3, "pool2": 4, "pool4": 16}


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as o
    o.lib()
    return o


@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 1 << 26)
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
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def _coeffs(augmented, seed):
    """Random coefficients of the sizes the host produces towards t -> T (|q_u|, |q_e| up to ~300, |l| <= 1.2, kappa ~ 1), as
    the struct and as the reference's."""
    from psld_amd._lib import RestoreCoeffs
    rng = np.random.default_rng(seed)
    q_u, q_e, l, kappa = rng.uniform(-300, 300, 2), rng.uniform(-300, 300, 2), rng.uniform(-1.2, 1.2, 3), rng.uniform(0.5, 2.0)
    k = RestoreCoeffs()
    k.augmented, k.kappa = augmented, kappa
    for i in range(2):
        k.q_u[i], k.q_e[i] = q_u[i], q_e[i]
    for i in range(3):
        k.l[i] = l[i]
    return k, F.Coeffs(q_u, q_e, l, kappa, bool(augmented), [0, 0], 0)


def _inputs(shape, task, augmented, seed=0):
    b, c, h, w = shape
    ct = 2 * c if augmented else c
    u, eps = _rand(b, ct, h, w, seed=seed + 1), _rand(b, ct, h, w, seed=seed + 2)
    y = _rand(*F.measurement_shape(shape, task), seed=seed + 3)
    mask = None
    if task == "mask":
        mask = (torch.rand(shape, generator=torch.Generator().manual_seed(seed + 4)) < 0.6).float()
        mask.view(-1)[0], mask.view(-1)[-1] = 1.0, 0.0
    return u, eps, y, mask


def _within(got, want, mag, n, what):
    want, mag = torch.from_numpy(want), torch.from_numpy(mag)
    err = (got.double().cpu() - want).abs()
    bound = U32 * want.abs() + n * U64 * mag
    assert bool((err <= bound).all()), (what, (err / bound.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("shape,task", OP_CASES)
@pytest.mark.parametrize("augmented", [1, 0])
def test_restore_kernels(ops, guard, augmented, shape, task):
    """ops.restore_measure and ops.restore_combine on guarded buffers and on ordinary ones: same bits, no band touched,
    inputs unchanged, wrapper-owned outputs inside the pool; values within the bound of this module's header."""
    k, q = _coeffs(augmented, seed=5 + augmented)
    op, blk = OPS[task]
    u, eps, y, mask = (None if t is None else t.to(DEV) for t in _inputs(shape, task, augmented))
    n = 4 * COUPLED[task] + 8
    tensors = dict(u=u, eps=eps, y=y, mask=mask)
    _, (g, cot) = G.run_guarded(guard, lambda u, eps, y, mask: ops.restore_measure(u, eps, y, mask, op, blk, k), tensors)
    cpu = lambda t: None if t is None else t.double().cpu().numpy()
    wg, ww, mg, mw = F.measure(cpu(u), cpu(eps), cpu(y), cpu(mask), task, q)
    assert g.shape == shape and cot.shape == u.shape and g.dtype == cot.dtype == torch.float32
    _within(g, wg, mg, n, "g")
    _within(cot, ww, mw, n + 1, "cotangent")
    dx = _rand(*u.shape, seed=9).to(DEV)
    plain, ret = G.run_guarded(guard, lambda eps, g, dx, out: ops.restore_combine(eps, g, dx, k, out),
                               dict(eps=eps, g=g, dx=dx, out=torch.full_like(eps, float("nan"))), outputs=["out"])
    assert ret.data_ptr() == plain["out"].data_ptr()
    want, mag = F.combine(cpu(eps), cpu(g), cpu(dx), q)
    _within(plain["out"], want, mag, 8, "combine")
    assert torch.equal(ops.restore_combine(eps, g, dx, k), plain["out"])        # the wrapper's own output buffer: the same


@pytest.mark.parametrize("task", ["mask", "gray", "pool2", "pool4"])
@pytest.mark.parametrize("augmented", [1, 0])
def test_restore_kernels_on_misaligned_buffers(ops, augmented, task):
    """A buffer that starts 4 bytes past a 16-byte boundary sends the launch to the element-wise form: the same values as
    the 16-byte form on aligned copies, bit for bit - each operand in turn."""
    shape = (2, 3, 32, 32)
    k, _ = _coeffs(augmented, seed=7)
    op, blk = OPS[task]
    u, eps, y, mask = (None if t is None else t.to(DEV) for t in _inputs(shape, task, augmented))
    off = lambda t: torch.zeros(t.numel() + 1, device=DEV, dtype=t.dtype)[1:].view(t.shape).copy_(t)
    g, cot = ops.restore_measure(u, eps, y, mask, op, blk, k)
    for which in ("u", "eps", "y") + (("mask",) if mask is not None else ()):
        args = {n: (off(t) if n == which else t) for n, t in dict(u=u, eps=eps, y=y, mask=mask).items()}
        for n, t in args.items():
            assert t is None or (t.data_ptr() % 16 != 0) == (n == which), (which, n)
        g2, cot2 = ops.restore_measure(args["u"], args["eps"], args["y"], args["mask"], op, blk, k)
        assert torch.equal(g2, g) and torch.equal(cot2, cot), which
    dx = _rand(*u.shape, seed=9).to(DEV)
    out = ops.restore_combine(eps, g, dx, k)
    for which in ("eps", "g", "dx", "out"):
        args = {n: (off(t) if n == which else t) for n, t in dict(eps=eps, g=g, dx=dx, out=torch.empty_like(eps)).items()}
        assert args[which].data_ptr() % 16 != 0
        assert torch.equal(ops.restore_combine(args["eps"], args["g"], args["dx"], k, args["out"]), out), which


def test_restore_kernels_refuse_bad_arguments(ops):
    """ValueError from the wrappers (RuntimeError for a dtype), before any launch."""
    k, _ = _coeffs(1, seed=1)
    u, e = torch.ones(2, 6, 8, 8, device=DEV), torch.ones(2, 6, 8, 8, device=DEV)
    y3, y1, yp = torch.ones(2, 3, 8, 8, device=DEV), torch.ones(2, 1, 8, 8, device=DEV), torch.ones(2, 3, 4, 4, device=DEV)
    half = lambda t: t[:, :3].contiguous()
    with pytest.raises(ValueError, match="eps of shape"):
        ops.restore_measure(u, half(e), y3, y3, 0, 1, k)
    with pytest.raises(ValueError, match="measurement of shape"):
        ops.restore_measure(u, e, yp, y3, 0, 1, k)                          # a pooled measurement for the mask operator
    with pytest.raises(ValueError, match="mask goes with"):
        ops.restore_measure(u, e, y3, None, 0, 1, k)
    with pytest.raises(ValueError, match="mask goes with"):
        ops.restore_measure(u, e, y1, y1, 1, 1, k)
    with pytest.raises(ValueError, match="mask of shape"):
        ops.restore_measure(u, e, y3, y1, 0, 1, k)
    with pytest.raises(ValueError, match="3 image channels"):
        ops.restore_measure(u[:, :4].contiguous(), e[:, :4].contiguous(), torch.ones(2, 1, 8, 8, device=DEV), None, 1, 1, k)
    with pytest.raises(ValueError, match="block size"):
        ops.restore_measure(u, e, yp, None, 2, 3, k)
    with pytest.raises(ValueError, match="multiple"):
        ops.restore_measure(torch.ones(2, 6, 6, 8, device=DEV), torch.ones(2, 6, 6, 8, device=DEV), yp, None, 2, 4, k)
    with pytest.raises(ValueError, match="operator code"):
        ops.restore_measure(u, e, y3, None, 3, 1, k)
    with pytest.raises(ValueError, match="even"):
        ops.restore_measure(half(u), half(e), y3, y3, 0, 1, k)              # augmented state with an odd channel count
    with pytest.raises(RuntimeError, match="float32"):
        ops.restore_measure(u.double(), e, y3, y3, 0, 1, k)
    with pytest.raises(ValueError, match="dx of shape"):
        ops.restore_combine(e, y3, half(e), k)
    with pytest.raises(ValueError, match="g of shape"):
        ops.restore_combine(e, y1, e, k)
    with pytest.raises(ValueError, match="out of shape"):
        ops.restore_combine(e, y3, e, k, half(e))
    with pytest.raises(ValueError, match="even"):
        ops.restore_combine(half(e), y3, half(e), k)
    for aug in (2, -1):
        k.augmented = aug
        with pytest.raises(ValueError, match="augmented"):
            ops.restore_measure(u, e, y3, y3, 0, 1, k)
        with pytest.raises(ValueError, match="augmented"):
            ops.restore_combine(e, y3, e, k)
    # the C entry points check on their own (host side, before the launch)
    k.augmented = 1
    import ctypes
    lib = ops.lib()
    p = lambda t: t.data_ptr()
    assert lib.psld_restore_measure_f32(p(u), p(e), p(y3), None, 0, 1, ctypes.byref(k), 2, 3, 8, 8, p(y3), p(e), None) != 0
    assert b"needs a mask" in lib.psld_last_error()
    assert lib.psld_restore_measure_f32(p(u), p(e), p(yp), None, 2, 4, ctypes.byref(k), 2, 3, 6, 8, p(y3), p(e), None) != 0
    assert b"multiple" in lib.psld_last_error()
    assert lib.psld_restore_measure_f32(p(u), p(e), p(y1), None, 1, 1, ctypes.byref(k), 2, 2, 8, 8, p(y3), p(e), None) != 0
    assert b"3 channels" in lib.psld_last_error()
    assert lib.psld_restore_combine_f32(p(e), p(y3), None, ctypes.byref(k), 2, 3, 64, p(e), None) != 0
    assert b"psld_restore_combine_f32" in lib.psld_last_error()
    assert bool((u == 1.0).all()) and bool((e == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# two-phase vjp_input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["psld", "vpsde"])
def test_two_phase_vjp_input(ops, name):
    """A callable cotangent sees the output a tensor-cotangent call returns, and dx is bit for bit that of a tensor-cotangent
    call given the same w - also when the callable launches the measure kernel between the two phases."""
    net, cfg, _ = _net(name)
    vp = name == "vpsde"
    x, t = _rand(2, 3 if vp else 6, 16, 16, seed=11).to(DEV), torch.full((2,), 0.3, device=DEV)
    w = _rand(2, 3 if vp else 6, 16, 16, seed=12).to(DEV)
    y1, dx1 = net.vjp_input(x, t, w)
    seen = []

    def w_fn(out):
        seen.append(out.clone())
        return w

    y2, dx2 = net.vjp_input(x, t, w_fn)
    assert len(seen) == 1 and torch.equal(seen[0], y1) and torch.equal(y2, y1) and torch.equal(dx2, dx1)
    assert float(dx1.abs().max()) > 0
    k, _ = _coeffs(0 if vp else 1, seed=3)
    yp = _rand(2, 3, 8, 8, seed=13).to(DEV)
    made = []

    def measured(out):
        made.append(ops.restore_measure(x, out, yp, None, 2, 2, k)[1])
        return made[0]

    y3, dx3 = net.vjp_input(x, t, measured)
    y4, dx4 = net.vjp_input(x, t, made[0])
    assert torch.equal(y3, y1) and torch.equal(y4, y1) and torch.equal(dx3, dx4)
    with pytest.raises(RuntimeError, match="float32"):
        net.vjp_input(x, t, lambda out: out.double())
    with pytest.raises(ValueError, match="cotangent of shape"):
        net.vjp_input(x, t, lambda out: out[:1].contiguous())
    y5, dx5 = net.vjp_input(x, t, w)                                         # an abandoned recorded pass leaves nothing behind
    assert torch.equal(y5, y1) and torch.equal(dx5, dx1)


# ---------------------------------------------------------------------------------------------------------------------
# PosteriorScoreFn on the tiny networks against oracle + autograd
# ---------------------------------------------------------------------------------------------------------------------
def _sde(cfg):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    return get_module("sde", cfg.model.sde.name)(cfg)


def _ref_coeffs(cfg, t, sigma_y, scale, v0):
    s = cfg.model.sde
    if s.name == "vpsde":
        return F.vp_coeffs(R.RefVP(s.beta_min, s.beta_max), t, sigma_y, scale, v0)
    return F.psld_coeffs(R.RefPSLD.from_config(cfg), t, sigma_y, scale, v0)


@pytest.mark.parametrize("task", ["mask", "gray", "pool2", "pool4"])
@pytest.mark.parametrize("name", ["psld", "vpsde"])
def test_posterior_score_fn_against_the_oracle(name, task):
    """eps' of one guided call against the CPU oracle network, torch autograd for J^T w and tests/restore_ref.py around it
    (its own coefficients): rel-L2 <= 1e-4."""
    from psld_amd.guidance import PosteriorScoreFn
    net, cfg, sd = _net(name)
    vp = name == "vpsde"
    sigma_y, scale, v0, t = 0.1, 1.3, 0.5, float(np.float32(0.4))
    x, _, y, mask = _inputs((2, 3, 16, 16), task, not vp, seed=20)
    fn = PosteriorScoreFn(net, _sde(cfg), task, sigma_y, scale, v0)
    fn.set_measurement(y.to(DEV), None if mask is None else mask.to(DEV))
    with torch.no_grad():
        got = fn(x.to(DEV), torch.full((2,), t, device=DEV))
        plain = net(x.to(DEV), torch.full((2,), t, device=DEV))
    q = _ref_coeffs(cfg, t, sigma_y, scale, v0)
    xr = x.clone().requires_grad_()
    eps = O.ncsnpp_forward(sd, cfg, xr, torch.full((2,), t))
    cpu = lambda v: None if v is None else v.detach().double().numpy()
    g, w, _, _ = F.measure(cpu(x), cpu(eps), cpu(y), cpu(mask), task, q)
    (dx,) = torch.autograd.grad(eps, xr, grad_outputs=torch.from_numpy(w).to(eps.dtype))
    want = torch.from_numpy(F.combine(cpu(eps), g, cpu(dx), q)[0])
    err, moved = rel_l2(got, want), rel_l2(plain, want)
    print(f"PosteriorScoreFn {name} {task}: rel-L2 vs oracle + autograd = {err:.3e} (the guidance moves eps by {moved:.2e})")
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert err <= 1e-4
    assert moved > 10 * 1e-4


def test_scale_zero_is_the_plain_forward(ops, monkeypatch):
    """torch.equal to net(x, t), no measurement needed, and neither kernel is launched; scale != 0 launches each once."""
    from psld_amd.guidance import PosteriorScoreFn
    net, cfg, _ = _net("psld")
    x, t = _rand(2, 6, 16, 16, seed=31).to(DEV), torch.full((2,), 0.4, device=DEV)
    calls = []
    measure, combine = ops.restore_measure, ops.restore_combine
    monkeypatch.setattr(ops, "restore_measure", lambda *a, **kw: (calls.append("measure"), measure(*a, **kw))[1])
    monkeypatch.setattr(ops, "restore_combine", lambda *a, **kw: (calls.append("combine"), combine(*a, **kw))[1])
    with torch.no_grad():
        want = net(x, t)
        got = PosteriorScoreFn(net, _sde(cfg), "gray", 0.1, scale=0.0)(x, t)
        assert torch.equal(got, want) and calls == []
        fn = PosteriorScoreFn(net, _sde(cfg), "gray", 0.1).set_measurement(_rand(2, 1, 16, 16, seed=32).to(DEV))
        assert not torch.equal(fn(x, t), want) and calls == ["measure", "combine"]


# ---------------------------------------------------------------------------------------------------------------------
# guided sampler runs with the analytic Gaussian eps against CPU float64 loops fed the same noise
# ---------------------------------------------------------------------------------------------------------------------
class _GaussScore:
    """eps of data N(0, v0) per pixel as a device ``score_fn`` built from differentiable torch operations: float64 on the
    float32 state, the 2 x 2 matrix of the (float32) time from the reference on the host, result rounded to float32."""

    def __init__(self, gauss):
        self.gauss, self.calls = gauss, 0

    def __call__(self, x32, t32):
        self.calls += 1
        j = self.gauss.jac(float(t32[0]))
        h = x32.shape[1] // 2
        x, m = x32[:, :h].double(), x32[:, h:].double()
        return torch.cat([j[0, 0] * x + j[0, 1] * m, j[1, 0] * x + j[1, 1] * m], 1).float()


def _seeded_noise(step, x):
    g = torch.Generator().manual_seed(2000 + step)
    return torch.randn(x.shape, generator=g, dtype=torch.float64).to(x.device)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _cpu_eps(gauss, u, t, y, mask, task, sigma_y, scale):
    """What the device computes, in float64 with its float32 roundings: eps of the float32 state at the float32 time rounded
    to float32, g and w rounded to float32, dx = J^T w rounded to float32, the combined eps rounded to float32."""
    u32, t32 = _f32(u), float(np.float32(t))
    e = _f32(gauss.eps(u32, t32))
    if scale == 0.0:
        return e
    q = gauss.coeffs(t32, sigma_y, scale)
    g, w, _, _ = F.measure(u32, e, y, mask, task, q)
    return _f32(F.combine(e, _f32(g), _f32(gauss.vjp(_f32(w), t32)), q)[0])


def _cpu_run(sampler, cfg, gauss, batch, ts, y, mask, task, sigma_y, scale):
    eps_nchw = lambda u, t: _cpu_eps(gauss, u, t, y, mask, task, sigma_y, scale)
    pairs = lambda u, t, tau: R.to_pairs(eps_nchw(R.from_pairs(u), t))
    noise = [_seeded_noise(i, batch) for i in range(len(ts) - 1)]
    if sampler == "ei_sde":
        steps = [(phi, c, S.chol2(p)) for phi, _, c, p in S.coeffs(gauss.ref, ts, 1.0)]
        return R.from_pairs(S.sample(steps, ts, R.to_pairs(batch.numpy()), pairs, lambda n, u: R.to_pairs(noise[n].numpy())))
    if sampler == "ei_ode":
        return R.from_pairs(R.sample(gauss.ref.coeffs(ts, 2), ts, R.to_pairs(batch.numpy()), pairs))
    score = lambda x32, t32: torch.from_numpy(eps_nchw(x32.double().numpy(), float(t32[0]))).float()
    return O.em_sample(O.PSLDOracle.from_config(cfg), score, batch, torch.from_numpy(ts), len(ts) - 1, denoise=False,
                       noise=noise).numpy()


_RUNS = {}


@pytest.mark.parametrize("sampler,task", [("ei_sde", "pool2"), ("em_sde", "mask"), ("ei_ode", "gray")])
def test_guided_sampler_runs(sampler, task):
    """6 quadratic steps on [4, 6, 8, 8] with seeded noise (ei_sde at lam = 1, em_sde, ei_ode at order 2) under
    PosteriorScoreFn around the analytic Gaussian eps (the torch-autograd path), against the CPU float64 loop of the same
    sampler fed the same noise: 1e-4 rel-L2, and the guidance moves the result by more than 10x that error."""
    import psld_amd
    from psld_amd.guidance import PosteriorScoreFn
    from psld_amd.registry import get_module
    from psld_amd.sde import PSLD
    psld_amd.import_modules_into_registry()
    cfg = copy.deepcopy(C.yaml_default())
    cfg.evaluation.sampler = C.Config({"name": sampler, "lam": 1.0, "order": 2})
    sde, gauss = PSLD(cfg), F.GaussPSLD(R.RefPSLD.from_config(cfg), 0.25)
    sigma_y, n = 0.1, 6
    ts = R.grid(n, "quadratic")
    gen = torch.Generator().manual_seed(77)
    batch = torch.randn(4, 6, 8, 8, generator=gen, dtype=torch.float64)
    batch[:, 3:] *= np.sqrt(gauss.ref.m)
    x0 = 0.5 * torch.randn(4, 3, 8, 8, generator=gen, dtype=torch.float64)
    mask = (torch.rand(4, 3, 8, 8, generator=gen) < 0.5).double() if task == "mask" else None
    y = F.forward(x0.numpy(), task, None if mask is None else mask.numpy())
    y = y + sigma_y * torch.randn(y.shape, generator=gen, dtype=torch.float64).numpy()
    y = _f32(y if mask is None else y * mask.numpy())
    mk = None if mask is None else mask.numpy()
    fn = PosteriorScoreFn(_GaussScore(gauss), sde, task, sigma_y, prior_var=0.25)
    fn.set_measurement(torch.from_numpy(y).to(DEV), None if mask is None else mask.to(DEV))
    s = get_module("samplers", sampler)(cfg, sde, fn)
    s.noise_fn = _seeded_noise
    x = s.sample(batch.to(DEV), torch.from_numpy(ts).to(DEV), n, denoise=False)
    assert x.dtype == torch.float64 and x.shape == (4, 6, 8, 8) and fn.net.calls == n
    want = torch.from_numpy(_cpu_run(sampler, cfg, gauss, batch, ts, y, mk, task, sigma_y, 1.0))
    free = torch.from_numpy(_cpu_run(sampler, cfg, gauss, batch, ts, y, mk, task, sigma_y, 0.0))
    err, moved = rel_l2(x, want), rel_l2(free, want)
    print(f"guided {sampler} ({task}), 6 quadratic steps: rel-L2 vs the CPU loop = {err:.3e}; guidance moves the result by {moved:.2e}")
    assert err < 1e-4
    assert moved > 10 * err and moved > 10 * 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["mask", "gray", "pool2", "pool4"])
def test_cli_restore(tmp_path, task):
    from psld_amd import cli
    out = str(tmp_path / task)
    momentum = task == "pool2"
    args = ["restore", "--config", "tiny", "--task", task, "--sigma-y", "0.05", "evaluation.n_samples=2",
            "evaluation.batch_size=2", "evaluation.n_discrete_steps=3", "evaluation.stride_type=quadratic",
            "evaluation.sampler.name=ei_sde", "evaluation.save_mode=np", "--synthetic-size", "4",
            f"evaluation.save_path={out}"] + (["evaluation.save_momentum=true"] if momentum else [])
    torch.manual_seed(5)                                                    # no checkpoint: the command draws its weights
    cli.main(args)
    assert sorted(os.listdir(out)) == ["batch", "corrupt", "images"] + (["momentum"] if momentum else [])
    arrays = {}
    for d in ("batch", "corrupt", "images"):
        assert os.listdir(os.path.join(out, d)) == ["output_gpu_0_0.npy"]
        a = arrays[d] = np.load(os.path.join(out, d, "output_gpu_0_0.npy"))
        assert a.dtype == np.uint8 and a.shape == (2, 16, 16, 3), d
    assert not np.array_equal(arrays["corrupt"], arrays["batch"])
    if task == "gray":
        assert np.array_equal(arrays["corrupt"][..., 0], arrays["corrupt"][..., 1])
    if task == "pool4":
        assert np.array_equal(arrays["corrupt"][:, ::4, ::4], arrays["corrupt"][:, 3::4, 3::4])
    if task == "mask":
        hole = arrays["corrupt"][:, 4:12, 4:12]
        assert not hole.any() and arrays["corrupt"][:, :4].any()
    if momentum:
        assert os.listdir(os.path.join(out, "momentum")) == ["output_gpu_0_0.npy"]
        m = np.load(os.path.join(out, "momentum", "output_gpu_0_0.npy"))
        assert m.dtype == np.float32 and m.shape == (2, 3, 16, 16) and np.isfinite(m).all()


def test_cli_sample_writes_the_momentum_half_when_asked(tmp_path):
    from psld_amd import cli
    base = ["sample", "--config", "tiny", "evaluation.n_samples=2", "evaluation.batch_size=2", "evaluation.n_discrete_steps=3",
            "evaluation.save_mode=np"]
    out = str(tmp_path / "plain")
    cli.main(base + [f"evaluation.save_path={out}"])
    assert os.listdir(out) == ["images"] and os.listdir(os.path.join(out, "images")) == ["output_gpu_0_0.npy"]
    out = str(tmp_path / "momentum")
    cli.main(base + [f"evaluation.save_path={out}", "evaluation.save_momentum=true"])
    assert sorted(os.listdir(out)) == ["images", "momentum"]
    m = np.load(os.path.join(out, "momentum", "output_gpu_0_0.npy"))
    assert m.dtype == np.float32 and m.shape == (2, 3, 16, 16) and np.isfinite(m).all()
    with pytest.raises(SystemExit, match="augmented"):
        cli.main(["sample", "--config", "tiny_vpsde", "evaluation.n_samples=2", "evaluation.batch_size=2",
                  "evaluation.n_discrete_steps=2", "evaluation.save_mode=np", f"evaluation.save_path={out}_vp",
                  "evaluation.save_momentum=true"])

"""The deconv operator of measurement-guided sampling on the GPU ("Deconvolution"): the three kernels of csrc/deconv.hip
against the float64 restatement tests/deconv_ref.py (values, guard bands, alignment forms, refusals), ``PosteriorScoreFn(...,
"deconv")`` on the tiny networks against the CPU oracle network differentiated by torch autograd, a guided ``ei_sde`` run with
the analytic Gaussian eps against the CPU float64 loop fed the same noise, and the ``restore`` command.

Bounds.
  * kernels.  A transform of an H x W plane is log2(HW / 2) butterfly levels and one level that separates (or merges) the two
    real sequences packed into one complex one.  Every value of every level is a sum of the plane's inputs with coefficients
    of modulus <= 1, so it is bounded by S = sum |inputs|; a level multiplies by a twiddle known to 2u and adds: its result
    carries an error of at most (2 + sqrt 5 + 1) u < 8u times S (u = 2^-53), and the errors of earlier levels pass through
    later ones with modulus <= 1.  So x^ and y^ err by at most 8u (log2(HW) + 1) S_x and ... S_y, S_x = sum mag(x0^) (which
    also covers the <= 4u mag(x0^) of forming x0^), S_y = sum |y|.  The filter g^ = m^ (y^ - h^ x^), m^ = conj(h^) (s2 + r2) /
    (s2 + r2 |h^|^2), is 12 more roundings of |m^| (S_y + |h^| S_x) at most; the inverse transform averages g^ over the
    frequencies and adds its own levels.  With T = (1 / HW) sum_omega |m^| (S_y + |h^| S_x) - deconv_ref.measure's mag:
        |g - want| <= 2^-24 |want| + 2 * 8 (2 log2(HW) + 12) u T,
    the factor 2 because numpy's transform, the reference, errs by no more than the same kind of bound.  The cotangent is
    formed from the unrounded g: one more rounding.  y^ alone: |y^ - want| <= 2 * 8 (log2(HW) + 1) u S_y (no float32 rounding:
    it is stored as float64).  A x / A^T x: as g with T = (1 / HW) sum_omega |h^| S_x.  h^ is an INPUT of the kernels (host
    float64): the tests hand the kernel and the reference the same bits of it - towards sigma_y = 0 the weight is 1 / h^, up
    to 4e9 for gauss:1.5, and a difference in the last bit of a tiny h^ would be a difference of the problem, not an error.
  * PosteriorScoreFn against oracle + autograd, and the sampler against the CPU loop: the project's 1e-4 rel-L2 gate.
  Measured values: profiles/r20/deconv.md.

scipy is imported only inside the functions of the reference modules (see the header of tests/test_sampler_ei_gpu.py)."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import deconv_ref as D
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests import guard as G
from tests import restore_ref as F
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_restore_gpu import _GaussScore, _coeffs, _f32, _ref_coeffs, _sde, _seeded_noise
from tests.test_sampler_ei_gpu import U64, _net, _rand, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
# (B, C, H, W): the smallest plane; several planes; H != W; ...; the largest plane (131 KiB of LDS); 300 planes, more than CUs
SHAPES = [(1, 1, 4, 4), (2, 3, 8, 8), (1, 3, 8, 16), (2, 3, 16, 16), (2, 3, 32, 32), (1, 3, 64, 64), (1, 1, 128, 128),
          (100, 3, 32, 32)]
R2 = 0.3
WORST = {}


def _levels(h, w):
    return int(math.log2(h * w))


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


def _spectrum(spec, h, w):
    """(k, full h^ [H, W] complex128, its half as the device tensor): the full one is the half's Hermitian extension bit for
    bit, so that the reference and the kernel (which reads the half alone) are given the same h^."""
    k = D.psf(spec, h, w)
    hh = D.hermitian(np.fft.fft2(k))
    return k, hh, torch.from_numpy(D.half(hh)).to(DEV)


def _within(got, want, mag, n, what):
    want, mag = torch.from_numpy(np.ascontiguousarray(want)), torch.from_numpy(np.ascontiguousarray(mag))
    err = (got.double().cpu() - want).abs()
    bound = U32 * want.abs() + n * U64 * mag
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma_y,spec", [(0.0, "gauss:1.5"), (0.05, "gauss:1.5"), (0.0, "box:3"), (0.05, "box:3")])
@pytest.mark.parametrize("augmented", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_deconv_kernels(ops, guard, shape, augmented, sigma_y, spec):
    """ops.restore_deconv_spectrum and ops.restore_deconv_measure on guarded buffers and on ordinary ones: same bits, no band
    touched, inputs unchanged, wrapper-owned outputs inside the pool; values within the bounds of this module's header."""
    b, c, h, w = shape
    kq, q = _coeffs(augmented, seed=5 + augmented)
    ct = 2 * c if augmented else c
    u, eps = _rand(b, ct, h, w, seed=1).to(DEV), _rand(b, ct, h, w, seed=2).to(DEV)
    y = _rand(b, c, h, w, seed=3).to(DEV)
    k, hh, hhat = _spectrum(spec, h, w)
    s2, lv = sigma_y ** 2, _levels(h, w)
    cpu = lambda t: t.double().cpu().numpy()
    _, yhat = G.run_guarded(guard, lambda y: ops.restore_deconv_spectrum(y), dict(y=y))
    assert yhat.shape == (b, c, h, w // 2 + 1, 2) and yhat.dtype == torch.float64
    sy = np.abs(cpu(y)).sum(axis=(2, 3), keepdims=True)[..., None] * np.ones(yhat.shape)
    want_y = D.half(np.fft.fft2(cpu(y)))
    err = np.abs(cpu(yhat) - want_y)
    bound = 2 * 8 * (lv + 1) * U64 * sy
    WORST["yhat"] = max(WORST.get("yhat", 0.0), float((err / bound).max()))
    assert (err <= bound).all(), ("yhat", float((err / bound).max()))
    _, (g, cot) = G.run_guarded(guard, lambda u, eps, yhat, hhat: ops.restore_deconv_measure(u, eps, yhat, hhat, kq, s2, R2),
                                dict(u=u, eps=eps, yhat=yhat, hhat=hhat))
    wg, ww, mg, mw = D.measure(cpu(u), cpu(eps), cpu(y), k, q, s2, R2, hh=hh)
    assert g.shape == shape and cot.shape == u.shape and g.dtype == cot.dtype == torch.float32
    n = 2 * 8 * (2 * lv + 12)
    rg = _within(g, wg, mg, n, "g")
    rc = _within(cot, ww, mw, n + 1, "cotangent")
    print(f"deconv kernels {shape} aug={augmented} sigma_y={sigma_y} {spec}: worst error / bound: yhat {float((err / bound).max()):.3f} "
          f"g {rg:.3f} cotangent {rc:.3f}; max |m^| {np.abs(D.weight(k, s2, R2, hh)[1]).max():.2e}")
    # the combine kernel serves this operator unchanged
    dx = _rand(*u.shape, seed=9).to(DEV)
    out = ops.restore_combine(eps, g, dx, kq)
    want, mag = F.combine(cpu(eps), cpu(g), cpu(dx), q)
    _within(out, want, mag, 8, "combine")


@pytest.mark.parametrize("spec", ["gauss:1.5", "box:3", "motion:3"])
@pytest.mark.parametrize("shape", [(1, 1, 4, 4), (1, 3, 8, 16), (2, 3, 32, 32), (1, 1, 128, 128), (100, 3, 32, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_apply_kernel(ops, guard, shape, spec):
    """A x and A^T x against the reference on guarded and ordinary buffers, and <A x, r> = <x, A^T r> on the device's values."""
    b, c, h, w = shape
    x, r = _rand(*shape, seed=21).to(DEV), _rand(*shape, seed=22).to(DEV)
    k, hh, hhat = _spectrum(spec, h, w)
    cpu = lambda t: t.double().cpu().numpy()
    _, ax = G.run_guarded(guard, lambda x, hhat: ops.restore_deconv_apply(x, hhat), dict(x=x, hhat=hhat))
    plain, ret = G.run_guarded(guard, lambda r, hhat, out: ops.restore_deconv_apply(r, hhat, True, out),
                               dict(r=r, hhat=hhat, out=torch.full_like(r, float("nan"))), outputs=["out"])
    atr = plain["out"]
    assert ret.data_ptr() == atr.data_ptr() and ax.shape == atr.shape == shape and ax.dtype == torch.float32
    n = 2 * 8 * (2 * _levels(h, w) + 12)
    t = np.abs(hh).mean()
    for got, src, fn, what in ((ax, x, D.forward, "A x"), (atr, r, D.adjoint, "A^T x")):
        mag = t * np.abs(cpu(src)).sum(axis=(2, 3), keepdims=True) * np.ones(shape)
        _within(got, fn(cpu(src), k), mag, n, what)
    lhs, rhs = (cpu(ax) * cpu(r)).sum(), (cpu(x) * cpu(atr)).sum()
    # both sides are float64 sums of float32-rounded values: 2^-24 of the magnitudes, plus the float64 term above
    slack = U32 * ((np.abs(cpu(ax)) * np.abs(cpu(r))).sum() + (np.abs(cpu(x)) * np.abs(cpu(atr))).sum())
    assert abs(lhs - rhs) <= 1.01 * slack, (lhs, rhs, slack)


@pytest.mark.parametrize("augmented", [1, 0])
def test_deconv_kernels_on_misaligned_buffers(ops, augmented):
    """A float32 buffer that starts 4 bytes past a 16-byte boundary sends the launch to the 4-byte form: the same values as
    the 16-byte form on aligned copies, bit for bit - each operand in turn."""
    shape = (2, 3, 32, 32)
    kq, _ = _coeffs(augmented, seed=7)
    ct = 6 if augmented else 3
    u, eps, y = _rand(2, ct, 32, 32, seed=1).to(DEV), _rand(2, ct, 32, 32, seed=2).to(DEV), _rand(*shape, seed=3).to(DEV)
    _, _, hhat = _spectrum("gauss:1.5", 32, 32)
    off = lambda t: torch.zeros(t.numel() + 1, device=DEV, dtype=t.dtype)[1:].view(t.shape).copy_(t)
    assert off(y).data_ptr() % 16 == 4 and y.data_ptr() % 16 == 0
    yhat = ops.restore_deconv_spectrum(y)
    assert torch.equal(ops.restore_deconv_spectrum(off(y)), yhat)
    g, cot = ops.restore_deconv_measure(u, eps, yhat, hhat, kq, 0.0025, R2)
    for which in ("u", "eps"):
        g2, cot2 = ops.restore_deconv_measure(off(u) if which == "u" else u, off(eps) if which == "eps" else eps, yhat, hhat,
                                              kq, 0.0025, R2)
        assert torch.equal(g2, g) and torch.equal(cot2, cot), which
    # the outputs: the C entry point on buffers of the test's own
    lib = ops.lib()
    g3, cot3 = off(torch.zeros_like(g)), torch.zeros_like(cot)
    assert lib.psld_restore_deconv_f32(u.data_ptr(), eps.data_ptr(), yhat.data_ptr(), hhat.data_ptr(), ctypes.byref(kq), 0.0025, R2,
                                       2, 3, 32, 32, g3.data_ptr(), cot3.data_ptr(), None) == 0
    assert torch.equal(g3, g) and torch.equal(cot3, cot)
    g4, cot4 = torch.zeros_like(g), off(torch.zeros_like(cot))
    assert lib.psld_restore_deconv_f32(u.data_ptr(), eps.data_ptr(), yhat.data_ptr(), hhat.data_ptr(), ctypes.byref(kq), 0.0025, R2,
                                       2, 3, 32, 32, g4.data_ptr(), cot4.data_ptr(), None) == 0
    assert torch.equal(g4, g) and torch.equal(cot4, cot)
    ax = ops.restore_deconv_apply(y, hhat)
    assert torch.equal(ops.restore_deconv_apply(off(y), hhat), ax)
    assert torch.equal(ops.restore_deconv_apply(y, hhat, False, off(torch.zeros_like(y))), ax)


def test_deconv_kernels_refuse_bad_arguments(ops):
    """ValueError from the wrappers (RuntimeError for a dtype) and a status from the C entry points, on the host, before any
    launch: nothing here reaches the device."""
    kq, _ = _coeffs(1, seed=1)
    u, e = torch.ones(2, 6, 8, 8, device=DEV), torch.ones(2, 6, 8, 8, device=DEV)
    y = torch.ones(2, 3, 8, 8, device=DEV)
    hhat = torch.ones(8, 5, 2, device=DEV, dtype=torch.float64)
    yhat = torch.ones(2, 3, 8, 5, 2, device=DEV, dtype=torch.float64)
    assert [ops.restore_deconv_supported(h, w) for h, w in ((4, 4), (128, 128), (8, 64), (2, 8), (256, 8), (8, 12), (8, 0), (-8, 8),
                                                            (6, 6))] == [True, True, True, False, False, False, False, False, False]
    half = lambda t: t[:, :3].contiguous()
    with pytest.raises(ValueError, match="eps of shape"):
        ops.restore_deconv_measure(u, half(e), yhat, hhat, kq, 0.01, R2)
    with pytest.raises(ValueError, match="measurement spectrum of shape"):
        ops.restore_deconv_measure(u, e, yhat[:, :2].contiguous(), hhat, kq, 0.01, R2)
    with pytest.raises(ValueError, match="PSF spectrum of shape"):
        ops.restore_deconv_measure(u, e, yhat, hhat[:, :4].contiguous(), kq, 0.01, R2)
    with pytest.raises(ValueError, match="even"):
        ops.restore_deconv_measure(half(u), half(e), yhat, hhat, kq, 0.01, R2)
    with pytest.raises(ValueError, match="positive sum"):
        ops.restore_deconv_measure(u, e, yhat, hhat, kq, 0.0, 0.0)
    with pytest.raises(ValueError, match="positive sum"):
        ops.restore_deconv_measure(u, e, yhat, hhat, kq, -0.01, R2)
    with pytest.raises(ValueError, match="positive sum"):
        ops.restore_deconv_measure(u, e, yhat, hhat, kq, float("nan"), R2)
    with pytest.raises(RuntimeError, match="float32"):
        ops.restore_deconv_measure(u.double(), e, yhat, hhat, kq, 0.01, R2)
    with pytest.raises(RuntimeError, match="float64"):
        ops.restore_deconv_measure(u, e, yhat.float(), hhat, kq, 0.01, R2)
    for bad in ((2, 6, 8, 12), (2, 6, 2, 8), (2, 6, 256, 8), (2, 6, 6, 6)):
        with pytest.raises(ValueError, match="power of two"):
            ops.restore_deconv_measure(torch.ones(bad, device=DEV), torch.ones(bad, device=DEV), yhat, hhat, kq, 0.01, R2)
        with pytest.raises(ValueError, match="power of two"):
            ops.restore_deconv_spectrum(torch.ones(bad, device=DEV))
        with pytest.raises(ValueError, match="power of two"):
            ops.restore_deconv_apply(torch.ones(bad, device=DEV), hhat)
    with pytest.raises(ValueError, match="no planes"):
        ops.restore_deconv_spectrum(torch.ones(0, 3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="out of shape"):
        ops.restore_deconv_apply(y, hhat, False, torch.ones(2, 3, 8, 4, device=DEV))
    for aug in (2, -1):
        kq.augmented = aug
        with pytest.raises(ValueError, match="augmented"):
            ops.restore_deconv_measure(u, e, yhat, hhat, kq, 0.01, R2)
    kq.augmented = 1
    # the C entry points check on their own
    lib = ops.lib()
    p = lambda t: t.data_ptr()
    g, cot = torch.ones_like(y), torch.ones_like(u)
    measure = lambda *a: lib.psld_restore_deconv_f32(*a)
    ok = [p(u), p(e), p(yhat), p(hhat), ctypes.byref(kq), 0.01, R2, 2, 3, 8, 8, p(g), p(cot), None]
    for i in (0, 1, 2, 3, 4, 11, 12):                                           # each null pointer in turn
        args = list(ok)
        args[i] = None
        assert measure(*args) != 0 and b"psld_restore_deconv_f32" in lib.psld_last_error()
    for i, v, what in ((9, 12, b"power of two"), (10, 6, b"power of two"), (9, 2, b"power of two"), (10, 256, b"power of two"),
                       (9, 0, b"power of two"), (7, 0, b"bad args"), (7, -2, b"bad args"), (8, 0, b"bad args"),
                       (5, -1.0, b"sigma_y"), (6, float("inf"), b"sigma_y"), (5, float("nan"), b"sigma_y")):
        args = list(ok)
        args[i] = v
        assert measure(*args) != 0 and what in lib.psld_last_error(), (i, v, lib.psld_last_error())
    kq.augmented = 3
    assert measure(*ok) != 0 and b"augmented" in lib.psld_last_error()
    kq.augmented = 1
    assert lib.psld_restore_deconv_spectrum_f32(None, 6, 8, 8, p(yhat), None) != 0
    assert lib.psld_restore_deconv_spectrum_f32(p(y), 6, 8, 8, None, None) != 0
    assert lib.psld_restore_deconv_spectrum_f32(p(y), 0, 8, 8, p(yhat), None) != 0
    assert lib.psld_restore_deconv_spectrum_f32(p(y), 6, 8, 24, p(yhat), None) != 0 and b"power of two" in lib.psld_last_error()
    assert lib.psld_restore_deconv_apply_f32(None, p(hhat), 0, 6, 8, 8, p(g), None) != 0
    assert lib.psld_restore_deconv_apply_f32(p(y), None, 0, 6, 8, 8, p(g), None) != 0
    assert lib.psld_restore_deconv_apply_f32(p(y), p(hhat), 0, 6, 8, 8, None, None) != 0
    assert lib.psld_restore_deconv_apply_f32(p(y), p(hhat), 2, 6, 8, 8, p(g), None) != 0 and b"adjoint" in lib.psld_last_error()
    assert lib.psld_restore_deconv_apply_f32(p(y), p(hhat), 0, -1, 8, 8, p(g), None) != 0
    assert lib.psld_restore_deconv_apply_f32(p(y), p(hhat), 0, 6, 512, 8, p(g), None) != 0 and b"power of two" in lib.psld_last_error()
    # the old measure entry point and the shape rule keep refusing operator code 3
    with pytest.raises(ValueError, match="operator code"):
        ops.restore_measurement_shape((2, 6, 8, 8), 3, 1, 1)
    assert lib.psld_restore_measure_f32(p(u), p(e), p(y), None, 3, 1, ctypes.byref(kq), 2, 3, 8, 8, p(g), p(cot), None) != 0
    assert b"operator code" in lib.psld_last_error()
    torch.cuda.synchronize()
    for t in (u, e, y, g, cot):
        assert bool((t == 1.0).all())
    assert bool((yhat == 1.0).all()) and bool((hhat == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# PosteriorScoreFn on the tiny networks against oracle + autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["gauss:1.5", "box:3"])
@pytest.mark.parametrize("name", ["psld", "vpsde"])
def test_posterior_score_fn_against_the_oracle(name, spec):
    """eps' of one guided call against the CPU oracle network, torch autograd for J^T w and tests/deconv_ref.py around it
    (its own coefficients and its own PSF): rel-L2 <= 1e-4."""
    from psld_amd.guidance import PosteriorScoreFn
    net, cfg, sd = _net(name)
    vp = name == "vpsde"
    sigma_y, scale, v0, t = 0.1, 1.3, 0.5, float(np.float32(0.4))
    shape = (2, 3, 16, 16)
    x, y = _rand(2, 3 if vp else 6, 16, 16, seed=21), _rand(*shape, seed=23)
    fn = PosteriorScoreFn(net, _sde(cfg), "deconv", sigma_y, scale, v0, psf=spec)
    fn.set_measurement(y.to(DEV))
    with torch.no_grad():
        got = fn(x.to(DEV), torch.full((2,), t, device=DEV))
        plain = net(x.to(DEV), torch.full((2,), t, device=DEV))
    q = _ref_coeffs(cfg, t, sigma_y, scale, v0)
    xr = x.clone().requires_grad_()
    eps = O.ncsnpp_forward(sd, cfg, xr, torch.full((2,), t))
    cpu = lambda v: v.detach().double().numpy()
    g, w, _, _ = D.measure(cpu(x), cpu(eps), cpu(y), D.psf(spec, 16, 16), q, sigma_y ** 2, q.r2)
    (dx,) = torch.autograd.grad(eps, xr, grad_outputs=torch.from_numpy(w).to(eps.dtype))
    want = torch.from_numpy(F.combine(cpu(eps), g, cpu(dx), q)[0])
    err, moved = rel_l2(got, want), rel_l2(plain, want)
    print(f"PosteriorScoreFn {name} deconv {spec}: rel-L2 vs oracle + autograd = {err:.3e} (the guidance moves eps by {moved:.2e})")
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert err <= 1e-4
    assert moved > 10 * 1e-4


def test_scale_zero_is_the_plain_forward(ops, monkeypatch):
    """torch.equal to net(x, t), no measurement needed, and no kernel of the guidance is launched; scale != 0 launches the
    deconv measure and the combine once each (and the measurement's spectrum once per measurement, not per call)."""
    from psld_amd.guidance import PosteriorScoreFn
    net, cfg, _ = _net("psld")
    x, t = _rand(2, 6, 16, 16, seed=31).to(DEV), torch.full((2,), 0.4, device=DEV)
    calls = []
    for name in ("restore_deconv_measure", "restore_combine", "restore_measure", "restore_deconv_spectrum", "restore_deconv_apply"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=getattr(ops, name), **kw: (calls.append(_n), _f(*a, **kw))[1])
    with torch.no_grad():
        want = net(x, t)
        off = PosteriorScoreFn(net, _sde(cfg), "deconv", 0.1, scale=0.0, psf="gauss:1.5")
        assert torch.equal(off(x, t), want) and calls == []
        off.set_measurement(_rand(2, 3, 16, 16, seed=32).to(DEV))
        assert torch.equal(off(x, t), want) and calls == []
        fn = PosteriorScoreFn(net, _sde(cfg), "deconv", 0.1, psf="gauss:1.5").set_measurement(_rand(2, 3, 16, 16, seed=32).to(DEV))
        first = fn(x, t)
        assert not torch.equal(first, want) and calls == ["restore_deconv_spectrum", "restore_deconv_measure", "restore_combine"]
        del calls[:]
        assert torch.equal(fn(x, t), first) and calls == ["restore_deconv_measure", "restore_combine"]
        fn.set_measurement(_rand(2, 3, 8, 8, seed=33).to(DEV))
        with pytest.raises(ValueError, match="measurement of shape"):
            fn(x, t)


# ---------------------------------------------------------------------------------------------------------------------
# a guided sampler run with the analytic Gaussian eps against the CPU float64 loop fed the same noise
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_eps(gauss, u, t, y, k, sigma_y, scale):
    """tests/test_restore_gpu._cpu_eps for the deconv operator: what the device computes, in float64 with its float32
    roundings."""
    u32, t32 = _f32(u), float(np.float32(t))
    e = _f32(gauss.eps(u32, t32))
    if scale == 0.0:
        return e
    q = gauss.coeffs(t32, sigma_y, scale)
    g, w, _, _ = D.measure(u32, e, y, k, q, sigma_y ** 2, q.r2)
    return _f32(F.combine(e, _f32(g), _f32(gauss.vjp(_f32(w), t32)), q)[0])


def test_guided_sampler_run():
    """6 quadratic steps of ei_sde at lam = 1 on [4, 6, 8, 8] with seeded noise under PosteriorScoreFn(..., "deconv") around the
    analytic Gaussian eps (the torch-autograd path), against the CPU float64 loop fed the same noise: 1e-4 rel-L2, and the
    guidance moves the result by more than 10x that."""
    import psld_amd
    from psld_amd.guidance import PosteriorScoreFn
    from psld_amd.registry import get_module
    from psld_amd.sde import PSLD
    psld_amd.import_modules_into_registry()
    cfg = copy.deepcopy(C.yaml_default())
    cfg.evaluation.sampler = C.Config({"name": "ei_sde", "lam": 1.0, "order": 2})
    sde, gauss = PSLD(cfg), F.GaussPSLD(R.RefPSLD.from_config(cfg), 0.25)
    sigma_y, n, spec = 0.1, 6, "gauss:1.0"
    ts = R.grid(n, "quadratic")
    gen = torch.Generator().manual_seed(77)
    batch = torch.randn(4, 6, 8, 8, generator=gen, dtype=torch.float64)
    batch[:, 3:] *= np.sqrt(gauss.ref.m)
    x0 = 0.5 * torch.randn(4, 3, 8, 8, generator=gen, dtype=torch.float64)
    k = D.psf(spec, 8, 8)
    y = _f32(D.forward(x0.numpy(), k) + sigma_y * torch.randn(x0.shape, generator=gen, dtype=torch.float64).numpy())
    fn = PosteriorScoreFn(_GaussScore(gauss), sde, "deconv", sigma_y, prior_var=0.25, psf=spec)
    fn.set_measurement(torch.from_numpy(y).to(DEV))
    s = get_module("samplers", "ei_sde")(cfg, sde, fn)
    s.noise_fn = _seeded_noise
    x = s.sample(batch.to(DEV), torch.from_numpy(ts).to(DEV), n, denoise=False)
    assert x.dtype == torch.float64 and x.shape == (4, 6, 8, 8) and fn.net.calls == n

    def run(scale):
        pairs = lambda u, t, tau: R.to_pairs(_cpu_eps(gauss, R.from_pairs(u), t, y, k, sigma_y, scale))
        noise = [_seeded_noise(i, batch) for i in range(n)]
        steps = [(phi, c, S.chol2(p)) for phi, _, c, p in S.coeffs(gauss.ref, ts, 1.0)]
        return torch.from_numpy(R.from_pairs(S.sample(steps, ts, R.to_pairs(batch.numpy()), pairs,
                                                      lambda i, u: R.to_pairs(noise[i].numpy()))))

    want, free = run(1.0), run(0.0)
    err, moved = rel_l2(x, want), rel_l2(free, want)
    print(f"guided ei_sde (deconv {spec}), 6 quadratic steps: rel-L2 vs the CPU loop = {err:.3e}; guidance moves the result by {moved:.2e}")
    assert err < 1e-4
    assert moved > 10 * err and moved > 10 * 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_restore_deconv(tmp_path):
    from psld_amd import cli
    out = str(tmp_path / "deconv")
    base = ["restore", "--config", "tiny", "--task", "deconv", "--sigma-y", "0.05", "evaluation.n_samples=2",
            "evaluation.batch_size=2", "evaluation.n_discrete_steps=3", "evaluation.stride_type=quadratic",
            "evaluation.sampler.name=ei_sde", "evaluation.save_mode=np", "--synthetic-size", "4", f"evaluation.save_path={out}"]
    torch.manual_seed(5)                                                    # no checkpoint: the command draws its weights
    cli.main(base + ["--psf", "gauss:1.0"])
    assert sorted(os.listdir(out)) == ["batch", "corrupt", "images"]
    arrays = {}
    for d in ("batch", "corrupt", "images"):
        assert os.listdir(os.path.join(out, d)) == ["output_gpu_0_0.npy"]
        a = arrays[d] = np.load(os.path.join(out, d, "output_gpu_0_0.npy"))
        assert a.dtype == np.uint8 and a.shape == (2, 16, 16, 3), d
    assert not np.array_equal(arrays["corrupt"], arrays["batch"])
    with pytest.raises(SystemExit, match="PSF"):
        cli.main(base)                                                       # deconv without --psf
    with pytest.raises(SystemExit, match="PSF"):
        cli.main([a if a != "deconv" else "gray" for a in base] + ["--psf", "gauss:1.0"])
    with pytest.raises(SystemExit, match="larger"):
        cli.main(base + ["--psf", "box:17"])


def test_worst_ratios_are_recorded():
    """Runs last: the worst error / bound of the kernel tests of this session (recorded in profiles/r20/deconv.md)."""
    print("deconv kernels, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())

"""The super-resolution operator of measurement-guided sampling on the GPU ("Super-resolution"): the measure
and apply kernels of csrc/deconv.hip against the float64 restatement tests/sr_ref.py (values, guard bands, alignment forms,
refusals), a cross-check against the pool kernels that needs no reference, ``PosteriorScoreFn(..., "sr2" | "sr4")`` on the tiny
networks against the CPU oracle network differentiated by torch autograd, guided sampler runs with the analytic Gaussian eps
against the CPU float64 loops fed the same noise, and the ``restore`` command.

Bounds (u = 2^-53; the per-level argument of tests/test_deconv_gpu.py).
  * A transform of an h x w plane is log2(hw) levels (log2(hw / 2) butterfly levels and the one that separates or merges the
    two real sequences packed into a complex one); every value of every level is a sum of the plane's inputs with coefficients
    of modulus <= 1, so it is bounded by S = sum |inputs|, and a level adds an error of at most 8u S; earlier errors pass
    through later levels with modulus <= 1.  A transform pair with a pointwise filter between (<= 12 roundings, which also
    cover forming its input and scaling its output) is therefore 8 (2 log2(hw) + 12) u times the bound on its OUTPUT values,
    (1 / hw) sum_omega |filter| S.
  * the measure kernel chains three pairs, L = log2(HW), L' = log2(HW / s^2).  A pair's own rounding is that factor times the
    bound on its output values, which is mean|filter| times the sum of the magnitudes of the inputs IT is given:
        z   = IFFT2(h^ FFT2 x0^):            own error <= 8 (2 L + 12) u T1,    T1 = mean|h^| sum mag(x0^);
        v   = IFFT2'(f FFT2' rho):           own error <= 8 (2 L' + 12) u T2,   T2 = mean|f| sum|rho|,  rho = y - D_s z,
                                             f = (s2 + r2) / (s2 + r2 Lambda);
        g   = IFFT2(conj(h^) FFT2(D_s^T v)): own error <= 8 (2 L + 12) u T3,    T3 = mean|h^| sum|v|
    (the 12 of a pair also cover forming its input - x0^, the subtraction from y, the scaling by 1 / hw - and its filter).
    An error made in z reaches g through the two later pairs, which in space are the convolutions with kf = IFFT2'(f) and
    with k: an elementwise error bound grows by at most their l1 norms |kf|_1 and |k|_1 (decimation and zero insertion only
    drop or move entries); an error made in v reaches g through |k|_1.  So with
        T = max(T3, |k|_1 T2, |k|_1 |kf|_1 T1)          (sr_ref.measure's mag: from the inputs and the reference's own rho, v)
    and the factor 2 for numpy's own transforms (the reference errs by no more than the same kind of bound):
        |g - want| <= 2^-24 |want| + 2 * 8 (4 L + 2 L' + 36) u T;
    the cotangent is formed from the unrounded g: one more rounding.  A x and A^T r: one pair each,
        <= 2^-24 |want| + 2 * 8 (2 L + 12) u mean|h^| sum|input|.
    The bound is derived, not fitted: a ratio above 1 is a bug in the kernel or in the derivation.  (A first version bounded
    sum|rho| and sum|v| by worst cases, n' T1 and n' T2: correct, but at 128 x 128 that float64 term was 1e5 times the float32
    rounding and would have let a wrong kernel pass; with the sums themselves the two terms are of one size.)
  * h^ and Lambda are INPUTS of the kernels (host float64): the tests hand the kernel and the reference the same bits.
  * the cross-check, PosteriorScoreFn against oracle + autograd, the samplers against the CPU loops: stated at each test.
  Measured values: profiles/r21/sr.md.

scipy is imported only inside the functions of the reference modules (see the header of tests/test_sampler_ei_gpu.py)."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import _lib
from psld_amd import config as C
from tests import deconv_ref as D
from tests import ei_ref as R
from tests import ei_sde_ref as S
from tests import guard as G
from tests import restore_ref as F
from tests import sr_ref as Q
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_restore_gpu import _GaussScore, _coeffs, _f32, _ref_coeffs, _sde, _seeded_noise
from tests.test_sampler_ei_gpu import U64, _net, _rand, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
# (B, C, H, W, s): the smallest low-resolution plane (4 x 4) at both factors; H != W in both orders; several planes; the largest
# plane (the full LDS budget, the low-resolution plane in the full one's storage); 300 planes, more than CUs
SHAPES = [(1, 1, 8, 8, 2), (1, 1, 16, 16, 4), (1, 3, 8, 16, 2), (1, 3, 32, 16, 4), (2, 3, 32, 32, 2), (2, 3, 32, 32, 4),
          (1, 1, 128, 128, 2), (1, 1, 128, 128, 4), (100, 3, 32, 32, 4)]
KERNELS = ["bicubic", "gauss:1.5", "block"]
R2 = 0.3
WORST = {}
_ids = lambda s: "x".join(map(str, s))


def _n_measure(h, w, s):
    return 2 * 8 * (4 * int(math.log2(h * w)) + 2 * int(math.log2(h * w // (s * s))) + 36)


def _n_apply(h, w):
    return 2 * 8 * (2 * int(math.log2(h * w)) + 12)


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


_SPECTRA = {}


def _spectra(spec, s, h, w):
    """(k, full h^ [H, W], full Lambda [H/s, W/s], h^'s half and Lambda's half as device tensors): the full ones are the
    halves' symmetric extensions bit for bit, so that the reference and the kernels (which read the halves alone) are given
    the same h^ and Lambda.  Computed once per case and left unchanged."""
    key = (spec, s, h, w)
    if key not in _SPECTRA:
        k = Q.kernel(spec, s, h, w)
        hh = D.hermitian(np.fft.fft2(k))
        half = np.ascontiguousarray(Q.lam(hh, s)[:, :w // s // 2 + 1])
        _SPECTRA[key] = (k, hh, Q.symmetric(half, w // s), torch.from_numpy(D.half(hh)).to(DEV), torch.from_numpy(half).to(DEV))
    return _SPECTRA[key]


def _within(got, want, mag, n, what):
    want, mag = torch.from_numpy(np.ascontiguousarray(want)), torch.from_numpy(np.ascontiguousarray(mag))
    err = (got.double().cpu() - want).abs()
    bound = U32 * want.abs() + n * U64 * mag
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


cpu = lambda t: t.double().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", KERNELS)
@pytest.mark.parametrize("sigma_y", [0.0, 0.05])
@pytest.mark.parametrize("augmented", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_sr_measure_kernel(ops, guard, shape, augmented, sigma_y, spec):
    """ops.restore_sr_measure on guarded buffers and on ordinary ones: same bits, no band touched, inputs unchanged,
    wrapper-owned outputs inside the pool; values within the bound of this module's header."""
    b, c, h, w, s = shape
    kq, q = _coeffs(augmented, seed=5 + augmented)
    ct = 2 * c if augmented else c
    u, eps = _rand(b, ct, h, w, seed=1).to(DEV), _rand(b, ct, h, w, seed=2).to(DEV)
    y = _rand(b, c, h // s, w // s, seed=3).to(DEV)
    k, hh, lm, hhat, lam = _spectra(spec, s, h, w)
    s2 = sigma_y ** 2
    _, (g, cot) = G.run_guarded(guard, lambda u, eps, y, hhat, lam: ops.restore_sr_measure(u, eps, y, hhat, lam, kq, s2, R2, s),
                                dict(u=u, eps=eps, y=y, hhat=hhat, lam=lam))
    wg, ww, mg, mw = Q.measure(cpu(u), cpu(eps), cpu(y), k, s, q, s2, R2, hh=hh, lm=lm)
    assert g.shape == (b, c, h, w) and cot.shape == u.shape and g.dtype == cot.dtype == torch.float32
    n = _n_measure(h, w, s)
    rg = _within(g, wg, mg, n, "g")
    rc = _within(cot, ww, mw, n + 1, "cotangent")
    print(f"sr measure {shape} aug={augmented} sigma_y={sigma_y} {spec}: worst error / bound: g {rg:.3f} cotangent {rc:.3f}; "
          f"max weight {np.abs(Q.solve_weight(lm, s2, R2)).max():.2e}")
    # the combine kernel serves this operator unchanged
    dx = _rand(*u.shape, seed=9).to(DEV)
    out = ops.restore_combine(eps, g, dx, kq)
    want, mag = F.combine(cpu(eps), cpu(g), cpu(dx), q)
    _within(out, want, mag, 8, "combine")


@pytest.mark.parametrize("spec", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_sr_apply_kernel(ops, guard, shape, spec):
    """A x (to low resolution) and A^T r (to full resolution) against the reference on guarded and ordinary buffers, and
    <A x, r> = <x, A^T r> on the device's values."""
    b, c, h, w, s = shape
    low = (b, c, h // s, w // s)
    x, r = _rand(b, c, h, w, seed=21).to(DEV), _rand(*low, seed=22).to(DEV)
    k, hh, _, hhat, _ = _spectra(spec, s, h, w)
    _, ax = G.run_guarded(guard, lambda x, hhat: ops.restore_sr_apply(x, hhat, s), dict(x=x, hhat=hhat))
    plain, ret = G.run_guarded(guard, lambda r, hhat, out: ops.restore_sr_apply(r, hhat, s, True, out),
                               dict(r=r, hhat=hhat, out=torch.full((b, c, h, w), float("nan"), device=DEV)), outputs=["out"])
    atr = plain["out"]
    assert ret.data_ptr() == atr.data_ptr() and ax.shape == low and atr.shape == (b, c, h, w) and ax.dtype == torch.float32
    n, t = _n_apply(h, w), np.abs(hh).mean()
    _within(ax, Q.forward(cpu(x), k, s, hh), t * np.abs(cpu(x)).sum(axis=(2, 3), keepdims=True) * np.ones(low), n, "A x")
    _within(atr, Q.adjoint(cpu(r), k, s, hh), t * np.abs(cpu(r)).sum(axis=(2, 3), keepdims=True) * np.ones((b, c, h, w)), n, "A^T r")
    lhs, rhs = (cpu(ax) * cpu(r)).sum(), (cpu(x) * cpu(atr)).sum()
    # both sides are float64 sums of float32-rounded values: 2^-24 of the magnitudes
    slack = U32 * ((np.abs(cpu(ax)) * np.abs(cpu(r))).sum() + (np.abs(cpu(x)) * np.abs(cpu(atr))).sum())
    assert abs(lhs - rhs) <= 1.01 * slack, (lhs, rhs, slack)


@pytest.mark.parametrize("sigma_y", [0.0, 0.05])
@pytest.mark.parametrize("augmented", [1, 0])
@pytest.mark.parametrize("shape", [(2, 3, 8, 16, 2), (2, 3, 32, 32, 2), (2, 3, 32, 32, 4), (1, 1, 128, 128, 4)], ids=_ids)
def test_block_kernel_agrees_with_the_pool_kernels(ops, shape, augmented, sigma_y):
    """No reference: with the ``block`` kernel A_sr = A_pool / s and A_sr A_sr^T = I / s^2, so for the measurement y / s with
    noise sigma / s
        g_sr = c g_pool,  c = (sigma^2 / s^2 + r2) / (sigma^2 + r2),    kappa_sr = scale / (sigma^2 / s^2 + r2) = kappa_pool / c:
    kappa g coincides, and with it eps' after restore_combine (dx, linear in g, scaled by c likewise).  y / s is exact in
    float32 (s is a power of two).  Gate, per element of eps': both outputs' float32 rounding and 8 float64 roundings of the
    combine's terms (F.combine's mag), plus kappa |q_e| times each g's own bound (2^-24 |g| + n u T, T and n from the two
    reference modules' magnitude propagation - magnitudes only, neither g is compared with a reference value), plus 2^-24 kappa max|l| (|dx_x| + |dx_m|) for rounding c dx to float32."""
    b, c, h, w, s = shape
    kq, q = _coeffs(augmented, seed=11 + augmented)
    ct = 2 * c if augmented else c
    u, eps = _rand(b, ct, h, w, seed=1).to(DEV), _rand(b, ct, h, w, seed=2).to(DEV)
    y, dx = _rand(b, c, h // s, w // s, seed=3).to(DEV), _rand(b, ct, h, w, seed=9).to(DEV)
    k, hh, lm, hhat, lam = _spectra("block", s, h, w)
    s2 = sigma_y ** 2
    ratio = (s2 / s ** 2 + R2) / (s2 + R2)
    kq.kappa = q.kappa = 1.3 / (s2 + R2)
    g_pool, _ = ops.restore_measure(u, eps, y, None, _lib.RESTORE_POOL, s, kq)
    out_pool = ops.restore_combine(eps, g_pool, dx, kq)
    kq.kappa = 1.3 / (s2 / s ** 2 + R2)
    g_sr, _ = ops.restore_sr_measure(u, eps, y / s, hhat, lam, kq, s2 / s ** 2, R2, s)
    dx_sr = (dx.double() * ratio).float()
    out_sr = ops.restore_combine(eps, g_sr, dx_sr, kq)
    # magnitudes only
    _, _, mag_pool, _ = F.measure(cpu(u), cpu(eps), cpu(y), None, f"pool{s}", q)
    _, _, mag_sr, _ = Q.measure(cpu(u), cpu(eps), cpu(y) / s, k, s, q, s2 / s ** 2, R2, hh=hh, lm=lm)
    _, mag_c = F.combine(cpu(eps), cpu(g_pool), cpu(dx), q)
    qe = np.abs(q.q_e[:2] if augmented else q.q_e[:1]).reshape(1, -1, 1, 1, 1)
    tile = lambda a: np.concatenate([a[:, None]] * qe.shape[1], axis=1)          # [B, halves, C, H, W]
    kp, ks = q.kappa, q.kappa / ratio
    gate_g = (kp * qe * tile(U32 * np.abs(cpu(g_pool)) + (4 * s * s + 8) * U64 * mag_pool)
              + ks * qe * tile(U32 * np.abs(cpu(g_sr)) + _n_measure(h, w, s) * U64 * mag_sr)).reshape(b, ct, h, w)
    dsum = np.abs(cpu(dx_sr))                                                  # each half of eps' takes dx from both halves
    if augmented:
        dsum = np.concatenate([dsum[:, :c] + dsum[:, c:]] * 2, axis=1)
    gate = 2 * (U32 * np.abs(cpu(out_pool)) + 8 * U64 * mag_c) + gate_g + U32 * ks * np.abs(q.l).max() * dsum
    err = np.abs(cpu(out_sr) - cpu(out_pool))
    worst = float((err / gate).max())
    WORST["block vs pool"] = max(WORST.get("block vs pool", 0.0), worst)
    print(f"sr block against pool {shape} aug={augmented} sigma_y={sigma_y}: worst difference / gate {worst:.3f}; "
          f"kappa g moves eps by {float(np.abs(cpu(out_pool) - cpu(eps)).max()):.2e}")
    assert (err <= gate).all(), worst
    assert float(np.abs(cpu(out_pool) - cpu(eps)).max()) > 1e3 * float(err.max())   # the agreement is not that of two zeros


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("augmented", [1, 0])
def test_sr_kernels_on_misaligned_buffers(ops, augmented, s):
    """A float32 buffer that starts 4 bytes past a 16-byte boundary sends the launch to the 4-byte form: the same values as
    the 16-byte form on aligned copies, bit for bit - each operand in turn."""
    kq, _ = _coeffs(augmented, seed=7)
    ct = 6 if augmented else 3
    u, eps = _rand(2, ct, 32, 32, seed=1).to(DEV), _rand(2, ct, 32, 32, seed=2).to(DEV)
    y, x = _rand(2, 3, 32 // s, 32 // s, seed=3).to(DEV), _rand(2, 3, 32, 32, seed=4).to(DEV)
    _, _, _, hhat, lam = _spectra("bicubic", s, 32, 32)
    off = lambda t: torch.zeros(t.numel() + 1, device=DEV, dtype=t.dtype)[1:].view(t.shape).copy_(t)
    assert off(y).data_ptr() % 16 == 4 and y.data_ptr() % 16 == 0
    g, cot = ops.restore_sr_measure(u, eps, y, hhat, lam, kq, 0.0025, R2, s)
    for which in ("u", "eps", "y"):
        g2, cot2 = ops.restore_sr_measure(off(u) if which == "u" else u, off(eps) if which == "eps" else eps,
                                          off(y) if which == "y" else y, hhat, lam, kq, 0.0025, R2, s)
        assert torch.equal(g2, g) and torch.equal(cot2, cot), which
    # the outputs: the C entry point on buffers of the test's own
    lib = ops.lib()
    for which in ("g", "cot"):
        g3, cot3 = torch.zeros_like(g), torch.zeros_like(cot)
        g3, cot3 = (off(g3), cot3) if which == "g" else (g3, off(cot3))
        assert lib.psld_restore_sr_f32(u.data_ptr(), eps.data_ptr(), y.data_ptr(), hhat.data_ptr(), lam.data_ptr(), ctypes.byref(kq),
                                       0.0025, R2, 2, 3, 32, 32, s, g3.data_ptr(), cot3.data_ptr(), None) == 0
        assert torch.equal(g3, g) and torch.equal(cot3, cot), which
    ax, atr = ops.restore_sr_apply(x, hhat, s), ops.restore_sr_apply(y, hhat, s, True)
    assert torch.equal(ops.restore_sr_apply(off(x), hhat, s), ax)
    assert torch.equal(ops.restore_sr_apply(x, hhat, s, False, off(torch.zeros_like(ax))), ax)
    assert torch.equal(ops.restore_sr_apply(off(y), hhat, s, True), atr)
    assert torch.equal(ops.restore_sr_apply(y, hhat, s, True, off(torch.zeros_like(atr))), atr)


def test_sr_kernels_refuse_bad_arguments(ops):
    """ValueError from the wrappers (RuntimeError for a dtype or a CPU tensor) and a status from the C entry points, on the
    host, before any launch: nothing here reaches the device."""
    kq, _ = _coeffs(1, seed=1)
    u, e = torch.ones(2, 6, 16, 16, device=DEV), torch.ones(2, 6, 16, 16, device=DEV)
    y = torch.ones(2, 3, 8, 8, device=DEV)
    hhat = torch.ones(16, 9, 2, device=DEV, dtype=torch.float64)
    lam = torch.ones(8, 5, device=DEV, dtype=torch.float64)
    sup = ops.restore_sr_supported
    assert [sup(h, w, s) for h, w, s in ((8, 8, 2), (16, 16, 4), (128, 128, 2), (128, 128, 4), (8, 64, 2), (32, 16, 4))] == [True] * 6
    assert [sup(h, w, s) for h, w, s in ((4, 8, 2), (8, 4, 2), (8, 16, 4), (16, 8, 4), (256, 8, 2), (12, 12, 2), (24, 24, 4),
                                         (9, 9, 3), (12, 12, 3), (16, 16, 3), (16, 16, 1), (16, 16, 8), (16, 16, 0), (16, 16, -2),
                                         (0, 16, 2), (-16, 16, 2))] == [False] * 16
    half = lambda t: t[:, :3].contiguous()
    measure = lambda *a: ops.restore_sr_measure(*a)
    with pytest.raises(ValueError, match="eps of shape"):
        measure(u, half(e), y, hhat, lam, kq, 0.01, R2, 2)
    for bad in ((2, 3, 16, 16), (2, 3, 4, 4), (2, 1, 8, 8), (1, 3, 8, 8), (2, 6, 8, 8)):      # a y of the wrong shape
        with pytest.raises(ValueError, match="measurement of shape"):
            measure(u, e, torch.ones(bad, device=DEV), hhat, lam, kq, 0.01, R2, 2)
    with pytest.raises(ValueError, match="measurement of shape"):
        measure(u, e, y, hhat, lam, kq, 0.01, R2, 4)                             # right for s = 2, not for 4
    with pytest.raises(ValueError, match="PSF spectrum of shape"):
        measure(u, e, y, hhat[:, :8].contiguous(), lam, kq, 0.01, R2, 2)
    with pytest.raises(ValueError, match="eigenvalues of shape"):
        measure(u, e, y, hhat, lam[:, :4].contiguous(), kq, 0.01, R2, 2)
    with pytest.raises(ValueError, match="even"):
        measure(half(u), half(e), y, hhat, lam, kq, 0.01, R2, 2)
    for s2, r2 in ((0.0, 0.0), (-0.01, R2), (float("nan"), R2), (0.01, float("inf"))):
        with pytest.raises(ValueError, match="positive sum"):
            measure(u, e, y, hhat, lam, kq, s2, r2, 2)
    with pytest.raises(RuntimeError, match="float32"):
        measure(u.double(), e, y, hhat, lam, kq, 0.01, R2, 2)
    with pytest.raises(RuntimeError, match="float64"):
        measure(u, e, y, hhat, lam.float(), kq, 0.01, R2, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        measure(u.cpu(), e.cpu(), y.cpu(), hhat.cpu(), lam.cpu(), kq, 0.01, R2, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.restore_sr_apply(y.cpu(), hhat, 2)
    # sizes: H/s < 4, no power of two, s = 3
    for bad, s in (((2, 6, 4, 8), 2), ((2, 6, 8, 16), 4), ((2, 6, 12, 12), 2), ((2, 6, 24, 24), 4), ((2, 6, 12, 12), 3),
                   ((2, 6, 256, 16), 2), ((2, 6, 16, 16), 8)):
        with pytest.raises(ValueError, match="power of two"):
            measure(torch.ones(bad, device=DEV), torch.ones(bad, device=DEV), y, hhat, lam, kq, 0.01, R2, s)
    with pytest.raises(ValueError, match="power of two"):
        ops.restore_sr_apply(torch.ones(2, 3, 12, 12, device=DEV), torch.ones(12, 7, 2, device=DEV, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="power of two"):
        ops.restore_sr_apply(torch.ones(2, 3, 16, 16, device=DEV), hhat, 3)
    with pytest.raises(ValueError, match="these planes need|this spectrum and factor need"):
        ops.restore_sr_apply(y, hhat, 2)                                       # low-resolution planes handed to A
    with pytest.raises(ValueError, match="this spectrum and factor need"):
        ops.restore_sr_apply(torch.ones(2, 3, 16, 16, device=DEV), hhat, 2, True)
    with pytest.raises(ValueError, match="out of shape"):
        ops.restore_sr_apply(torch.ones(2, 3, 16, 16, device=DEV), hhat, 2, False, torch.ones(2, 3, 16, 16, device=DEV))
    # an h^ that is not 16-byte aligned (the kernels read it as 16-byte complex numbers)
    shifted = torch.ones(16 * 9 * 2 + 1, device=DEV, dtype=torch.float64)[1:].view(16, 9, 2)
    assert shifted.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        measure(u, e, y, shifted, lam, kq, 0.01, R2, 2)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.restore_sr_apply(torch.ones(2, 3, 16, 16, device=DEV), shifted, 2)
    for aug in (2, -1):
        kq.augmented = aug
        with pytest.raises(ValueError, match="augmented"):
            measure(u, e, y, hhat, lam, kq, 0.01, R2, 2)
    kq.augmented = 1
    # the C entry points check on their own
    lib = ops.lib()
    p = lambda t: t.data_ptr()
    g, cot = torch.ones(2, 3, 16, 16, device=DEV), torch.ones_like(u)
    call = lambda *a: lib.psld_restore_sr_f32(*a)
    ok = [p(u), p(e), p(y), p(hhat), p(lam), ctypes.byref(kq), 0.01, R2, 2, 3, 16, 16, 2, p(g), p(cot), None]
    for i in (0, 1, 2, 3, 4, 5, 13, 14):                                        # each null pointer in turn
        args = list(ok)
        args[i] = None
        assert call(*args) != 0 and b"psld_restore_sr_f32" in lib.psld_last_error()
    for i, v, what in ((10, 12, b"power of two"), (11, 24, b"power of two"), (10, 4, b"power of two"), (11, 256, b"power of two"),
                       (10, 0, b"power of two"), (12, 3, b"power of two"), (12, 8, b"power of two"), (12, 0, b"power of two"),
                       (8, 0, b"bad args"), (8, -2, b"bad args"), (9, 0, b"bad args"), (6, -1.0, b"sigma_y"),
                       (7, float("inf"), b"sigma_y"), (6, float("nan"), b"sigma_y"), (3, p(hhat) + 8, b"aligned"),
                       (4, p(lam) + 4, b"aligned")):
        args = list(ok)
        args[i] = v
        assert call(*args) != 0 and what in lib.psld_last_error(), (i, v, lib.psld_last_error())
    kq.augmented = 3
    assert call(*ok) != 0 and b"augmented" in lib.psld_last_error()
    kq.augmented = 1
    x = torch.ones(2, 3, 16, 16, device=DEV)
    apply = lambda *a: lib.psld_restore_sr_apply_f32(*a)
    assert apply(None, p(hhat), 0, 6, 16, 16, 2, p(y), None) != 0
    assert apply(p(x), None, 0, 6, 16, 16, 2, p(y), None) != 0
    assert apply(p(x), p(hhat), 0, 6, 16, 16, 2, None, None) != 0
    assert apply(p(x), p(hhat), 2, 6, 16, 16, 2, p(y), None) != 0 and b"adjoint" in lib.psld_last_error()
    assert apply(p(x), p(hhat), 0, -1, 16, 16, 2, p(y), None) != 0
    assert apply(p(x), p(hhat), 0, 6, 16, 16, 3, p(y), None) != 0 and b"power of two" in lib.psld_last_error()
    assert apply(p(x), p(hhat), 0, 6, 16, 8, 4, p(y), None) != 0 and b"power of two" in lib.psld_last_error()
    assert apply(p(x), p(hhat) + 8, 0, 6, 16, 16, 2, p(y), None) != 0 and b"aligned" in lib.psld_last_error()
    # the old measure entry point and the shape rule keep refusing operator code 3
    with pytest.raises(ValueError, match="operator code"):
        ops.restore_measurement_shape((2, 6, 8, 8), 3, 1, 1)
    assert lib.psld_restore_measure_f32(p(u), p(e), p(x), None, 3, 1, ctypes.byref(kq), 2, 3, 16, 16, p(g), p(cot), None) != 0
    assert b"operator code" in lib.psld_last_error()
    assert lib.psld_version() == 14
    torch.cuda.synchronize()
    for t in (u, e, y, x, g, cot, hhat, lam):
        assert bool((t == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# PosteriorScoreFn on the tiny networks against oracle + autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,spec", [("sr2", None), ("sr4", None), ("sr2", "gauss:1.5"), ("sr4", "block")])
@pytest.mark.parametrize("name", ["psld", "vpsde"])
def test_posterior_score_fn_against_the_oracle(name, task, spec):
    """eps' of one guided call against the CPU oracle network, torch autograd for J^T w and tests/sr_ref.py around it (its own
    coefficients and its own kernel): rel-L2 <= 1e-4, the project's gate."""
    from psld_amd.guidance import PosteriorScoreFn
    net, cfg, sd = _net(name)
    vp = name == "vpsde"
    s = int(task[2])
    sigma_y, scale, v0, t = 0.1, 1.3, 0.5, float(np.float32(0.4))
    x, y = _rand(2, 3 if vp else 6, 16, 16, seed=21), _rand(2, 3, 16 // s, 16 // s, seed=23)
    fn = PosteriorScoreFn(net, _sde(cfg), task, sigma_y, scale, v0, psf=spec)
    fn.set_measurement(y.to(DEV))
    with torch.no_grad():
        got = fn(x.to(DEV), torch.full((2,), t, device=DEV))
        plain = net(x.to(DEV), torch.full((2,), t, device=DEV))
    q = _ref_coeffs(cfg, t, sigma_y, scale, v0)
    xr = x.clone().requires_grad_()
    eps = O.ncsnpp_forward(sd, cfg, xr, torch.full((2,), t))
    c64 = lambda v: v.detach().double().numpy()
    g, w, _, _ = Q.measure(c64(x), c64(eps), c64(y), Q.kernel(spec or "bicubic", s, 16, 16), s, q, sigma_y ** 2, q.r2)
    (dx,) = torch.autograd.grad(eps, xr, grad_outputs=torch.from_numpy(w).to(eps.dtype))
    want = torch.from_numpy(F.combine(c64(eps), g, c64(dx), q)[0])
    err, moved = rel_l2(got, want), rel_l2(plain, want)
    print(f"PosteriorScoreFn {name} {task} {spec}: rel-L2 vs oracle + autograd = {err:.3e} (the guidance moves eps by {moved:.2e})")
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert err <= 1e-4
    assert moved > 10 * 1e-4


def test_scale_zero_is_the_plain_forward(ops, monkeypatch):
    """torch.equal to net(x, t), no measurement needed, and no kernel of the guidance is launched; scale != 0 launches the
    sr measure and the combine once each and nothing else of the guidance."""
    from psld_amd.guidance import PosteriorScoreFn
    net, cfg, _ = _net("psld")
    x, t = _rand(2, 6, 16, 16, seed=31).to(DEV), torch.full((2,), 0.4, device=DEV)
    calls = []
    for name in ("restore_sr_measure", "restore_sr_apply", "restore_combine", "restore_measure", "restore_deconv_measure",
                 "restore_deconv_spectrum", "restore_deconv_apply"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=getattr(ops, name), **kw: (calls.append(_n), _f(*a, **kw))[1])
    with torch.no_grad():
        want = net(x, t)
        off = PosteriorScoreFn(net, _sde(cfg), "sr4", 0.1, scale=0.0)
        assert torch.equal(off(x, t), want) and calls == []
        off.set_measurement(_rand(2, 3, 4, 4, seed=32).to(DEV))
        assert torch.equal(off(x, t), want) and calls == []
        fn = PosteriorScoreFn(net, _sde(cfg), "sr4", 0.1).set_measurement(_rand(2, 3, 4, 4, seed=32).to(DEV))
        first = fn(x, t)
        assert not torch.equal(first, want) and calls == ["restore_sr_measure", "restore_combine"]
        del calls[:]
        assert torch.equal(fn(x, t), first) and calls == ["restore_sr_measure", "restore_combine"]
        for bad in ((2, 3, 8, 8), (2, 3, 16, 16), (2, 1, 4, 4)):                  # sr2's shape, the image's, one channel
            fn.set_measurement(_rand(*bad, seed=33).to(DEV))
            with pytest.raises(ValueError, match="measurement of shape"):
                fn(x, t)
        # an image too small for the factor: 8 / 4 < 4
        fn.set_measurement(_rand(2, 3, 2, 2, seed=34).to(DEV))
        with pytest.raises(ValueError, match="powers of two from 16 to 128"):
            fn(_rand(2, 6, 8, 8, seed=35).to(DEV), t)


# ---------------------------------------------------------------------------------------------------------------------
# guided sampler runs with the analytic Gaussian eps against the CPU float64 loops fed the same noise
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_eps(gauss, u, t, y, k, s, sigma_y, scale):
    """tests/test_restore_gpu._cpu_eps for the super-resolution operator: what the device computes, in float64 with its
    float32 roundings."""
    u32, t32 = _f32(u), float(np.float32(t))
    e = _f32(gauss.eps(u32, t32))
    if scale == 0.0:
        return e
    q = gauss.coeffs(t32, sigma_y, scale)
    g, w, _, _ = Q.measure(u32, e, y, k, s, q, sigma_y ** 2, q.r2)
    return _f32(F.combine(e, _f32(g), _f32(gauss.vjp(_f32(w), t32)), q)[0])


def _cpu_run(sampler, cfg, gauss, batch, ts, y, k, s, sigma_y, scale):
    eps_nchw = lambda u, t: _cpu_eps(gauss, u, t, y, k, s, sigma_y, scale)
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


@pytest.mark.parametrize("sampler,spec", [("ei_sde", "bicubic"), ("em_sde", "gauss:1.0"), ("ei_ode", "block")])
def test_guided_sampler_runs(sampler, spec):
    """6 quadratic steps on [4, 6, 8, 8] with seeded noise (ei_sde at lam = 1, em_sde, ei_ode at order 2) under
    PosteriorScoreFn(..., "sr2") around the analytic Gaussian eps (the torch-autograd path), against the CPU float64 loop of
    the same sampler fed the same noise: 1e-4 rel-L2, and the guidance moves the result by more than 10x that."""
    import psld_amd
    from psld_amd.guidance import PosteriorScoreFn
    from psld_amd.registry import get_module
    from psld_amd.sde import PSLD
    psld_amd.import_modules_into_registry()
    cfg = copy.deepcopy(C.yaml_default())
    cfg.evaluation.sampler = C.Config({"name": sampler, "lam": 1.0, "order": 2})
    sde, gauss = PSLD(cfg), F.GaussPSLD(R.RefPSLD.from_config(cfg), 0.25)
    sigma_y, n, s = 0.1, 6, 2
    ts = R.grid(n, "quadratic")
    gen = torch.Generator().manual_seed(77)
    batch = torch.randn(4, 6, 8, 8, generator=gen, dtype=torch.float64)
    batch[:, 3:] *= np.sqrt(gauss.ref.m)
    x0 = 0.5 * torch.randn(4, 3, 8, 8, generator=gen, dtype=torch.float64)
    k = Q.kernel(spec, s, 8, 8)
    y = _f32(Q.forward(x0.numpy(), k, s) + sigma_y * torch.randn(4, 3, 4, 4, generator=gen, dtype=torch.float64).numpy())
    fn = PosteriorScoreFn(_GaussScore(gauss), sde, "sr2", sigma_y, prior_var=0.25, psf=spec)
    fn.set_measurement(torch.from_numpy(y).to(DEV))
    smp = get_module("samplers", sampler)(cfg, sde, fn)
    smp.noise_fn = _seeded_noise
    x = smp.sample(batch.to(DEV), torch.from_numpy(ts).to(DEV), n, denoise=False)
    assert x.dtype == torch.float64 and x.shape == (4, 6, 8, 8) and fn.net.calls == n
    want = torch.from_numpy(_cpu_run(sampler, cfg, gauss, batch, ts, y, k, s, sigma_y, 1.0))
    free = torch.from_numpy(_cpu_run(sampler, cfg, gauss, batch, ts, y, k, s, sigma_y, 0.0))
    err, moved = rel_l2(x, want), rel_l2(free, want)
    print(f"guided {sampler} (sr2 {spec}), 6 quadratic steps: rel-L2 vs the CPU loop = {err:.3e}; guidance moves the result by {moved:.2e}")
    assert err < 1e-4
    assert moved > 10 * err and moved > 10 * 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_restore_sr(tmp_path):
    from psld_amd import cli
    out = str(tmp_path / "sr")
    base = ["restore", "--config", "tiny", "--task", "sr4", "--sigma-y", "0.05", "evaluation.n_samples=2",
            "evaluation.batch_size=2", "evaluation.n_discrete_steps=3", "evaluation.stride_type=quadratic",
            "evaluation.sampler.name=ei_sde", "evaluation.save_mode=np", "--synthetic-size", "4", f"evaluation.save_path={out}"]
    torch.manual_seed(5)                                                    # no checkpoint: the command draws its weights
    cli.main(base)                                                           # no --psf: bicubic
    assert sorted(os.listdir(out)) == ["batch", "corrupt", "images"]
    arrays = {}
    for d in ("batch", "corrupt", "images"):
        assert os.listdir(os.path.join(out, d)) == ["output_gpu_0_0.npy"]
        a = arrays[d] = np.load(os.path.join(out, d, "output_gpu_0_0.npy"))
        assert a.dtype == np.uint8 and a.shape == (2, 16, 16, 3), d
    assert not np.array_equal(arrays["corrupt"], arrays["batch"])
    blocks = arrays["corrupt"].reshape(2, 4, 4, 4, 4, 3)                      # the 4 x 4 measurement replicated 4 x 4
    assert (blocks == blocks[:, :, :1, :, :1]).all()
    with pytest.raises(SystemExit, match="PSF"):
        cli.main([a if a != "sr4" else "gray" for a in base] + ["--psf", "bicubic"])
    with pytest.raises(SystemExit, match="odd"):
        cli.main(base + ["--psf", "box:4"])
    with pytest.raises(SystemExit, match="larger"):
        cli.main(base + ["--psf", "box:17"])


def test_worst_ratios_are_recorded():
    """Runs last: the worst error / bound of the kernel tests of this session (recorded in profiles/r21/sr.md)."""
    print("sr kernels, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())

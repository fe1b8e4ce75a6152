"""Float64 reference of the super-resolution operator of measurement-guided sampling (a helper module of
tests/test_sr_cpu.py and tests/test_sr_gpu.py), on top of tests/restore_ref.py and tests/deconv_ref.py.

Written from the formulas of DESIGN section 13, "Super-resolution" with ``numpy.fft``, independently of ``psld_amd`` (which it
does not import).  ``A x = D_s (k (*) x)`` per channel: a periodic blur, then the samples ``(s i, s j)``; images ``[B, C, H, W]``,
measurements ``[B, C, H/s, W/s]``.

  * ``cubic`` / ``taps`` / ``kernel``: the kernels on the H x W torus as CONVOLUTION kernels (``bicubic`` and ``block`` are given
    as correlations ``y[i] = sum_o w[o] x[s i + o]``, so ``k[-o] = w[o]``; the rest is ``deconv_ref.psf``);
  * ``dense``: the matrix of A over one plane, from the definition (no transform);
  * ``forward`` / ``adjoint``: A x and A^T r through the full complex transform;
  * ``lam``: the eigenvalues of A A^T on the low-resolution grid, the alias sum of |h^|^2;
  * ``measure``: what the measure kernel computes, g = (s2 + r2) A^T (s2 I + r2 A A^T)^-1 (y - A x0^) and the cotangent, with
    the magnitudes the error bound of tests/test_sr_gpu.py needs;
  * ``operator_matrix``: A over one image (for ``restore_ref.exact_guided_eps``); ``guided_eps``: the guided eps of Gaussian
    data through measure / combine.
"""
from __future__ import annotations

import numpy as np

from tests import deconv_ref as D
from tests import restore_ref as F


def cubic(x: float) -> float:
    """Keys' cubic convolution kernel with a = -0.5."""
    x, a = abs(float(x)), -0.5
    if x <= 1.0:
        return (a + 2.0) * x ** 3 - (a + 3.0) * x ** 2 + 1.0
    if x < 2.0:
        return a * x ** 3 - 5.0 * a * x ** 2 + 8.0 * a * x - 4.0 * a
    return 0.0


def taps(spec: str, s: int):
    """(offsets, weights) of one axis of ``bicubic`` (4 s taps at -3 s / 2 .. 5 s / 2 - 1, cubic((o - (s - 1) / 2) / s),
    normalised) or ``block`` (s taps 1 / s at 0 .. s - 1): y[i] = sum_o w[o] x[s i + o]."""
    if spec == "block":
        return list(range(s)), [1.0 / s] * s
    assert spec == "bicubic"
    offs = list(range(-3 * s // 2, 5 * s // 2))
    wts = [cubic((o - (s - 1) / 2.0) / s) for o in offs]
    total = sum(wts)
    return offs, [v / total for v in wts]


def kernel(spec, s: int, h: int, w: int) -> np.ndarray:
    """float64 [h, w]: the convolution kernel k with A x = D_s (k (*) x)."""
    if isinstance(spec, str) and spec in ("bicubic", "block"):
        offs, wts = taps(spec, s)
        k = np.zeros((h, w))
        for oi, wi in zip(offs, wts):
            for oj, wj in zip(offs, wts):
                k[(-oi) % h, (-oj) % w] += wi * wj
        return k
    return D.psf(spec, h, w)


def dense(k: np.ndarray, s: int) -> np.ndarray:
    """A [h/s * w/s, h * w] of one plane from the definition: (A x)[i, j] = sum_n k[n] x[s i - n1, s j - n2]."""
    h, w = k.shape
    a = np.zeros((h // s, w // s, h, w))
    for i in range(h // s):
        for j in range(w // s):
            for n1 in range(h):
                for n2 in range(w):
                    a[i, j, (s * i - n1) % h, (s * j - n2) % w] += k[n1, n2]
    return a.reshape(h // s * (w // s), h * w)


def forward(x: np.ndarray, k: np.ndarray, s: int, hh=None) -> np.ndarray:
    hh = np.fft.fft2(k) if hh is None else hh
    return np.real(np.fft.ifft2(hh * np.fft.fft2(np.asarray(x, float))))[..., ::s, ::s]


def adjoint(r: np.ndarray, k: np.ndarray, s: int, hh=None) -> np.ndarray:
    hh = np.fft.fft2(k) if hh is None else hh
    r = np.asarray(r, float)
    up = np.zeros(r.shape[:-2] + (r.shape[-2] * s, r.shape[-1] * s))
    up[..., ::s, ::s] = r
    return np.real(np.fft.ifft2(np.conj(hh) * np.fft.fft2(up)))


def lam(hh: np.ndarray, s: int) -> np.ndarray:
    """Lambda [h/s, w/s] from the full spectrum h^ [h, w]: (1 / s^2) sum_{a, b < s} |h^[m1 + a h/s, m2 + b w/s]|^2."""
    h, w = hh.shape
    hl, wl = h // s, w // s
    out = np.zeros((hl, wl))
    for a in range(s):
        for b in range(s):
            out += np.abs(hh[a * hl:(a + 1) * hl, b * wl:(b + 1) * wl]) ** 2
    return out / s ** 2


def solve_weight(lm: np.ndarray, s2: float, r2: float) -> np.ndarray:
    """(s2 + r2) / (s2 + r2 Lambda), 0 where the denominator is exactly 0."""
    den = s2 + r2 * lm
    return np.where(den == 0.0, 0.0, (s2 + r2) / np.where(den == 0.0, 1.0, den))


def symmetric(half_lam: np.ndarray, wl: int) -> np.ndarray:
    """The full Lambda [h/s, w/s] that the half ``[:, :wl/2 + 1]`` stands for: Lambda[-m] = Lambda[m], bit for bit."""
    hl = half_lam.shape[0]
    full = np.zeros((hl, wl))
    full[:, :wl // 2 + 1] = half_lam
    rows = (-np.arange(hl)) % hl
    for m2 in range(wl // 2 + 1, wl):
        full[:, m2] = half_lam[rows, wl - m2]
    return full


def measure(u, eps, y, k: np.ndarray, s: int, q: F.Coeffs, s2: float, r2: float, hh=None, lm=None):
    """(g, w, mag_g, mag_w).  ``hh`` / ``lm``: the full spectrum [H, W] and the full Lambda [H/s, W/s] to use instead of the
    computed ones (they are INPUTS of the kernels: a test hands both sides the same bits).  mag_g, one number per plane: the
    T of the error bound of tests/test_sr_gpu.py (derived there).  A transform pair's rounding is proportional to the bound on
    its output values, mean|filter| times the sum of the magnitudes of ITS inputs, and reaches g through the later pairs,
    which are convolutions with the spatial kernels kf = IFFT2'(f) and k: amplified by at most their l1 norms.  So
        T1 = mean|h^| sum mag(x0^),   T2 = mean|f| sum|rho|,   T3 = mean|h^| sum|v|,
        T  = max(T3, |k|_1 T2, |k|_1 |kf|_1 T1)."""
    x0, mag0 = F.x0_hat(np.asarray(u, float), np.asarray(eps, float), q)
    y = np.asarray(y, float)
    hh = np.fft.fft2(k) if hh is None else np.asarray(hh)
    lm = lam(hh, s) if lm is None else np.asarray(lm)
    f = solve_weight(lm, s2, r2)
    rho = y - forward(x0, k, s, hh)
    v = np.real(np.fft.ifft2(f * np.fft.fft2(rho)))
    g = adjoint(v, k, s, hh)
    plane = lambda a: np.abs(a).sum(axis=(2, 3), keepdims=True)
    mh, k1, kf1 = np.abs(hh).mean(), np.abs(np.real(np.fft.ifft2(hh))).sum(), np.abs(np.real(np.fft.ifft2(f))).sum()
    t1, t2, t3 = mh * mag0.sum(axis=(2, 3), keepdims=True), np.abs(f).mean() * plane(rho), mh * plane(v)
    mag = np.maximum(t3, np.maximum(k1 * t2, k1 * kf1 * t1)) * np.ones_like(g)
    if q.augmented:
        return (g, np.concatenate([q.q_e[0] * g, q.q_e[1] * g], axis=1), mag,
                np.concatenate([abs(q.q_e[0]) * mag, abs(q.q_e[1]) * mag], axis=1))
    return g, q.q_e[0] * g, mag, abs(q.q_e[0]) * mag


def operator_matrix(image_shape, k: np.ndarray, s: int) -> np.ndarray:
    """The dense matrix [n / s^2, n] of A over one image (batch 1) from ``forward`` of the unit images."""
    n = int(np.prod(image_shape))
    return np.stack([forward(e.reshape(image_shape), k, s).reshape(-1) for e in np.eye(n)], axis=1)


def guided_eps(gauss, u, t: float, y, k: np.ndarray, s: int, sigma_y: float, scale: float = 1.0):
    """The guided eps of Gaussian data through measure / ``restore_ref.combine`` with the closed-form Jacobian."""
    q = gauss.coeffs(t, sigma_y, scale)
    e = gauss.eps(u, t)
    g, w, _, _ = measure(u, e, y, k, s, q, sigma_y ** 2, q.r2)
    return F.combine(e, g, gauss.vjp(w, t), q)[0]

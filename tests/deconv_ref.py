"""Float64 reference of the deconv operator of measurement-guided sampling (a helper module of tests/test_deconv_cpu.py and
tests/test_deconv_gpu.py), on top of tests/restore_ref.py.

Written from the formulas of DESIGN section 13, "Deconvolution" with ``numpy.fft``, independently of ``psld_amd`` (which it
does not import).  ``A x = k (*) x`` per channel with a periodic boundary, the same PSF for every image and channel; images ``[B, C, H, W]``.

  * ``psf``: the PSF specifications on the H x W torus, middle tap at [0, 0];
  * ``forward`` / ``adjoint``: A x and A^T r through the full complex transform;
  * ``measure``: what the measure kernel computes, g = (s2 + r2) A^T (s2 I + r2 A A^T)^-1 (y - A x0^) and the cotangent, with
    the magnitudes the error bound of tests/test_deconv_gpu.py needs;
  * ``operator_matrix``: the dense circulant matrix of one small image (for ``restore_ref.exact_guided_eps``);
  * ``guided_eps``: the guided eps of Gaussian data through measure / combine.
"""
from __future__ import annotations

import numpy as np

from tests import restore_ref as F


def psf(spec, h: int, w: int) -> np.ndarray:
    """float64 [h, w]: ``gauss:S`` exp(-d^2 / 2 S^2) of the wrapped distance, normalised; ``box:K`` K x K uniform; ``motion:L``
    1 x L horizontal uniform; an array [kh, kw] (odd sizes) as given - each wrapped so that its middle tap is at [0, 0]."""
    if isinstance(spec, str):
        kind, arg = spec.split(":")
        if kind == "gauss":
            s = float(arg)
            k = np.zeros((h, w))
            for i in range(h):
                for j in range(w):
                    k[i, j] = np.exp(-(min(i, h - i) ** 2 + min(j, w - j) ** 2) / (2.0 * s * s))
            return k / k.sum()
        n = int(arg)
        taps = np.full((n, n), 1.0 / n ** 2) if kind == "box" else np.full((1, n), 1.0 / n)
    else:
        taps = np.asarray(spec, float)
    kh, kw = taps.shape
    assert kh % 2 == 1 and kw % 2 == 1 and kh <= h and kw <= w
    k = np.zeros((h, w))
    for i in range(kh):
        for j in range(kw):
            k[(i - kh // 2) % h, (j - kw // 2) % w] += taps[i, j]
    return k


def forward(x: np.ndarray, k: np.ndarray) -> np.ndarray:
    """(A x)[n] = sum_m k[m] x[n - m] over the torus, per plane."""
    return np.real(np.fft.ifft2(np.fft.fft2(k) * np.fft.fft2(np.asarray(x, float))))


def adjoint(r: np.ndarray, k: np.ndarray) -> np.ndarray:
    return np.real(np.fft.ifft2(np.conj(np.fft.fft2(k)) * np.fft.fft2(np.asarray(r, float))))


def weight(k: np.ndarray, s2: float, r2: float, hh=None):
    """(h^, m^): m^ = conj(h^) (s2 + r2) / (s2 + r2 |h^|^2), 0 where the denominator is exactly 0.  ``hh``: the full spectrum
    [H, W] to use instead of FFT2(k) (the kernels take h^ as an input: a test hands both sides the same bits)."""
    hh = np.fft.fft2(k) if hh is None else np.asarray(hh)
    den = s2 + r2 * np.abs(hh) ** 2
    safe = np.where(den == 0.0, 1.0, den)
    return hh, np.where(den == 0.0, 0.0, np.conj(hh) * (s2 + r2) / safe)


def half(spec: np.ndarray) -> np.ndarray:
    """The Hermitian half [..., H, W/2 + 1] of a full spectrum as float64 [..., H, W/2 + 1, 2], the kernels' layout."""
    hs = spec[..., :spec.shape[-1] // 2 + 1]
    return np.ascontiguousarray(np.stack([hs.real, hs.imag], axis=-1))


def hermitian(spec: np.ndarray) -> np.ndarray:
    """The full spectrum [H, W] that the half ``spec[:, :W/2 + 1]`` stands for: column k2 > W/2 is the conjugate of column
    W - k2 at row -k1, bit for bit (a computed FFT2 of a real plane has that symmetry only up to rounding)."""
    h, w = spec.shape
    full = np.array(spec, dtype=np.complex128)
    rows = (-np.arange(h)) % h
    for k2 in range(w // 2 + 1, w):
        full[:, k2] = np.conj(spec[rows, w - k2])
    return full


def measure(u, eps, y, k: np.ndarray, q: F.Coeffs, s2: float, r2: float, hh=None):
    """(g, w, mag_g, mag_w): g = IFFT2(m^ (y^ - h^ FFT2(x0^))), w = (q_e[0] g | q_e[1] g).  mag_g, one number per plane and
    the same for each of its elements: (1 / HW) sum_omega |m^| (sum|y| + |h^| sum mag(x0^)) - every value that flows through
    the transforms is bounded by the sum of the magnitudes of the plane it comes from, times the weights it meets."""
    x0, mag0 = F.x0_hat(np.asarray(u, float), np.asarray(eps, float), q)
    y = np.asarray(y, float)
    hh, mm = weight(k, s2, r2, hh)
    g = np.real(np.fft.ifft2(mm * (np.fft.fft2(y) - hh * np.fft.fft2(x0))))
    sy, sx = np.abs(y).sum(axis=(2, 3), keepdims=True), mag0.sum(axis=(2, 3), keepdims=True)
    mag = (np.abs(mm)[None, None] * (sy + np.abs(hh)[None, None] * sx)).mean(axis=(2, 3), keepdims=True) * np.ones_like(g)
    if q.augmented:
        return (g, np.concatenate([q.q_e[0] * g, q.q_e[1] * g], axis=1), mag,
                np.concatenate([abs(q.q_e[0]) * mag, abs(q.q_e[1]) * mag], axis=1))
    return g, q.q_e[0] * g, mag, abs(q.q_e[0]) * mag


def operator_matrix(image_shape, k: np.ndarray) -> np.ndarray:
    """The dense matrix [n, n] of A over one image (batch 1) from ``forward`` of the unit images."""
    n = int(np.prod(image_shape))
    return np.stack([forward(e.reshape(image_shape), k).reshape(-1) for e in np.eye(n)], axis=1)


def guided_eps(gauss, u, t: float, y, k: np.ndarray, sigma_y: float, scale: float = 1.0):
    """The guided eps of Gaussian data through measure / ``restore_ref.combine`` with the closed-form Jacobian."""
    q = gauss.coeffs(t, sigma_y, scale)
    e = gauss.eps(u, t)
    g, w, _, _ = measure(u, e, y, k, q, sigma_y ** 2, q.r2)
    return F.combine(e, g, gauss.vjp(w, t), q)[0]

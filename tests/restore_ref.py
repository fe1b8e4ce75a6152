"""Float64 reference of measurement-guided (posterior) sampling (a helper module of tests/test_restore_cpu.py and
tests/test_restore_gpu.py).

Written from the formulas of DESIGN section 13 on top of tests/ei_ref.py (the SDEs' scalars), independently of
``psld_amd.guidance`` (which it does not import).  NumPy float64 throughout; images are ``[B, C, H, W]``, PSLD states
``[B, 2C, H, W] = [x | m]``, VP-SDE states ``[B, C, H, W]``.

  * coefficients: ``psld_coeffs`` / ``vp_coeffs`` -> ``Coeffs`` (q_u, q_e, l, kappa, and a, r2 for the tests);
  * the three operators with their transposes (``forward`` / ``adjoint``), each with orthonormal rows;
  * ``measure`` / ``combine``: what the two kernels compute, with the sum of the magnitudes of the terms for the bounds;
  * Gaussian data ``x0 ~ N(0, v0)`` per pixel: its eps and Jacobian in closed form (``GaussPSLD`` / ``GaussVP``), the guided
    eps built from measure / combine, and the exact posterior ``u_t | y`` by dense linear algebra on tiny images.
"""
from __future__ import annotations

import math

import numpy as np

from tests import ei_ref as R

TASKS = {"mask": ("mask", 1), "gray": ("gray", 1), "pool2": ("pool", 2), "pool4": ("pool", 4)}


class Coeffs:
    """q_u [2], q_e [2], l = (l11, l21, l22) (VP: entry 0 of each, l[0] = sigma), kappa; a = mean of u_t for x0 = 1 (VP:
    alpha), r2 = Var(x0 | u_t) under the N(0, v0) pixel prior."""

    def __init__(self, q_u, q_e, l, kappa, augmented, a, r2):
        self.q_u, self.q_e, self.l = np.asarray(q_u, float), np.asarray(q_e, float), np.asarray(l, float)
        self.kappa, self.augmented, self.a, self.r2 = float(kappa), bool(augmented), np.asarray(a, float), float(r2)


def psld_mean_vector(ref: R.RefPSLD, t: float) -> np.ndarray:
    """a_t: the mean of u_t for x0 = 1, m0 = 0 (first column of the flow from time 0)."""
    return ref.flow(t, 0.0) @ np.array([1.0, 0.0])


def psld_coeffs(ref: R.RefPSLD, t: float, sigma_y: float, scale: float = 1.0, v0: float = 1.0) -> Coeffs:
    a, l, sig = psld_mean_vector(ref, t), ref.chol(t), ref.sigma(t)
    p = a / (a @ a)
    r2 = 1.0 / (1.0 / v0 + a @ np.linalg.solve(sig, a))
    q_e = l.T @ p                                            # x0^ = p . (u - L eps) = p . u - (L^T p) . eps
    return Coeffs(p, q_e, [l[0, 0], l[1, 0], l[1, 1]], scale / (sigma_y ** 2 + r2), True, a, r2)


def vp_coeffs(ref: R.RefVP, t: float, sigma_y: float, scale: float = 1.0, v0: float = 1.0) -> Coeffs:
    alpha, sigma = math.exp(ref.log_alpha(t)), ref.sigma(t)
    r2 = v0 * sigma ** 2 / (sigma ** 2 + v0 * alpha ** 2)
    return Coeffs([1.0 / alpha, 0.0], [sigma / alpha, 0.0], [sigma, 0.0, 0.0], scale / (sigma_y ** 2 + r2), False,
                  [alpha, 0.0], r2)


# ---- operators -----------------------------------------------------------------------------------------------------------
def forward(x: np.ndarray, task: str, mask=None) -> np.ndarray:
    kind, k = TASKS[task]
    if kind == "mask":
        return mask * x
    if kind == "gray":
        assert x.shape[1] == 3
        return x.sum(axis=1, keepdims=True) / math.sqrt(3.0)
    b, c, h, w = x.shape
    assert h % k == 0 and w % k == 0
    return x.reshape(b, c, h // k, k, w // k, k).sum(axis=(3, 5)) / k


def adjoint(r: np.ndarray, task: str, mask=None) -> np.ndarray:
    kind, k = TASKS[task]
    if kind == "mask":
        return mask * r
    if kind == "gray":
        return np.repeat(r, 3, axis=1) / math.sqrt(3.0)
    return np.repeat(np.repeat(r, k, axis=2), k, axis=3) / k


def measurement_shape(image_shape, task: str):
    b, c, h, w = image_shape
    kind, k = TASKS[task]
    return {"mask": (b, c, h, w), "gray": (b, 1, h, w), "pool": (b, c, h // k, w // k)}[kind]


def split(u: np.ndarray, augmented: bool):
    if not augmented:
        return u, None
    c = u.shape[1] // 2
    return u[:, :c], u[:, c:]


# ---- the two kernels --------------------------------------------------------------------------------------------------------
def x0_hat(u, eps, q: Coeffs):
    """(x0^, sum of the magnitudes of its terms)."""
    ux, um = split(u, q.augmented)
    ex, em = split(eps, q.augmented)
    terms = [q.q_u[0] * ux, -q.q_e[0] * ex]
    if q.augmented:
        terms = [q.q_u[0] * ux, q.q_u[1] * um, -q.q_e[0] * ex, -q.q_e[1] * em]
    return sum(terms), sum(np.abs(v) for v in terms)


def measure(u, eps, y, mask, task: str, q: Coeffs):
    """(g, w, mag_g, mag_w): g = A^T (y - A x0^), w = (q_e[0] g | q_e[1] g); mag_*: the sums of the magnitudes of the terms
    each element of g / w is built from (|A^T| (|y| + |A| mag_x0), then times |q_e|)."""
    x0, mag0 = x0_hat(np.asarray(u, float), np.asarray(eps, float), q)
    y = np.asarray(y, float)
    mask = None if mask is None else np.asarray(mask, float)
    g = adjoint(y - forward(x0, task, mask), task, mask)
    mag = adjoint(np.abs(y) + forward(mag0, task, mask), task, mask)
    if q.augmented:
        return (g, np.concatenate([q.q_e[0] * g, q.q_e[1] * g], axis=1), mag,
                np.concatenate([abs(q.q_e[0]) * mag, abs(q.q_e[1]) * mag], axis=1))
    return g, q.q_e[0] * g, mag, abs(q.q_e[0]) * mag


def combine(eps, g, dx, q: Coeffs):
    """(eps', mag): eps' = eps - kappa (q_e g - L^T dx)."""
    eps, g, dx = np.asarray(eps, float), np.asarray(g, float), np.asarray(dx, float)
    if not q.augmented:
        terms = [eps, -q.kappa * q.q_e[0] * g, q.kappa * q.l[0] * dx]
        return sum(terms), sum(np.abs(v) for v in terms)
    ex, em = split(eps, True)
    dxx, dxm = split(dx, True)
    tx = [ex, -q.kappa * q.q_e[0] * g, q.kappa * q.l[0] * dxx, q.kappa * q.l[1] * dxm]
    tm = [em, -q.kappa * q.q_e[1] * g, q.kappa * q.l[2] * dxm]
    return (np.concatenate([sum(tx), sum(tm)], axis=1),
            np.concatenate([sum(np.abs(v) for v in tx), sum(np.abs(v) for v in tm)], axis=1))


# ---- Gaussian data: x0 ~ N(0, v0) per pixel (PSLD: m0 ~ N(0, kappa M)) ---------------------------------------------------------
class GaussPSLD:
    """eps = J u per pixel pair with J = L^T C^-1, C = v0 a a^T + Sigma_t the covariance of u_t: -L^T times the exact score."""
    augmented = True

    def __init__(self, ref: R.RefPSLD, v0: float):
        self.ref, self.v0 = ref, float(v0)

    def coeffs(self, t, sigma_y, scale=1.0):
        return psld_coeffs(self.ref, t, sigma_y, scale, self.v0)

    def jac(self, t: float) -> np.ndarray:
        a = psld_mean_vector(self.ref, t)
        return self.ref.chol(t).T @ np.linalg.inv(self.v0 * np.outer(a, a) + self.ref.sigma(t))

    def eps(self, u, t):
        j = self.jac(t)
        x, m = split(u, True)
        return np.concatenate([j[0, 0] * x + j[0, 1] * m, j[1, 0] * x + j[1, 1] * m], axis=1)

    def vjp(self, w, t):
        j = self.jac(t)
        wx, wm = split(w, True)
        return np.concatenate([j[0, 0] * wx + j[1, 0] * wm, j[0, 1] * wx + j[1, 1] * wm], axis=1)

    def pixel(self, t):
        """(a [2], Sigma [2, 2], L^T [2, 2]) of the per-pixel state."""
        return psld_mean_vector(self.ref, t), self.ref.sigma(t), self.ref.chol(t).T


class GaussVP:
    augmented = False

    def __init__(self, ref: R.RefVP, v0: float):
        self.ref, self.v0 = ref, float(v0)

    def coeffs(self, t, sigma_y, scale=1.0):
        return vp_coeffs(self.ref, t, sigma_y, scale, self.v0)

    def jac(self, t: float) -> float:
        alpha, sigma = math.exp(self.ref.log_alpha(t)), self.ref.sigma(t)
        return sigma / (self.v0 * alpha ** 2 + sigma ** 2)

    def eps(self, u, t):
        return self.jac(t) * u

    def vjp(self, w, t):
        return self.jac(t) * w

    def pixel(self, t):
        sigma = self.ref.sigma(t)
        return np.array([math.exp(self.ref.log_alpha(t))]), np.array([[sigma ** 2]]), np.array([[sigma]])


def guided_eps(gauss, u, t: float, y, mask, task: str, sigma_y: float, scale: float = 1.0):
    """The guided eps of Gaussian data through measure / combine with the closed-form Jacobian."""
    q = gauss.coeffs(t, sigma_y, scale)
    e = gauss.eps(u, t)
    g, w, _, _ = measure(u, e, y, mask, task, q)
    return combine(e, g, gauss.vjp(w, t), q)[0]


def operator_matrix(image_shape, task: str, mask=None):
    """(A [rows, n], keep): the dense operator of one image (batch 1) from ``forward`` of the unit images, without its zero
    rows (the pixels a mask drops); ``keep`` marks the entries of the flat measurement that the rows stand for."""
    n = int(np.prod(image_shape))
    cols = [forward(e.reshape(image_shape), task, mask).reshape(-1) for e in np.eye(n)]
    a = np.stack(cols, axis=1)
    keep = np.abs(a).sum(axis=1) > 0
    return a[keep], keep


def posterior_x0(a_mat: np.ndarray, y_rows: np.ndarray, sigma_y: float, v0: float):
    """(mean [n], covariance [n, n]) of x0 | y for x0 ~ N(0, v0 I), y = A x0 + N(0, sigma_y^2 I)."""
    n = a_mat.shape[1]
    cov = np.linalg.inv(np.eye(n) / v0 + a_mat.T @ a_mat / sigma_y ** 2)
    return cov @ a_mat.T @ y_rows / sigma_y ** 2, cov


def posterior_state(gauss, t: float, mean_x0, cov_x0):
    """(mean, covariance) of u_t | y over the pixel-major state (pixel i holds entries [i d, (i + 1) d), d = 2 for PSLD):
    u_t = a x0 + noise, noise ~ N(0, Sigma_t) per pixel."""
    a, sig, _ = gauss.pixel(t)
    n = mean_x0.size
    return np.kron(mean_x0, a), np.kron(cov_x0, np.outer(a, a)) + np.kron(np.eye(n), sig)


def to_pixel_major(u: np.ndarray, augmented: bool) -> np.ndarray:
    """State of ONE image [1, (2)C, H, W] -> flat vector, pixel-major (x then m of a pixel side by side)."""
    if not augmented:
        return u.reshape(-1)
    x, m = split(u, True)
    return np.stack([x.reshape(-1), m.reshape(-1)], axis=-1).reshape(-1)


def from_pixel_major(v: np.ndarray, image_shape, augmented: bool) -> np.ndarray:
    if not augmented:
        return v.reshape(image_shape)
    p = v.reshape(-1, 2)
    return np.concatenate([p[:, 0].reshape(image_shape), p[:, 1].reshape(image_shape)], axis=1)


def exact_guided_eps(gauss, u, t: float, a_mat, y_rows, sigma_y: float) -> np.ndarray:
    """-L^T grad log p(u_t | y) of ONE image, by dense linear algebra on the posterior of u_t."""
    image_shape = (1, u.shape[1] // (2 if gauss.augmented else 1)) + u.shape[2:]
    mean, cov = posterior_state(gauss, t, *posterior_x0(a_mat, y_rows, sigma_y, gauss.v0))
    score = -np.linalg.solve(cov, to_pixel_major(u, gauss.augmented) - mean)
    lt = gauss.pixel(t)[2]
    n = score.size // lt.shape[0]
    return from_pixel_major(-(np.kron(np.eye(n), lt) @ score), image_shape, gauss.augmented)

"""Float64 reference of the exponential-integrator sampler ``ei_ode`` (a helper module of tests/test_ei_*.py).

Written from the formulas of DESIGN section 11, independently of ``psld_amd.ei`` (which it does not import): where the
product uses Gauss-Legendre panels and a quadrature of the rotation rate, this module uses ``scipy.integrate.quad``
(epsabs = epsrel = 1e-13) for every coefficient and ``solve_ivp(DOP853)`` of ``R' = A R`` from ``R_T = L_T`` for the frame.
Everything is per pixel pair u = (x, m) in forward time t; sampler grids are tau = T - t, ascending.

scipy is imported where it is used, as everywhere in this project: loading it while the test modules are collected puts it
into the process ahead of every GPU test.

Also here: the two-point-mixture eps of the accuracy tests (data +-1 per pixel, exact score), a tight ODE solution of the
probability flow, and the sampler loop for any ``eps_fn`` (so the CPU oracle network can drive it).
"""
from __future__ import annotations

import math
import warnings

import numpy as np

T = 1.0


def grid(n: int, stride: str, eval_eps: float = 1e-3) -> np.ndarray:
    """The wrapper's sampling times (SDEWrapper.sampling_times) in float64 NumPy."""
    t_final = T - eval_eps
    ts = np.linspace(0.0, t_final, n + 1)
    if stride == "quadratic":
        ts = t_final * (1.0 - (ts / t_final) ** 2.0)[::-1]
    return np.ascontiguousarray(ts)


def rot(theta: float) -> np.ndarray:
    return np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])


def lagrange(j: int, times, s: float) -> float:
    v = 1.0
    for i, ti in enumerate(times):
        if i != j:
            v *= (s - ti) / (times[j] - ti)
    return v


class RefPSLD:
    def __init__(self, nu=4.01, gamma=0.01, beta_min=8.0, beta_max=8.0, kappa=0.04, numerical_eps=1e-9):
        self.nu, self.ga, self.b0, self.b1, self.eps = nu, gamma, beta_min, beta_max, numerical_eps
        self.mi = (gamma - nu) ** 2 / 4
        self.m = 1.0 / self.mi
        self.mm_0 = kappa * self.m
        self.lam = -(nu + gamma) / 4
        self.ft = 0.5 * np.array([[-gamma, self.mi], [-1.0, -nu]])
        self.dt = np.diag([gamma, self.m * nu])
        self._frame = None

    @classmethod
    def from_config(cls, cfg):
        s = cfg.model.sde
        assert s.decomp_mode == "lower"
        return cls(s.nu, s.gamma, s.beta_min, s.beta_max, s.kappa, s.numerical_eps)

    def beta(self, t):
        return self.b0 + t * (self.b1 - self.b0)

    def b(self, t):
        return self.b0 * t + 0.5 * t * t * (self.b1 - self.b0)

    def sigma(self, t) -> np.ndarray:
        """Covariance of u_t for x_0 fixed and m_0 ~ N(0, kappa M), with numerical_eps on the diagonal (psld.py:86-152)."""
        nu, ga, mi, m, mm_0 = self.nu, self.ga, self.mi, self.m, self.mm_0
        lam = (nu + ga) / 2
        b = self.b(t)
        b2 = b * b
        sc, em1 = math.exp(-lam * b), math.exp(lam * b) - 1
        xx = (mi ** 2 / 4 * b2 * mm_0 - mi / 2 * b2 + (ga - nu) / 2 * b + em1) * sc
        xm = (mi * (ga - nu) / 8 * b2 * mm_0 + mi / 2 * b * mm_0 + (nu - ga) / 4 * b2) * sc
        mm = (mi / 4 * b2 * mm_0 + (ga - nu) / 2 * b * mm_0 - b2 / 2 + m * (nu - ga) / 2 * b + m * em1 + mm_0) * sc
        return np.array([[xx + self.eps, xm], [xm, mm + self.eps]])

    def chol(self, t) -> np.ndarray:
        s = self.sigma(t)
        l11 = math.sqrt(s[0, 0])
        l21 = s[0, 1] / l11
        return np.array([[l11, 0.0], [l21, math.sqrt(s[1, 1] - l21 * l21)]])

    def chol_inv(self, t) -> np.ndarray:
        l = self.chol(t)
        return np.array([[1 / l[0, 0], 0.0], [-l[1, 0] / (l[0, 0] * l[1, 1]), 1 / l[1, 1]]])

    def flow(self, t_to, t_from) -> np.ndarray:
        db = self.b(t_to) - self.b(t_from)
        return math.exp(self.lam * db) * (np.eye(2) + db * (self.ft - self.lam * np.eye(2)))

    def a_mat(self, t) -> np.ndarray:
        return self.beta(t) * (self.ft + 0.5 * self.dt @ np.linalg.inv(self.sigma(t)))

    # ---- the rotated frame ------------------------------------------------------------------------------------------
    def frame(self, t_min: float = 5e-4):
        """Dense DOP853 solution of R' = A R from R_T = L_T down to ``t_min``."""
        if self._frame is None or self._frame[0] > t_min:
            from scipy.integrate import solve_ivp
            sol = solve_ivp(lambda t, r: (self.a_mat(t) @ r.reshape(2, 2)).reshape(-1), (T, t_min), self.chol(T).reshape(-1),
                            method="DOP853", rtol=1e-13, atol=1e-15, dense_output=True)
            assert sol.success
            self._frame = (t_min, sol.sol)
        return self._frame[1]

    def r_mat(self, t) -> np.ndarray:
        return self.chol(T) if t >= T else self.frame()(t).reshape(2, 2)

    def theta(self, t) -> float:
        """Angle of the rotation nearest to L_t^-1 R_t (it is a rotation up to the numerical_eps on Sigma's diagonal)."""
        p = self.chol_inv(t) @ self.r_mat(t)
        return math.atan2(p[1, 0] - p[0, 1], p[0, 0] + p[1, 1])

    # ---- coefficients -----------------------------------------------------------------------------------------------
    def step_coeffs(self, t_hist, t_next, k_eff: int, cache=None):
        """(Phi, [C_0 .. C_{k_eff-1}]) of the step t_hist[0] -> t_next with history times t_hist (newest first)."""
        from scipy.integrate import quad
        t_n = t_hist[0]
        cache = {} if cache is None else cache

        def base(s):
            v = cache.get(s)
            if v is None:
                v = cache[s] = (self.flow(t_next, s) @ (0.5 * self.beta(s) * self.dt) @ self.chol_inv(s).T
                                @ rot(self.theta(s)))
            return v

        times = list(t_hist[:k_eff])
        cs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for j in range(k_eff):
                integ = np.array([[quad(lambda s: base(s)[r, c] * lagrange(j, times, s), t_n, t_next, epsabs=1e-13,
                                        epsrel=1e-13, limit=400)[0] for c in range(2)] for r in range(2)])
                cs.append(integ @ rot(self.theta(times[j])).T)
        return self.flow(t_next, t_n), cs

    def coeffs(self, ts, order: int):
        """Per step of the sampler grid ``ts``: (Phi, [C_j])."""
        t = T - np.asarray(ts, dtype=np.float64)
        out = []
        for n in range(t.size - 1):
            k = min(order, n + 1)
            out.append(self.step_coeffs([float(t[n - i]) for i in range(k)], float(t[n + 1]), k))
        return out

    def all_orders(self, ts):
        """{order: coeffs(ts, order)} for orders 1-3, sharing the integrand evaluations of a step between the orders."""
        t = T - np.asarray(ts, dtype=np.float64)
        out = {1: [], 2: [], 3: []}
        for n in range(t.size - 1):
            cache, done = {}, {}
            for order in (1, 2, 3):
                k = min(order, n + 1)
                if k not in done:
                    done[k] = self.step_coeffs([float(t[n - i]) for i in range(k)], float(t[n + 1]), k, cache)
                out[order].append(done[k])
        return out

    # ---- probability flow and the two-point mixture ----------------------------------------------------------------------
    def mixture_eps(self, u: np.ndarray, t: float) -> np.ndarray:
        """eps of the exact score of the data distribution {-1, +1} per pixel (momentum m_0 ~ N(0, kappa M)):
        p_t = 1/2 N(mu_t, Sigma_t) + 1/2 N(-mu_t, Sigma_t), mu_t = Phi(t, 0) (1, 0)^T, score = -Sigma^-1 (u - mu tanh(mu^T
        Sigma^-1 u)) = -L^-T eps.  ``u``: [..., 2] pairs."""
        mu = self.flow(t, 0.0) @ np.array([1.0, 0.0])
        si = np.linalg.inv(self.sigma(t))
        w = np.tanh(u @ (si @ mu))
        return (u - w[..., None] * mu) @ self.chol_inv(t).T

    def pf_rhs(self, u: np.ndarray, t: float, eps: np.ndarray) -> np.ndarray:
        """du/dt = F u + 1/2 beta D~ L^-T eps on [..., 2] pairs."""
        beta = self.beta(t)
        return u @ (beta * self.ft).T + eps @ (0.5 * beta * self.dt @ self.chol_inv(t).T).T

    def solve_mixture(self, u0: np.ndarray, t_end: float) -> np.ndarray:
        """Tight solution of the mixture's probability-flow ODE from T to ``t_end``; ``u0`` [n, 2]."""
        from scipy.integrate import solve_ivp
        shape = u0.shape

        def rhs(t, y):
            u = y.reshape(shape)
            return self.pf_rhs(u, t, self.mixture_eps(u, t)).reshape(-1)

        sol = solve_ivp(rhs, (T, t_end), u0.reshape(-1), method="DOP853", rtol=1e-12, atol=1e-12)
        assert sol.success
        return sol.y[:, -1].reshape(shape)


class RefVP:
    def __init__(self, beta_min=0.1, beta_max=20.0):
        self.b0, self.b1 = beta_min, beta_max

    def beta(self, t):
        return self.b0 + t * (self.b1 - self.b0)

    def log_alpha(self, t):
        return -0.25 * t * t * (self.b1 - self.b0) - 0.5 * t * self.b0

    def sigma(self, t):
        return math.sqrt(-math.expm1(2.0 * self.log_alpha(t)))

    def step_coeffs(self, t_hist, t_next, k_eff: int):
        from scipy.integrate import quad
        t_n = t_hist[0]
        times = list(t_hist[:k_eff])
        base = lambda s: math.exp(self.log_alpha(t_next) - self.log_alpha(s)) * 0.5 * self.beta(s) / self.sigma(s)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cs = [quad(lambda s: base(s) * lagrange(j, times, s), t_n, t_next, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
                  for j in range(k_eff)]
        return math.exp(self.log_alpha(t_next) - self.log_alpha(t_n)), cs

    def coeffs(self, ts, order: int):
        t = T - np.asarray(ts, dtype=np.float64)
        return [self.step_coeffs([float(t[n - i]) for i in range(min(order, n + 1))], float(t[n + 1]), min(order, n + 1))
                for n in range(t.size - 1)]


# ---- the sampler loop --------------------------------------------------------------------------------------------------
def sample(coeffs, ts, u0: np.ndarray, eps_fn, augmented: bool = True, pair_axis: int = -1):
    """The multistep loop u <- Phi u + sum_j C_j eps_{n-j} in float64.  ``eps_fn(u, t_n, tau_n) -> eps`` of u's shape.
    Augmented states carry the pair (x, m) along ``pair_axis`` of length 2 (use ``to_pairs`` / ``from_pairs`` for NCHW)."""
    u = np.array(u0, dtype=np.float64)
    hist = []
    for n, (phi, cs) in enumerate(coeffs):
        hist.insert(0, np.asarray(eps_fn(u, T - float(ts[n]), float(ts[n])), dtype=np.float64))
        del hist[len(cs):]
        if augmented:
            um = np.moveaxis(u, pair_axis, -1)
            new = um @ np.asarray(phi).T
            for c, e in zip(cs, hist):
                new = new + np.moveaxis(e, pair_axis, -1) @ np.asarray(c).T
            u = np.moveaxis(new, -1, pair_axis)
        else:
            u = phi * u + sum(c * e for c, e in zip(cs, hist))
    return u


def to_pairs(u: np.ndarray) -> np.ndarray:
    """[B, 2C, H, W] = [x | m] -> [B, C, H, W, 2]."""
    c = u.shape[1] // 2
    return np.stack([u[:, :c], u[:, c:]], axis=-1)


def from_pairs(p: np.ndarray) -> np.ndarray:
    return np.concatenate([p[..., 0], p[..., 1]], axis=1)


def start_points(m: float):
    """The 96 start points of the accuracy tests: default_rng(0), 96 standard normals for x, then 96 more scaled by sqrt(M)
    for the momentum, laid out as the state [B=2, 2C=6, 4, 4] = [x | m]."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal(96)
    mom = rng.standard_normal(96) * math.sqrt(m)
    return np.concatenate([x.reshape(2, 3, 4, 4), mom.reshape(2, 3, 4, 4)], axis=1)

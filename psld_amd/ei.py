"""Host plans of the few-step exponential-integrator samplers ``ei_ode`` and ``ei_sde`` (section 12; at
the end of this file).  Neither is in the reference.

``plan(sde, ts, order)`` turns the sampler's time grid into one coefficient set per step, in NumPy float64:

    u_{n+1} = Phi(t_{n+1}, t_n) u_n + sum_{j < k_eff} C_j eps_{n-j},        k_eff = min(order, n + 1)

with ``t = T - ts`` the forward time, ``Phi`` the closed-form flow of the linear drift and

    C_j = [ int_{t_n}^{t_{n+1}} Phi(t_{n+1}, s) 1/2 beta(s) D L_s^{-T} Q(theta_s) l_j(s) ds ] Q(theta_{t_{n-j}})^T

(PSLD; ``l_j`` the Lagrange basis over the k_eff history times, ``Q(theta)`` the 2x2 rotation that makes
``R_t = L_t Q(theta_t)`` a solution of ``R' = A R``: the network's output is held polynomial in that frame, where it
varies slowly, instead of in the Cholesky frame, which turns by ~10 rad towards t -> 0).  VP-SDE is the scalar case
``c_j = int alpha_{t'} / alpha_s 1/2 beta(s) / sigma_s l_j(s) ds`` (order 1: DDIM).

Quadrature: Gauss-Legendre with ``NQ`` nodes on panels whose end times differ by at most a factor 2 (the integrands steepen
like 1 / sqrt(xx_t) towards t = eval_eps); theta at every node by cumulative panel quadrature from theta(T) = 0.  Everything
is vectorised over all panels of all steps: a 1000-step plan is a sub-second host job.  Plans are cached per
(SDE parameters, grid, order).
"""
from __future__ import annotations

import collections

import numpy as np

from ._lib import EiCoeffs as _EiStruct, EiSdeCoeffs as _EiSdeStruct

NQ = 16                                       # Gauss-Legendre nodes per panel
_CACHE: "collections.OrderedDict" = collections.OrderedDict()
_CACHE_MAX = 16


class EiCoeffs:
    """Coefficients of one step ``t -> t_next`` (forward times).  Augmented (PSLD): ``phi`` [2, 2], ``c`` [n_hist, 2, 2],
    acting on the pair (x, m) of one pixel; VP-SDE: ``phi`` a float, ``c`` [n_hist].  ``c[j]`` multiplies the network output
    of j steps ago (j = 0: the one evaluated at ``t``).  ``theta`` / ``theta_next``: the frame angle at both ends (PSLD)."""
    __slots__ = ("phi", "c", "n_hist", "augmented", "t", "t_next", "theta", "theta_next", "_struct")

    def __init__(self, phi, c, augmented: bool, t: float, t_next: float, theta: float = 0.0, theta_next: float = 0.0):
        self.phi, self.c, self.n_hist, self.augmented = phi, c, int(len(c)), bool(augmented)
        self.t, self.t_next, self.theta, self.theta_next = float(t), float(t_next), float(theta), float(theta_next)
        self._struct = None

    def struct(self) -> _EiStruct:
        """The ``psld_ei_coeffs_t`` of this step (float64 throughout)."""
        if self._struct is None:
            k = _EiStruct()
            k.n_hist, k.augmented = self.n_hist, 1 if self.augmented else 0
            phi = np.asarray(self.phi, dtype=np.float64).reshape(-1)
            for i in range(4):
                k.phi[i] = float(phi[i]) if i < phi.size else 0.0
            for j in range(3):
                row = np.asarray(self.c[j], dtype=np.float64).reshape(-1) if j < self.n_hist else np.zeros(0)
                for i in range(4):
                    k.c[j][i] = float(row[i]) if i < row.size else 0.0
            self._struct = k
        return self._struct


def _gauss():
    """Nodes and weights on [-1, 1], and S[i, k] = int_{-1}^{x_i} l_k(x) dx for the Lagrange basis l_k of the nodes, through
    the Legendre expansion l_k = sum_m (2m + 1) / 2 w_k P_m(x_k) P_m (exact: the rule integrates degree 2 NQ - 1)."""
    x, w = np.polynomial.legendre.leggauss(NQ)
    v = np.polynomial.legendre.legvander(x, NQ)                   # v[i, m] = P_m(x_i), m = 0 .. NQ
    ip = np.empty((NQ, NQ))                                        # ip[i, m] = int_{-1}^{x_i} P_m
    ip[:, 0] = x + 1.0
    for m in range(1, NQ):
        ip[:, m] = (v[:, m + 1] - v[:, m - 1]) / (2 * m + 1)
    a = (2 * np.arange(NQ) + 1) / 2 * w[:, None] * v[:, :NQ]       # a[k, m]
    return x, w, ip @ a.T


_GX, _GW, _GS = _gauss()


def _panels(t: np.ndarray):
    """Split every step [t_n, t_{n+1}] (descending) geometrically into panels with end-time ratio <= 2.  Returns the panel
    ends ``a``, ``b`` [P], the step of each panel [P] and the index of every step's first panel [N]."""
    n = t.size - 1
    npan = np.maximum(1, np.ceil(np.log2(t[:-1] / t[1:]) - 1e-9)).astype(np.int64)
    first = np.cumsum(npan) - npan
    step = np.repeat(np.arange(n), npan)
    i = np.arange(step.size) - first[step]
    t0, t1, m = t[:-1][step], t[1:][step], npan[step]
    a = np.where(i == 0, t0, t0 * (t1 / t0) ** (i / m))
    b = np.where(i == m - 1, t1, t0 * (t1 / t0) ** ((i + 1) / m))
    return a, b, step, first


def _lagrange(s: np.ndarray, t: np.ndarray, step: np.ndarray, order: int):
    """l[j] [P, NQ]: the Lagrange basis in t over the history times t_n, t_{n-1}, ... (k_eff = min(order, n + 1) of them) of
    each panel's step, evaluated at the nodes; zero where j >= k_eff."""
    keff = np.minimum(order, step + 1)
    out = []
    for j in range(order):
        lj = np.where(j < keff, 1.0, 0.0)[:, None] * np.ones_like(s)
        tj = t[np.maximum(step - j, 0)]
        for i in range(order):
            if i == j:
                continue
            use = (i < keff) & (j < keff)
            ti = t[np.maximum(step - i, 0)]
            den = np.where(use, tj - ti, 1.0)
            lj = lj * np.where(use[:, None], (s - ti[:, None]) / den[:, None], 1.0)
        out.append(lj)
    return out


def _rot(theta: np.ndarray) -> np.ndarray:
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


class _Psld:
    """Vectorised float64 restatement of the PSLD scalars the plan needs (PSLD._cov_host / _inv_coeff_host in NumPy)."""

    def __init__(self, sde):
        self.beta_0, self.beta_1 = float(sde.beta_0), float(sde.beta_1)
        self.nu, self.ga, self.mi, self.m = float(sde.nu), float(sde.gamma), float(sde.m_inv), float(sde.m)
        self.mm_0, self.eps, self.lower = float(sde.mm_0), float(sde.eps), sde.decomp_mode == "lower"
        self.lam = -(self.nu + self.ga) / 4
        self.ft = 0.5 * np.array([[-self.ga, self.mi], [-1.0, -self.nu]])            # F~
        self.nil = self.ft - self.lam * np.eye(2)                                     # nilpotent: critical damping
        self.dt = np.array([self.ga, self.m * self.nu])                                # diagonal of D~

    def beta(self, t):
        return self.beta_0 + t * (self.beta_1 - self.beta_0)

    def b(self, t):
        return self.beta_0 * t + 0.5 * (t ** 2) * (self.beta_1 - self.beta_0)

    def cov(self, t):
        nu, ga, mi, m, mm_0 = self.nu, self.ga, self.mi, self.m, self.mm_0
        lam = (nu + ga) / 2
        b = self.b(t)
        b2 = b ** 2
        sc, isc = np.exp(-lam * b), np.exp(lam * b)
        xx = (mi ** 2 / 4 * b2 * mm_0 + (-mi / 2) * b2 + (ga - nu) / 2 * b + (isc - 1)) * sc
        xm = (mi * (ga - nu) / 8 * b2 * mm_0 + mi / 2 * b * mm_0 + (nu - ga) / 4 * b2) * sc
        mm = (mi / 4 * b2 * mm_0 + (ga - nu) / 2 * b * mm_0 + (-1 / 2) * b2 + m * (nu - ga) / 2 * b + m * (isc - 1)
              + mm_0) * sc
        return xx + self.eps, xm, mm + self.eps

    def factors(self, t):
        """(L_t, L_t^{-T}) [..., 2, 2] of get_coeff / get_inv_coeff."""
        xx, xm, mm = self.cov(t)
        det = xx * mm - xm ** 2
        z = np.zeros_like(xx)
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.lower:
                l11 = np.sqrt(xx)
                l21 = xm / l11
                fac = (l11, z, l21, np.sqrt(mm - l21 ** 2))
                inv = (np.sqrt(1 / xx), -xm / (np.sqrt(xx) * np.sqrt(det)), z, np.sqrt(xx / det))
            else:
                u22 = np.sqrt(mm)
                u12 = xm / u22
                fac = (np.sqrt(xx - u12 ** 2), u12, z, u22)
                inv = (np.sqrt(mm / det), z, -xm / (np.sqrt(mm) * np.sqrt(det)), np.sqrt(1 / mm))
        mat = lambda c: np.stack([np.stack([c[0], c[1]], -1), np.stack([c[2], c[3]], -1)], -2)
        fac, inv = mat(fac), mat(inv)
        if not (np.all(np.isfinite(fac)) and np.all(np.isfinite(inv))):
            raise ValueError("Numerical precision error.")
        return fac, inv

    def flow(self, db):
        """Phi for an increment db of b_t: e^{lam db} (I + db (F~ - lam I))."""
        db = np.asarray(db, dtype=np.float64)
        return np.exp(self.lam * db)[..., None, None] * (np.eye(2) + db[..., None, None] * self.nil)

    def theta_rate(self, t, fac, inv):
        """d theta / dt = -(L^-1 A L)_12 (lower factor; +(.)_21 for the upper one), A = F + 1/2 beta D~ Sigma^-1."""
        beta = self.beta(t)[..., None, None]
        linv = np.swapaxes(inv, -1, -2)
        a = beta * (self.ft + 0.5 * self.dt[:, None] * (inv @ linv))
        mloc = linv @ a @ fac
        return -mloc[..., 0, 1] if self.lower else mloc[..., 1, 0]


def _psld_plan(sde, t: np.ndarray, order: int):
    if sde.mode != "score_xm":
        raise ValueError(f"ei_ode needs the PSLD mode score_xm (nu != 0 and gamma != 0), got {sde.mode}: the network "
                         "predicts only half of eps there and the rotated frame R_t = L_t Q(theta_t) cannot be formed")
    p = _Psld(sde)
    n = t.size - 1
    a, b, step, first = _panels(t)
    jac = (b - a) / 2
    s = ((a + b) / 2)[:, None] + jac[:, None] * _GX[None, :]                  # [P, NQ]
    fac, inv = p.factors(s)
    rate = p.theta_rate(s, fac, inv)
    pan = jac * (rate @ _GW)                                                  # int of the rate over each panel
    start = np.cumsum(pan) - pan                                              # theta at each panel's first end
    theta = start[:, None] + jac[:, None] * (rate @ _GS.T)
    theta_t = np.concatenate([[0.0], np.cumsum(pan)[np.append(first[1:] - 1, pan.size - 1)]])   # at t_0 .. t_N
    # integrand without the Lagrange factor: Phi(t', s) 1/2 beta(s) D~ L_s^{-T} Q(theta_s)
    db = p.b(t[1:])[step][:, None] - p.b(s)
    g = p.flow(db) @ ((0.5 * p.beta(s))[..., None, None] * p.dt[:, None] * inv) @ _rot(theta)
    wq = (jac[:, None] * _GW[None, :])[..., None, None]
    lag = _lagrange(s, t, step, order)
    qt = np.swapaxes(_rot(theta_t), -1, -2)                                   # Q(theta_{t_n})^T
    cj = []
    for j in range(order):
        raw = np.add.reduceat((wq * g * lag[j][..., None, None]).sum(axis=1), first, axis=0)     # [N, 2, 2]
        cj.append(raw @ qt[np.maximum(np.arange(n) - j, 0)])
    phi = p.flow(p.b(t[1:]) - p.b(t[:-1]))
    out = []
    for i in range(n):
        k = min(order, i + 1)
        out.append(EiCoeffs(phi[i], np.stack([cj[j][i] for j in range(k)]), True, t[i], t[i + 1], theta_t[i], theta_t[i + 1]))
    return out


def _vp_plan(sde, t: np.ndarray, order: int):
    b0, b1 = float(sde.beta_0), float(sde.beta_1)
    lmc = lambda u: -0.25 * u ** 2 * (b1 - b0) - 0.5 * u * b0
    n = t.size - 1
    a, b, step, first = _panels(t)
    jac = (b - a) / 2
    s = ((a + b) / 2)[:, None] + jac[:, None] * _GX[None, :]
    sigma = np.sqrt(-np.expm1(2.0 * lmc(s)))
    g = np.exp(lmc(t[1:])[step][:, None] - lmc(s)) * 0.5 * (b0 + s * (b1 - b0)) / sigma
    wq = jac[:, None] * _GW[None, :]
    lag = _lagrange(s, t, step, order)
    cj = [np.add.reduceat((wq * g * lag[j]).sum(axis=1), first) for j in range(order)]
    phi = np.exp(lmc(t[1:]) - lmc(t[:-1]))
    return [EiCoeffs(float(phi[i]), np.array([cj[j][i] for j in range(min(order, i + 1))]), False, t[i], t[i + 1])
            for i in range(n)]


def check_order(order) -> int:
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= int(order) <= 3:
        raise ValueError(f"ei_ode: evaluation.sampler.order must be 1, 2 or 3, got {order!r}")
    return int(order)


def plan(sde, ts, order: int = 2):
    """One ``EiCoeffs`` per step of the sampler grid ``ts`` (the samplers' time tau = T - t, ascending from 0; a sequence,
    array or tensor of N + 1 values) for the PSLD (mode score_xm) or VP-SDE ``sde``."""
    from .sde import PSLD
    from .vpsde import VPSDE
    order = check_order(order)
    tau = np.asarray(ts.detach().cpu().numpy() if hasattr(ts, "detach") else ts, dtype=np.float64).reshape(-1)
    t = float(sde.T) - tau
    if t.size < 2 or not np.all(np.diff(t) < 0) or not t[-1] > 0:
        raise ValueError("ei_ode: the time grid must ascend strictly from 0 and end before T")
    if isinstance(sde, PSLD):
        key = ("psld", sde.beta_0, sde.beta_1, sde.nu, sde.gamma, sde.kappa, sde.eps, sde.decomp_mode)
        build = _psld_plan
    elif isinstance(sde, VPSDE):
        key = ("vpsde", sde.beta_0, sde.beta_1)
        build = _vp_plan
    else:
        raise TypeError(f"ei_ode: no plan for an SDE of type {type(sde).__name__}")
    key = key + (tuple(tau.tolist()), order)
    hit = _CACHE.get(key)
    if hit is None:
        hit = _CACHE[key] = build(sde, t, order)
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return hit


# ---- ei_sde: the stochastic lambda family at order 1 --------------------------------------------------
SUB_LOG = 0.0025      # largest ln(t_a / t_b) of one RK4 sub-step: F^_lam grows like (1 + lam^2) / (2 t) towards t = eval_eps
SUB_DB = 0.02         # ... and the largest increment of b_t, which bounds what the conjugation by Phi contributes


class EiSdeCoeffs:
    """Coefficients of one stochastic step ``u <- phi u + c eps + s z`` from ``t`` to ``t_next`` (forward times).  Augmented
    (PSLD): ``phi``, ``c``, ``s`` [2, 2] acting on the pair (x, m) of one pixel, ``s`` lower-triangular; VP-SDE: floats.
    ``psi`` is the transition matrix Psi^_lam(t_next, t) they were formed from."""
    __slots__ = ("phi", "c", "s", "psi", "augmented", "t", "t_next", "lam", "_struct")

    def __init__(self, phi, c, s, psi, augmented: bool, t: float, t_next: float, lam: float):
        self.phi, self.c, self.s, self.psi, self.augmented = phi, c, s, psi, bool(augmented)
        self.t, self.t_next, self.lam, self._struct = float(t), float(t_next), float(lam), None

    def struct(self) -> _EiSdeStruct:
        """The ``psld_ei_sde_coeffs_t`` of this step (float64 throughout; the VP-SDE scalars in entry 0)."""
        if self._struct is None:
            k = _EiSdeStruct()
            k.augmented = 1 if self.augmented else 0
            for name in ("phi", "c", "s"):
                v = np.asarray(getattr(self, name), dtype=np.float64).reshape(-1)
                for i in range(4):
                    getattr(k, name)[i] = float(v[i]) if i < v.size else 0.0
            self._struct = k
        return self._struct


def check_lam(lam) -> float:
    if isinstance(lam, (bool, np.bool_)) or not isinstance(lam, (int, float, np.integer, np.floating)) \
            or not np.isfinite(lam) or lam < 0:
        raise ValueError(f"ei_sde: evaluation.sampler.lam must be a finite number >= 0, got {lam!r}")
    return float(lam)


def _psi_hat(p: _Psld, t: np.ndarray, lam: float) -> np.ndarray:
    """Psi^_lam(t_{n+1}, t_n) [N, 2, 2] of F^_lam = beta (F~ + (1 + lam^2) / 2 D~ Sigma^-1), all steps in lock-step.  With
    Psi^(s, t_n) = Phi(s, t_n) V(s): V' = Phi(t_n, s) G(s) Phi(s, t_n) V, G = (1 + lam^2) / 2 beta D~ Sigma^-1, V(t_n) = I,
    so the linear drift stays exact and only the 1 / t part is integrated: classical RK4 on sub-steps geometric in t.  The
    one-step propagators of all sub-steps are formed at once; what remains sequential is their ordered product."""
    t0, t1 = t[:-1], t[1:]
    m = int(max(8, np.ceil(np.log(t0 / t1).max() * (1 + lam * lam) / 2 / SUB_LOG),
                np.ceil(np.abs(p.b(t0) - p.b(t1)).max() / SUB_DB)))
    frac = np.arange(m + 1)[:, None] / m
    ends = t0[None, :] * (t1 / t0)[None, :] ** frac                           # [m + 1, N]
    ends[0], ends[-1] = t0, t1
    a, b = ends[:-1], ends[1:]
    h = (b - a)[..., None, None]                                              # < 0
    s = np.stack([a, (a + b) / 2, b])                                         # [3, m, N]: the RK4 abscissae
    _, inv = p.factors(s)
    g = ((1 + lam * lam) / 2 * p.beta(s))[..., None, None] * p.dt[:, None] * (inv @ np.swapaxes(inv, -1, -2))
    db = p.b(s) - p.b(t0)[None, None, :]
    hm = p.flow(-db) @ g @ p.flow(db)
    eye = np.eye(2)
    k1 = hm[0]
    k2 = hm[1] @ (eye + h / 2 * k1)
    k3 = hm[1] @ (eye + h / 2 * k2)
    k4 = hm[2] @ (eye + h * k3)
    prop = eye + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)                          # [m, N, 2, 2]
    v = prop[0]
    for i in range(1, m):
        v = prop[i] @ v
    return p.flow(p.b(t1) - p.b(t0)) @ v


def _chol2(pm: np.ndarray) -> np.ndarray:
    """Lower Cholesky factors of [N, 2, 2] symmetric matrices."""
    s00 = np.sqrt(pm[:, 0, 0])
    s10 = pm[:, 1, 0] / s00
    s11 = np.sqrt(pm[:, 1, 1] - s10 ** 2)
    out = np.zeros_like(pm)
    out[:, 0, 0], out[:, 1, 0], out[:, 1, 1] = s00, s10, s11
    if not np.all(np.isfinite(out)):
        raise ValueError("ei_sde: the noise covariance of a step is not positive definite")
    return out


def _psld_plan_sde(sde, t: np.ndarray, lam: float):
    if sde.mode != "score_xm":
        raise ValueError(f"ei_sde needs the PSLD mode score_xm (nu != 0 and gamma != 0), got {sde.mode}: the network "
                         "predicts only half of eps there and C = (Psi^ - Phi) L_t needs both halves")
    p = _Psld(sde)
    psi = _psi_hat(p, t, lam)
    phi = p.flow(p.b(t[1:]) - p.b(t[:-1]))
    fac, _ = p.factors(t)
    xx, xm, mm = p.cov(t)
    sig = np.stack([np.stack([xx, xm], -1), np.stack([xm, mm], -1)], -2)
    pm = sig[1:] - psi @ sig[:-1] @ np.swapaxes(psi, -1, -2)
    s = _chol2((pm + np.swapaxes(pm, -1, -2)) / 2)
    c = (psi - phi) @ fac[:-1]
    return [EiSdeCoeffs(phi[i], c[i], s[i], psi[i], True, t[i], t[i + 1], lam) for i in range(t.size - 1)]


def _vp_plan_sde(sde, t: np.ndarray, lam: float):
    b0, b1 = float(sde.beta_0), float(sde.beta_1)
    lmc = lambda u: -0.25 * u ** 2 * (b1 - b0) - 0.5 * u * b0                  # ln alpha
    la = lmc(t)
    lsig = 0.5 * np.log(-np.expm1(2.0 * la))                                  # ln sigma
    lr = (lsig[1:] - la[1:]) - (lsig[:-1] - la[:-1])                          # ln of the ratio of sigma / alpha: < 0
    phi = np.exp(la[1:] - la[:-1])
    psi = np.exp(lsig[1:] - lsig[:-1] + lam * lam * lr)
    sig = np.exp(lsig)
    c = (psi - phi) * sig[:-1]
    s = sig[1:] * np.sqrt(-np.expm1(2.0 * lam * lam * lr))                    # s^2 = sigma_s^2 - psi^2 sigma_t^2
    return [EiSdeCoeffs(float(phi[i]), float(c[i]), float(s[i]), float(psi[i]), False, t[i], t[i + 1], lam)
            for i in range(t.size - 1)]


def _from_order_one(sde, k: EiCoeffs) -> EiSdeCoeffs:
    """lam = 0: Phi and C_0 of ``plan(sde, ts, 1)`` as they are, S = 0, Psi^ = Phi + C_0 L_t^-1."""
    if k.augmented:
        fac, _ = _Psld(sde).factors(np.float64(k.t))
        return EiSdeCoeffs(k.phi, k.c[0], np.zeros((2, 2)), k.phi + k.c[0] @ np.linalg.inv(fac), True, k.t, k.t_next, 0.0)
    la = -0.25 * k.t ** 2 * (float(sde.beta_1) - float(sde.beta_0)) - 0.5 * k.t * float(sde.beta_0)
    return EiSdeCoeffs(k.phi, float(k.c[0]), 0.0, k.phi + float(k.c[0]) / np.sqrt(-np.expm1(2.0 * la)), False, k.t, k.t_next, 0.0)


def plan_sde(sde, ts, lam: float = 1.0):
    """One ``EiSdeCoeffs`` per step of the sampler grid ``ts`` (as for ``plan``) for the member ``lam`` of the stochastic
    family: 0 is ``plan(sde, ts, 1)`` with no noise, 1 the reverse SDE."""
    from .sde import PSLD
    from .vpsde import VPSDE
    lam = check_lam(lam)
    tau = np.asarray(ts.detach().cpu().numpy() if hasattr(ts, "detach") else ts, dtype=np.float64).reshape(-1)
    t = float(sde.T) - tau
    if t.size < 2 or not np.all(np.diff(t) < 0) or not t[-1] > 0:
        raise ValueError("ei_sde: the time grid must ascend strictly from 0 and end before T")
    if isinstance(sde, PSLD):
        key = ("psld_sde", sde.beta_0, sde.beta_1, sde.nu, sde.gamma, sde.kappa, sde.eps, sde.decomp_mode)
        build = _psld_plan_sde
    elif isinstance(sde, VPSDE):
        key = ("vpsde_sde", sde.beta_0, sde.beta_1)
        build = _vp_plan_sde
    else:
        raise TypeError(f"ei_sde: no plan for an SDE of type {type(sde).__name__}")
    key = key + (tuple(tau.tolist()), lam)
    hit = _CACHE.get(key)
    if hit is None:
        if lam == 0.0:                                                        # the probability flow: ei_ode's own order 1
            hit = [_from_order_one(sde, k) for k in plan(sde, ts, 1)]
        else:
            hit = build(sde, t, lam)
        _CACHE[key] = hit
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return hit

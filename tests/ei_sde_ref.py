"""Float64 reference of the stochastic exponential-integrator sampler ``ei_sde`` (a helper module of tests/test_ei_sde_cpu.py
and tests/test_sampler_ei_sde_gpu.py).

Written from the formulas of DESIGN section 12 on top of tests/ei_ref.py (the SDE's scalars), independently of
``psld_amd.ei`` (which it does not import): where the product integrates the conjugated equation V' = Phi^-1 G Phi V with
RK4 on geometric sub-steps, this module hands ``d Psi^ / ds = F^_lam(s) Psi^`` as it stands to ``solve_ivp(DOP853)`` at
rtol = 1e-12, one step at a time.  Everything is per pixel pair u = (x, m) in forward time t; a step goes from t to s < t.

scipy is imported where it is used (see the header of tests/test_sampler_ei_gpu.py).

Also here: the closed forms of the two ends of the family (lam = 0 through ei_ref's order-1 coefficients, lam = 1 the
Gaussian posterior), the VP-SDE scalars, the eps of point-mass data, and the sampler loop with explicit noise.
"""
from __future__ import annotations

import math

import numpy as np

from tests import ei_ref as R

T = R.T


# ---- PSLD ------------------------------------------------------------------------------------------------------------------
def f_hat(ref: R.RefPSLD, t: float, lam: float) -> np.ndarray:
    """F^_lam(t) = beta (F~ + (1 + lam^2) / 2 D~ Sigma_t^-1)."""
    return ref.beta(t) * (ref.ft + 0.5 * (1.0 + lam * lam) * ref.dt @ np.linalg.inv(ref.sigma(t)))


def psi_hat(ref: R.RefPSLD, t: float, s: float, lam: float) -> np.ndarray:
    """Transition matrix of F^_lam from t down to s."""
    from scipy.integrate import solve_ivp
    sol = solve_ivp(lambda tau, y: (f_hat(ref, tau, lam) @ y.reshape(2, 2)).reshape(-1), (t, s), np.eye(2).reshape(-1),
                    method="DOP853", rtol=1e-12, atol=1e-14)
    assert sol.success
    return sol.y[:, -1].reshape(2, 2)


def step_coeffs(ref: R.RefPSLD, t: float, s: float, lam: float, chol=None):
    """(Phi, Psi^, C, P) of the step t -> s; ``chol``: the factor L_t to use (default: the lower one)."""
    phi, psi = ref.flow(s, t), psi_hat(ref, t, s, lam)
    l = ref.chol(t) if chol is None else chol
    return phi, psi, (psi - phi) @ l, ref.sigma(s) - psi @ ref.sigma(t) @ psi.T


def coeffs(ref: R.RefPSLD, ts, lam: float):
    t = T - np.asarray(ts, dtype=np.float64)
    return [step_coeffs(ref, float(t[n]), float(t[n + 1]), lam) for n in range(t.size - 1)]


def posterior(ref: R.RefPSLD, t: float, s: float):
    """lam = 1 in closed form: Psi^ = Sigma_s Phi(t, s)^T Sigma_t^-1 and P = Sigma_s - Psi^ Phi(t, s) Sigma_s, the mean map
    and the covariance of u_s given u_t for point-mass data."""
    fwd, ss, st = ref.flow(t, s), ref.sigma(s), ref.sigma(t)
    psi = ss @ fwd.T @ np.linalg.inv(st)
    return psi, ss - psi @ fwd @ ss


def chol2(p: np.ndarray) -> np.ndarray:
    s00 = math.sqrt(p[0, 0])
    s10 = p[1, 0] / s00
    return np.array([[s00, 0.0], [s10, math.sqrt(p[1, 1] - s10 * s10)]])


def point_mass_eps(ref: R.RefPSLD, u: np.ndarray, t: float, x0: np.ndarray) -> np.ndarray:
    """eps of the exact score of the data x_0 (one value per pixel, momentum m_0 ~ N(0, kappa M)): L_t^-1 (u - mu_t) with
    mu_t = Phi(t, 0) (x_0, 0)^T.  ``u``: [..., 2] pairs, ``x0``: u's shape without the pair axis."""
    mu = x0[..., None] * (ref.flow(t, 0.0) @ np.array([1.0, 0.0]))
    return (u - mu) @ ref.chol_inv(t).T


# ---- VP-SDE ----------------------------------------------------------------------------------------------------------------
def vp_step(ref: R.RefVP, t: float, s: float, lam: float):
    """(phi, psi^, c, s^2) of DDIM's eta-family written as in the issue."""
    al_t, al_s = math.exp(ref.log_alpha(t)), math.exp(ref.log_alpha(s))
    sg_t, sg_s = ref.sigma(t), ref.sigma(s)
    phi = al_s / al_t
    psi = (sg_s / sg_t) * ((sg_s / al_s) / (sg_t / al_t)) ** (lam * lam)
    return phi, psi, (psi - phi) * sg_t, sg_s ** 2 - psi ** 2 * sg_t ** 2


def vp_coeffs(ref: R.RefVP, ts, lam: float):
    t = T - np.asarray(ts, dtype=np.float64)
    out = []
    for n in range(t.size - 1):
        phi, _, c, s2 = vp_step(ref, float(t[n]), float(t[n + 1]), lam)
        out.append((phi, c, math.sqrt(max(s2, 0.0))))
    return out


# ---- the sampler loop ------------------------------------------------------------------------------------------------------
def sample(steps, ts, u0: np.ndarray, eps_fn, noise_fn, augmented: bool = True):
    """u <- Phi u + C eps(u, t_n) + S z_n in float64 over ``steps`` = [(Phi, C, S)].  ``eps_fn(u, t_n, tau_n)`` and
    ``noise_fn(n, u)`` return arrays of u's shape; augmented states are [..., 2] pairs."""
    u = np.array(u0, dtype=np.float64)
    for n, (phi, c, s) in enumerate(steps):
        e = np.asarray(eps_fn(u, T - float(ts[n]), float(ts[n])), dtype=np.float64)
        z = None if noise_fn is None else np.asarray(noise_fn(n, u), dtype=np.float64)
        if augmented:
            u = u @ np.asarray(phi).T + e @ np.asarray(c).T + (0.0 if z is None else z @ np.asarray(s).T)
        else:
            u = phi * u + c * e + (0.0 if z is None else s * z)
    return u

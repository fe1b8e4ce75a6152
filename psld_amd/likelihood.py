"""Log-likelihood (bits/dim) of a score model through its probability-flow ODE (Song et al. 2021, app. D.2; DESIGN
section 8).

With the forward-time probability-flow drift ``F(u, t) = f(u, t) - 1/2 g(t)^2 s(u, t)`` the density along a solution of
``du/dt = F`` obeys ``d/dt log p_t(u(t)) = -div F``, hence

    log p_eps(u(eps)) = log p_T(u(T)) + int_eps^T div F(u(t), t) dt.

``PFLikelihood.log_prob`` integrates the augmented state ``[u, int div F]`` from ``t = eps`` to ``T`` with the device-side
RK45 of ``samplers.rk45_integrate`` and adds the prior's log-density of the end point.  ``div F`` is the analytic divergence
of the linear drift plus a Hutchinson estimate ``z^T (d(-1/2 g^2 s)/du) z`` with ONE probe ``z`` held fixed along the
trajectory: per right-hand-side evaluation one network forward and one vector-Jacobian product with respect to the network
input (``NCSNpp.vjp_input``: the data-gradient launches of the backward alone, no parameter gradient), around it the kernels
``ops.pf_cotangent`` (cotangent ``w = A^T z``) and ``ops.pf_div_rhs`` (drift and per-sample ``z . vjp``).

Sign and time conventions against the samplers: ``sde.reverse_sde(u, tau, score_fn, probability_flow=True)`` works in
SAMPLER time ``tau = T - t`` and returns ``f_bar = -f + 1/2 g^2 s = -F(u, T - tau)``; this module works in FORWARD time
``t`` (the time the network is conditioned on), so its drift is ``-f_bar`` and integration runs with ``t`` increasing, from
data to prior.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from . import ops
from ._lib import EmCoeffs
from .samplers import rk45_integrate

Tensor = torch.Tensor
LEVELS_NORM = 127.5     # uint8 levels per unit of network input under images_to_tensor(norm=True): x = img / 127.5 - 1


# ---- host algebra (no launches) ------------------------------------------------------------------------------------------
def psld_cotangent_coeffs(sde, t: float):
    """``(a_xx, a_xm, a_mx, a_mm)`` with ``w_x = a_xx z_x + a_xm z_m``, ``w_m = a_mx z_x + a_mm z_m``: the transpose of the
    linear map ``eps -> -1/2 g(t)^2 s(eps)``, ``s = -L_t^{-T} eps`` as ``get_score`` builds it (inverse-Cholesky coefficients
    cast to float32, psld.py:253-258), at forward time ``t``.  In the ``score_m`` (lower) / ``score_x`` (upper) modes the
    network predicts one half and only ``a_mm`` / ``a_xx`` survives: ``w = a_mm z_m`` / ``w = a_xx z_x``.  What
    ``psld_pf_cotangent_f32`` evaluates from the same ``em_coeffs``."""
    k = sde.em_coeffs(float(t), 0.0, True)
    hx, hm = 0.5 * k.beta * k.gamma, 0.5 * k.beta * k.m * k.nu
    if k.score_mode == 1:
        return 0.0, 0.0, 0.0, hm * k.c22
    if k.score_mode == 2:
        return hx * k.c11, 0.0, 0.0, 0.0
    return hx * k.c11, hm * k.c21, hx * k.c12, hm * k.c22


def vp_cotangent_coeff(sde, t: float) -> float:
    """VP-SDE: ``w = 1/2 beta(t) / sigma_t z`` (``s = -eps / sigma_t``, ``g^2 = beta``)."""
    return 0.5 * float(sde.beta_t(float(t))) / float(sde._std(float(t)))


def linear_divergence(sde, t: float, dims: int) -> float:
    """Divergence of the linear drift ``f``: PSLD ``-1/2 beta (gamma + nu)`` per pixel pair, VP ``-1/2 beta`` per pixel;
    ``dims`` = C*H*W of the image."""
    beta = float(sde.beta_t(float(t)))
    if _is_psld(sde):
        return -0.5 * beta * (sde.gamma + sde.nu) * dims
    return -0.5 * beta * dims


def momentum_entropy(mm_0: float, dims: int) -> float:
    """Differential entropy ``H(q) = D/2 log(2 pi e mm_0)`` of ``q = N(0, mm_0 I)`` over ``dims`` = D coordinates."""
    return 0.5 * dims * math.log(2.0 * math.pi * math.e * mm_0)


def bits_per_dim(logp, dims: int, levels: float = LEVELS_NORM):
    """``-logp / (D ln 2) + log2(levels)``: nats of a density over network-input units -> bits per dimension of the uint8
    image (``levels`` uint8 steps per unit of network input; 127.5 for the [-1, 1] mapping, 255 for [0, 1])."""
    return -logp / (dims * math.log(2.0)) + math.log2(levels)


def _is_psld(sde) -> bool:
    return str(getattr(sde, "type", "")).startswith("psld")


class PFLikelihood:
    """``PFLikelihood(config, sde, score_fn).log_prob(u0)`` / ``.bpd(x0)``.

    ``score_fn``: an ``NCSNpp`` (its ``vjp_input`` is the hot path; put it in ``eval()`` mode - the pass runs in the module's
    current mode), or any object with ``vjp_input(x, t, w) -> (eps, dx)``; a plain callable ``eps = score_fn(x, t)`` built
    from torch operations is differentiated with ``torch.autograd`` (analytic scores, user models).
    ``rtol`` / ``atol``: RK45 tolerances, 1e-5 as in Song et al.'s likelihood code and the ``bb_ode`` scripts;
    ``eps``: start time, default ``config.evaluation.eval_eps``; ``probe``: ``'rademacher'`` (device hash,
    ``ops.rademacher``) or ``'gaussian'``."""

    def __init__(self, config, sde, score_fn, rtol: float = 1e-5, atol: float = 1e-5, eps: Optional[float] = None,
                 probe: str = "rademacher"):
        if probe not in ("rademacher", "gaussian"):
            raise ValueError(f"probe kind {probe!r}: 'rademacher' or 'gaussian'")
        self.config, self.sde, self.score_fn = config, sde, score_fn
        self.rtol, self.atol = float(rtol), float(atol)
        self.eps = float(config.evaluation.eval_eps if eps is None else eps)
        self.probe = probe
        self.psld = _is_psld(sde)
        self.nfe = 0

    # ---- pieces ------------------------------------------------------------------------------------------------------
    def _coeffs(self, t: float):
        """(EmCoeffs, vp_std) of forward time ``t`` - one host-computed set per evaluation, as in the samplers."""
        if self.psld:
            return self.sde.em_coeffs(t, 0.0, True), 0.0
        k = EmCoeffs()
        k.beta = float(self.sde.beta_t(t))
        return k, float(self.sde._std(t))

    def _vjp(self, x32: Tensor, t32: Tensor, w: Tensor):
        fn = self.score_fn
        if hasattr(fn, "vjp_input"):
            return fn.vjp_input(x32, t32, w)
        with torch.enable_grad():
            x = x32.detach().clone().requires_grad_()
            y = fn(x, t32)
            (dx,) = torch.autograd.grad(y, x, grad_outputs=w.to(y.dtype))
        return y.detach().to(torch.float32).contiguous(), dx.detach().to(torch.float32).contiguous()

    def rhs_terms(self, u32: Tensor, t: float, z: Tensor):
        """One right-hand-side evaluation at the float32 state ``u32`` and forward time ``t`` (rounded to float32, as
        ``BBODESampler._rhs`` does): ``(out, eps_pred, vjp)`` with ``out`` the flat float64 ``[F, div]`` of ops.pf_div_rhs."""
        self.nfe += 1
        t32 = float(np.float32(t))
        k, vp_std = self._coeffs(t32)
        tv = torch.full((u32.shape[0],), t32, device=u32.device, dtype=torch.float32)
        w = ops.pf_cotangent(z, k, vp_std)
        eps_pred, vjp = self._vjp(u32, tv, w)
        out = ops.pf_div_rhs(ops.f32_to_f64(u32), eps_pred.contiguous(), vjp.contiguous(), z, k, vp_std)
        return out, eps_pred, vjp

    def draw_probes(self, shape, n_probes: int, seed: int, device) -> Tensor:
        """``[n_probes, *shape]`` float32 probes of this object's kind from ``seed``."""
        z = torch.empty((n_probes,) + tuple(shape), device=device, dtype=torch.float32)
        if self.probe == "rademacher":
            return ops.rademacher(z, seed)
        gen = torch.Generator(device=device).manual_seed(int(seed))
        return z.normal_(generator=gen)

    # ---- log-density ---------------------------------------------------------------------------------------------------
    def log_prob_terms(self, u0: Tensor, probes: Optional[Tensor] = None, n_probes: int = 1, seed: int = 0):
        """``(prior[B], integral[B], nfe)`` float64 with ``log p_eps(u0) = prior + integral``: ``prior = prior_logp(u(T))``,
        ``integral = int_eps^T div F dt``, both averaged over the probes; ``nfe`` counts every right-hand-side evaluation.
        The tape of a recorded forward is single-use, so each probe integrates the ODE anew (its trajectory differs from
        another probe's only through the step controller, which also sees the accumulated divergence)."""
        if not u0.is_cuda:
            raise RuntimeError("psld_amd likelihood needs device tensors (no CPU fallback)")
        shape = tuple(u0.shape)
        b = shape[0]
        if probes is None:
            probes = self.draw_probes(shape, int(n_probes), seed, u0.device)
        else:
            probes = probes.to(device=u0.device, dtype=torch.float32)
            if tuple(probes.shape) == shape:
                probes = probes[None]
            if tuple(probes.shape[1:]) != shape:
                raise ValueError(f"probes of shape {tuple(probes.shape)} for a state of shape {shape}")
        probes = probes.contiguous()
        u64 = u0.detach().to(torch.float64).contiguous()
        n = u64.numel()
        prior = torch.zeros(b, device=u0.device, dtype=torch.float64)
        integral = torch.zeros(b, device=u0.device, dtype=torch.float64)
        nfe0 = self.nfe
        with torch.no_grad():
            for z in probes:
                y = torch.zeros(n + b, device=u0.device, dtype=torch.float64)
                y[:n] = u64.view(-1)
                y32 = ops.f64_to_f32(y)
                y, _ = rk45_integrate(lambda t, y64, y32_: self.rhs_terms(y32_[:n].view(shape), t, z)[0], y, y32, self.eps,
                                      float(self.sde.T), self.rtol, self.atol)
                prior += self.sde.prior_logp(y[:n].view(shape))
                integral += y[n:]
        k = probes.shape[0]
        return prior / k, integral / k, self.nfe - nfe0

    def log_prob(self, u0: Tensor, probes: Optional[Tensor] = None, n_probes: int = 1, seed: int = 0):
        """``(logp[B] float64, nfe)``: ``log p_eps(u0)`` of the state ``u0`` (PSLD: ``[x | m]``, ``[B, 2C, H, W]``) taken as
        ``u(eps)``.  ``probes``: ``[n_probes, *u0.shape]`` (or ``u0.shape``) overrides the generator."""
        prior, integral, nfe = self.log_prob_terms(u0, probes, n_probes, seed)
        return prior + integral, nfe

    def bpd(self, x0: Tensor, n_momentum: int = 1, dequantize: bool = False, probes: Optional[Tensor] = None,
            n_probes: int = 1, seed: int = 0, momenta: Optional[Tensor] = None, levels: float = LEVELS_NORM) -> dict:
        """Bits per dimension of images ``x0`` ``[B, C, H, W]`` in network-input units.

        VP-SDE: ``logp = log p_eps(x0)``.  PSLD: data has no momentum, and the model's density lives on ``(x, m)``; with
        any density ``q`` over ``m0``, Jensen's inequality applied to ``log p(x0) = log E_{m0~q}[p_eps(x0, m0) / q(m0)]``
        gives the LOWER BOUND

            log p(x0) >= E_{m0~q}[log p_eps(x0, m0)] + H(q),

        evaluated with ``q = N(0, mm_0 I)`` - the momentum distribution the loss trains with (``sde.mm_0``) - whose
        entropy is ``H(q) = D/2 log(2 pi e mm_0)``, ``D = C*H*W``; the expectation is a Monte-Carlo mean over
        ``n_momentum`` draws.  So for PSLD ``bpd`` is an UPPER bound on the bits/dim (the one CLD reports).

        ``bits/dim = -logp / (D ln 2) + log2(levels)``.  ``dequantize`` adds uniform noise of one uint8 level.
        ``momenta`` ``[n_momentum, B, C, H, W]`` overrides the momentum draws (test hook).  Returns ``bpd``, ``logp``,
        ``prior``, ``integral`` (float64 ``[B]``, the last two averaged over the draws), ``entropy``, ``offset``
        (``log2(levels)``) and ``nfe``."""
        if not x0.is_cuda:
            raise RuntimeError("psld_amd likelihood needs device tensors (no CPU fallback)")
        x0 = x0.detach().to(torch.float32)
        gen = torch.Generator(device=x0.device).manual_seed(int(seed) + 0x5EED)
        if dequantize:
            x0 = x0 + torch.rand(x0.shape, device=x0.device, generator=gen) / levels
        dims = int(np.prod(x0.shape[1:]))
        if self.psld:
            mm_0 = float(self.sde.mm_0)
            if momenta is None:
                momenta = math.sqrt(mm_0) * torch.randn((int(n_momentum),) + tuple(x0.shape), device=x0.device, generator=gen)
            prior = integral = 0.0
            nfe = 0
            for m0 in momenta:
                p, i, n = self.log_prob_terms(torch.cat([x0, m0.to(x0)], dim=1), probes, n_probes, seed)
                prior, integral, nfe = prior + p, integral + i, nfe + n
            prior, integral = prior / len(momenta), integral / len(momenta)
            entropy = momentum_entropy(mm_0, dims)
        else:
            prior, integral, nfe = self.log_prob_terms(x0, probes, n_probes, seed)
            entropy = 0.0
        logp = prior + integral + entropy
        return {"bpd": bits_per_dim(logp, dims, levels), "logp": logp, "prior": prior, "integral": integral,
                "entropy": entropy, "offset": math.log2(levels), "nfe": nfe}

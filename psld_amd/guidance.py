"""Guidance fronts of a score network: each is a ``score_fn`` ``(x32, t32) -> eps`` for every sampler, so no sampler changes.

``CFGScoreFn``: classifier-free guidance for a label-conditioned NCSN++ (``model.score_fn.label_classes`` > 0).

``CFGScoreFn(net, labels, scale)`` is a ``score_fn`` for every sampler: ``(x32, t32) -> eps`` with

    eps = eps_uncond + scale * (eps_cond - eps_uncond)

from ONE network call on the doubled batch ``[x; x]``, ``[t; t]``, ``[labels; no label]`` and one combine kernel
(``ops.cfg_combine``).  ``scale == 1`` is plain conditional sampling and ``scale == 0`` plain unconditional sampling: each
runs its B-batch alone and launches no combine.  The samplers see an opaque callable, so none of them changes; there is
no ``vjp_input`` here, so ``PFLikelihood`` takes its plain-callable path.

``PosteriorScoreFn``: measurement guidance for linear inverse problems ``y = A x0 + noise`` with the unconditional network
(at the end of this file).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops


class CFGScoreFn:
    def __init__(self, net, labels, scale: float = 1.0):
        k = int(getattr(net, "label_classes", 0) or 0)
        if k <= 0:
            raise ValueError("CFGScoreFn needs a network built with model.score_fn.label_classes > 0")
        if torch.is_tensor(labels):
            if labels.dtype != torch.int64 or labels.dim() != 1:
                raise ValueError("CFGScoreFn: labels must be an int or an int64 [B] tensor")
        elif not 0 <= int(labels) <= k:
            raise ValueError(f"CFGScoreFn: label {labels} outside [0, {k}]")
        self.net = net
        self.labels = labels
        self.scale = float(scale)
        self._cache = {}

    # what wrappers and samplers ask of a score network besides calling it
    @property
    def training(self) -> bool:
        return self.net.training

    def eval(self):
        self.net.eval()
        return self

    def parameters(self):
        return self.net.parameters()

    def _labels(self, b: int, device) -> torch.Tensor:
        y = self.labels
        if torch.is_tensor(y):
            if y.shape[0] < b:
                raise ValueError(f"CFGScoreFn: {y.shape[0]} labels for a batch of {b}")
            return y[:b].to(device).contiguous()
        key = (b, str(device))
        if key not in self._cache:
            self._cache[key] = torch.full((b,), int(y), device=device, dtype=torch.int64)
        return self._cache[key]

    def __call__(self, x32: torch.Tensor, t32: torch.Tensor) -> torch.Tensor:
        b = x32.shape[0]
        if self.scale == 0.0:
            return self.net(x32, t32)
        y = self._labels(b, x32.device)
        if self.scale == 1.0:
            return self.net(x32, t32, y=y)
        null = torch.full_like(y, self.net.label_classes)
        eps2 = self.net(torch.cat([x32, x32]), torch.cat([t32, t32]), y=torch.cat([y, null]))
        return ops.cfg_combine(eps2.contiguous(), self.scale)


# ---- measurement guidance -----------------------------------------------------------------------------
# task -> (operator code, block size); mask, gray and pool have orthonormal rows (A A^T = I on their range) and share
# ops.restore_measure; deconv (a periodic blur, DESIGN section 13, "Deconvolution") has not, and has kernels of its own:
# DECONV is a host-side tag that is never handed to the library (whose operator code 3 stays refused); so is SR (sr2 / sr4: a
# periodic blur followed by keeping every 2nd / 4th sample, DESIGN section 13, "Super-resolution")
DECONV = -1
SR = -2
OPERATORS = {"mask": (_lib.RESTORE_MASK, 1), "gray": (_lib.RESTORE_GRAY, 1), "pool2": (_lib.RESTORE_POOL, 2),
             "pool4": (_lib.RESTORE_POOL, 4), "deconv": (DECONV, 1), "sr2": (SR, 2), "sr4": (SR, 4)}
SR_DEFAULT_PSF = "bicubic"


def check_task(task, psf="unchecked") -> str:
    """The task's name if it is one; with ``psf`` given also: a PSF is required with ``deconv``, optional with ``sr2`` / ``sr4``
    (default ``bicubic``) and refused with every other task."""
    if task not in OPERATORS:
        raise ValueError(f"restore: task must be one of {sorted(OPERATORS)}, got {task!r}")
    if (isinstance(psf, str) and psf == "unchecked") or OPERATORS[task][0] == SR:
        return task
    if (psf is not None) != (task == "deconv"):
        raise ValueError("restore: a PSF (gauss:S | box:K | motion:L | file.npy) is required with the task deconv, optional with "
                         f"sr2 / sr4 (which also take bicubic | block) and goes with no other (task {task!r}, psf {psf!r})")
    return task


# ---- the deconv operator: A x = k (*) x per channel, periodic boundary ------------------------------------------------------
def parse_psf(psf, h: int, w: int) -> np.ndarray:
    """The PSF on the ``h x w`` torus, float64 ``[h, w]`` with its middle tap at ``[0, 0]``.  ``psf``: ``gauss:S`` (``exp(-d^2 /
    2 S^2)`` of the wrapped distance ``d``, ``S > 0``, normalised to sum 1), ``box:K`` (K x K uniform, K odd), ``motion:L`` (1 x L
    horizontal uniform, L odd), the path of a ``.npy`` file or an array: float ``[kh, kw]``, both odd and no larger than the
    image, used as given."""
    h, w = int(h), int(w)
    if isinstance(psf, str) and not psf.endswith(".npy"):
        kind, _, arg = psf.partition(":")
        try:
            val = float(arg)
        except ValueError:
            raise ValueError(f"restore: PSF {psf!r} is not gauss:S | box:K | motion:L | file.npy") from None
        if kind == "gauss":
            if not (val > 0.0 and math.isfinite(val)):
                raise ValueError(f"restore: PSF {psf!r}: S must be > 0")
            dy = np.minimum(np.arange(h), h - np.arange(h)).astype(np.float64)[:, None]
            dx = np.minimum(np.arange(w), w - np.arange(w)).astype(np.float64)[None, :]
            k = np.exp(-(dy * dy + dx * dx) / (2.0 * val * val))
            return k / k.sum()
        if kind not in ("box", "motion"):
            raise ValueError(f"restore: PSF {psf!r} is not gauss:S | box:K | motion:L | file.npy")
        n = int(val)
        if n != val or n < 1 or n % 2 == 0:
            raise ValueError(f"restore: PSF {psf!r}: the size must be an odd whole number (an even size has no middle tap)")
        taps = np.full((n, n) if kind == "box" else (1, n), 1.0 / (n * n if kind == "box" else n))
    else:
        taps = np.asarray(np.load(psf) if isinstance(psf, str) else psf, dtype=np.float64)
        if taps.ndim != 2 or taps.shape[0] % 2 == 0 or taps.shape[1] % 2 == 0:
            raise ValueError(f"restore: a PSF array must be [kh, kw] with both sizes odd, got shape {taps.shape}")
        if not np.isfinite(taps).all():
            raise ValueError("restore: the PSF array holds values that are not finite")
    kh, kw = taps.shape
    if kh > h or kw > w:
        raise ValueError(f"restore: a {kh} x {kw} PSF is larger than the {h} x {w} image")
    k = np.zeros((h, w))
    rows, cols = (np.arange(kh) - kh // 2) % h, (np.arange(kw) - kw // 2) % w
    k[np.ix_(rows, cols)] = taps
    return k


def psf_spectrum(psf, h: int, w: int) -> np.ndarray:
    """``h^ = FFT2`` of ``parse_psf(psf, h, w)`` in host float64: the Hermitian half, complex128 ``[h, w/2 + 1]``."""
    return np.fft.rfft2(parse_psf(psf, h, w))


def _psf_key(psf):
    return psf if isinstance(psf, str) else (np.asarray(psf, dtype=np.float64).tobytes(), np.asarray(psf).shape)


_HHAT = {}


def device_spectrum(psf, h: int, w: int, device) -> torch.Tensor:
    """``psf_spectrum`` as the float64 ``[h, w/2 + 1, 2]`` device tensor the deconv kernels read (kept per PSF, size, device)."""
    key = (_psf_key(psf), int(h), int(w), str(device))
    if key not in _HHAT:
        if len(_HHAT) > 64:
            _HHAT.clear()
        hh = psf_spectrum(psf, h, w)
        _HHAT[key] = torch.from_numpy(np.stack([hh.real, hh.imag], axis=-1).copy()).to(device).contiguous()
    return _HHAT[key]


def _apply_deconv(x: torch.Tensor, psf, adjoint: bool) -> torch.Tensor:
    """``k (*) x`` (adjoint: the correlation) over the last two dimensions: the apply kernel on device tensors (float32
    arithmetic in memory, as the kernels'), ``torch.fft`` in float64 on CPU tensors."""
    if x.dim() != 4:
        raise ValueError(f"restore: images of shape {tuple(x.shape)} are not [B, C, H, W]")
    h, w = x.shape[-2:]
    if x.is_cuda:
        hhat = device_spectrum(psf, h, w, x.device)
        return ops.restore_deconv_apply(x.detach().to(torch.float32).contiguous(), hhat, adjoint).to(x.dtype)
    hh = torch.from_numpy(psf_spectrum(psf, h, w))
    xf = torch.fft.rfft2(x.detach().to(torch.float64))
    return torch.fft.irfft2(xf * (hh.conj() if adjoint else hh), s=(h, w)).to(x.dtype)


# ---- the super-resolution operator: A x = D_s (k (*) x), (D_s z)[i, j] = z[s i, s j] ----------------------------------------------
def _cubic(x: np.ndarray) -> np.ndarray:
    """The Keys cubic with a = -0.5."""
    x, a = np.abs(x), -0.5
    return np.where(x <= 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a, 0.0))


def sr_kernel(psf, s: int, h: int, w: int) -> np.ndarray:
    """The convolution kernel ``k`` of ``A x = D_s (k (*) x)`` on the ``h x w`` torus, float64 ``[h, w]``.  ``psf``: ``bicubic`` (the
    default, ``None``): the anti-aliased Keys cubic (a = -0.5), per axis the 4 s taps ``w[o] = cubic((o - (s - 1) / 2) / s)`` at
    offsets ``o = -3 s / 2 .. 5 s / 2 - 1`` from ``s i``, normalised to sum 1 - ``y[i] = sum_o w[o] x[s i + o]``, a correlation, so
    ``k[-o] = w[o]``; ``block``: the mean of each ``s x s`` block (offsets ``0 .. s - 1``; ``A`` is the ``pool`` operator divided
    by ``s``); or anything ``parse_psf`` takes, centred on the sampled pixel ``(s i, s j)``.  ``bicubic`` and ``block`` are
    centred on the block, the others sample the blurred image at the block's top-left pixel."""
    s, h, w = int(s), int(h), int(w)
    if s not in (2, 4) or h % s or w % s:
        raise ValueError(f"restore: super-resolution takes the factors 2 and 4 and a map they divide, got {s} and {h} x {w}")
    psf = SR_DEFAULT_PSF if psf is None else psf
    if not (isinstance(psf, str) and psf in ("bicubic", "block")):
        return parse_psf(psf, h, w)
    if psf == "bicubic":
        offs = np.arange(-3 * s // 2, 5 * s // 2)
        taps = _cubic((offs - (s - 1) / 2.0) / s)
        taps = taps / taps.sum()
    else:
        offs, taps = np.arange(s), np.full(s, 1.0 / s)
    rows, cols = np.zeros(h), np.zeros(w)
    np.add.at(rows, (-offs) % h, taps)
    np.add.at(cols, (-offs) % w, taps)
    return np.outer(rows, cols)


def sr_spectrum(psf, s: int, h: int, w: int):
    """``(h^, Lambda)`` in host float64: ``h^ = FFT2(sr_kernel(...))`` as the Hermitian half, complex128 ``[h, w/2 + 1]``, and the
    eigenvalues of ``A A^T`` on the low-resolution grid, ``Lambda[m1, m2] = (1 / s^2) sum_{a, b < s} |h^[m1 + a h/s, m2 + b w/s]|^2``
    for ``m2 <= w / 2s``: float64 ``[h/s, w/(2s) + 1]`` ("Super-resolution")."""
    k = sr_kernel(psf, s, h, w)
    hl, wl = h // s, w // s
    power = np.abs(np.fft.fft2(k)) ** 2
    lam = power.reshape(s, hl, s, wl).sum(axis=(0, 2)) / (s * s)
    return np.fft.rfft2(k), np.ascontiguousarray(lam[:, :wl // 2 + 1])


_SR = {}


def sr_device_spectra(psf, s: int, h: int, w: int, device):
    """``sr_spectrum`` as the device tensors the kernels read: ``h^`` float64 ``[h, w/2 + 1, 2]`` and ``Lambda`` float64
    ``[h/s, w/(2s) + 1]`` (kept per kernel, factor, size, device)."""
    psf = SR_DEFAULT_PSF if psf is None else psf
    key = (_psf_key(psf), int(s), int(h), int(w), str(device))
    if key not in _SR:
        if len(_SR) > 64:
            _SR.clear()
        hh, lam = sr_spectrum(psf, s, h, w)
        _SR[key] = (torch.from_numpy(np.stack([hh.real, hh.imag], axis=-1).copy()).to(device).contiguous(),
                    torch.from_numpy(lam).to(device).contiguous())
    return _SR[key]


def _apply_sr(x: torch.Tensor, psf, s: int, adjoint: bool) -> torch.Tensor:
    """``D_s (k (*) x)`` ``[B, C, H/s, W/s]`` of images (adjoint: ``A^T r`` ``[B, C, H, W]`` of measurements): the apply kernel on
    device tensors, ``torch.fft`` in float64 on CPU tensors."""
    if x.dim() != 4:
        raise ValueError(f"restore: images of shape {tuple(x.shape)} are not [B, C, H, W]")
    h, w = (x.shape[-2] * s, x.shape[-1] * s) if adjoint else x.shape[-2:]
    if x.is_cuda:
        hhat, _ = sr_device_spectra(psf, s, h, w, x.device)
        return ops.restore_sr_apply(x.detach().to(torch.float32).contiguous(), hhat, s, adjoint).to(x.dtype)
    hh = torch.from_numpy(sr_spectrum(psf, s, h, w)[0])
    x64 = x.detach().to(torch.float64)
    if adjoint:
        up = torch.zeros(tuple(x.shape[:2]) + (h, w), dtype=torch.float64)
        up[..., ::s, ::s] = x64
        return torch.fft.irfft2(torch.fft.rfft2(up) * hh.conj(), s=(h, w)).to(x.dtype)
    return torch.fft.irfft2(torch.fft.rfft2(x64) * hh, s=(h, w))[..., ::s, ::s].contiguous().to(x.dtype)


def apply_operator(x: torch.Tensor, task: str, mask=None, psf=None) -> torch.Tensor:
    """``A x`` of images ``x`` ``[B, C, H, W]`` (setting a problem up; the per-step arithmetic is ``ops.restore_measure`` /
    ``ops.restore_deconv_measure``): mask ``M . x``, gray ``(x_R + x_G + x_B) / sqrt(3)``, pool the block sums over ``k``,
    deconv the periodic convolution with the PSF ``psf`` (``parse_psf``) - on device tensors by the apply kernel; sr2 / sr4 that
    convolution with ``sr_kernel(psf, s, H, W)`` sampled at ``(s i, s j)``, ``[B, C, H/s, W/s]`` at image intensity."""
    op, k = OPERATORS[check_task(task, psf)]
    if op == DECONV:
        return _apply_deconv(x, psf, False)
    if op == SR:
        return _apply_sr(x, psf, k, False)
    want = ops.restore_measurement_shape(x.shape, op, k, 0)
    if op == _lib.RESTORE_MASK:
        if mask is None or tuple(mask.shape) != want:
            raise ValueError(f"restore: the mask operator needs a mask of shape {want}")
        return x * mask.to(x.dtype)
    if op == _lib.RESTORE_GRAY:
        return x.sum(dim=1, keepdim=True) / math.sqrt(3.0)
    b, c, h, w = x.shape
    return x.reshape(b, c, h // k, k, w // k, k).sum(dim=(3, 5)) / k


def apply_adjoint(y: torch.Tensor, task: str, mask=None, psf=None) -> torch.Tensor:
    """``A^T y`` at image shape: the measurement itself (mask), the mean grey value in all three channels (gray), the block
    mean in every pixel of its block (pool) - the measurement shown at image scale; deconv: the correlation with the PSF."""
    op, k = OPERATORS[check_task(task, psf)]
    if op == DECONV:
        return _apply_deconv(y, psf, True)
    if op == SR:
        return _apply_sr(y, psf, k, True)
    if op == _lib.RESTORE_MASK:
        return y * mask.to(y.dtype)
    if op == _lib.RESTORE_GRAY:
        return (y / math.sqrt(3.0)).expand(-1, 3, -1, -1).contiguous()
    return (y / k).repeat_interleave(k, dim=2).repeat_interleave(k, dim=3)


def _uniform_time(t32) -> float:
    """The one time of a sampler's network call (as ``predict_x_from_eps``: one coefficient set serves the whole batch)."""
    if torch.is_tensor(t32):
        vals = t32.detach().reshape(-1).tolist()
        if not vals or any(v != vals[0] for v in vals):
            raise ValueError("PosteriorScoreFn takes ONE time for the whole batch (its coefficients are host scalars)")
        return float(vals[0])
    return float(t32)


def posterior_coeffs(sde, t: float, sigma_y: float, scale: float = 1.0, prior_var: float = 1.0) -> _lib.RestoreCoeffs:
    """The ``psld_restore_coeffs_t`` of forward time ``t`` in host float64.

    PSLD (mode score_xm, lower factor): ``Sigma_t = L L^T`` the perturbation covariance for ``xx_0 = 0``, ``mm_0 = kappa M``,
    ``a_t`` the mean of ``u_t`` for ``x0 = 1, m0 = 0`` (first column of ``predict_x_from_eps``'s matrix), ``p = a / (a . a)``:
    ``q_u = p``, ``q_e = (p_x l11 + p_m l21, p_m l22)``, ``r_t^2 = 1 / (1 / v0 + a^T Sigma^-1 a)``.  VP-SDE: ``q_u = 1 / alpha``,
    ``q_e = sigma / alpha``, ``r_t^2 = v0 sigma^2 / (sigma^2 + v0 alpha^2)``.  ``kappa = scale / (sigma_y^2 + r_t^2)``."""
    from .sde import PSLD
    from .vpsde import VPSDE
    v0, t = float(prior_var), float(t)
    q = _lib.RestoreCoeffs()
    if isinstance(sde, PSLD):
        if sde.mode != "score_xm" or sde.decomp_mode != "lower":
            raise ValueError(f"PosteriorScoreFn needs the PSLD mode score_xm with the lower factor, got {sde.mode} / "
                             f"{sde.decomp_mode}: the Tweedie estimate u - L eps needs both halves of eps")
        xx, xm, mm = sde._cov_host(0.0, float(sde.mm_0), t)
        l11 = math.sqrt(xx)
        l21 = xm / l11
        l22 = math.sqrt(mm - l21 * l21)
        b = float(sde.b_t(t))
        sf = math.exp((sde.nu + sde.gamma) / 4 * b)
        ax, am = ((sde.nu - sde.gamma) / 4 * b + 1) / sf, (-0.5 * b) / sf
        aa = ax * ax + am * am
        px, pm = ax / aa, am / aa
        z1 = ax / l11
        z2 = (am - l21 * z1) / l22
        r2 = v0 / (1.0 + v0 * (z1 * z1 + z2 * z2))                 # 1 / (1 / v0 + a^T Sigma^-1 a), defined at v0 = 0 too
        q.augmented = 1
        q.q_u[0], q.q_u[1] = px, pm
        q.q_e[0], q.q_e[1] = px * l11 + pm * l21, pm * l22
        q.l[0], q.l[1], q.l[2] = l11, l21, l22
    elif isinstance(sde, VPSDE):
        la = float(sde._lmc(t))
        alpha, s2 = math.exp(la), -math.expm1(2.0 * la)
        sigma = math.sqrt(s2)
        r2 = v0 * s2 / (s2 + v0 * alpha * alpha)
        q.augmented = 0
        q.q_u[0], q.q_e[0], q.l[0] = 1.0 / alpha, sigma / alpha, sigma
    else:
        raise TypeError(f"PosteriorScoreFn: no coefficients for an SDE of type {type(sde).__name__}")
    var = float(sigma_y) ** 2 + r2
    if not (var > 0.0 and math.isfinite(var)) or not all(math.isfinite(v) for v in (*q.q_u, *q.q_e, *q.l)):
        raise ValueError(f"PosteriorScoreFn: sigma_y^2 + r_t^2 = {var!r} at t = {t} is not a positive number "
                         f"(sigma_y = {sigma_y}, prior_var = {prior_var})")
    q.kappa = float(scale) / var
    q.r2, q.sigma_y2 = r2, float(sigma_y) ** 2      # python attributes beside the struct's fields: what the deconv measure step takes
    return q


class PosteriorScoreFn:
    """``PosteriorScoreFn(net, sde, operator, sigma_y, scale=1.0, prior_var=1.0)``: the unconditional network ``net`` guided
    towards a measurement ``y = A x0 + N(0, sigma_y^2)`` set with ``set_measurement(y, mask=None)``; ``operator`` is one of
    ``mask | gray | pool2 | pool4``.  A call returns

        eps' = eps - kappa L^T (q_u g - J^T (q_e g)),   g = A^T (y - A x0^(u, eps)),   kappa = scale / (sigma_y^2 + r_t^2)

    i.e. ``-L^T`` times the score plus ``scale * grad_u log N(y; A x0^(u), (sigma_y^2 + r_t^2) I)`` with the Jacobian ``J`` of
    the network kept (exact for Gaussian data; PiGDM's weighting otherwise).  Per call: ONE
    ``net.vjp_input`` (recorded forward + input-gradient-only backward) with ``ops.restore_measure`` between its two phases,
    then ``ops.restore_combine``.  ``scale == 0`` is the plain forward, bit for bit, and launches neither kernel.  A ``net``
    without ``vjp_input`` (a torch callable) is differentiated with ``torch.autograd`` under ``torch.enable_grad()``.

    The guided pass is a RECORDING pass: its arithmetic is the record arithmetic (``ops.set_record_math``), not the
    evaluation arithmetic of the plain sampling forward (``ops.set_math_mode`` / ``ops.set_eval_math``), as for ``bpd``.
    Labels are out of scope here: a ``CFGScoreFn`` is refused as ``net``.

    ``operator="deconv"`` with ``psf=`` (``parse_psf``: ``gauss:S | box:K | motion:L``, a ``.npy`` path or an array; required
    with this operator, refused with the others) is a periodic blur ``A x = k (*) x`` ("Deconvolution").  Its rows are not
    orthonormal, so ``g`` is ``(sigma_y^2 + r_t^2) A^T (sigma_y^2 I + r_t^2 A A^T)^-1 (y - A x0^)``, computed per plane in the
    2-D DFT domain by ``ops.restore_deconv_measure`` from the PSF's spectrum (host float64, held on the device) and the
    measurement's (``ops.restore_deconv_spectrum``, once per measurement, at the first guided call).  The measurement has
    the image's shape; H and W are powers of two from 4 to 128.

    ``operator="sr2" | "sr4"`` ("Super-resolution") is that blur followed by keeping every 2nd / 4th sample,
    ``A = D_s C_k`` with ``k = sr_kernel(psf, s, H, W)`` (``psf`` optional, default ``bicubic``; also ``block`` and what
    ``parse_psf`` takes): the measurement is ``[B, C, H/s, W/s]`` at image intensity.  ``A A^T`` is circulant on the
    low-resolution grid, so the same ``g`` costs three transform pairs per plane (``ops.restore_sr_measure``); H and W are
    powers of two up to 128 with ``H/s >= 4`` and ``W/s >= 4``."""

    def __init__(self, net, sde, operator: str, sigma_y: float, scale: float = 1.0, prior_var: float = 1.0, psf=None):
        if isinstance(net, CFGScoreFn):
            raise ValueError("PosteriorScoreFn: labels are out of scope here - pass the network itself, not a CFGScoreFn")
        self.net, self.sde = net, sde
        self.operator = check_task(operator, psf)
        self.op, self.k = OPERATORS[operator]
        self.psf = SR_DEFAULT_PSF if self.op == SR and psf is None else psf
        if self.op == SR:
            sr_kernel(self.psf, self.k, 128, 128)        # refuses a malformed PSF now; its size is checked against the image's
        elif psf is not None:
            parse_psf(psf, 128, 128)
        self.yhat = None
        self.sigma_y, self.scale, self.prior_var = float(sigma_y), float(scale), float(prior_var)
        if not math.isfinite(self.scale) or not math.isfinite(self.sigma_y) or self.sigma_y < 0:
            raise ValueError(f"PosteriorScoreFn: sigma_y must be >= 0 and scale finite, got {sigma_y!r}, {scale!r}")
        posterior_coeffs(sde, float(sde.T), self.sigma_y, self.scale, self.prior_var)      # refuses what no time can serve
        self.y = self.mask = self._pin = None
        self._coeffs = {}

    # what wrappers and samplers ask of a score network besides calling it
    @property
    def training(self) -> bool:
        return bool(getattr(self.net, "training", False))

    def eval(self):
        if hasattr(self.net, "eval"):
            self.net.eval()
        return self

    def parameters(self):
        return self.net.parameters()

    def set_measurement(self, y: torch.Tensor, mask=None):
        """``y``: the measurement (mask ``[B, C, H, W]``, gray ``[B, 1, H, W]``, pool ``[B, C, H/k, W/k]``), ``mask``: {0, 1}
        ``[B, C, H, W]``, for the mask operator and no other; sr2 / sr4 ``[B, C, H/s, W/s]``.  Kept as contiguous float32 device
        tensors."""
        if (mask is not None) != (self.op == _lib.RESTORE_MASK):
            raise ValueError("PosteriorScoreFn: a mask goes with the mask operator and with no other")
        if y.dim() != 4:
            raise ValueError(f"PosteriorScoreFn: measurement of shape {tuple(y.shape)} is not [B, C, H, W]")
        if mask is not None and tuple(mask.shape) != tuple(y.shape):
            raise ValueError(f"PosteriorScoreFn: mask of shape {tuple(mask.shape)} for a measurement of shape {tuple(y.shape)}")
        self.y = y.detach().to(torch.float32).contiguous()
        self.mask = None if mask is None else mask.detach().to(device=y.device, dtype=torch.float32).contiguous()
        self.yhat = None                                  # deconv: the measurement's spectrum, made by the first guided call
        return self

    def coeffs(self, t: float) -> _lib.RestoreCoeffs:
        q = self._coeffs.get(t)
        if q is None:
            if len(self._coeffs) > 4096:
                self._coeffs.clear()
            q = self._coeffs[t] = posterior_coeffs(self.sde, t, self.sigma_y, self.scale, self.prior_var)
        return q

    def _measurement_for(self, x32):
        if self.y is None:
            raise RuntimeError("PosteriorScoreFn: set_measurement(y, mask) first")
        augmented = 0 if self.sde.type == "vpsde" else 1
        if self.op == DECONV:
            # the measurement has the image's shape; what the kernels read is its spectrum and the PSF's
            want = ops.restore_measurement_shape(x32.shape, _lib.RESTORE_MASK, 1, augmented)
            if tuple(self.y.shape) != want or self.y.device != x32.device:
                raise ValueError(f"PosteriorScoreFn: measurement of shape {tuple(self.y.shape)} on {self.y.device}, the operator "
                                 f"deconv and a state of shape {tuple(x32.shape)} on {x32.device} need {want}")
            h, w = want[2:]
            hhat = device_spectrum(self.psf, h, w, x32.device) if x32.is_cuda else None
            if hhat is None or not ops.restore_deconv_supported(h, w):
                raise ValueError(f"PosteriorScoreFn: the deconv operator needs device tensors and a map whose sides are powers "
                                 f"of two from 4 to 128, got {h} x {w} on {x32.device}")
            if self.yhat is None:
                self.yhat = ops.restore_deconv_spectrum(self.y)
            return self.yhat, hhat
        if self.op == SR:
            b, c, h, w = ops.restore_measurement_shape(x32.shape, _lib.RESTORE_MASK, 1, augmented)
            if not x32.is_cuda or not ops.restore_sr_supported(h, w, self.k):
                raise ValueError(f"PosteriorScoreFn: the operator {self.operator} needs device tensors and a map whose sides are "
                                 f"powers of two from {4 * self.k} to 128, got {h} x {w} on {x32.device}")
            want = (b, c, h // self.k, w // self.k)
            if tuple(self.y.shape) != want or self.y.device != x32.device:
                raise ValueError(f"PosteriorScoreFn: measurement of shape {tuple(self.y.shape)} on {self.y.device}, the operator "
                                 f"{self.operator} and a state of shape {tuple(x32.shape)} on {x32.device} need {want}")
            return self.y, sr_device_spectra(self.psf, self.k, h, w, x32.device)
        want = ops.restore_measurement_shape(x32.shape, self.op, self.k, augmented)
        if tuple(self.y.shape) != want or self.y.device != x32.device:
            raise ValueError(f"PosteriorScoreFn: measurement of shape {tuple(self.y.shape)} on {self.y.device}, the operator "
                             f"{self.operator} and a state of shape {tuple(x32.shape)} on {x32.device} need {want}")
        return self.y, self.mask

    def _time_reader(self, t32):
        """Start fetching the call's time; the returned function hands it over as a host float (and refuses a ``t32`` whose
        entries differ).  A device ``t32`` is copied to pinned memory asynchronously NOW, ahead of the forward on the stream,
        and waited for only between the two phases - when the forward is already queued - so that reading it never leaves
        the device idle behind a drained queue."""
        if not (torch.is_tensor(t32) and t32.is_cuda):
            t = _uniform_time(t32)
            return lambda: t
        n = t32.numel()
        if self._pin is None or self._pin.numel() < n or self._pin.dtype != t32.dtype:
            self._pin = torch.empty(max(n, 1), dtype=t32.dtype).pin_memory()
        buf = self._pin[:n]
        buf.copy_(t32.detach().reshape(-1), non_blocking=True)
        done = torch.cuda.Event()
        done.record()

        def read():
            done.synchronize()
            return _uniform_time(buf)
        return read

    def __call__(self, x32: torch.Tensor, t32: torch.Tensor) -> torch.Tensor:
        if self.scale == 0.0:
            return self.net(x32, t32)
        y, mask = self._measurement_for(x32)
        read_time = self._time_reader(t32)
        x32 = x32.contiguous()
        kept = []

        def w_fn(out):
            q = self.coeffs(read_time())
            if self.op == DECONV:                           # (y, mask) are (the measurement's spectrum, the PSF's)
                g, w = ops.restore_deconv_measure(x32, out, y, mask, q, q.sigma_y2, q.r2)
            elif self.op == SR:                             # (y, mask) are (the measurement, (the kernel's spectrum, Lambda))
                g, w = ops.restore_sr_measure(x32, out, y, mask[0], mask[1], q, q.sigma_y2, q.r2, self.k)
            else:
                g, w = ops.restore_measure(x32, out, y, mask, self.op, self.k, q)
            kept.extend((g, q))
            return w

        if hasattr(self.net, "vjp_input"):
            eps, dx = self.net.vjp_input(x32, t32, w_fn)
        else:
            with torch.enable_grad():
                x = x32.detach().clone().requires_grad_()
                out = self.net(x, t32)
                eps = out.detach().to(torch.float32).contiguous()
                (dx,) = torch.autograd.grad(out, x, grad_outputs=w_fn(eps).to(out.dtype))
            dx = dx.detach().to(torch.float32)
        g, q = kept
        return ops.restore_combine(eps.contiguous(), g, dx.contiguous(), q)

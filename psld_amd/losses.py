"""HSM / DSM score-matching loss with the reference's interface (main/losses.py:69-130).

``PSLDScoreLoss(config, sde).forward(x_0, t, score_fn, eps=None) -> scalar`` with an autograd graph
through ``score_fn``.  Perturbation, the f64->f32 casts and the squared-error reduction (+ its
gradient) are libpsld_hip kernels; ``torch.randn`` draws eps exactly as the reference does.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .registry import get_module, register_module


def label_dropout_p(config) -> float:
    """The label-dropout probability of a training configuration: ``training.label_dropout`` (absent: 0.1) for a network
    with ``model.score_fn.label_classes`` > 0, else 0 - the key is ignored for a network without labels."""
    if int(config.model.score_fn.get("label_classes", 0) or 0) <= 0:
        return 0.0
    return float(config.training.get("label_dropout", 0.1))


def label_drop_mask(batch: int, p: float, device=None, generator=None):
    """Which samples of a batch train without their label (classifier-free guidance): ``u < p`` for ONE ``torch.rand(batch)``
    draw, or None - and no draw at all - for p <= 0.  The callers make this draw after the loss's other draws (momentum,
    eps), so a run without labels consumes the RNG stream exactly as it always did."""
    if p <= 0:
        return None
    return torch.rand(batch, device=device, generator=generator) < p


def _conditional(score_fn, y, p: float, batch: int, device, drop=None):
    """``score_fn`` with the labels (and this step's dropout mask) bound; ``score_fn`` itself when there are none."""
    if y is None:
        return score_fn
    if drop is None:
        drop = label_drop_mask(batch, p, device)
    return lambda z, t: score_fn(z, t, y=y, drop=drop)


class _SqErr(torch.autograd.Function):
    """loss = mean|sum (target - pred)^2; the kernel also emits d loss / d pred."""

    @staticmethod
    def forward(ctx, pred, target, reduce_mean):
        loss, grad = ops.sqerr_loss(target, pred.contiguous(), reduce_mean, want_grad=True)
        ctx.save_for_backward(grad)
        ctx.divisor = pred.numel() if reduce_mean else 1
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        # the gradient handed on carries 1 / divisor: the network's backward pass, which runs next, places its fp16 data
        # gradients by it (record f16: ops.take_grad_shift; a host integer, nothing else reads it)
        ops.set_loss_divisor(ctx.divisor)
        return grad * g, None, None   # g is the 0-d upstream gradient (1.0 for loss.backward())


def importance_sampling(config, sde) -> bool:
    """``training.loss.importance_sampling`` (absent: false): draw the training times from the tabulated density of the
    likelihood weight instead of uniformly.  Only with weighting 'nll' on a PSLD SDE: ValueError else."""
    on = bool(config.training.loss.get("importance_sampling", False))
    if on and not (config.training.loss.weighting == "nll" and getattr(sde, "type", "").startswith("psld")):
        raise ValueError("training.loss.importance_sampling needs training.loss.weighting=nll and the PSLD SDE "
                         f"(got weighting={config.training.loss.weighting!r}, sde={getattr(sde, 'type', type(sde).__name__)!r})")
    return on


def refuse_f16_nll():
    """fp16 record math places its data gradients by a shift that assumes gradients of about 2/N; under the likelihood
    weighting they are up to 1e5 times larger (w(t) ~ 1/t at t = train_eps)."""
    if "f16" in ops.pass_arith(True):
        raise ValueError("training.loss.weighting=nll cannot be combined with fp16 training math (--train-math f16 / "
                         "PSLD_MATH=f16_train): its gradient shift assumes gradients of about 2/N; use bf16x3 or the default")


class _NllScoreErr(torch.autograd.Function):
    """loss (f64) = mean|sum of the g(t)^2-weighted score error, times the per-sample weights; the kernel also emits
    d loss / d pred."""

    @staticmethod
    def forward(ctx, pred, eps, t, coeffs, t_weight, params, score_mode, reduce_mean):
        loss, grad = ops.nll_score_loss(eps, pred.contiguous(), t, coeffs, t_weight, params, score_mode, reduce_mean,
                                        want_grad=True)
        ctx.save_for_backward(grad)
        ctx.divisor = eps.numel() if reduce_mean else 1     # N = B*2C*H*W in every score mode
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        ops.set_loss_divisor(ctx.divisor)       # as _SqErr
        return grad * g.to(grad.dtype), None, None, None, None, None, None, None


@register_module(category="losses", name="psld_score_loss")
class PSLDScoreLoss(nn.Module):
    def __init__(self, config, sde):
        super().__init__()
        assert config.training.loss.weighting in ["fid", "nll"]
        assert config.training.mode in ["hsm", "dsm"]
        assert isinstance(sde, get_module("sde", "psld"))
        self.sde = sde
        self.l_type = config.training.loss.l_type
        self.weighting = config.training.loss.weighting
        if self.weighting == "nll" and self.l_type != "l2":
            raise ValueError("l_type can only be `l2` when using nll weighting")       # losses.py:88-90
        self.importance_sampling = importance_sampling(config, sde)
        if self.weighting == "nll":
            refuse_f16_nll()
        self.mode = config.training.mode
        self.decomp_mode = config.model.sde.decomp_mode
        self.reduce_strategy = "mean" if config.training.loss.reduce_mean else "sum"
        self.label_dropout = label_dropout_p(config)

    def prefetch(self, t):
        """The perturbation coefficients ``forward`` will ask for (SDEWrapper computes and checks them early)."""
        self.sde.prefetch_coeffs(t, 0, self.sde.mm_0 if self.mode == "hsm" else 0.0)

    def forward(self, x_0, t, score_fn, eps=None, m_draw=None, y=None, drop=None, t_weight=None):
        """``eps`` / ``m_draw``: the two normal draws of losses.py:96,108 when the caller has made them already (tests;
        the captured training step, which keeps every RNG call outside its hipGraph).
        ``y``: int64 [B] class labels for a network with ``label_classes``; each sample runs without its label with
        probability ``training.label_dropout`` (``drop``: that mask when the caller has drawn it already) - the one extra
        ``torch.rand(B)`` comes AFTER the momentum and eps draws.
        ``t_weight``: f64 [B] importance weights of the times (weighting 'nll' only): each sample's loss is multiplied by its
        weight before the reduction."""
        sde = self.sde
        if self.weighting == "nll":
            return self._forward_nll(x_0, t, score_fn, eps, m_draw, y, drop, t_weight)
        assert t_weight is None, "t_weight belongs to weighting 'nll'"
        # losses.py:96-102: DSM samples the momentum, HSM marginalises it; the momentum is drawn in BOTH modes (HSM
        # discards it), so a seeded run consumes the device RNG stream exactly like the reference
        if m_draw is None:
            m_draw = torch.randn_like(x_0)
        if self.mode == "hsm":
            m_0, mm_0 = None, sde.mm_0
        else:
            m_0, mm_0 = np.sqrt(sde.mm_0) * m_draw, 0.0
        if eps is None:
            eps = torch.randn(x_0.shape[0], 2 * x_0.shape[1], *x_0.shape[2:], device=x_0.device)
        assert eps.shape[1] == 2 * x_0.shape[1]
        eps = eps.contiguous()
        score_fn = _conditional(score_fn, y, self.label_dropout, x_0.shape[0], x_0.device, drop)
        z_t = sde.perturb_f32(x_0, m_0, 0, mm_0, t, eps)                # losses.py:113-114
        t32 = ops.f64_to_f32(t.contiguous()) if t.dtype == torch.float64 else t.float()
        eps_pred = score_fn(z_t, t32)                                   # losses.py:115
        if sde.mode == "score_m" and self.decomp_mode == "lower":      # losses.py:118-127
            target = torch.chunk(eps, 2, dim=1)[1].contiguous()
        elif sde.mode == "score_x" and self.decomp_mode == "upper":
            target = torch.chunk(eps, 2, dim=1)[0].contiguous()
        else:
            target = eps
        assert eps_pred.shape == target.shape
        return _SqErr.apply(eps_pred, target, self.reduce_strategy == "mean")

    def _forward_nll(self, x_0, t, score_fn, eps, m_draw, y, drop, t_weight):
        """The composition of losses.py:55-63 with PSLD's get_score and likelihood_weighting (the reference's TODO at
        losses.py:74): same draws, same perturbation, then mean|sum of (score(eps_pred) - score(eps))^2 g(t)^2 in f64."""
        sde = self.sde
        refuse_f16_nll()
        if m_draw is None:
            m_draw = torch.randn_like(x_0)
        if self.mode == "hsm":
            m_0, mm_0 = None, sde.mm_0
        else:
            m_0, mm_0 = np.sqrt(sde.mm_0) * m_draw, 0.0
        if eps is None:
            eps = torch.randn(x_0.shape[0], 2 * x_0.shape[1], *x_0.shape[2:], device=x_0.device)
        assert eps.shape[1] == 2 * x_0.shape[1]
        eps = eps.contiguous()
        score_fn = _conditional(score_fn, y, self.label_dropout, x_0.shape[0], x_0.device, drop)
        tb = sde._coeff_table(t, 0, mm_0)       # ONE table: the perturbation and the score coefficients of the loss
        z_t, _, _ = ops.perturb(x_0.contiguous(), None if m_0 is None else m_0.contiguous(), eps, tb, sde._params,
                                want_f32=True)
        t64 = t.to(torch.float64).contiguous()
        eps_pred = score_fn(z_t, ops.f64_to_f32(t64))
        if t_weight is not None:
            t_weight = t_weight.to(torch.float64).contiguous()
        return _NllScoreErr.apply(eps_pred, eps, t64, tb, t_weight, sde._params, sde._score_mode(),
                                  self.reduce_strategy == "mean")


class _VpScoreLoss(torch.autograd.Function):
    """L1 criterion (mode 1) / g(t)^2-weighted score error (mode 2); the kernel also emits d loss / d pred."""

    @staticmethod
    def forward(ctx, pred, target, t, beta0, beta1, mode, reduce_mean):
        loss, grad = ops.vp_score_loss(target, pred.contiguous(), t, beta0, beta1, mode, reduce_mean, want_grad=True)
        ctx.save_for_backward(grad)
        ctx.divisor = pred.numel() if reduce_mean else 1
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        ops.set_loss_divisor(ctx.divisor)       # as _SqErr
        return grad * g.to(grad.dtype), None, None, None, None, None, None


@register_module(category="losses", name="score_loss")
class ScoreLoss(nn.Module):
    """Loss for non-augmented score models (VP-SDE), main/losses.py:21-65: the eps-prediction criterion (MSE, or L1
    for ``l_type='l1'``) for weighting 'fid', the g(t)^2-weighted score error for weighting 'nll'."""

    def __init__(self, config, sde):
        super().__init__()
        assert config.training.loss.weighting in ["nll", "fid"]
        self.sde = sde
        self.l_type = config.training.loss.l_type
        self.weighting = config.training.loss.weighting
        if self.weighting == "nll" and self.l_type != "l2":
            raise ValueError("l_type can only be `l2` when using nll weighting")       # losses.py:33-35
        importance_sampling(config, sde)         # PSLD only: refuses the key here
        self.reduce_strategy = "mean" if config.training.loss.reduce_mean else "sum"
        self.label_dropout = label_dropout_p(config)

    def forward(self, x_0, t, score_fn, eps=None, y=None, drop=None):
        """``y`` / ``drop``: as in PSLDScoreLoss.forward (the dropout draw follows the eps draw)."""
        if eps is None:
            eps = torch.randn_like(x_0)
        assert eps.shape == x_0.shape
        eps = eps.contiguous()
        score_fn = _conditional(score_fn, y, self.label_dropout, x_0.shape[0], x_0.device, drop)
        x_t = self.sde.perturb_f32(x_0, t, eps)                          # losses.py:48-49
        t32 = ops.f64_to_f32(t.contiguous()) if t.dtype == torch.float64 else t.float()
        eps_pred = score_fn(x_t, t32)
        mean = self.reduce_strategy == "mean"
        if self.weighting == "nll":                                      # losses.py:55-63 (f64 loss: t is f64)
            return _VpScoreLoss.apply(eps_pred, eps, t.to(torch.float64).contiguous(), self.sde.beta_0, self.sde.beta_1,
                                      2, mean)
        if self.l_type != "l2":                                          # losses.py:38-39: nn.L1Loss
            return _VpScoreLoss.apply(eps_pred, eps, None, 0.0, 0.0, 1, mean)
        return _SqErr.apply(eps_pred, eps, mean)


class _SoftmaxXent(torch.autograd.Function):
    """loss = mean|sum cross entropy; the kernel also emits d loss / d logits and the top-1 hit count."""

    @staticmethod
    def forward(ctx, logits, labels, reduce_mean):
        scale = 1.0 / logits.shape[0] if reduce_mean else 1.0
        loss, grad, correct = ops.softmax_xent(logits.contiguous(), labels.contiguous(), scale, scale)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(correct)
        ctx.divisor = logits.shape[0] if reduce_mean else 1
        return loss, correct

    @staticmethod
    def backward(ctx, g, _g_correct):
        (grad,) = ctx.saved_tensors
        ops.set_loss_divisor(ctx.divisor)       # as _SqErr: the batch for the mean, 1 for the sum
        return grad * g, None, None


@register_module(category="losses", name="tce_loss")
class PSLDTimeCELoss(nn.Module):
    """Loss of the noise-conditioned classifier used for guidance (main/losses.py:132-178).
    ``forward(x_0, y, t, clf_fn) -> (loss, top-1 accuracy as a fraction in [0, 1] like util.compute_top_k)``; ``config`` is the root node holding
    ``.diffusion`` and ``.clf``.  Both ``randn_like`` draws of the reference are made, in its order (the momentum
    draw is discarded in HSM mode, exactly like there)."""

    def __init__(self, config, sde):
        super().__init__()
        assert config.diffusion.training.mode in ["hsm", "dsm"]
        assert isinstance(sde, get_module("sde", "psld"))
        self.sde = sde
        self.l_type = config.clf.training.loss.l_type
        self.mode = config.diffusion.training.mode
        self.reduce_strategy = "mean" if config.diffusion.training.loss.reduce_mean else "sum"

    def forward(self, x_0, y, t, clf_fn, m0_draw=None, eps=None):
        sde = self.sde
        if m0_draw is None:
            m0_draw = torch.randn_like(x_0)                              # losses.py:152 (drawn in both modes)
        if self.mode == "hsm":
            m_0, mm_0 = None, sde.mm_0
        else:
            m_0, mm_0 = np.sqrt(sde.mm_0) * m0_draw, 0.0
        if eps is None:
            eps = torch.randn(x_0.shape[0], 2 * x_0.shape[1], *x_0.shape[2:], device=x_0.device)   # :164
        u_t = sde.perturb_f32(x_0, m_0, 0, mm_0, t, eps.contiguous())   # losses.py:167 + the .type(float32) of :170
        t32 = ops.f64_to_f32(t.contiguous()) if t.dtype == torch.float64 else t.float()   # layers.py: timesteps.float()
        y_pred = clf_fn(u_t, t32)
        loss, correct = _SoftmaxXent.apply(y_pred, y, self.reduce_strategy == "mean")
        return loss, correct * (1.0 / y_pred.shape[0])                  # losses.py:11-15 compute_top_k(k=1): a fraction

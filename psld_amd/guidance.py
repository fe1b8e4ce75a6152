"""Classifier-free guidance for a label-conditioned NCSN++ (``model.score_fn.label_classes`` > 0).

``CFGScoreFn(net, labels, scale)`` is a ``score_fn`` for every sampler: ``(x32, t32) -> eps`` with

    eps = eps_uncond + scale * (eps_cond - eps_uncond)

from ONE network call on the doubled batch ``[x; x]``, ``[t; t]``, ``[labels; no label]`` and one combine kernel
(``ops.cfg_combine``).  ``scale == 1`` is plain conditional sampling and ``scale == 0`` plain unconditional sampling: each
runs its B-batch alone and launches no combine.  The samplers see an opaque callable, so none of them changes; there is
no ``vjp_input`` here, so ``PFLikelihood`` takes its plain-callable path.
"""
from __future__ import annotations

import torch

from . import ops


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

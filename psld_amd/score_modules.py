"""Parameter holders of the NCSN++ score network with the reference's attribute names (and its initialisers): what
``state_dict()`` sees.  The forward of every block lives in the executor (score_exec.py)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------
# initialisers (song_sde/layers.py:39-76)
# ----------------------------------------------------------------------------------------------
def default_init(shape, scale: float = 1.0) -> Tensor:
    """variance_scaling(scale, 'fan_avg', 'uniform') with in_axis=1, out_axis=0; scale 0 -> 1e-10."""
    scale = 1e-10 if scale == 0 else scale
    rf = float(np.prod(shape)) / shape[1] / shape[0]
    fan_in, fan_out = shape[1] * rf, shape[0] * rf
    variance = scale / ((fan_in + fan_out) / 2)
    return (torch.rand(*shape) * 2.0 - 1.0) * math.sqrt(3 * variance)


# ----------------------------------------------------------------------------------------------
# parameter holders with the reference's attribute names
# ----------------------------------------------------------------------------------------------
class GaussianFourierProjection(nn.Module):
    """layerspp.py:32-41: fixed random frequencies, requires_grad=False."""

    def __init__(self, embedding_size=256, scale=1.0):
        super().__init__()
        self.W = nn.Parameter(torch.randn(embedding_size) * scale, requires_grad=False)


class _Affine(nn.Module):
    """weight / bias holder: nn.Linear ([out,in]), nn.Conv2d (OIHW), nn.GroupNorm ([C])."""

    def __init__(self, weight: Tensor, bias: Tensor):
        super().__init__()
        self.weight = nn.Parameter(weight)
        self.bias = nn.Parameter(bias)


def _linear(in_dim, out_dim):
    return _Affine(default_init((out_dim, in_dim)), torch.zeros(out_dim))  # ncsnpp.py:99-105


def _conv(in_ch, out_ch, k, init_scale=1.0):
    return _Affine(default_init((out_ch, in_ch, k, k), init_scale), torch.zeros(out_ch))  # layers.py:85-109


def _groupnorm(ch):
    return _Affine(torch.ones(ch), torch.zeros(ch))


class NIN(nn.Module):
    """layers.py:531-540: W is [in, out]."""

    def __init__(self, in_dim, num_units, init_scale=0.1):
        super().__init__()
        self.W = nn.Parameter(default_init((in_dim, num_units), init_scale))
        self.b = nn.Parameter(torch.zeros(num_units))


class ResnetBlockBigGANpp(nn.Module):
    """layerspp.py:212-240 (parameters); forward lives in the executor below."""

    def __init__(self, in_ch, out_ch=None, temb_dim=None, up=False, down=False, dropout=0.1, init_scale=0.0):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        self.GroupNorm_0 = _groupnorm(in_ch)
        self.Conv_0 = _conv(in_ch, out_ch, 3)
        if temb_dim is not None:
            self.Dense_0 = _linear(temb_dim, out_ch)
        self.GroupNorm_1 = _groupnorm(out_ch)
        self.Dropout_0 = nn.Dropout(dropout)  # parameter-free; the rate is read by the executor
        self.Conv_1 = _conv(out_ch, out_ch, 3, init_scale)
        self.has_shortcut = in_ch != out_ch or up or down
        if self.has_shortcut:
            self.Conv_2 = _conv(in_ch, out_ch, 1)
        self.in_ch, self.out_ch, self.up, self.down = in_ch, out_ch, up, down


class AttnBlockpp(nn.Module):
    """layerspp.py:62-73."""

    def __init__(self, channels, init_scale=0.0):
        super().__init__()
        self.GroupNorm_0 = _groupnorm(channels)
        self.NIN_0 = NIN(channels, channels)
        self.NIN_1 = NIN(channels, channels)
        self.NIN_2 = NIN(channels, channels)
        self.NIN_3 = NIN(channels, channels, init_scale=init_scale)
        self.channels = channels


class Downsample(nn.Module):
    """layerspp.py:129-147 with with_conv=True: fir -> up_or_down_sampling.Conv2d named Conv2d_0,
    else conv3x3(stride 2, pad 0) named Conv_0."""

    def __init__(self, in_ch, out_ch, fir):
        super().__init__()
        if fir:
            self.Conv2d_0 = _conv(in_ch, out_ch, 3)
        else:
            self.Conv_0 = _conv(in_ch, out_ch, 3)
        self.fir, self.in_ch, self.out_ch = fir, in_ch, out_ch

    @property
    def conv(self):
        return self.Conv2d_0 if self.fir else self.Conv_0

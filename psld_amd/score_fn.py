"""NCSN++ score network on MI355X: the reference's module surface, a HIP executor underneath.

Surface kept from the reference:
  * ``NCSNpp(config)`` registered as ``score_fn/ncsnpp`` (ncsnpp.py:35-39), ``forward(x, time_cond)``
    with ``x: f32[B,C,H,W]`` (NCHW) and ``time_cond: f32[B]`` -> ``f32[B,out_ch,H,W]`` (ncsnpp.py:287,438);
  * an ``nn.Module`` whose ``state_dict()`` has exactly the reference's keys, shapes and order
    (``all_modules.<i>.<Sub>.<param>``; conv weights OIHW, ``NIN.W`` as [in,out],
    ``GaussianFourierProjection.W`` frozen) so published checkpoints load with ``strict=True``;
  * ``deepcopy`` works (train_sde.py:41), parameters are ordinary ``nn.Parameter``s usable by any
    optimizer / EMA loop, gradients arrive in ``p.grad`` after ``loss.backward()``.

What is different underneath: no eager ATen graph.  ``forward`` runs a fixed program of
libpsld_hip kernels over NHWC activations; with grad enabled the whole network is ONE
``torch.autograd.Function`` whose backward replays a hand-written tape (dgrad / wgrad / GN-bwd
kernels) and writes parameter gradients straight into one flat fp32 buffer (``p.grad`` are views
of it), which is what the fused clip+Adam+EMA kernel and the RCCL bucket reducer consume.

Supported config branches = the ones the north-star configs take: resblock_type
'biggan', progressive 'none', progressive_input 'none' | 'residual', embedding 'fourier' |
'positional', fir True | False, nonlinearity 'swish'.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch
import torch.nn as nn

from . import ops
from .registry import register_module
from .score_exec import _Exec
from .score_modules import (NIN, AttnBlockpp, Downsample, GaussianFourierProjection, ResnetBlockBigGANpp,  # noqa: F401
                            _Affine, _conv, _groupnorm, _linear, default_init)
from .score_routes import _pick_nsplit  # noqa: F401  (tests / tools import it from here)
from .score_tape import _SLAB_FLUSH_BYTES, _CatNode, _Node  # noqa: F401
from .score_weights import _frag_entry, _packed_entry, _pfrag_entry, _qkv_entry, _temb_entry, pfrag_tail
from .weight_cache import Entry, WeightCache

Tensor = torch.Tensor
# arith -> (forward tag, data-gradient tag) of NCSNpp._wfrag: the three-limb pair predates the suffix scheme
_WFRAG_TAG = {a: ("wfrag" + sfx, "wfrag_d" + sfx) if sfx else ("wfrag", "dwfrag") for a, sfx in ops.ARITH_SUFFIX.items()}
_ALIGN = 64  # floats: every parameter starts on a 256-byte boundary inside the flat buffers


class _Pending:
    """Counts forward passes whose backward has not run yet (released on backward or when autograd drops
    the graph) — bookkeeping for diagnostics; several outstanding graphs are fine because a backward that
    finds populated gradients accumulates into them (see ``NCSNpp._begin_backward``)."""

    def __init__(self, net):
        self.net = net
        self.live = True
        net._pending += 1

    def release(self):
        if self.live:
            self.live = False
            self.net._pending -= 1

    def __del__(self):
        self.release()


class _NCSNppFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, anchor, net, lab=None, drop=None):
        ex = _Exec(net, record=True)
        ex.watermark = net._watermark_hook
        ex.want_dx = bool(x.requires_grad)
        y = ex.run(x, t, lab, drop)
        ctx.ex = ex
        ctx.net = net
        ctx.pending = _Pending(net)
        return y

    @staticmethod
    def backward(ctx, gy):
        ex, net = ctx.ex, ctx.net
        if ex is None:
            raise RuntimeError("psld_amd.NCSNpp: backward through the same forward pass twice is not supported")
        ctx.ex = None
        net._begin_backward(side=ex.side)
        ex.backward(gy)
        net._end_backward()
        ctx.pending.release()
        return ex.dx_nchw, None, None, None, None, None


class _NCSNppParamFn(torch.autograd.Function):
    """Same executor, with every trainable parameter an INPUT of the autograd node: backward hands their gradients
    (views of the flat gradient buffer) to autograd, which runs each parameter's AccumulateGrad node - the place where
    torch ``DistributedDataParallel`` (Lightning ``strategy="ddp"``, train_sde.py:114) hangs its reducer hooks.
    ``_NCSNppFn`` assigns ``p.grad`` itself and never reaches those nodes."""

    @staticmethod
    def forward(ctx, x, t, net, lab, drop, *params):
        ex = _Exec(net, record=True)
        ex.want_dx = bool(x.requires_grad)
        y = ex.run(x, t, lab, drop)
        ctx.ex = ex
        ctx.net = net
        ctx.pending = _Pending(net)
        ctx.n_params = len(params)
        return y

    @staticmethod
    def backward(ctx, gy):
        ex, net = ctx.ex, ctx.net
        if ex is None:
            raise RuntimeError("psld_amd.NCSNpp: backward through the same forward pass twice is not supported")
        ctx.ex = None
        net._begin_backward(visible=True, side=ex.side)
        ex.backward(gy)
        grads = net._end_backward_visible()
        ctx.pending.release()
        assert len(grads) == ctx.n_params
        return (ex.dx_nchw, None, None, None, None) + grads


@register_module(category="score_fn", name="ncsnpp")
class NCSNpp(nn.Module):
    """NCSN++ (ncsnpp.py:35-285 for the module list; forward in ``_Exec.run``)."""

    is_classifier = False

    def _net_config(self, config):
        return config.model.score_fn

    def __init__(self, config):
        super().__init__()
        self.config = config.model
        sf = self.sf = self._net_config(config)
        if sf.nonlinearity.lower() != "swish":
            raise NotImplementedError("only nonlinearity='swish' is on the north-star path")
        if sf.resblock_type.lower() != "biggan" or sf.progressive.lower() != "none":
            raise NotImplementedError("only resblock_type='biggan', progressive='none' are supported")
        self.nf = nf = sf.nf
        ch_mult = list(sf.ch_mult)
        self.num_res_blocks = nres = sf.num_res_blocks
        self.attn_resolutions = list(sf.attn_resolutions)
        self.num_resolutions = nlev = len(ch_mult)
        self.all_resolutions = [config.data.image_size // (2 ** i) for i in range(nlev)]
        self.noise_cond = sf.noise_cond
        self.skip_rescale = sf.skip_rescale
        self.progressive_input = pin = sf.progressive_input.lower()
        self.embedding_type = emb = sf.embedding_type.lower()
        if pin not in ("none", "residual"):
            raise NotImplementedError("progressive_input must be 'none' or 'residual'")
        if emb not in ("fourier", "positional"):
            raise ValueError(f"embedding type {emb} unknown.")
        init_scale = sf.init_scale
        dropout = sf.dropout
        fir = sf.fir

        modules: List[nn.Module] = []
        if emb == "fourier":
            assert config.training.continuous, "Fourier features are only used for continuous training."
            modules.append(GaussianFourierProjection(embedding_size=nf, scale=sf.fourier_scale))
            embed_dim = 2 * nf
        else:
            embed_dim = nf
        if self.noise_cond:
            modules.append(_linear(embed_dim, nf * 4))
            modules.append(_linear(nf * 4, nf * 4))
        # class conditioning (no counterpart in the reference: ncsnpp.py:288 leaves it as a TODO): K classes -> one embedding
        # table [K + 1, 4 nf] added to the time embedding, row K = "no label"; zero-initialised, so the network starts as its
        # unconditional twin.  A DIRECT parameter: it precedes all_modules in parameters(), i.e. sits at the front of the flat
        # buffers, where the gradients produced last in the backward pass (the time MLP's) belong (ddp.BucketReducer)
        self.label_classes = int(sf.get("label_classes", 0) or 0)
        self.label_emb = None
        if self.label_classes:
            if self.is_classifier:
                raise ValueError("label_classes is a key of model.score_fn: the classifier's number of logits is clf_fn.n_cls")
            if self.label_classes < 0 or not self.noise_cond:
                raise ValueError("model.score_fn.label_classes needs a positive class count and noise_cond=True")
            self.label_emb = nn.Parameter(torch.zeros(self.label_classes + 1, nf * 4))
        temb_dim = nf * 4 if self.noise_cond else None
        rb = lambda **kw: ResnetBlockBigGANpp(temb_dim=temb_dim, dropout=dropout, init_scale=init_scale, **kw)

        channels = sf.in_ch
        input_pyramid_ch = channels
        modules.append(_conv(channels, nf, 3))
        hs_c = [nf]
        in_ch = nf
        for lvl in range(nlev):
            for _ in range(nres):
                out_ch = nf * ch_mult[lvl]
                modules.append(rb(in_ch=in_ch, out_ch=out_ch))
                in_ch = out_ch
                if self.all_resolutions[lvl] in self.attn_resolutions:
                    modules.append(AttnBlockpp(in_ch, init_scale))
                hs_c.append(in_ch)
            if lvl != nlev - 1:
                modules.append(rb(in_ch=in_ch, down=True))
                if pin == "residual":
                    modules.append(Downsample(input_pyramid_ch, in_ch, fir))
                    input_pyramid_ch = in_ch
                hs_c.append(in_ch)
        in_ch = hs_c[-1]
        modules.append(rb(in_ch=in_ch))
        modules.append(AttnBlockpp(in_ch, init_scale))
        modules.append(rb(in_ch=in_ch))
        if self.is_classifier:
            # ncsnpp_clf.py:196-199: flatten (NCHW order) + bias-free Linear to the class logits
            self.n_cls = sf.n_cls
            modules.append(nn.Linear(in_ch * self.all_resolutions[-1] ** 2, self.n_cls, bias=False))
        else:
            for lvl in reversed(range(nlev)):
                for _ in range(nres + 1):
                    out_ch = nf * ch_mult[lvl]
                    modules.append(rb(in_ch=in_ch + hs_c.pop(), out_ch=out_ch))
                    in_ch = out_ch
                if self.all_resolutions[lvl] in self.attn_resolutions:
                    modules.append(AttnBlockpp(in_ch, init_scale))
                if lvl != 0:
                    modules.append(rb(in_ch=in_ch, up=True))
            assert not hs_c
            modules.append(_groupnorm(in_ch))
            modules.append(_conv(in_ch, sf.out_ch, 3, init_scale))
        self.all_modules = nn.ModuleList(modules)

        self._init_runtime()
        # parameter-gradient kernels on a side stream: None = automatic (small batches, see _Exec._run); True / False or
        # PSLD_OVERLAP_WGRAD=1 / 0 force it
        _ow = os.environ.get("PSLD_OVERLAP_WGRAD")
        self.overlap_wgrad = None if _ow is None else _ow == "1"
        self.side_group = 32        # side-stream calls per fork: one event + one stream wait per group (profiles/r02/graph_fork_cost.txt)
        # dgamma / dbeta / bias gradients / split-K slab reductions of a backward pass in batched launches (_Exec.defer_param,
        # _Exec.reduce_slabs); False: one launch per layer, right where the reference's autograd would compute them
        self.defer_param_grads = True
        # None (auto): parameters become inputs of the autograd node (gradients delivered through AccumulateGrad, so
        # torch DDP / Lightning's ddp strategy can reduce them) when a multi-rank process group exists and no
        # BucketReducer is attached; True / False (or PSLD_AUTOGRAD_PARAMS=1 / 0) force it.
        _ap = os.environ.get("PSLD_AUTOGRAD_PARAMS")
        self.autograd_params = None if _ap is None else _ap == "1"
        self.use_graphs = os.environ.get("PSLD_GRAPHS", "0") == "1"

    def _init_runtime(self):
        """Executor state (never part of state_dict, started afresh by deepcopy): flat parameter / gradient storage,
        arenas, job tables, persistent buffers, derived weights, captured graphs, side stream."""
        self._flat: Optional[Tensor] = None
        self._flat_grad: Optional[Tensor] = None
        self._offsets = None
        # derived weights; a batched refresh needs two entries of a limb / Winograd family, one of a gathered copy
        self._wcache = WeightCache({"limb": (ops.pack_frag_batch, 2), "limb_tail": (ops.pack_frag_batch_tail, 2),
                                    "wino": (ops.pack_wino_batch, 2),
                                    "limb_x3": (ops.pack_frag_batch_x3, 2), "wino_x3": (ops.pack_wino_batch_x3, 2),
                                    "limb_f16": (ops.pack_frag_batch_f16, 2), "wino_f16": (ops.pack_wino_batch_f16, 2),
                                    "qkv_bias": (ops.copy_batch, 1), "temb": (ops.copy_batch, 1)})
        self._anchor = None
        self._reducer = None
        self._posfreq = None
        self._module_offs = None
        self._tables = ops.TableCache()
        self._parena = self._sarena = None
        self._persistent = {}
        self._plist = None
        self._tlist = None
        self._gviews = None
        self._pending = 0
        self._backward_count = 0    # finished backward passes (FusedAdam.step refuses to re-apply a consumed gradient)
        self._dropout_seed_dev = None   # static int64 device word supplied by a captured training step (wrapper.py)
        self._accumulating = False
        self._grad_stale = False
        self._scratch_grad = None
        self._sviews = None
        self._graphs = {}
        self._side = None

    def pin_scratch(self):
        """A captured hipGraph replays raw pointers into the parameter / slab arenas and the cached job tables: keep every
        buffer they ever pointed to alive (outgrown arena buffers are retained, tables are not evicted)."""
        self._param_arena().pinned = True
        self._slab_arena().pinned = True
        self._tables.pinned = True

    def _param_arena(self) -> "ops.Arena":
        dev = self._params()[0].device
        if self._parena is None or self._parena.device != dev:
            self._parena = ops.Arena(dev, 64 << 20)
        return self._parena

    def _slab_arena(self) -> "ops.Arena":
        dev = self._params()[0].device
        if self._sarena is None or self._sarena.device != dev:
            self._sarena = ops.Arena(dev, _SLAB_FLUSH_BYTES + (256 << 20))
        return self._sarena

    def _persist(self, name: str, shape) -> Tensor:
        """A float32 buffer that keeps its address for this network, name and shape."""
        dev = self._params()[0].device
        key = (name, tuple(shape), dev)
        t = self._persistent.get(key)
        if t is None:
            t = self._persistent[key] = torch.empty(tuple(shape), device=dev, dtype=torch.float32)
        return t

    def _side_stream(self):
        dev = next(self.parameters()).device
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        return self._side

    # ---- flat parameter / gradient storage ----------------------------------------------------------
    def _params(self) -> List[nn.Parameter]:
        """Cached parameter list (the module structure never changes after construction)."""
        if self._plist is None:
            self._plist = list(self.parameters())
        return self._plist

    def _layout(self):
        offs, off = {}, 0
        for p in self._params():
            offs[id(p)] = off
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        return offs, off

    def flatten_parameters(self) -> Tensor:
        """Make every parameter a view into one contiguous fp32 buffer (idempotent).  Needed by the
        fused optimiser / EMA / all-reduce; deepcopy() and .to() are followed by a re-flatten."""
        params = self._params()
        flat = self._flat
        if flat is not None:
            # fast validation: every 16th parameter (and the last) still points into the flat buffer
            offs = self._offsets
            base = flat.data_ptr()
            if all(q.data_ptr() == base + 4 * offs[id(q)] for q in params[::16]) and \
                    params[-1].data_ptr() == base + 4 * offs[id(params[-1])]:
                return flat
        dev = params[0].device
        offs, total = self._layout()
        ok = flat is not None and flat.device == dev and flat.numel() == total and all(
            p.data_ptr() == flat.data_ptr() + 4 * offs[id(p)] for p in params)
        if not ok:
            flat = torch.zeros(total, device=dev, dtype=torch.float32)
            for p in params:
                o = offs[id(p)]
                flat[o:o + p.numel()].copy_(p.data.reshape(-1))
                p.data = flat[o:o + p.numel()].view(p.shape)
            self._flat = flat
            self._flat_grad = None
            self._gviews = None
            self._scratch_grad = self._sviews = None
            self._wcache.clear()
        self._offsets = offs
        self._module_offs = None
        return self._flat

    def flat_grad(self) -> Tensor:
        self.flatten_parameters()
        if self._flat_grad is None or self._flat_grad.device != self._flat.device or \
                self._flat_grad.numel() != self._flat.numel():
            self._flat_grad = torch.zeros_like(self._flat)
            self._gviews = None
            self._gviews = self._views_of(self._flat_grad)
        return self._flat_grad

    def _views_of(self, buf: Tensor):
        return {id(q): buf[self._offsets[id(q)]:self._offsets[id(q)] + q.numel()].view(q.shape) for q in self._params()}

    def _grad_view(self, p: nn.Parameter) -> Tensor:
        """View of the buffer the CURRENT backward writes into (the flat gradient, or the scratch buffer when
        this pass has to be accumulated onto existing gradients)."""
        if self._gviews is None:
            self._gviews = self._views_of(self._flat_grad)
        if self._accumulating:
            if self._sviews is None:
                self._sviews = self._views_of(self._scratch_grad)
            return self._sviews[id(p)]
        return self._gviews[id(p)]

    def _module_offset(self, module: nn.Module) -> int:
        if self._module_offs is None:
            self._module_offs = {}
            for m in self.all_modules:
                ps = list(m.parameters())
                if ps:
                    self._module_offs[id(m)] = min(self._offsets[id(p)] for p in ps)
        return self._module_offs.get(id(module), 0)

    def weights_changed(self):
        """Call after writing parameters through raw pointers (fused optimiser / EMA kernels)."""
        self._wcache.invalidate()

    # ---- derived weights (weight_cache.py): cached until the weights change, refreshed in place ------------------
    def _packed(self, conv: _Affine, dgrad: bool = False) -> Tensor:
        """[co][tap][ci] (forward) or [ci][flip tap][co] (data-gradient) copy of an OIHW weight."""
        return self._wcache.get(conv.weight, "dpack" if dgrad else "pack", _packed_entry, dgrad)

    def _frag(self, conv: _Affine, dgrad: bool) -> Tensor:
        """bf16 limb fragments of a 3x3 weight (ops.conv3x3_frag)."""
        return self._wcache.get(conv.weight, "dfrag" if dgrad else "frag", _frag_entry, dgrad, False)

    def _wfrag(self, conv: _Affine, dgrad: bool = False, arith: str = "x6") -> Tensor:
        """Winograd-transformed fragments of a 3x3 weight (ops.conv3x3_wino_frag) in ``arith``: tags "wfrag" / "dwfrag", and
        "wfrag_x3" / "wfrag_d_x3", "wfrag_f16" / "wfrag_d_f16"."""
        return self._wcache.get(conv.weight, _WFRAG_TAG[arith][dgrad], _frag_entry, dgrad, True, arith)

    def _pfrag(self, owner: nn.Parameter, tag: str, n: int, k: int, sn: int, sk: int, into: Optional[Tensor] = None,
               chunk0: int = 0, chunks_total: int = 0, n0: int = 0, n_total: int = 0, arith: str = "x6") -> Tensor:
        """Limb fragments (ops.gemm_frag) of the [n][k] view of ONE parameter (element (i, j) at i*sn + j*sk), refreshed
        together with the 3x3 fragments by the batched launch.  ``into``: the buffer to fill (several parameters that
        share one fragment set: q | k | v) - then ``chunk0`` / ``chunks_total`` place this parameter's K range inside the
        set's K dimension (psld_pack_frag_batch).  ``arith``: the fragments' form; the entry's tag is ``tag`` with its suffix
        ("fwd_x3", "qkv_d_f16", ...).
        A set that is no whole number of 128 x 64 tiles (score_weights.pfrag_tail: channel widths in steps of 32) is packed
        as padded three-limb tail fragments (ops.gemm_frag_tail); ``n0`` / ``n_total`` then place the parameter's rows
        inside a shared set's N dimension."""
        return self._wcache.get(owner, tag + ops.ARITH_SUFFIX[arith], _pfrag_entry, tag, arith, n, k, sn, sk, into, chunk0,
                                chunks_total, n0, n_total)

    def _qkv_frags(self, mod):
        """Fragments of an attention block's q | k | v projections as ONE GEMM operand each way - forward B[n][k] =
        [W_q | W_k | W_v][k][n] (N = 3c), data gradient B[n][k] = [W_q | W_k | W_v][n][k] (K = 3c) - and the concatenated
        bias.  Packed straight from the three parameters into shared buffers by the batched refresh of all fragments (no
        concatenated copy of the weights, no launch of their own after the first step); the biases of ALL attention blocks
        are gathered by one batched copy when they change."""
        n0 = mod.NIN_0
        c = n0.W.shape[0]
        e = self._wcache.entry(n0.b, "qkv", _qkv_entry, mod)
        pf, pd = e.out[:2]
        fb = pf.numel() // 3
        for i, nin in enumerate((n0, mod.NIN_1, mod.NIN_2)):
            if pfrag_tail(3 * c, c):
                # c % 128 != 0: a projection's rows start inside a 128-row tile of the padded set
                self._pfrag(nin.W, "qkv_f", c, c, 1, c, into=pf, n0=i * c, n_total=3 * c)
                self._pfrag(nin.W, "qkv_d", c, c, c, 1, into=pd, chunk0=i * (c // 32), chunks_total=3 * (c // 32))
                continue
            # forward: rows n of the set are output channels -> each projection is a contiguous third of the set
            self._pfrag(nin.W, "qkv_f", c, c, 1, c, into=pf[i * fb:(i + 1) * fb])
            # data gradient: the three projections are concatenated along K
            self._pfrag(nin.W, "qkv_d", c, c, c, 1, into=pd, chunk0=i * (c // 32), chunks_total=3 * (c // 32))
        return self._wcache.fresh(e)

    def _qkv_frags_x3(self, mod, dgrad: bool = False, f16: bool = False):
        """The forward (``dgrad``: data-gradient) q | k | v fragment set of _qkv_frags in a reduced arithmetic: two limbs, or
        (``f16``) one fp16 plane (whole-tile sets only: c % 128 == 0)."""
        arith = "f16" if f16 else "x3"
        n0, sfx = mod.NIN_0, ops.ARITH_SUFFIX[arith]
        c = n0.W.shape[0]
        fb = ops.gemm_frag_bytes_f16(c, c) if f16 else ops.gemm_frag_bytes_x3(c, c)
        # the holder of the shared buffer (no family: the "qkv_d" / "qkv_f" entries of the three projections fill it)
        pf = self._wcache.entry(n0.W, ("qkv_set_d" if dgrad else "qkv_set") + sfx, lambda w: Entry(
            w, out=torch.empty(3 * fb, dtype=torch.uint8, device=w.device), build=lambda prev: prev)).out
        for i, nin in enumerate((n0, mod.NIN_1, mod.NIN_2)):
            if dgrad:       # concatenated along K, as in _qkv_frags
                self._pfrag(nin.W, "qkv_d", c, c, c, 1, into=pf, chunk0=i * (c // 32), chunks_total=3 * (c // 32), arith=arith)
            else:
                self._pfrag(nin.W, "qkv_f", c, c, 1, c, into=pf[i * fb:(i + 1) * fb], arith=arith)
        return pf

    def _temb_plan(self):
        """Gathered time-embedding projections ``(wcat, bcat, offsets)``: wcat [sum C_out][4*nf] and bcat [sum C_out]
        hold Dense_0.weight / .bias of every ResBlock back to back, offsets maps each block to its first row.  None when
        the network is not noise-conditioned."""
        if not self.noise_cond:
            return None
        first = next(m for m in self.all_modules if isinstance(m, ResnetBlockBigGANpp))
        return self._wcache.get(first.Dense_0.weight, "temb", _temb_entry, self.all_modules)

    def _pos_freq(self, device):
        if self._posfreq is None or self._posfreq.device != device:
            half = self.nf // 2
            e = math.log(10000) / (half - 1)                                   # layers.py:500-507
            self._posfreq = torch.exp(torch.arange(half, dtype=torch.float32) * -e).to(device)
        return self._posfreq

    # ---- backward bookkeeping ------------------------------------------------------------------------
    def mark_grads_stale(self):
        """The next backward overwrites the gradient buffer (what ``zero_grad`` means for this module)."""
        self._grad_stale = True

    def _trainable(self) -> List[nn.Parameter]:
        if self._tlist is None or len(self._tlist[1]) != sum(p.requires_grad for p in self._params()):
            self._tlist = (None, [p for p in self._params() if p.requires_grad])
        return self._tlist[1]

    def _params_visible(self) -> bool:
        """Should this forward hand the parameters to autograd (see ``autograd_params``)?"""
        if self.autograd_params is not None:
            return self.autograd_params
        import torch.distributed as dist
        return self._reducer is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def _begin_backward(self, visible: bool = False, side=None):
        """``side``: the stream THIS pass runs its parameter-gradient kernels on (None: everything on one stream)."""
        self.flat_grad()
        # torch semantics: a populated .grad is accumulated into.  Kernels WRITE their results, so in that
        # case this pass goes to a scratch buffer that is added afterwards (one extra 0.4 GB pass).
        probe = next((p for p in self._params() if p.requires_grad), None)
        if visible:
            # autograd adds what backward returns INTO a populated .grad: it must not be handed the very memory
            # .grad aliases, whatever zero_grad() marked
            self._accumulating = probe is not None and probe.grad is not None
        else:
            self._accumulating = probe is not None and (probe.grad is not None) and not self._grad_stale
        self._grad_stale = False
        target = self._flat_grad
        if self._accumulating:
            if self._scratch_grad is None or self._scratch_grad.numel() != self._flat_grad.numel() or \
                    self._scratch_grad.device != self._flat_grad.device:
                self._scratch_grad = torch.zeros_like(self._flat_grad)
                self._sviews = None
            target = self._scratch_grad
        if self._reducer is not None:
            self._reducer.begin(target)
            self._reducer.producer_streams = [side] if side is not None else []

    def _watermark_hook(self, offset: int):
        if self._reducer is not None:
            self._reducer.ready_from(offset)

    def _end_backward(self):
        self._backward_count += 1
        if self._reducer is not None:
            self._reducer.finish()
        if self._accumulating:
            ops.axpby(self._scratch_grad, 1.0, None, 0.0, self._flat_grad, accumulate=True)
            self._accumulating = False
        for p in self._params():
            if not p.requires_grad:
                continue
            gv = self._gviews[id(p)]
            if p.grad is None or p.grad.data_ptr() == gv.data_ptr():
                p.grad = gv
            else:
                p.grad.add_(gv)  # caller kept a foreign .grad tensor: accumulate like autograd would

    def _end_backward_visible(self):
        """Gradients of the trainable parameters, in ``_trainable()`` order, for autograd to accumulate: fresh view
        objects of the buffer this pass wrote (a view nobody else references is adopted by AccumulateGrad as ``.grad``
        without a copy, so ``p.grad`` keeps aliasing the flat gradient buffer the fused optimiser reads)."""
        src = self._scratch_grad if self._accumulating else self._flat_grad
        self._accumulating = False
        self._backward_count += 1
        offs = self._offsets
        return tuple(src[offs[id(p)]:offs[id(p)] + p.numel()].view(p.shape) for p in self._trainable())

    def adopt_foreign_grads(self) -> int:
        """Copy every ``p.grad`` that does NOT alias the flat gradient buffer into its slot (a reducer that swaps
        ``.grad`` for its own bucket views - DDP ``gradient_as_bucket_view=True`` - leaves the reduced values there);
        returns how many were copied.  Called by ``FusedAdam.step``."""
        self.flat_grad()
        if self._gviews is None:
            self._gviews = self._views_of(self._flat_grad)
        tr = self._trainable()
        # probe three parameters first: a reducer that swaps .grad does so for all of them
        if not any(q.grad is not None and q.grad.data_ptr() != self._gviews[id(q)].data_ptr()
                   for q in (tr[0], tr[len(tr) // 2], tr[-1])):
            return 0
        dst, src = [], []
        for p in tr:
            gv = self._gviews[id(p)]
            if p.grad is not None and p.grad.data_ptr() != gv.data_ptr():
                dst.append(gv)
                src.append(p.grad)
        if dst:
            torch._foreach_copy_(dst, src)
        return len(dst)

    def set_reducer(self, reducer):
        """Attach a gradient reducer (psld_amd.ddp.BucketReducer) fed during backward."""
        self._reducer = reducer

    # ---- forward -----------------------------------------------------------------------------------------
    def _labels(self, x: Tensor, y: Optional[Tensor], drop: Optional[Tensor] = None):
        """``(lab, drop)`` as the executor takes them: int64 [B] rows of ``label_emb`` (``y`` None: the "no label" row K for
        every sample) and the optional uint8 [B] mask of the samples that read row K whatever their label; (None, None) for a
        network without labels, which refuses ``y``."""
        k = self.label_classes
        if k == 0:
            if y is not None or drop is not None:
                raise ValueError("NCSNpp: y / drop given to a network built without model.score_fn.label_classes")
            return None, None
        b = x.shape[0]
        if y is None:
            return torch.full((b,), k, device=x.device, dtype=torch.int64), None
        if not torch.is_tensor(y) or y.dtype != torch.int64 or tuple(y.shape) != (b,) or y.device != x.device:
            raise ValueError(f"NCSNpp: y must be an int64 tensor of shape ({b},) on {x.device}")
        if drop is not None:
            if tuple(drop.shape) != (b,) or drop.device != x.device:
                raise ValueError(f"NCSNpp: drop must be a mask of shape ({b},) on {x.device}")
            drop = drop.to(torch.uint8).contiguous()
        return y.contiguous(), drop

    def forward(self, x: Tensor, time_cond: Tensor, y: Optional[Tensor] = None, drop: Optional[Tensor] = None) -> Tensor:
        """``y`` (networks with ``label_classes`` = K > 0): int64 [B] class labels in [0, K] on the device, K and ``y=None``
        meaning "no label"; ``drop``: optional mask [B], true where a sample is to run without its label (label dropout)."""
        if not x.is_cuda:
            raise RuntimeError("psld_amd.NCSNpp runs on MI355X only: the HIP extension has no CPU fallback "
                               "(use oracle/psld_oracle.py as the CPU checker)")
        if x.dtype != torch.float32 or time_cond.dtype != torch.float32:
            raise RuntimeError("NCSNpp expects float32 x and time_cond (ncsnpp.py:287; psld.py:354)")
        ops.lib()
        x = x.contiguous()
        t = time_cond.contiguous()
        lab, drop = self._labels(x, y, drop)
        self.flatten_parameters()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self._params())
        if need_grad or (torch.is_grad_enabled() and x.requires_grad):
            self.flat_grad()
            if self._anchor is None or self._anchor.device != x.device:
                self._anchor = torch.zeros(1, device=x.device, requires_grad=True)
            if need_grad and self._params_visible():
                if self._reducer is not None:
                    raise RuntimeError("psld_amd.NCSNpp: autograd_params (gradients through AccumulateGrad, for torch DDP) "
                                       "and a BucketReducer are two gradient exchanges: detach one of them")
                return _NCSNppParamFn.apply(x, t, self, lab, drop, *self._trainable())
            return _NCSNppFn.apply(x, t, self._anchor, self, lab, drop)
        if self.use_graphs and not self.training:
            return self._graph_forward(x, t, lab, drop)
        with torch.no_grad():
            return _Exec(self, record=False).run(x, t, lab, drop)

    def vjp_input(self, x: Tensor, time_cond: Tensor, w, y: Optional[Tensor] = None):
        """``(y, dx)``: the network output at ``(x, time_cond)`` and the vector-Jacobian product ``w^T dy/dx`` (NCHW, fp32),
        from ONE recorded forward in the module's current train / eval state (eval: no dropout) and one backward that runs
        the data-gradient launches alone (``_Exec.input_grad_only``).  No autograd node is built and no parameter gradient
        is touched: nothing is written into ``flat_grad()`` or any ``p.grad``, so an EMA copy that is only being evaluated
        needs no gradient buffer.  ``dx`` is bit for bit the ``x.grad`` of ``forward(x.requires_grad_()).backward(w)``.
        The pass runs in the record arithmetic in force (``ops.pass_arith(record=True)``), like any recording pass.

        Two phases: ``w`` may be a callable ``w_fn(out) -> w`` for a cotangent that depends on the output (measurement
        guidance, psld_amd.guidance.PosteriorScoreFn).  It is called between the recorded forward and the backward, with the
        output that is also returned, and hands back the float32 cotangent of that shape.  Whatever it launches runs on the
        current stream and allocates through torch alone: the executor's arena and workspaces hold the recorded pass until
        the backward has run."""
        if not x.is_cuda:
            raise RuntimeError("psld_amd.NCSNpp runs on MI355X only: the HIP extension has no CPU fallback "
                               "(use oracle/psld_oracle.py as the CPU checker)")
        two_phase = not torch.is_tensor(w) and callable(w)
        if x.dtype != torch.float32 or time_cond.dtype != torch.float32 or (not two_phase and w.dtype != torch.float32):
            raise RuntimeError("NCSNpp.vjp_input expects float32 x, time_cond and w")
        ops.lib()
        lab, drop = self._labels(x, y)
        self.flatten_parameters()
        with torch.no_grad():
            ex = _Exec(self, record=True, input_grad_only=True)
            ex.want_dx = True
            out = ex.run(x.detach().contiguous(), time_cond.detach().contiguous(), lab, drop)
            if two_phase:
                w = w(out)
                if not torch.is_tensor(w) or w.dtype != torch.float32:
                    raise RuntimeError("NCSNpp.vjp_input: the cotangent callable must return a float32 tensor")
            if w.shape != out.shape:
                raise ValueError(f"vjp_input: cotangent of shape {tuple(w.shape)} for an output of shape {tuple(out.shape)}")
            ex.backward(w.detach())
        return out, ex.dx_nchw

    # ---- HIP-graph replay of the inference forward (launch-bound regime: small sampling batches) ----------
    def enable_graphs(self, flag: bool = True):
        """Capture the eval-mode forward into a HIP graph per input shape and replay it: one graph launch
        instead of ~600 kernel launches issued from Python (the reference samples at 16 images/GPU,
        where the forward is launch-bound).  Weights may keep changing (EMA): packed copies are refreshed
        in place before a replay."""
        self.use_graphs = bool(flag)
        if not flag:
            self._graphs = {}

    def _graph_forward(self, x: Tensor, t: Tensor, lab: Optional[Tensor] = None, drop: Optional[Tensor] = None) -> Tensor:
        if drop is not None:            # label dropout belongs to training passes: not worth a capture of its own
            with torch.no_grad():
                return _Exec(self, record=False).run(x, t, lab, drop)
        key = (tuple(x.shape), x.device.index, ops.pass_arith(False))     # a capture replays the launches of its arithmetic
        ent = self._graphs.get(key)
        if lab is not None:
            # the labels are a static input like x and t, refreshed before every replay; their range is checked here, outside
            # the capture (the label kernels' own check is an assert on the stream)
            ops.check_labels(lab, self.label_classes + 1)
        if ent is None:
            sx, st = x.clone(), t.clone()
            sl = lab.clone() if lab is not None else None
            cur = torch.cuda.current_stream()
            warm = torch.cuda.Stream(device=x.device)
            warm.wait_stream(cur)
            with torch.cuda.stream(warm), torch.no_grad():
                for _ in range(2):   # packs weights, sizes workspaces, one-time kernel attributes
                    _Exec(self, record=False).run(sx, st, sl)
            cur.wait_stream(warm)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                sy = _Exec(self, record=False).run(sx, st, sl)
            ent = self._graphs[key] = [graph, sx, st, sy, None, sl]
            self.pin_scratch()       # the graph holds raw pointers into arenas / job tables: no eviction, no freeing from now on
        graph, sx, st, sy, stamp, sl = ent
        now = (self._wcache.epoch, self._flat._version)
        if stamp != now:
            self._wcache.refresh(forward_only=True)              # refresh, in the same storage, what the graph reads
            ent[4] = now
        sx.copy_(x)
        st.copy_(t)
        if sl is not None:
            sl.copy_(lab)
        graph.replay()
        return sy.clone()

    def __deepcopy__(self, memo):
        """Modules and configuration are copied, the executor state starts afresh (_init_runtime)."""
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        new._init_runtime()
        for k, v in self.__dict__.items():
            if k not in new.__dict__:
                new.__dict__[k] = copy.deepcopy(v, memo)
        # detach copied params from the source's flat buffer (they are re-flattened on first use)
        for p in new.parameters():
            p.data = p.data.clone()
        return new


@register_module(category="clf_fn", name="ncsnpp_clf")
class NCSNppClassifier(NCSNpp):
    """Noise-conditioned classifier for guidance (ncsnpp_clf.py:36-283): the NCSN++ time
    embedding, stem, down path and middle block - the same modules, kernels and executor as ``NCSNpp`` - followed
    by flatten + Linear(bias=False) to ``n_cls`` logits.  Built from the ``clf`` config node (reads
    ``model.clf_fn``); ``clf(x f32[B,in_ch,H,W], t f32[B]) -> f32[B,n_cls]`` with autograd to the parameters
    (training, ``tce_loss``) and to ``x`` (the guidance gradient of ``cc_em_sde``)."""

    is_classifier = True

    def _net_config(self, config):
        return config.model.clf_fn

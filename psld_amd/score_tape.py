"""Executor base of the NCSN++ score network: graph nodes, the kernel-launch helpers shared by every block (3x3
convolutions, pointwise GEMMs and their gradients dispatched on the routes of score_routes.py, GroupNorm backward, bias gradients,
few-channel convolutions), the side stream, the deferred parameter-gradient reductions and the backward tape.  The
network's program - which block runs when - is score_exec.py."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import score_routes as R
from .score_modules import _Affine
from .score_routes import _pick_nsplit
from .score_weights import PointwiseWeight, _built_entry

Tensor = torch.Tensor


class _Node:
    """``gp``: GroupNorm partial sums of ``v`` left behind by the limb kernel that produced it (ops.gn_part_buffer),
    or None: the GroupNorm that reads the node then skips its statistics pass over the tensor.
    ``used``: a consumer has read the node (forward order): the FIRST consumer's backward is the last writer of ``g``.
    ``want_gsum``: the producer has a bias whose gradient is the column sum of ``g``; ``gsum`` [b][c]: those sums per
    image, left by the last writer when it was a one-pass GroupNorm backward (_Exec.gn_backward), else None."""
    __slots__ = ("v", "g", "gp", "used", "want_gsum", "gsum")

    def __init__(self, v, gp=None, want_gsum=False):
        self.v = v
        self.g = None
        self.gp = gp
        self.used = False
        self.want_gsum = want_gsum
        self.gsum = None


class _CatNode:
    """torch.cat([a, b], dim=channels) that is never materialised: the consuming residual block reads both sources
    (two-source convolution kernels, per-source GroupNorm over each source's share of the groups) and writes the
    gradients straight into the sources' buffers."""
    __slots__ = ("a", "b")

    def __init__(self, a: _Node, b: _Node):
        self.a = a
        self.b = b


_SLAB_FLUSH_BYTES = 1 << 30     # parked split-K slabs are reduced (one launch) once they pass this many bytes


def _gbuf(node: _Node):
    """Gradient buffer of a node and whether it already holds a partial sum."""
    if node.g is None:
        node.g = torch.empty_like(node.v)
        return node.g, False
    return node.g, True


def _fir_kernel(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.float32)
    k = np.outer(k, k)
    k /= np.sum(k)
    return k


class _ExecBase:
    """One forward (and, if ``record``, the tape of its backward) over NHWC tensors: state and launch helpers."""

    def __init__(self, net: "NCSNpp", record: bool, input_grad_only: bool = False):
        self.net = net
        # the backward of this pass is wanted for the gradient w.r.t. the network input alone (NCSNpp.vjp_input): every
        # launch whose only products are parameter gradients is off - whatever on_side carries (weight and bias gradients,
        # the slab flush), the deferred reductions and the time-embedding MLP's backward (t gets no gradient, so all of it
        # ends in parameters) - and g() hands out no view of the flat gradient.  The data-gradient launches are those of the
        # full backward, argument for argument
        self.input_grad_only = bool(input_grad_only) and record
        self.tape = [] if record else None
        self.record = record
        sf = net.sf
        self.s = ops.INV_SQRT2 if sf.skip_rescale else 1.0
        self.drop_p = float(sf.dropout) if net.training else 0.0  # nn.Dropout: active in train mode
        # Dropout masks are derived in the kernels from (seed, element index).  The per-pass part of the seed stays in
        # DEVICE memory (one int64 drawn on the device: no host synchronisation per forward, and a hipGraph-captured
        # training step - which supplies its own static seed word, refreshed before every replay - draws fresh masks);
        # the per-block part is a host constant.
        self.seed_dev = None
        if self.drop_p > 0:
            self.seed_dev = net._dropout_seed_dev if net._dropout_seed_dev is not None else \
                torch.randint(0, 2 ** 62, (1,), device=net._params()[0].device, dtype=torch.int64)
        self.n_drop = 0
        fk = tuple(sf.fir_kernel) if sf.fir else (1, 1)
        self.k_down = _fir_kernel(fk)
        self.k_up = self.k_down * 4.0
        p = self.k_down.shape[0] - 2
        self.pad_up = ((p + 1) // 2 + 1, p // 2)       # up_or_down_sampling.py:222-224
        self.pad_down = ((p + 1) // 2, p // 2)         # :255-257
        self.temb_act: Optional[_Node] = None
        self.watermark = None  # callable(flat_offset) for the DDP reducer
        # weight / bias gradients are off the dependency chain of backward: they run on a side HIP stream so
        # that their MFMA-bound kernels overlap the HBM-bound kernels of the chain (GN backward, reductions)
        # (decided in _run, once the batch is known: net.overlap_wgrad None = automatic)
        self.side = None
        self.side_queue = []        # (fn, tensors) waiting for the next fork
        self.side_group = net.side_group
        self.want_dx = False        # gradient w.r.t. the network input requested (x.requires_grad)
        # this pass's arithmetic, most preferred first (ops.pass_arith: the one reader of math mode, record math, eval math and
        # record f16).  A launch site takes the first rung it has a form for (pick):
        #   Winograd forward, GroupNorm-fused forward                'f16', 'x3', 'x6'
        #   Winograd data gradient                                   'f16' with the pass's operand shift, 'x3', 'x6'
        #   Winograd-domain weight gradient                          'x3', 'x6'
        #   LIMB pointwise forward / data gradient                   'f16' / 'x3' where its gemm_split_*_wanted holds, else 'x6'
        #                                                            (the data gradient's 'f16' form carries the shift)
        #   everything else (LIMB_TAIL, direct limb 3x3, attention products, tile engine, NIN / pointwise weight gradients)  'x6'
        # 'x3' and 'f16' are NOT fp32-equivalent; the forward of a recording fp16 pass is unshifted
        self.arith = ops.pass_arith(record)
        self.split = bool(self.arith)       # a limb math mode: the bf16 limb kernels (csrc/conv_split.hip) where a route names them
        # the sites without a policy, resolved once for the pass
        self.a_wino = self.pick(ops.ARITHS)
        self.a_wgrad = self.pick(("x3", "x6"))
        self.gshift = 0
        self.limb_planes = os.environ.get("PSLD_LIMB_PLANES", "1") != "0"    # A/B switch for tools/bench_sample.py
        # forward attention in one kernel (attention.hip) wherever it takes the shape (B=128: 8x8 maps 17 vs 54 us of the
        # three-kernel path, 16x16 maps 62-65 vs 72 us, tools/bench_attn.py); PSLD_FUSED_ATTN=0: the three kernels
        self.fused_attn = os.environ.get("PSLD_FUSED_ATTN", "1") != "0"
        # bias / time-embedding gradients as column sums a one-pass GroupNorm backward forms of the dx it writes
        # (ops.gn_bwd colsum_img) instead of a column-sum pass over that tensor (PSLD_GN_BWD_COLSUM=0: the passes)
        self.gn_bwd_colsum = os.environ.get("PSLD_GN_BWD_COLSUM", "1") == "1"
        self.dx_nchw = None
        # Parameter gradients that are reductions over the batch (GroupNorm dgamma / dbeta, bias gradients) or over split-K
        # slabs are not on the dependency chain of backward: their inputs are parked in two persistent arenas and reduced
        # by ONE launch per kind at the end of the pass (net.defer_param_grads; earlier when a gradient bucket is about to
        # be exchanged, or when the parked slabs pass _SLAB_FLUSH_BYTES)
        self.defer = bool(net.defer_param_grads) and record
        self.dense_batched = False
        self.dense_ok = False
        self.dense_pending = []         # (first column of dtp_all, C_out, Dense_0) of blocks whose Dense_0 gradient is parked
        self.pjobs, self.pblocks = [], 0
        self.sjobs, self.sitems, self.sbytes = [], 0, 0

    # -- helpers ------------------------------------------------------------------------------
    def push(self, fn, module=None):
        if self.tape is not None:
            self.tape.append((fn, module))

    def g(self, p: nn.Parameter) -> Optional[Tensor]:
        return None if self.input_grad_only else self.net._grad_view(p)

    def on_side(self, fn, *tensors):
        """Run ``fn`` (kernel launches only) on the side stream, ordered after everything queued so far
        on the compute stream.  ``tensors`` are inputs that the compute stream may free afterwards.
        The work is forked in groups of ``side_group`` calls: one event + one stream wait per group instead of per call
        (a cross-stream edge costs ~3.5 us inside a captured graph and ~10 us of host time outside; measured:
        profiles/r02/graph_fork_cost.txt).  Until its group is launched a call keeps its inputs alive by reference."""
        if self.input_grad_only:        # parameter gradients only: nothing to run, nothing to fork
            return
        if self.side is None:
            fn()
            return
        self.side_queue.append((fn, tensors))
        if len(self.side_queue) >= self.side_group:
            self.flush_side()

    def flush_side(self):
        if not self.side_queue:
            return
        queue, self.side_queue = self.side_queue, []
        ev = torch.cuda.Event()
        cur = torch.cuda.current_stream()
        ev.record(cur)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side), ops.stream_scope():
            for fn, _ in queue:
                fn()
        for _, tensors in queue:
            for t in tensors:
                if t is not None:
                    t.record_stream(self.side)

    def join_side(self):
        if self.side is not None:
            self.flush_side()
            cur = torch.cuda.current_stream()
            cur.wait_stream(self.side)

    # -- deferred reductions ------------------------------------------------------------------------------------
    @staticmethod
    def use(node: _Node) -> bool:
        """Mark ``node`` as read by a consumer; True for the first one (forward order) - its backward runs last among
        the consumers', so whatever it writes into ``node.g`` last is the final gradient."""
        first = not node.used
        node.used = True
        return first

    def defer_param(self, src: Tensor, rows: int, ld: int, c: int, dst1: Tensor, dst2: Optional[Tensor] = None,
                    alpha: float = 1.0, src_off: int = 0):
        """dst1 (and dst2) [c] = alpha * sum over ``rows`` rows of ``src`` (row stride ld): now, or with every other such
        reduction of the pass in one launch (flush_params)."""
        if self.input_grad_only:
            return
        if not self.defer:
            ops.param_reduce2(src if src_off == 0 else src.view(-1)[src_off:], None, rows, ld, c, dst1, None, alpha)
            if dst2 is not None:
                ops.axpby(dst1, 1.0, None, 0.0, dst2)
            return
        self.pjobs.append(ops.param_job(src, rows, ld, c, dst1, dst2, alpha, src_off) + (self.pblocks,))
        self.pblocks += (c + 63) // 64

    def flush_params(self):
        if self.pjobs:
            jobs, blocks = self.pjobs, self.pblocks
            self.pjobs, self.pblocks = [], 0
            rows = [v for job in jobs for v in job]
            table = self.net._tables.get(rows, self.net._params()[0].device)
            ops.param_reduce_batch(table, len(jobs), blocks, sum(4 * (j[1] + 1) * j[3] for j in jobs))

    def slabs_for(self, nbytes: int, device) -> Tensor:
        """Split-K slab storage: the stream's workspace when the reduction follows at once, else a slice of the slab arena
        that stays untouched until flush_slabs."""
        if not self.defer:
            return ops.workspace(nbytes, device)
        return self.net._slab_arena().alloc(nbytes)

    def reduce_slabs(self, slabs: Tensor, nsplit: int, n: int, out: Tensor, layout: int = 0, cout: int = 1, taps: int = 1,
                     cin: int = 1, alpha: float = 1.0, more: bool = False):
        """``more``: further jobs on the SAME slab allocation follow (no flush - which rewinds the arena - in between)."""
        units = ops.slab_units(n, layout, taps, cin) if self.defer else 0
        if units == 0 or out.data_ptr() % 16:
            ops.reduce_slabs(slabs, nsplit, n, out, layout=layout, cout=cout, taps=taps, cin=cin, alpha=alpha)
            return
        self.sjobs.append(ops.slab_job(slabs, nsplit, n, out, layout, taps, cin, alpha) + (self.sitems, units))
        self.sitems += units
        self.sbytes += 4 * n * nsplit
        if self.sbytes >= _SLAB_FLUSH_BYTES and not more:
            self.flush_slabs()

    def flush_slabs(self):
        """One reduction launch for every parked weight gradient - on the stream their producers ran on (callers are
        on_side closures) - after which the arena is reused."""
        if self.sjobs:
            jobs, items = self.sjobs, self.sitems
            self.sjobs, self.sitems, self.sbytes = [], 0, 0
            rows = [v for job in jobs for v in job]
            table = self.net._tables.get(rows, self.net._params()[0].device)
            ops.reduce_slabs_batch(table, len(jobs), items, sum(4 * j[2] * (j[1] + 1) for j in jobs))
            self.net._slab_arena().reset()

    def flush_dense(self):
        """Dense_0 weight gradients of the blocks finished since the last flush: ONE GEMM over their (contiguous) columns of
        dtp_all and one scatter into the flat gradient - the per-bucket form of time_embedding.bwd's batched GEMM."""
        pend, self.dense_pending = self.dense_pending, []
        if not pend:
            return
        net, dtp_all, act = self.net, self.dtp_all, self.temb_act.v
        b, total = dtp_all.shape
        kd = act.shape[1]
        lo, hi = min(o for o, _, _ in pend), max(o + c for o, c, _ in pend)
        if hi - lo == sum(c for _, c, _ in pend) and lo % 4 == 0 and ops.gemm_tn_split_supported(hi - lo, kd, b):
            dwcat = net._persist("dwcat", (total, kd))
            ops.gemm_tn_split(hi - lo, kd, b, dtp_all[:, lo:hi], total, act, kd, dwcat[lo:hi], kd, 1)
            rows, first = [], 0
            for o, c, d0 in pend:
                n4 = c * kd // 4
                rows += [dwcat.data_ptr() + 4 * o * kd, self.g(d0.weight).data_ptr(), n4, first]
                first += n4
            ops.copy_batch(net._tables.get(rows, dwcat.device), len(pend), first)
        else:
            for o, c, d0 in pend:
                if o % 4 == 0 and ops.gemm_tn_split_supported(c, kd, b):          # 16-byte aligned column slice
                    ops.gemm_tn_split(c, kd, b, dtp_all[:, o:o + c], total, act, kd, self.g(d0.weight), kd, 1)
                else:
                    ops.gemm_raw(1, 0, c, kd, b, dtp_all[:, o:o + c], total, 0, act, kd, 0, self.g(d0.weight), kd, 0)

    def flush_deferred(self):
        self.on_side(self.flush_slabs)
        self.flush_params()
        self.flush_dense()

    def finish_backward(self):
        """After the last entry of the backward tape: the parked reductions, then the side stream joins."""
        if self.defer and not self.input_grad_only:
            self.flush_deferred()
        self.join_side()

    def gn_backward(self, dy: Tensor, x: Tensor, st, gamma: Tensor, beta: Tensor, dgamma: Tensor, dbeta: Tensor, act: bool,
                    dx: Tensor, accumulate_dx: bool = False, add: Optional[Tensor] = None, add_scale: float = 1.0,
                    drop_p: float = 0.0, seed: int = 0, seed_dev=None, groups: Optional[int] = None,
                    colsum_img: Optional[Tensor] = None, ld_img: int = 0, last_writer_of: Optional[_Node] = None):
        """GroupNorm(+SiLU, dropout) backward; dgamma / dbeta follow from its per-image sums by a deferred reduction.
        ``last_writer_of``: the node whose gradient ``dx`` is, when this call writes it last: if the node's producer wants
        the column sums of that gradient (a bias gradient) and a one-pass kernel takes the shape, they are formed here."""
        b, h, w, c = x.shape
        pa = self.net._param_arena()
        node = last_writer_of
        # large maps with a third operand - and maps above 32x32 in any case - go through the whole-row team kernel unless
        # per-IMAGE column sums are asked for: its sums / column sums come per (image, team member), k rows per image
        k = ops.gn_bwd_team_wanted(b, h * w, c, groups, add is not None or accumulate_dx) if colsum_img is None else 0
        fold = node is not None and node.want_gsum and colsum_img is None and self.gn_bwd_colsum and \
            (k > 0 or ops.gn_bwd_colsum_supported(b, h * w, c, groups))
        rows = b * max(k, 1)
        sums = pa.floats(rows, 2, c)
        if fold:
            colsum_img, ld_img = pa.floats(rows, c), c
        if k:
            ops.gn_bwd_team(dy, x, st, gamma, beta, act, dx, accumulate_dx=accumulate_dx, drop_p=drop_p, seed=seed,
                            groups=groups, add=add, add_scale=add_scale, seed_dev=seed_dev, sums=sums, colsum_rows=colsum_img,
                            ld_rows=ld_img)
        else:
            ops.gn_bwd(dy, x, st, gamma, beta, act, dx, accumulate_dx=accumulate_dx, drop_p=drop_p, seed=seed, groups=groups,
                       add=add, add_scale=add_scale, seed_dev=seed_dev, sums=sums, colsum_img=colsum_img, ld_img=ld_img)
        self.defer_param(sums, rows, 2 * c, c, dbeta)
        self.defer_param(sums, rows, 2 * c, c, dgamma, src_off=c)
        if fold:
            node.gsum = colsum_img

    def bias_from(self, node: _Node, dout: Tensor, bias: nn.Parameter, alpha: float = 1.0,
                  bias2: Optional[nn.Parameter] = None) -> bool:
        """Bias gradient(s) = alpha * column sums of a node's final gradient ``dout``: from the sums its last writer left
        (True: nothing launched now), else by a pass over ``dout`` (False; call it where that pass may run)."""
        gsum, node.gsum = node.gsum, None
        if self.input_grad_only:
            return True
        if gsum is not None:
            self.defer_param(gsum, gsum.shape[0], gsum.shape[1], gsum.shape[1], self.g(bias),
                             self.g(bias2) if bias2 is not None else None, alpha)
            return True
        return False

    def wgrad(self, dy: Tensor, x: Tensor, conv: _Affine, k: int, stride: int, pad: int, alpha: float = 1.0,
              x2: Optional[Tensor] = None, route: Optional[str] = None):
        """dW (OIHW, scaled by alpha) of ``conv`` from the output gradient and the conv's input: split-K partial
        slabs in the stream's workspace, then one deterministic reduction straight into the flat gradient.
        ``x2``: second source when the input is an unmaterialised concatenation (limb kernels only).
        ``route``: the 3x3 stride-1 pad-1 route a block plan chose (score_routes.wgrad_route); None: looked up here."""
        b, oh, ow, cout = dy.shape
        c1 = x.shape[-1]
        c2 = x2.shape[-1] if x2 is not None else 0
        cin = c1 + c2
        taps = k * k
        n = cout * taps * cin
        assert x2 is None or self.split, "two-source weight gradients exist on the limb kernels only"
        if route is None and (k, stride, pad) == (3, 1, 1):
            route = R.wgrad_route(self.split, cout, c1, c2, b, oh, ow, isinstance(x, ops.LimbPlanes))
        if route == R.WINO:
            # Winograd domain (wgrad_wino.hip): 16 limb products per 2x2 tile instead of 36; its own slabs and reduction
            # (G^T . G over 16 positions), written straight into the flat gradient
            # (the stream's workspace: the reduction follows at once, nothing is parked in the slab arena)
            launch = ops.conv3x3_wgrad_wino_x3 if self.a_wgrad == "x3" else ops.conv3x3_wgrad_wino
            launch(dy, cout, x, self.g(conv.weight), x2=x2, alpha=alpha)
            return
        if route == R.LIMB:
            nsplit = R.wgrad_limb_nsplit(cout, cin, b, oh, ow, isinstance(x, ops.LimbPlanes))
            slabs = self.slabs_for(4 * n * nsplit, dy.device)
            ops.conv3x3_wgrad_split(dy, cout, x, slabs, cin, 0, nsplit, x2)
            self.reduce_slabs(slabs, nsplit, n, self.g(conv.weight), layout=1, cout=cout, taps=taps, cin=cin, alpha=alpha)
            return
        pw = R.pointwise_wgrad_route(self.split, cout, c1, c2, b * oh * ow) if (k, stride, pad) == (1, 1, 0) else R.TILE
        if pw != R.TILE:        # (a 1x1 convolution's tile-engine form is conv2d_wgrad_nhwc below, not pw_wgrad's GEMM)
            self.pw_wgrad(pw, cout, c1, b * oh * ow, dy, cout, x, c1, (self.g(conv.weight),), alpha, x2, c2)
            return
        assert x2 is None, "unsupported two-source weight gradient"
        tiles = ((cout + 127) // 128) * ((cin + 127) // 128) * taps
        nsplit = _pick_nsplit(tiles, b * oh * ow)
        slabs = self.slabs_for(4 * n * nsplit, dy.device)
        ops.conv2d_wgrad_nhwc(dy, cout, x, k, k, stride, pad, oh, ow, slabs, cin, 0, nsplit)
        self.reduce_slabs(slabs, nsplit, n, self.g(conv.weight), layout=1, cout=cout, taps=taps, cin=cin, alpha=alpha)

    @staticmethod
    def node_stats(node: _Node, gamma: Tensor, beta: Tensor, groups: Optional[int] = None):
        """GroupNorm statistics of a node: from the producer's partial sums when it left some and the group size is a
        multiple of their 8 channels, else by a pass over the tensor."""
        c = node.v.shape[-1]
        g = groups if groups is not None else ops.gn_groups(c)
        if node.gp is not None and (c // g) % getattr(node.gp, "fine_width", 8) == 0:
            return ops.gn_stats_from_part(node.gp, node.v.shape, gamma, beta, groups=groups)
        return ops.gn_stats(node.v, gamma, beta, groups=groups)

    def part_for(self, b: int, hw: int, c: int, device, limb_kernel: bool):
        """Partial-sum buffer for the epilogue of a limb kernel writing a [b, hw, c] output (None: not applicable)."""
        if self.split and limb_kernel and ops.gn_part_supported(b, hw, c):
            return ops.gn_part_buffer(b, hw, c, device)
        return None

    def bmm(self, ta: int, tb: int, M: int, N: int, K: int, A: Tensor, lda: int, sa: int, B: Tensor, ldb: int, sb: int,
            Cc: Tensor, ldc: int, sc: int, batch: int, alpha: float = 1.0):
        """Batched activation x activation product (attention): the limb kernel R.batched_route names (whole tiles, or the
        last column tile cut short), fp32 engine otherwise and for operands that are not 16-byte aligned."""
        route = R.batched_route(self.split, ta, tb, M, N, K)
        if route != R.TILE and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0:
            launch = ops.bgemm_split if route == R.LIMB else ops.bgemm_split_tail
            launch(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, Cc, ldc, sc, batch, alpha)
        else:
            ops.gemm_raw(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, Cc, ldc, sc, batch,
                         ops.epilogue(alpha=alpha) if alpha != 1.0 else None)

    def bias_grad(self, dy: Tensor, out: Tensor, alpha: float = 1.0, per_image=None, ld: Optional[int] = None,
                  ld_per_image: int = 0):
        """``per_image``: True (or a [b, c] tensor) to also get the per-image sums back; ``ld``: row stride of
        ``dy`` when it is a column slice of a wider buffer."""
        b = dy.shape[0]
        c = dy.shape[-1]
        hw = dy.numel() // (b * c)
        ldx = ld if ld is not None else c
        if c % 4 == 0 and c <= 1024 and ldx % 4 == 0 and dy.data_ptr() % 16 == 0:
            if per_image is True:
                per_image = torch.empty((b, c), device=dy.device, dtype=torch.float32)
            ops.bias_grad(dy, ldx, b, hw, c, out, alpha, per_image, ld_per_image)
            return per_image
        assert ld_per_image in (0, c), "strided per-image sums need the vector path (c % 4 == 0)"
        tmp = per_image if isinstance(per_image, Tensor) else torch.empty((b, c), device=dy.device, dtype=torch.float32)
        ops.colsum(dy, ldx, b, hw, c, tmp)
        ops.colsum(tmp, c, 1, b, c, out, alpha)
        return tmp

    def pick(self, forms) -> str:
        """The first rung of the pass's ladder among the ``forms`` a site has ('x6' under math mode 'f32', where none is used)."""
        return next((a for a in self.arith if a in forms), "x6")

    def pw_arith(self, k1: int, k2: int, m: int, n: int) -> str:
        """The arithmetic of a LIMB pointwise launch [m][k1 + k2] -> [m][n]: the first reduced rung whose policy wants it."""
        for a in self.arith:
            if (a == "f16" and ops.gemm_split_f16_wanted(k1, k2, m, n)) or (a == "x3" and ops.gemm_split_x3_wanted(k1, k2, m, n)):
                return a
        return "x6"

    def wino_dgrad(self, dy: Tensor, frag: Tensor, cin: int, out: Tensor, epi=None):
        """A Winograd data-gradient launch on fragments in the pass's arithmetic; the fp16 form carries its operand shift."""
        if self.a_wino == "f16":
            ops.conv3x3_wino_f16s(dy, None, frag, cin, out, self.gshift, epi, allow_split=True)
        elif self.a_wino == "x3":
            ops.conv3x3_wino_x3(dy, None, frag, cin, out, epi, allow_split=True)
        else:
            ops.conv3x3_wino(dy, None, frag, cin, out, epi, allow_split=True)

    def wino_wanted(self, c1: int, c2: int, b: int, h: int, w: int, cout: int) -> bool:
        """The ONE place the executor asks whether a convolution runs in Winograd form (score_routes.wino_wanted): every
        route lookup and block plan of this executor receives this method."""
        return R.wino_wanted(c1, c2, b, h, w, cout)

    def conv3(self, x: Tensor, conv: _Affine, out: Tensor, epi, x2: Optional[Tensor] = None, route: Optional[str] = None):
        """3x3 stride-1 pad-1 convolution of an NHWC tensor (or of the channel concatenation of x and x2) on ``route``
        (score_routes.conv3_route; None: looked up here)."""
        b, h, w, c = x.shape
        c2 = x2.shape[-1] if x2 is not None else 0
        cout = conv.weight.shape[0]
        if route is None:
            route = R.conv3_route(self.split, c, c2, b, h, w, cout, isinstance(x, ops.LimbPlanes), self.wino_wanted)
        if route == R.WINO:
            a = self.a_wino
            launch = ops.conv3x3_wino_f16 if a == "f16" else ops.conv3x3_wino_x3 if a == "x3" else ops.conv3x3_wino
            launch(x, x2, self.net._wfrag(conv, False, a), cout, out, epi, allow_split=True)      # Winograd F(2x2, 3x3)
        elif route == R.LIMB:
            ops.conv3x3_split(x, x2, self.net._frag(conv, False), cout, out, epi)
        else:
            ops.conv2d_nhwc(x, x2, self.net._packed(conv), cout, 3, 3, 1, 1, 1, h, w, out, epi)

    def conv3_gn(self, x: Tensor, st, x2: Optional[Tensor], st2, conv: _Affine, out: Tensor, epi):
        """SiLU(GroupNorm(.)) + 3x3 convolution in one launch (ops.conv3x3_wino_gn; inference forward only)."""
        cout = conv.weight.shape[0]
        a = self.a_wino
        launch = ops.conv3x3_wino_gn_f16 if a == "f16" else ops.conv3x3_wino_gn_x3 if a == "x3" else ops.conv3x3_wino_gn
        launch(x, st, x2, st2, True, self.net._wfrag(conv, False, a), cout, out, epi, allow_split=True)

    # -- pointwise GEMMs (1x1 shortcuts, NIN projections, the pyramid's im2col GEMM) on a score_routes.pointwise_* route ------
    def pw_fwd(self, route: str, a1: Tensor, a2: Optional[Tensor], m: int, w: PointwiseWeight, y: Tensor, epi):
        """y[m][w.n] = epi([a1 | a2] W^T).  LIMB runs the first reduced form of the pass's ladder that its policy (pw_arith)
        wants, else three limbs (LIMB_TAIL has three limbs only);
        TILE is the tile engine's 1x1 convolution for an "oi" weight (it alone takes a second source), its GEMM for NIN."""
        n = w.n
        if route == R.LIMB_TAIL:
            ops.gemm_split_tail(a1, m, w.frag(tail=True), n, y, epi)
        elif route == R.LIMB:
            a = self.pw_arith(a1.shape[-1], a2.shape[-1] if a2 is not None else 0, m, n)
            launch = ops.gemm_split_f16 if a == "f16" else ops.gemm_split_x3 if a == "x3" else ops.gemm_split
            launch(a1, a2, m, w.frag(arith=a), n, y, epi)
        elif w.kind == "oi":
            ops.conv2d_nhwc(a1, a2, w.w, n, 1, 1, 1, 0, 1, a1.shape[1], a1.shape[2], y, epi)
        else:
            wt, tb, ld = w.tile(False)
            ops.gemm_raw(0, tb, m, n, w.k, a1, w.k, 0, wt, ld, 0, y, n, 0, epi=epi)

    def pw_dgrad(self, route: str, dy: Tensor, m: int, w: PointwiseWeight, dx: Tensor, epi=None, cols=None):
        """dx[m][w.k] = epi(dy[m][w.n] W).  ``cols`` = (lo, hi), limb routes: input channels lo .. hi alone, into a dx that wide
        (one source of an unmaterialised concatenation: a data gradient's fragments are ordered by output-channel tile, so a
        source's share is a contiguous slice of them).  LIMB: the arithmetic by the policy of pw_fwd, on the launch's own width;
        the fp16 form with the pass's operand shift."""
        n = w.k
        if route == R.TILE:
            wt, tb, ld = w.tile(True)
            return ops.gemm_raw(0, tb, m, n, w.n, dy, w.n, 0, wt, ld, 0, dx, n, 0, epi=epi)
        a = self.pw_arith(w.n, 0, m, n if cols is None else cols[1] - cols[0]) if route == R.LIMB else "x6"
        frag = w.frag(True, a, tail=route == R.LIMB_TAIL)
        if cols is not None:
            frag, n = frag[frag.numel() * cols[0] // n:frag.numel() * cols[1] // n], cols[1] - cols[0]
        if route == R.LIMB_TAIL:
            ops.gemm_split_tail(dy, m, frag, n, dx, epi)
        elif a == "f16":        # a data gradient's fp16 form carries the pass's operand shift
            ops.gemm_split_f16s(dy, None, m, frag, n, dx, self.gshift, epi)
        elif a == "x3":
            ops.gemm_split_x3(dy, None, m, frag, n, dx, epi)
        else:
            ops.gemm_split(dy, None, m, frag, n, dx, epi)

    def pw_wgrad(self, route: str, M: int, N: int, K: int, A: Tensor, lda: int, B: Tensor, ldb: int, outs, alpha: float = 1.0,
                 B2: Optional[Tensor] = None, N2: int = 0):
        """alpha * A[K][M]^T [B | B2][K][N + N2] (K = pixels) as split-K slabs, then their reduction into ``outs``: the one
        gradient [M][N + N2], or several that share its columns equally (q | k | v: cut apart by the batched reduction)."""
        nt = N + N2
        nsplit = _pick_nsplit(-(-M // 128) * -(-nt // 128), K) if route == R.TILE else R._tn_split(M, nt, K)
        slabs = self.slabs_for(4 * M * nt * nsplit, A.device)
        if route == R.TILE:
            ops.gemm_tn_splitk(M, nt, K, A, lda, B, ldb, slabs, nsplit)
        elif route == R.LIMB_TAIL:
            ops.gemm_tn_split_tail(M, N, K, A, lda, B, ldb, slabs, nt, nsplit)
        else:
            ops.gemm_tn_split(M, N, K, A, lda, B, ldb, slabs, nt, nsplit, B2, N2, N2)
        if len(outs) == 1:
            return self.reduce_slabs(slabs, nsplit, M * nt, outs[0], alpha=alpha)
        slabs, n = slabs.view(torch.float32), nt // len(outs)
        for i, out in enumerate(outs):
            self.reduce_slabs(slabs[i * n:], nsplit, M * n, out, layout=2, taps=n, cin=nt, alpha=alpha, more=i + 1 < len(outs))

    # -- few-channel 3x3 convolutions (6-channel stem / first pyramid level in, 6-channel head out) as K = 64 GEMMs ----
    # K = 9*6 = 54 does not fit the tile engine's 32-channel chunking, so these convolutions used its scalar-gather
    # fallback (1.3 % of a step for 0.1 % of the FLOPs); an explicit im2col of the few-channel tensor (33 MB at
    # B = 128) turns them into fast-path GEMMs.
    def small_in_weights(self, conv: _Affine) -> Tensor:
        """[cout][64]: the OIHW rows (ci*9 + tap, 54 values) zero-padded."""
        co, ci = conv.weight.shape[0], conv.weight.shape[1]

        def build(prev):
            out = prev if prev is not None else torch.zeros((co, 64), device=conv.weight.device, dtype=torch.float32)
            ops.scale_copy2d(conv.weight.detach(), ci * 9, out, 64, co, ci * 9)
            return out
        return self.net._wcache.get(conv.weight, "small_in", _built_entry, build)

    def small_in_conv(self, x: Tensor, conv: _Affine, stride: int, pad: int, oh: int, ow: int, out: Tensor, epi):
        """Forward of a 3x3 convolution whose input has <= 7 channels; returns the im2col matrix for the wgrad."""
        cols = ops.im2col3x3_small(x, oh, ow, stride, pad)
        m, cout = cols.shape[0], conv.weight.shape[0]
        ops.gemm_raw(0, 1, m, cout, 64, cols, 64, 0, self.small_in_weights(conv), 64, 0, out, cout, 0, 1, epi)
        return cols

    def small_in_wgrad(self, dy: Tensor, cols: Tensor, conv: _Affine, alpha: float = 1.0):
        cout, k = conv.weight.shape[0], conv.weight.shape[1] * 9
        m = cols.shape[0]
        nsplit = _pick_nsplit(((cout + 127) // 128), m)
        slabs = ops.workspace(4 * cout * 64 * (nsplit + 1), dy.device)
        ops.gemm_tn_splitk(cout, 64, m, dy, cout, cols, 64, slabs, nsplit)
        tmp = slabs.view(torch.float32)[nsplit * cout * 64:(nsplit + 1) * cout * 64]
        ops.reduce_slabs(slabs, nsplit, cout * 64, tmp)
        ops.scale_copy2d(tmp, 64, self.g(conv.weight), k, cout, k, alpha)

    def small_out_backward(self, dy: Tensor, a: Tensor, conv: _Affine, da: Tensor):
        """Data and weight gradient of a 3x3 stride-1 pad-1 convolution with <= 7 OUTPUT channels (the head)."""
        co, ci = conv.weight.shape[0], conv.weight.shape[1]
        b, h, w, _ = dy.shape
        cols = ops.im2col3x3_small(dy, h, w, 1, 1, flip=True)            # [M][64], column = co*9 + tap (mirrored)
        m = cols.shape[0]

        def build(prev):                                                  # [ci][co*9 + tap] = w[co][ci][tap]
            out = prev if prev is not None else torch.zeros((ci, 64), device=conv.weight.device, dtype=torch.float32)
            for o in range(co):
                ops.scale_copy2d(conv.weight.detach(), 9, out, 64, ci, 9, src_off=o * ci * 9, dst_off=o * 9)
            return out
        wd = self.net._wcache.get(conv.weight, "small_out", _built_entry, build)
        ops.gemm_raw(0, 1, m, ci, 64, cols, 64, 0, wd, 64, 0, da, ci, 0)

        def side():
            nsplit = _pick_nsplit((ci + 127) // 128, m)
            slabs = ops.workspace(4 * 64 * ci * (nsplit + 1), dy.device)
            ops.gemm_tn_splitk(64, ci, m, cols, 64, a, ci, slabs, nsplit)   # [co*9 + tap][ci]
            tmp = slabs.view(torch.float32)[nsplit * 64 * ci:(nsplit + 1) * 64 * ci]
            ops.reduce_slabs(slabs, nsplit, 64 * ci, tmp)
            ops.reduce_slabs(tmp, 1, co * 9 * ci, self.g(conv.weight), layout=1, cout=co, taps=9, cin=ci)
            self.bias_grad(dy, self.g(conv.bias))
        self.on_side(side, dy, a, cols)

    def dgrad(self, dy: Tensor, conv: _Affine, k: int, stride: int, pad: int, ih: int, iw: int, out: Tensor,
              alpha: float = 1.0, accumulate: bool = False, route: Optional[str] = None):
        """``route``: the 3x3 stride-1 pad-1 route a block plan chose (score_routes.conv3_route of the transposed shape);
        None: looked up here."""
        cin = conv.weight.shape[1]
        epi = ops.epilogue(alpha=alpha, accumulate=accumulate) if (alpha != 1.0 or accumulate) else None
        if route is None and (k, stride, pad) == (3, 1, 1):
            route = R.conv3_route(self.split, dy.shape[-1], 0, dy.shape[0], ih, iw, cin, wino=self.wino_wanted)
        if route == R.WINO:
            self.wino_dgrad(dy, self.net._wfrag(conv, True, self.a_wino), cin, out, epi)        # Winograd F(2x2, 3x3)
            return
        if route == R.LIMB:
            ops.conv3x3_split(dy, None, self.net._frag(conv, True), cin, out, epi)
            return
        wd = self.net._packed(conv, dgrad=True)
        ops.conv2d_nhwc(dy, None, wd, cin, k, k, 1, k - 1 - pad, stride, ih, iw, out, epi)

    def resample(self, x: Tensor, up: bool) -> Tensor:
        if up:
            return ops.upfirdn2d_raw(x, self.k_up, 2, 1, self.pad_up, layout=1)
        return ops.upfirdn2d_raw(x, self.k_down, 1, 2, self.pad_down, layout=1)

    def resample_bwd(self, gy: Tensor, up: bool, in_hw, out: Tensor, accumulate: bool):
        if up:
            ops.upfirdn2d_bwd_raw(gy, self.k_up, 2, 1, self.pad_up, in_hw, 1, out=out, accumulate=accumulate)
        else:
            ops.upfirdn2d_bwd_raw(gy, self.k_down, 1, 2, self.pad_down, in_hw, 1, out=out, accumulate=accumulate)

    def backward(self, grad_out_nchw: Tensor):
        with ops.stream_scope():
            self._backward(grad_out_nchw)

    def _backward(self, grad_out_nchw: Tensor):
        net = self.net
        # the operand shift of this pass's fp16 data gradients: a host integer from the divisor the loss published (consumed here)
        shift = ops.take_grad_shift()
        self.gshift = shift if "f16" in self.arith else 0
        g_out = grad_out_nchw.contiguous()
        self.head_grad.g = g_out if net.is_classifier else ops.nchw_to_nhwc(g_out)
        # every pass: gn_backward and the resblock column sums allocate from the arena whether or not the reductions are
        # deferred (with defer off the offset was never rewound and the buffer doubled until OOM); the previous
        # pass's readers of it are stream-ordered before this pass's writers
        net._param_arena().reset()
        red = net._reducer
        for fn, module in reversed(self.tape):
            fn()
            if module is not None and self.watermark is not None:
                off = net._module_offset(module)
                if self.defer and red is not None and red.would_launch(off):
                    self.flush_deferred()       # a bucket is about to be exchanged: its parked reductions first
                self.flush_side()       # the reducer may launch a bucket now: its gradients must at least be enqueued
                self.watermark(off)
        self.finish_backward()
        self.tape = None

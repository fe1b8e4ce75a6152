"""The NCSN++ forward as a program of libpsld_hip launches over NHWC tensors (and, when recording, the closures of its
backward): time embedding, residual blocks, attention, input pyramid, concatenations, stem and head.  Kernel-level helpers
and the tape machinery come from score_tape.py; which kernel runs each 3x3 convolution and pointwise GEMM from score_routes.py."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import ops
from . import score_routes as R
from .score_modules import NIN, AttnBlockpp, Downsample, ResnetBlockBigGANpp
from .score_tape import _CatNode, _ExecBase, _Node, _fir_kernel, _gbuf
from .score_weights import PointwiseWeight

Tensor = torch.Tensor
_OVERLAP_MAX_PIXELS = 65536     # batch x H x W at the input resolution up to which weight gradients go to a side stream


class _Exec(_ExecBase):
    """One forward (and, if ``record``, the tape of its backward) over NHWC tensors."""

    # -- time embedding (ncsnpp.py:289-313) ------------------------------------------------------
    def time_embedding(self, t: Tensor, lab: Optional[Tensor] = None, drop: Optional[Tensor] = None):
        """``lab`` / ``drop`` (networks with label_classes, NCSNpp._labels): rows of ``label_emb`` and the dropout mask."""
        net = self.net
        mods = net.all_modules
        i = 0
        if net.embedding_type == "fourier":
            emb = ops.time_embed(t, mods[0].W, True)
            i = 1
        else:
            emb = ops.time_embed(t, net._pos_freq(t.device), False)
        if not net.noise_cond:
            self.temb_act = None
            return i
        l1, l2 = mods[i], mods[i + 1]
        t1 = ops.linear(emb, l1.weight, l1.bias)
        s1 = ops.silu(t1)
        temb = ops.linear(s1, l2.weight, l2.bias)
        if lab is not None:
            # the one place the class label enters: temb += label_emb[lab] (row K where the sample runs without a label).
            # Inside a stream capture the labels' range check is the capturer's (NCSNpp._graph_forward)
            ops.label_embed_add(temb, net.label_emb.detach(), lab, drop, verify=not torch.cuda.is_current_stream_capturing())
        st = _Node(ops.silu(temb))
        self.temb_act = st
        b = t.shape[0]
        # Dense_0(act(temb)) of EVERY ResBlock in one GEMM against the gathered projection weights
        # (layerspp.py:262-263 runs one small Linear per block); the blocks read column slices of tp_all
        plan = net._temb_plan()
        self.tp_all = self.dtp_all = None
        if plan is not None:
            wcat, bcat, self.temb_offsets = plan
            total = wcat.shape[0]
            self.tp_all = torch.empty((b, total), device=t.device, dtype=torch.float32)
            ops.gemm_raw(0, 1, b, total, wcat.shape[1], st.v, wcat.shape[1], 0, wcat, wcat.shape[1], 0, self.tp_all,
                         total, 0, 1, ops.epilogue(bias=bcat))
            if self.record:
                # persistent (same address every step: the batched reduction tables hold pointers into it); written and
                # read inside ONE backward pass, so forward passes whose backward is still pending can share it
                self.dtp_all = net._persist("dtp_all", (b, total))
        tp_all, dtp_all = self.tp_all, self.dtp_all
        # Dense_0's weight gradients of ALL blocks as one GEMM dtp_all^T act(temb) at the end of the pass (57 eight-workgroup
        # launches of ~10 us otherwise) - unless a bucket reducer needs each block's gradients final at its own watermark
        # With a reducer (and no side stream) the same GEMM runs once per BUCKET, over the columns of the blocks finished since
        # the last one (flush_dense, called with the other parked reductions before a bucket is exchanged).
        self.dense_ok = self.dtp_all is not None and self.defer and self.split and \
            ops.gemm_tn_split_supported(total, wcat.shape[1], b)
        self.dense_batched = self.dense_ok and net._reducer is None
        dense_batched = self.dense_batched

        def bwd():
            if self.input_grad_only:    # t gets no gradient: the whole chain from here ends in parameters
                return
            self.join_side()            # every block wrote its slice of dtp_all / accumulated into st.g
            if dense_batched:
                kd = wcat.shape[1]
                dwcat = net._persist("dwcat", (total, kd))
                ops.gemm_tn_split(total, kd, b, dtp_all, total, st.v, kd, dwcat, kd, 1)
                rows, first = [], 0
                for m_, o in self.temb_offsets.items():
                    w_ = m_.Dense_0.weight
                    n4 = w_.numel() // 4
                    rows += [dwcat.data_ptr() + 4 * o * kd, self.g(w_).data_ptr(), n4, first]
                    first += n4
                ops.copy_batch(net._tables.get(rows, dwcat.device), len(self.temb_offsets), first)
            if dtp_all is not None:     # d act(temb) = sum over blocks dtp_i W_i = dtp_all Wcat: one GEMM
                gb, acc = _gbuf(st)
                kd = wcat.shape[1]
                # M = batch is one tile tall and K = sum of the blocks' C_out is long (14592 for C10): cut K into
                # ranges that run as the batches of one launch, then add the partial products in range order
                ks = next((k for k in (256, 128, 64) if total % k == 0), 0)
                if not acc and ks and total // ks >= 8 and (b * kd) % 4 == 0:
                    ns = total // ks
                    slabs = ops.workspace(4 * ns * b * kd, dtp_all.device).view(torch.float32)
                    ops.gemm_raw(0, 0, b, kd, ks, dtp_all, total, ks, wcat, kd, ks * kd, slabs, kd, b * kd, ns)
                    ops.reduce_slabs(slabs, ns, b * kd, gb)
                else:
                    ops.gemm_raw(0, 0, b, kd, total, dtp_all, total, 0, wcat, kd, 0, gb, kd, 0,
                                 epi=ops.epilogue(accumulate=True) if acc else None)
            if st.g is None:
                return
            dtemb = ops.silu_bwd(temb, st.g)
            n2, k2 = l2.weight.shape
            ops.gemm_raw(1, 0, n2, k2, b, dtemb, n2, 0, s1, k2, 0, self.g(l2.weight), k2, 0)
            ops.colsum(dtemb, n2, 1, b, n2, self.g(l2.bias))
            if lab is not None:         # every row of the table is written: rows without a sample get zeros
                ops.label_embed_grad(dtemb, lab, drop, self.g(net.label_emb), verify=False)
            ds1 = torch.empty_like(s1)
            ops.gemm_raw(0, 0, b, k2, n2, dtemb, n2, 0, l2.weight, k2, 0, ds1, k2, 0)
            dt1 = ops.silu_bwd(t1, ds1)
            n1, k1 = l1.weight.shape
            ops.gemm_raw(1, 0, n1, k1, b, dt1, n1, 0, emb, k1, 0, self.g(l1.weight), k1, 0)
            ops.colsum(dt1, n1, 1, b, n1, self.g(l1.bias))

        self.push(bwd, l1)
        return i + 2

    # -- ResnetBlockBigGANpp.forward (layerspp.py:242-274) -------------------------------------------
    def resblock(self, x, mod: ResnetBlockBigGANpp) -> _Node:
        """``x``: a node, or a _CatNode (see concat): then every consumer below reads the two sources side by side."""
        net, s = self.net, self.s
        gn0, gn1 = mod.GroupNorm_0, mod.GroupNorm_1
        xb: Optional[_Node] = None
        if isinstance(x, _CatNode):
            x, xb = x.a, x.b
        xb_v = xb.v if xb is not None else None
        first_x = self.use(x)
        first_xb = self.use(xb) if xb is not None else False
        b, h, w, c1 = x.v.shape
        cin = c1 + (xb.v.shape[-1] if xb is not None else 0)
        cout = mod.out_ch
        up, down = mod.up, mod.down
        a0b, st0b, g1, g2 = None, None, None, None
        if xb is None:
            st0 = self.node_stats(x, gn0.weight, gn0.bias)
        else:
            # GroupNorm over the concatenation = each source normalised over its own share of the groups
            cpg = cin // ops.gn_groups(cin)
            g1, g2 = c1 // cpg, (cin - c1) // cpg
            gam, bet = gn0.weight.detach(), gn0.bias.detach()
            st0 = self.node_stats(x, gam[:c1], bet[:c1], groups=g1)
            st0b = self.node_stats(xb, gam[c1:], bet[c1:], groups=g2)
        # Every kernel choice of the block, made once (score_routes.block_plan).  Where the direct limb kernels run a
        # convolution, its activations go to it as bf16 LIMB PLANES: GroupNorm's apply pass writes them already split (6 B
        # per element instead of 4), the forward convolution stages its halo tile by LDS-DMA with no split in the MFMA
        # kernel and the weight gradient stages its x operand without one (ops.conv3x3_split / conv3x3_wgrad_split on
        # LimbPlanes; both bitwise the fp32-input result).  Inference forward (no tape): GroupNorm's apply pass + SiLU
        # run inside the Winograd convolution's input staging where that pays - the activated tensor is needed nowhere else.
        ho, wo = (h // 2, w // 2) if down else ((h * 2, w * 2) if up else (h, w))
        plan = R.block_plan(self.split, self.limb_planes, self.record, self.drop_p > 0, c1, cin - c1, b, h, w, cout, up, down,
                            self.wino_wanted, mod.has_shortcut)
        fuse0, fuse1 = plan.conv0 == R.WINO_GN, plan.conv1 == R.WINO_GN
        apply0 = ops.gn_apply_limb if plan.lp0 else ops.gn_apply
        a0 = None
        if not fuse0:
            if xb is not None:
                a0b = apply0(xb.v, st0b, True)
            a0 = apply0(x.v, st0, True)
        if fuse0:
            a0r, xr = None, x.v
        elif up or down:
            a0r = self.resample(a0, up)
            xr = self.resample(x.v, up)
            del a0
        else:
            a0r, xr = a0, x.v
        tp, tp_ld, tp_off = None, 0, None
        if self.temb_act is not None:
            tp_off = self.temb_offsets[mod] if self.tp_all is not None else None
            if tp_off is not None:
                tp, tp_ld = self.tp_all[:, tp_off:tp_off + cout], self.tp_all.shape[1]
            else:
                tp = ops.linear(self.temb_act.v, mod.Dense_0.weight, mod.Dense_0.bias)
        h1 = torch.empty((b, ho, wo, cout), device=x.v.device, dtype=torch.float32)
        h1p = ops.gn_part_buffer(b, ho * wo, cout, h1.device) if plan.part0 else None
        epi0 = ops.epilogue(bias=mod.Conv_0.bias, rowbias=tp, rows_per_img=ho * wo, ld_rowbias=tp_ld, gn_part=h1p, gn_hw=ho * wo)
        if fuse0:
            self.conv3_gn(x.v, st0, xb_v, st0b, mod.Conv_0, h1, epi0)
        else:
            self.conv3(a0r, mod.Conv_0, h1, epi0, x2=a0b, route=plan.conv0)
        st1 = self.node_stats(_Node(h1, h1p), gn1.weight, gn1.bias)
        drop_p, seed, seed_dev = 0.0, 0, None
        if self.drop_p > 0:
            drop_p = self.drop_p
            self.n_drop += 1
            seed = (self.n_drop * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
            seed_dev = self.seed_dev
        a1 = None if fuse1 else \
            (ops.gn_apply_limb if plan.lp1 else ops.gn_apply)(h1, st1, True, drop_p=drop_p, seed=seed, seed_dev=seed_dev)
        out = torch.empty((b, ho, wo, cout), device=x.v.device, dtype=torch.float32)
        if mod.has_shortcut:
            w2 = PointwiseWeight(net, mod.Conv_2.weight, cout, cin, "oi")
            self.pw_fwd(plan.shortcut, xr, xb_v, b * ho * wo, w2, out, ops.epilogue(bias=mod.Conv_2.bias))
            res = out
        else:
            res = xr
        outp = ops.gn_part_buffer(b, ho * wo, cout, out.device) if plan.part1 else None
        epi1 = ops.epilogue(bias=mod.Conv_1.bias, residual=res, ld_residual=cout, out_scale=s, gn_part=outp, gn_hw=ho * wo)
        if fuse1:
            self.conv3_gn(h1, st1, None, None, mod.Conv_1, out, epi1)
        else:
            self.conv3(a1, mod.Conv_1, out, epi1, route=plan.conv1)
        on = _Node(out, outp, want_gsum=True)       # Conv_1.bias (and Conv_2.bias) = s * column sums of its gradient
        if not self.record:
            return on
        temb_act = self.temb_act
        dtp_all = self.dtp_all
        xr_saved = xr if mod.has_shortcut else None

        def bwd():
            dout = on.g
            on.g = None
            # Conv_1 / Conv_2 bias: s * column sums of dout - left behind by the last writer of dout where that was a
            # one-pass GroupNorm backward, else a pass over dout on the side stream
            have_bias = self.bias_from(on, dout, mod.Conv_1.bias, s, mod.Conv_2.bias if mod.has_shortcut else None)

            # Conv_1 (the 1/sqrt(2) of skip_rescale is folded into alpha); parameter gradients on the side stream
            def side1():
                self.wgrad(dout, a1, mod.Conv_1, 3, 1, 1, alpha=s, route=plan.wgrad1)
                if not have_bias:
                    self.bias_grad(dout, self.g(mod.Conv_1.bias), alpha=s)
                if mod.has_shortcut:
                    self.wgrad(dout, xr_saved, mod.Conv_2, 1, 1, 0, alpha=s, x2=xb_v)
                    if not have_bias:
                        # Conv_2.bias sees the same output gradient as Conv_1.bias: copy the sum just computed
                        ops.axpby(self.g(mod.Conv_1.bias), 1.0, None, 0.0, self.g(mod.Conv_2.bias))

            self.on_side(side1, dout, a1, xr_saved, xb_v)
            da1 = torch.empty_like(h1)
            self.dgrad(dout, mod.Conv_1, 3, 1, 1, ho, wo, da1, alpha=s, route=plan.dgrad1)
            dh1 = torch.empty_like(h1)
            # Conv_0's bias gradient and the per-image sums of dh1 (the time-embedding gradient) as a by-product of the
            # GroupNorm backward that writes dh1 (no pass over dh1), where its one-pass kernels take the shape
            csum = self.gn_bwd_colsum and ops.gn_bwd_colsum_supported(b, ho * wo, cout)
            per_img, ldp = None, 0
            if csum:
                if temb_act is not None and tp_off is not None and dtp_all is not None:
                    per_img, ldp = dtp_all[:, tp_off:tp_off + cout], dtp_all.shape[1]
                else:
                    per_img, ldp = net._param_arena().floats(b, cout), cout
            self.gn_backward(da1, h1, st1, gn1.weight, gn1.bias, self.g(gn1.weight), self.g(gn1.bias), True, dh1,
                             drop_p=drop_p, seed=seed, seed_dev=seed_dev, colsum_img=per_img, ld_img=ldp)
            if csum:        # Conv_0.bias = sum over the batch of the per-image sums = Dense_0.bias
                self.defer_param(per_img, b, ldp, cout, self.g(mod.Conv_0.bias),
                                 self.g(mod.Dense_0.bias) if temb_act is not None else None)
            dtp_pre = per_img
            del da1

            # Conv_0 + time-embedding bias
            def side0():
                self.wgrad(dh1, a0r, mod.Conv_0, 3, 1, 1, x2=a0b, route=plan.wgrad0)
                if temb_act is None:
                    if not csum:
                        self.bias_grad(dh1, self.g(mod.Conv_0.bias))
                    return
                d0 = mod.Dense_0
                kd = d0.weight.shape[1]
                if tp_off is not None and dtp_all is not None:
                    # per-image sums straight into this block's columns of dtp_all; its share of d act(temb) is added
                    # by ONE GEMM over all blocks at the end (time_embedding.bwd)
                    ldt = dtp_all.shape[1]
                    dtp = dtp_all[:, tp_off:tp_off + cout]
                    if not csum:
                        self.bias_grad(dh1, self.g(mod.Conv_0.bias), per_image=dtp, ld_per_image=ldt)
                    if self.dense_batched:
                        pass                # one GEMM over all blocks at the end (time_embedding.bwd)
                    elif self.dense_ok and self.side is None and ops.gemm_tn_split_supported(cout, kd, b):
                        self.dense_pending.append((tp_off, cout, d0))       # one GEMM per gradient bucket (flush_dense)
                    elif self.split and ops.gemm_tn_split_supported(cout, kd, b) and dtp.data_ptr() % 16 == 0:
                        # one "slab" = the gradient itself: K = batch is short enough for a single range
                        ops.gemm_tn_split(cout, kd, b, dtp, ldt, temb_act.v, kd, self.g(d0.weight), kd, 1)
                    else:
                        ops.gemm_raw(1, 0, cout, kd, b, dtp, ldt, 0, temb_act.v, kd, 0, self.g(d0.weight), kd, 0)
                else:
                    dtp = dtp_pre if csum else self.bias_grad(dh1, self.g(mod.Conv_0.bias), per_image=True)
                    ops.gemm_raw(1, 0, cout, kd, b, dtp, cout, 0, temb_act.v, kd, 0, self.g(d0.weight), kd, 0)
                    gb, acc = _gbuf(temb_act)
                    ops.gemm_raw(0, 0, b, kd, cout, dtp, cout, 0, d0.weight, kd, 0, gb, kd, 0,
                                 epi=ops.epilogue(accumulate=True) if acc else None)
                if not csum:
                    # d Dense_0.bias = sum over the batch of dtp = the conv bias gradient just computed
                    ops.axpby(self.g(mod.Conv_0.bias), 1.0, None, 0.0, self.g(d0.bias))

            self.on_side(side0, dh1, a0r, a0b)
            if xb is not None:
                self._resblock_cat_bwd(mod, w2, x, xb, dout, dh1, st0, st0b, g1, g2, first_x, first_xb, plan.dgrad0)
                return
            da0r = torch.empty((b, ho, wo, cin), device=dout.device, dtype=torch.float32)
            self.dgrad(dh1, mod.Conv_0, 3, 1, 1, ho, wo, da0r, route=plan.dgrad0[0])
            # (no `del dh1`: side0 above may still be waiting for its fork and looks the name up when it runs)
            xg, acc = _gbuf(x)
            identity = False
            if mod.has_shortcut:
                if up or down:
                    dxr = torch.empty((b, ho, wo, cin), device=dout.device, dtype=torch.float32)
                    self.pw_dgrad(plan.shortcut_dgrad, dout, b * ho * wo, w2, dxr, ops.epilogue(alpha=s))
                    self.resample_bwd(dxr, up, (h, w), xg, acc)
                    del dxr
                else:
                    self.pw_dgrad(plan.shortcut_dgrad, dout, b * ho * wo, w2, xg, ops.epilogue(alpha=s, accumulate=acc))
            else:
                identity = True          # out = (x + h)/sqrt(2): the x branch's gradient s*dout rides on GroupNorm_0's backward
            if up or down:
                da0 = torch.empty((b, h, w, cin), device=dout.device, dtype=torch.float32)
                self.resample_bwd(da0r, up, (h, w), da0, False)
            else:
                da0 = da0r
            # this block read x first (forward order): its GroupNorm_0 backward writes x's gradient last
            self.gn_backward(da0, x.v, st0, gn0.weight, gn0.bias, self.g(gn0.weight), self.g(gn0.bias), True, xg,
                             accumulate_dx=not identity or acc, add=dout if identity else None, add_scale=s,
                             last_writer_of=x if first_x else None)

        self.push(bwd, mod)
        return on

    def _resblock_cat_bwd(self, mod, w2: PointwiseWeight, xa: _Node, xb: _Node, dout: Tensor, dh1: Tensor, sta, stb, g1: int,
                          g2: int, first_a: bool, first_b: bool, routes):
        """Input side of the backward of a residual block fed by an unmaterialised concatenation: the data gradients
        of Conv_0 and of the 1x1 shortcut are computed per source (the fragments of a data gradient are ordered by
        output-channel tile, so each source's share is a contiguous slice) and GroupNorm_0's backward runs per source
        over its groups; everything accumulates straight into the two sources' gradient buffers.  ``w2``: the shortcut's
        weight (score_routes.cat_ok: its data gradient runs on the full-tile limb kernels); ``routes``: the plan's per-source
        routes of Conv_0's data gradient (both Winograd or both direct: one fragment buffer is sliced)."""
        net, s = self.net, self.s
        gn0 = mod.GroupNorm_0
        b, h, w, cout = dout.shape
        m = b * h * w
        c1 = xa.v.shape[-1]
        cin = c1 + xb.v.shape[-1]
        wino = routes[0] == R.WINO
        # [cin/128 tiles][...]: data gradient of the 3x3 (Winograd fragments carry read-ahead padding at the end)
        a = self.a_wino if wino else "x6"       # two-limb / fp16 fragments are sliced the same way
        f3 = net._wfrag(mod.Conv_0, True, a) if wino else net._frag(mod.Conv_0, True)
        cut3 = (f3.numel() - (R.WINO_FRAG_PAD_BYTES if wino else 0)) * c1 // cin
        gam, bet = gn0.weight.detach(), gn0.bias.detach()
        dgam, dbet = self.g(gn0.weight), self.g(gn0.bias)
        cut = (lambda t, lo, hi: t[lo:hi]) if dgam is not None else (lambda t, lo, hi: None)    # (input-gradient-only: none)
        for node, lo, hi, fr3, st, g, first, route in ((xa, 0, c1, f3[:cut3], sta, g1, first_a, routes[0]),
                                                      (xb, c1, cin, f3[cut3:], stb, g2, first_b, routes[1])):
            c = hi - lo
            xg, acc = _gbuf(node)
            self.pw_dgrad(R.LIMB, dout, m, w2, xg, ops.epilogue(alpha=s, accumulate=acc), cols=(lo, hi))
            da0 = torch.empty_like(node.v)
            if route == R.WINO:
                self.wino_dgrad(dh1, fr3, c, da0)
            else:
                ops.conv3x3_split(dh1, None, fr3, c, da0)
            self.gn_backward(da0, node.v, st, gam[lo:hi], bet[lo:hi], cut(dgam, lo, hi), cut(dbet, lo, hi), True, xg,
                             accumulate_dx=True, groups=g, last_writer_of=node if first else None)

    # -- AttnBlockpp.forward (layerspp.py:75-91) -----------------------------------------------------
    def attn(self, x: _Node, mod: AttnBlockpp) -> _Node:
        s = self.s
        b, h, w, c = x.v.shape
        hw = h * w
        m = b * hw
        dev = x.v.device
        gn = mod.GroupNorm_0
        first_x = self.use(x)
        st = self.node_stats(x, gn.weight, gn.bias)
        hn = ops.gn_apply(x.v, st, False)
        n0, n1, n2, n3 = mod.NIN_0, mod.NIN_1, mod.NIN_2, mod.NIN_3
        scale = float(int(c) ** (-0.5))
        plan = R.attn_plan(self.split, c, m)
        # (weight, output) of the projections of hn.  Limb kernels: q|k|v come from ONE GEMM against the concatenated
        # projections (N = 3c) into one buffer; tile engine: one GEMM and one buffer each
        if plan.fused:
            wq = PointwiseWeight(self.net, mod, 3 * c, c, "qkv", self.net._qkv_frags(mod))
            qkv = torch.empty((b, hw, 3 * c), device=dev, dtype=torch.float32)
            proj = [(wq, qkv, wq.qkv[2])]
            q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
        else:
            proj = [(PointwiseWeight(self.net, nin.W, c, c, "io"), torch.empty((b, hw, c), device=dev, dtype=torch.float32), nin.b)
                    for nin in (n0, n1, n2)]
            q, k, v = (y for _, y, _ in proj)
        ld = q.stride(-2)       # 3c or c
        for wp, y, bias in proj:
            self.pw_fwd(plan.route, hn, None, m, wp, y, ops.epilogue(bias=bias))
        ho = torch.empty((b, hw, c), device=dev, dtype=torch.float32)
        if self.split and self.fused_attn and ops.attn_fwd_supported(hw, c):
            # QK^T -> softmax -> PV in ONE kernel: the [B, HW, HW] scores never reach HBM; the probabilities are written
            # only when a backward pass will read them
            p = torch.empty((b, hw, hw), device=dev, dtype=torch.float32) if self.record else None
            ops.attn_fwd(q, k, v, ld, b, hw, c, scale, ho, p)
        else:
            p = torch.empty((b, hw, hw), device=dev, dtype=torch.float32)
            self.bmm(0, 1, hw, hw, c, q, ld, hw * ld, k, ld, hw * ld, p, hw, hw * hw, b, scale)
            ops.softmax_rows(p, p, b * hw, hw)
            self.bmm(0, 0, hw, c, hw, p, hw, hw * hw, v, ld, hw * ld, ho, c, hw * c, b)
        out = torch.empty_like(x.v)
        outp = self.part_for(b, hw, c, dev, plan.route == R.LIMB)       # (the tail launch leaves no GroupNorm partial sums)
        epi_out = ops.epilogue(bias=n3.b, residual=x.v, ld_residual=c, out_scale=s, gn_part=outp, gn_hw=hw)
        w3 = PointwiseWeight(self.net, n3.W, c, c, "io")
        self.pw_fwd(plan.route, ho, None, m, w3, out, epi_out)
        on = _Node(out, outp, want_gsum=True)       # NIN_3.b = s * column sums of its gradient
        if not self.record:
            return on

        def nin_wgrad(a_in: Tensor, dy: Tensor, nin: NIN, alpha: float, ldd: int, bias: bool = True):
            # dW[in,out] = a_in^T dy  (K = B*HW -> split-K slabs); dy may be a column slice (row stride ldd)
            self.pw_wgrad(plan.wgrad, c, c, m, a_in, c, dy, ldd, (self.g(nin.W),), alpha)
            if bias:
                self.bias_grad(dy.view(b, hw, 1, c) if ldd == c else dy, self.g(nin.b), alpha=alpha, ld=ldd)

        def bwd():
            dout = on.g
            on.g = None
            have_b3 = self.bias_from(on, dout, n3.b, s)
            self.on_side(lambda: nin_wgrad(ho, dout, n3, s, c, bias=not have_b3), ho, dout)
            dho = torch.empty_like(ho)
            self.pw_dgrad(plan.route, dout, m, w3, dho, ops.epilogue(alpha=s))
            # dP = dho v^T ; dv = P^T dho
            dp = torch.empty_like(p)
            self.bmm(0, 1, hw, hw, c, dho, c, hw * c, v, ld, hw * ld, dp, hw, hw * hw, b)
            dproj = [torch.empty_like(y) for _, y, _ in proj]
            dqkv = dproj[0]             # (the [m][3c] buffer, where there is one)
            dq, dk, dv = (dqkv[..., :c], dqkv[..., c:2 * c], dqkv[..., 2 * c:]) if plan.fused else dproj
            self.bmm(1, 0, hw, c, hw, p, hw, hw * hw, dho, c, hw * c, dv, ld, hw * ld, b)
            ds = dp
            ops.softmax_rows_bwd(p, dp, ds, b * hw, hw)
            self.bmm(0, 0, hw, c, hw, ds, hw, hw * hw, k, ld, hw * ld, dq, ld, hw * ld, b, scale)
            self.bmm(1, 0, hw, c, hw, ds, hw, hw * hw, q, ld, hw * ld, dk, ld, hw * ld, b, scale)
            dhn = torch.empty_like(hn)
            # q / k / v bias gradients: ONE column-sum pass over the [m, 3c] gradient buffer, written to the three parameters
            seg = plan.fused and 3 * c <= 1024
            if seg:
                self.on_side(lambda: ops.bias_grad_seg(dqkv, 3 * c, b, hw, (self.g(n0.b), self.g(n1.b), self.g(n2.b)), c), dqkv)
            # ... and their weight gradients from ONE GEMM hn^T [dq | dk | dv] (N = 3c: hn is staged and split once instead
            # of three times); the batched slab reduction cuts the [c][3c] result into the three parameters
            if plan.qkv_one and self.defer:
                self.on_side(lambda: self.pw_wgrad(plan.qkv_wgrad, c, 3 * c, m, hn, c, dqkv, 3 * c,
                                                   (self.g(n0.W), self.g(n1.W), self.g(n2.W))), hn, dqkv)
                if not seg:
                    for nin, d in ((n0, dq), (n1, dk), (n2, dv)):
                        self.on_side(lambda nin=nin, d=d: self.bias_grad(d, self.g(nin.b), ld=ld), d)
            else:
                for nin, d in ((n0, dq), (n1, dk), (n2, dv)):
                    self.on_side(lambda nin=nin, d=d: nin_wgrad(hn, d, nin, 1.0, ld, bias=not seg), hn, d)
            for i, ((wp, _, _), d) in enumerate(zip(proj, dproj)):     # (three accumulating launches on the tile engine)
                self.pw_dgrad(plan.route, d, m, wp, dhn, ops.epilogue(accumulate=True) if i else None)
            xg, acc = _gbuf(x)
            self.gn_backward(dhn, x.v, st, gn.weight, gn.bias, self.g(gn.weight), self.g(gn.bias), False, xg,
                             accumulate_dx=acc, add=dout, add_scale=s, last_writer_of=x if first_x else None)

        self.push(bwd, mod)
        return on

    # -- progressive_input == 'residual' (ncsnpp.py:350-357; layerspp.py:149-163) ---------------------
    def pyramid(self, pyr, h: _Node, mod: Downsample, first: bool) -> _Node:
        """pyr: NCHW input tensor (first level) or the previous combined node (NHWC)."""
        s = self.s
        conv = mod.conv
        cout = mod.out_ch
        self.use(h)
        if not first:
            self.use(pyr)
        if mod.fir:
            k = _fir_kernel(self.net.sf.fir_kernel)
            pad = (2, 2)  # up_or_down_sampling.py:173-176: p = (4-2) + (3-1)
            if first:
                xf = ops.nchw_to_nhwc(ops.upfirdn2d_raw(pyr, k, 1, 1, pad, layout=0))
            else:
                xf = ops.upfirdn2d_raw(pyr.v, k, 1, 1, pad, layout=1)
        else:
            raise NotImplementedError("progressive_input='residual' with fir=False is not on the north-star path")
        b, fh, fw, cin = xf.shape
        oh, ow = (fh - 3) // 2 + 1, (fw - 3) // 2 + 1
        out = torch.empty((b, oh, ow, cout), device=xf.device, dtype=torch.float32)
        epi = ops.epilogue(bias=conv.bias, residual=h.v, ld_residual=cout, out_scale=s)
        cols = None
        m = b * oh * ow
        # many-channel levels on the limb kernels: explicit im2col (K order = the packed OHWI weights') + pointwise GEMM
        small, limb, r_fwd, r_bwd = R.pyramid_plan(self.split, cin, cout, m)
        wp = PointwiseWeight(self.net, conv, cout, 9 * cin, "ohwi")
        if small:
            cols = self.small_in_conv(xf, conv, 2, 0, oh, ow, out, epi)
        elif limb:
            patches = ops.im2col3x3(xf, 2, 0, oh, ow)
            self.pw_fwd(r_fwd, patches, None, m, wp, out, epi)
            del patches
        else:
            ops.conv2d_nhwc(xf, None, self.net._packed(conv), cout, 3, 3, 2, 0, 1, oh, ow, out, epi)
        on = _Node(out, want_gsum=True)             # conv.bias = s * column sums of its gradient
        if not self.record:
            return on

        def bwd():
            dout = on.g
            on.g = None
            have_bias = self.bias_from(on, dout, conv.bias, s)
            hg, acc = _gbuf(h)
            ops.axpby(dout, s, None, 0.0, hg, accumulate=acc)
            def side():
                if small:
                    self.small_in_wgrad(dout, cols, conv, alpha=s)
                else:
                    self.wgrad(dout, xf, conv, 3, 2, 0, alpha=s)
                if not have_bias:
                    self.bias_grad(dout, self.g(conv.bias), alpha=s)

            self.on_side(side, dout, xf)
            if not first:
                dxf = torch.empty_like(xf)
                if limb:
                    dpatches = torch.empty((m, 9 * cin), device=dout.device, dtype=torch.float32)
                    self.pw_dgrad(r_bwd, dout, m, wp, dpatches, ops.epilogue(alpha=s))
                    ops.col2im3x3(dpatches, xf.shape, 2, 0, oh, ow, out=dxf)
                    del dpatches
                else:
                    self.dgrad(dout, conv, 3, 2, 0, fh, fw, dxf, alpha=s)
                pg, pacc = _gbuf(pyr)
                ops.upfirdn2d_bwd_raw(dxf, k, 1, 1, pad, (pyr.v.shape[1], pyr.v.shape[2]), 1, out=pg, accumulate=pacc)
            elif self.want_dx:
                # first level reads the network input itself (NCHW): conv dgrad -> NCHW -> FIR backward
                dxf = torch.empty_like(xf)
                self.dgrad(dout, conv, 3, 2, 0, fh, fw, dxf, alpha=s)
                dxf_nchw = ops.nhwc_to_nchw(dxf)
                acc = self.dx_nchw is not None
                if not acc:
                    self.dx_nchw = torch.empty_like(pyr)
                ops.upfirdn2d_bwd_raw(dxf_nchw, k, 1, 1, pad, (pyr.shape[2], pyr.shape[3]), 0, out=self.dx_nchw,
                                      accumulate=acc)

        self.push(bwd, mod)
        return on

    def _cat_ok(self, a: _Node, bnode: _Node, mod) -> bool:
        """Can ``mod`` (a residual block) consume the concatenation of a and b without it being materialised?"""
        if not isinstance(mod, ResnetBlockBigGANpp):
            return False
        b, h, w, c1 = a.v.shape
        return R.cat_ok(self.split, self.record, c1, bnode.v.shape[-1], b, h, w, mod.out_ch, mod.up, mod.down,
                        mod.has_shortcut, self.wino_wanted)

    def concat(self, a: _Node, bnode: _Node, consumer=None):
        """torch.cat([h, hs.pop()], dim=1) (ncsnpp.py:374) in NHWC; not materialised when ``consumer`` reads two sources."""
        if consumer is not None and self._cat_ok(a, bnode, consumer):
            return _CatNode(a, bnode)
        self.use(a)
        self.use(bnode)
        b, h, w, c1 = a.v.shape
        c2 = bnode.v.shape[-1]
        rows = b * h * w
        cat = torch.empty((b, h, w, c1 + c2), device=a.v.device, dtype=torch.float32)
        ops.copy2d(a.v, c1, cat, c1 + c2, rows, c1)
        ops.copy2d(bnode.v, c2, cat, c1 + c2, rows, c2, dst_off=c1)
        cn = _Node(cat)
        if self.record:
            def bwd():
                g = cn.g
                cn.g = None
                ga, acc = _gbuf(a)
                ops.copy2d(g, c1 + c2, ga, c1, rows, c1, accumulate=acc)
                gb, acc = _gbuf(bnode)
                ops.copy2d(g, c1 + c2, gb, c2, rows, c2, accumulate=acc, src_off=c1)

            self.push(bwd)
        return cn

    # -- whole network (ncsnpp.py:287-438) --------------------------------------------------------------
    def run(self, x: Tensor, t: Tensor, lab: Optional[Tensor] = None, drop: Optional[Tensor] = None) -> Tensor:
        with ops.stream_scope():
            return self._run(x, t, lab, drop)

    def _run(self, x: Tensor, t: Tensor, lab: Optional[Tensor] = None, drop: Optional[Tensor] = None) -> Tensor:
        net = self.net
        mods = net.all_modules
        mi = self.time_embedding(t, lab, drop)
        pin = net.progressive_input
        x_nhwc = ops.nchw_to_nhwc(x)
        stem = mods[mi]
        mi += 1
        b, hh, ww, _ = x_nhwc.shape
        if self.record:
            # Parameter-gradient kernels on a side stream.  Automatic rule: on while the kernels of the backward chain
            # cannot fill the chip by themselves (32x32 images: B = 16 +9 %, B = 32 +5 %, B = 64 +1.3 %, B = 128 +0.3 % images/s - and per-kernel HIP
            # event timings would be inflated by the concurrent MFMA kernel: off there)
            use = net.overlap_wgrad if net.overlap_wgrad is not None else (b * hh * ww <= _OVERLAP_MAX_PIXELS)
            self.side = net._side_stream() if use and not self.input_grad_only else None
        h0 = torch.empty((b, hh, ww, stem.weight.shape[0]), device=x.device, dtype=torch.float32)
        stem_small = x_nhwc.shape[-1] * 9 <= 64 and stem.weight.shape[0] % 4 == 0
        stem_cols = None
        if stem_small:
            stem_cols = self.small_in_conv(x_nhwc, stem, 1, 1, hh, ww, h0, ops.epilogue(bias=stem.bias))
        else:
            ops.conv2d_nhwc(x_nhwc, None, net._packed(stem), stem.weight.shape[0], 3, 3, 1, 1, 1, hh, ww, h0,
                            ops.epilogue(bias=stem.bias))
        n0 = _Node(h0, want_gsum=True)              # stem.bias = column sums of its gradient
        if self.record:
            def stem_bwd():
                g0 = n0.g
                n0.g = None
                have_bias = self.bias_from(n0, g0, stem.bias)

                def side():
                    if stem_small:
                        self.small_in_wgrad(g0, stem_cols, stem)
                    else:
                        self.wgrad(g0, x_nhwc, stem, 3, 1, 1)
                    if not have_bias:
                        self.bias_grad(g0, self.g(stem.bias))

                self.on_side(side, g0, x_nhwc)
                if self.want_dx:
                    dxs = torch.empty_like(x_nhwc)
                    self.dgrad(g0, stem, 3, 1, 1, hh, ww, dxs)
                    dxs = ops.nhwc_to_nchw(dxs)
                    if self.dx_nchw is None:
                        self.dx_nchw = dxs
                    else:
                        ops.axpby(dxs, 1.0, None, 0.0, self.dx_nchw, accumulate=True)

            self.push(stem_bwd, stem)
        hs: List[_Node] = [n0]
        pyr = x
        first_pyr = True
        for lvl in range(net.num_resolutions):
            for _ in range(net.num_res_blocks):
                hnode = self.resblock(hs[-1], mods[mi])
                mi += 1
                if hnode.v.shape[2] in net.attn_resolutions:
                    hnode = self.attn(hnode, mods[mi])
                    mi += 1
                hs.append(hnode)
            if lvl != net.num_resolutions - 1:
                hnode = self.resblock(hs[-1], mods[mi])
                mi += 1
                if pin == "residual":
                    hnode = self.pyramid(pyr, hnode, mods[mi], first_pyr)
                    mi += 1
                    pyr = hnode
                    first_pyr = False
                hs.append(hnode)
        hnode = hs[-1]
        hnode = self.resblock(hnode, mods[mi]); mi += 1
        hnode = self.attn(hnode, mods[mi]); mi += 1
        hnode = self.resblock(hnode, mods[mi]); mi += 1
        if net.is_classifier:
            assert mi + 1 == len(mods)
            return self.clf_head(hnode, mods[mi])
        for lvl in reversed(range(net.num_resolutions)):
            for _ in range(net.num_res_blocks + 1):
                hnode = self.resblock(self.concat(hnode, hs.pop(), mods[mi]), mods[mi])
                mi += 1
            if hnode.v.shape[2] in net.attn_resolutions:
                hnode = self.attn(hnode, mods[mi])
                mi += 1
            if lvl != 0:
                hnode = self.resblock(hnode, mods[mi])
                mi += 1
        assert not hs
        gnf, head = mods[mi], mods[mi + 1]
        assert mi + 2 == len(mods)
        first_last = self.use(hnode)
        stf = self.node_stats(hnode, gnf.weight, gnf.bias)
        af = ops.gn_apply(hnode.v, stf, True)
        oc = head.weight.shape[0]
        y = torch.empty((b, hh, ww, oc), device=x.device, dtype=torch.float32)
        if R.head_fewout(af.shape[-1], oc):
            ops.conv3x3_fewout(af, net._packed(head), head.bias, oc, y)
        else:
            ops.conv2d_nhwc(af, None, net._packed(head), oc, 3, 3, 1, 1, 1, hh, ww, y, ops.epilogue(bias=head.bias))
        if self.record:
            last = hnode
            self.head_grad = _Node(y)
            hg = self.head_grad

            def head_bwd():
                dy = hg.g

                daf = torch.empty_like(af)
                if oc * 9 <= 64 and af.shape[-1] % 4 == 0:
                    self.small_out_backward(dy, af, head, daf)
                else:
                    def side():
                        self.wgrad(dy, af, head, 3, 1, 1)
                        self.bias_grad(dy, self.g(head.bias))

                    self.on_side(side, dy, af)
                    self.dgrad(dy, head, 3, 1, 1, hh, ww, daf)
                xg, acc = _gbuf(last)
                self.gn_backward(daf, last.v, stf, gnf.weight, gnf.bias, self.g(gnf.weight), self.g(gnf.bias), True, xg,
                                 accumulate_dx=acc, last_writer_of=last if first_last else None)

            self.push(head_bwd, gnf)
        return ops.nhwc_to_nchw(y)

    # -- NCSNppClassifier head (ncsnpp_clf.py:277-283): flatten in NCHW order + Linear(bias=False) ------------------
    def clf_head(self, hnode: _Node, lin: nn.Linear) -> Tensor:
        self.use(hnode)
        b, h, w, c = hnode.v.shape
        flat = ops.nhwc_to_nchw(hnode.v).view(b, c * h * w)
        n_cls, k = lin.weight.shape
        logits = ops.linear(flat, lin.weight)
        if self.record:
            hg = self.head_grad = _Node(logits)

            def head_bwd():
                dy = hg.g                                                   # [B, n_cls]
                self.on_side(lambda: ops.gemm_raw(1, 0, n_cls, k, b, dy, n_cls, 0, flat, k, 0, self.g(lin.weight), k, 0),
                             dy, flat)
                dflat = torch.empty_like(flat)
                ops.gemm_raw(0, 0, b, k, n_cls, dy, n_cls, 0, lin.weight, k, 0, dflat, k, 0)
                xg, acc = _gbuf(hnode)
                ops.axpby(ops.nchw_to_nhwc(dflat.view(b, c, h, w)), 1.0, None, 0.0, xg, accumulate=acc)

            self.push(head_bwd, lin)
        return logits

"""Derived-weight entries of NCSNpp (weight_cache.py): ``make(owner, *args) -> Entry``, called on first use; PointwiseWeight."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops
from .score_modules import ResnetBlockBigGANpp
from .weight_cache import Entry

Tensor = torch.Tensor


def _packed_entry(w: Tensor, dgrad: bool) -> Entry:
    co, ci, kh, kw = w.shape

    def build(prev):
        out = prev if prev is not None else \
            torch.empty((ci, kh * kw, co) if dgrad else (co, kh * kw, ci), device=w.device, dtype=torch.float32)
        (ops.pack_dgrad if dgrad else ops.pack_ohwi)(w.detach(), out)
        return out
    return Entry(w, build=build, graph=not dgrad)


def _frag_entry(w: Tensor, dgrad: bool, wino: bool, arith: str = "x6") -> Entry:
    """Fragments of a 3x3 weight for the direct limb kernels (three limbs only) or in Winograd form (any arithmetic)."""
    row = ops.conv3x3_wino_frag_entry if wino else ops.conv3x3_frag_entry

    def build(prev):
        if not wino:
            return ops.conv3x3_frag(w.detach(), dgrad, prev)
        if arith == "x3":
            return (ops.conv3x3_wino_dgrad_frag_x3 if dgrad else ops.conv3x3_wino_frag_x3)(w.detach(), prev)
        if arith == "f16":
            return (ops.conv3x3_wino_dgrad_frag_f16 if dgrad else ops.conv3x3_wino_frag_f16)(w.detach(), prev)
        return ops.conv3x3_wino_frag(w.detach(), dgrad, prev)
    return Entry(w, build=build, family=("wino" if wino else "limb") + ops.ARITH_SUFFIX[arith],
                 rows=lambda out: [(row(w, dgrad, out), w.shape[0] * w.shape[1] // 8)], graph=not dgrad)


def _pfrag_packers(arith: str):
    """(packer of one pointwise fragment set, its batched form) in ``arith``."""
    return {"x6": (ops.gemm_frag, ops.pack_frag_batch), "x3": (ops.gemm_frag_x3, ops.pack_frag_batch_x3),
            "f16": (ops.gemm_frag_f16, ops.pack_frag_batch_f16)}[arith]


def pfrag_tail(n: int, k: int, n_total: int = 0, chunks_total: int = 0) -> bool:
    """The fragment set of an [n_total or n][32 * chunks_total or k] matrix is no whole number of 128 x 64 tiles: it is
    packed by the tail packers (ops.gemm_frag_tail) and read by ops.gemm_split_tail."""
    return (n_total or n) % 128 != 0 or (32 * chunks_total or k) % 64 != 0


def _pfrag_tail_entry(p: Tensor, tag: str, n: int, k: int, sn: int, sk: int, into: Optional[Tensor], chunk0: int,
                      chunks_total: int, n0: int, n_total: int) -> Entry:
    """Three-limb fragments of a tail set ("limb_tail" family); ``into`` with the row / K placement of a shared set."""
    def rows(out):
        return [ops.gemm_frag_tail_entry(p, out, n, k, sn, sk, n0, n_total, chunk0, chunks_total)]

    def build(prev):
        if into is None:
            return ops.gemm_frag_tail(p.detach(), n, k, sn, sk, prev)
        (row, items), = rows(into)
        ops.pack_frag_batch_tail(torch.tensor(row + [0], dtype=torch.int64, device=p.device), 1, items)
        return into
    return Entry(p, build=build, family="limb_tail", rows=rows, graph=tag in ("fwd", "qkv_f"))


def _pfrag_entry(p: Tensor, tag: str, arith: str, n: int, k: int, sn: int, sk: int, into: Optional[Tensor], chunk0: int,
                 chunks_total: int, n0: int = 0, n_total: int = 0) -> Entry:
    """``tag``: the cache tag without the arithmetic's suffix; 'x3' / 'f16' (whole-tile sets only) have batch families of their own."""
    if pfrag_tail(n, k, n_total, chunks_total):
        assert arith == "x6", arith
        return _pfrag_tail_entry(p, tag, n, k, sn, sk, into, chunk0, chunks_total, n0, n_total)
    pack, pack_batch = _pfrag_packers(arith)

    def rows(out):
        return [([p.data_ptr(), out.data_ptr(), n, k | (chunk0 << 20) | (chunks_total << 40), 1, sn, sk], n * k // 8)]

    def build(prev):
        if into is None:
            return pack(p.detach(), n, k, sn, sk, prev)
        # a one-entry table through the batched entry point (the only one that takes a K placement)
        (row, items), = rows(into)
        pack_batch(torch.tensor(row + [0], dtype=torch.int64, device=p.device), 1, items)
        return into
    return Entry(p, build=build, family="limb" + ops.ARITH_SUFFIX[arith], rows=rows, graph=tag in ("fwd", "qkv_f"))


def _built_entry(owner: Tensor, build) -> Entry:
    """Fragments built by ``build(prev)`` from ``owner`` (and possibly sibling parameters)."""
    return Entry(owner, build=build, graph=True)


def _qkv_entry(b0: Tensor, mod: "AttnBlockpp") -> Entry:
    """out: the forward and data-gradient q | k | v fragment sets (filled by the "qkv_f" / "qkv_d" entries) and the
    gathered [b_q | b_k | b_v] (filled by the "qkv_bias" family's batched copy)."""
    c = b0.numel()
    if pfrag_tail(3 * c, c):        # c % 128 != 0: padded sets (N = 3c forward, K = 3c data gradient)
        fbf, fbd = ops.gemm_frag_bytes_tail(3 * c, c), ops.gemm_frag_bytes_tail(c, 3 * c)
    else:
        fbf = fbd = 3 * ops.gemm_frag_bytes(c, c)
    out = (torch.empty(fbf, dtype=torch.uint8, device=b0.device),
           torch.empty(fbd, dtype=torch.uint8, device=b0.device),
           torch.empty(3 * c, dtype=torch.float32, device=b0.device))

    def rows(out):
        bq = out[2]
        return [([nin.b.data_ptr(), bq.data_ptr() + 4 * i * c, c // 4], c // 4)
                for i, nin in enumerate((mod.NIN_0, mod.NIN_1, mod.NIN_2))]
    return Entry(b0, out=out, family="qkv_bias", rows=rows, graph=True)


def _temb_entry(w0: Tensor, modules) -> Entry:
    """out: (wcat, bcat, {block: first row}) of NCSNpp._temb_plan, filled by the "temb" family's batched copy."""
    offsets, total = {}, 0
    for m in modules:
        if isinstance(m, ResnetBlockBigGANpp):
            offsets[m] = total
            total += m.Dense_0.weight.shape[0]
    out = (torch.empty((total, w0.shape[1]), device=w0.device, dtype=torch.float32),
           torch.empty((total,), device=w0.device, dtype=torch.float32), offsets)

    def rows(out):
        wcat, bcat, offsets = out
        r = []
        for m, o in offsets.items():
            w, bias = m.Dense_0.weight, m.Dense_0.bias
            for src, dst, n in ((w, wcat[o], w.numel()), (bias, bcat[o:], bias.numel())):
                assert n % 4 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
                r.append(([src.data_ptr(), dst.data_ptr(), n // 4], n // 4))
        return r
    return Entry(w0, out=out, family="temb", rows=rows, graph=True)


class PointwiseWeight(NamedTuple):
    """A pointwise weight as the B operand of y[m][n] = a[m][k] B^T (n = the layer's outputs; data gradient: n and k swapped) in
    the form a route of score_routes.pointwise_route launches on: limb fragments (a front for NCSNpp._pfrag / _qkv_frags /
    _wcache.get: tags and entries are theirs) or the stored matrix as ops.gemm_raw takes it.  ``kind``, and what ``w`` then is:
    "oi" a 1x1 Conv weight, stored [n][k]; "io" NIN.W, stored [k][n]; "qkv" an attention block (its shared q | k | v set, n = 3c);
    "ohwi" the pyramid's 3x3 stride-2 convolution as the [n][k = 9 cin] GEMM over im2col patches (packed from NCSNpp._packed,
    by the tail packer on LIMB_TAIL).  The last two have fragments only."""
    net: object
    w: object
    n: int
    k: int
    kind: str
    qkv: tuple = ()     # "qkv": this pass's NCSNpp._qkv_frags(w) = (forward fragments, data-gradient fragments, gathered bias)

    def tile(self, dgrad: bool):
        """(stored matrix, tb, ld) for ops.gemm_raw ("oi" / "io")."""
        oi = self.kind == "oi"
        return self.w, int(oi != dgrad), self.k if oi else self.n

    def frag(self, dgrad: bool = False, arith: str = "x6", tail: bool = False) -> Tensor:
        """Fragments of B[n][k], or of B[k][n] for the data gradient, in ``arith`` ('x3' / 'f16': whole-tile sets only, so not with
        ``tail``)."""
        net, w, kind = self.net, self.w, self.kind
        n, k = (self.k, self.n) if dgrad else (self.n, self.k)
        assert not (tail and arith != "x6")
        if kind == "qkv":
            return net._qkv_frags_x3(w, dgrad, arith == "f16") if arith != "x6" else self.qkv[int(dgrad)]
        if kind == "ohwi":
            pack = ops.gemm_frag_tail if tail else _pfrag_packers(arith)[0]
            sn, sk = (1, n) if dgrad else (k, 1)
            return net._wcache.get(w.weight, ("s2dgrad" if dgrad else "s2fwd") + ops.ARITH_SUFFIX[arith], _built_entry,
                                   lambda prev: pack(net._packed(w), n, k, sn, sk, prev))
        _, rows, ld = self.tile(dgrad)          # rows: B's rows are the stored matrix's rows
        return net._pfrag(w, "dgrad" if dgrad else "fwd", n, k, *((ld, 1) if rows else (1, ld)), arith=arith)

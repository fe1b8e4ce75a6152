"""Fused attention forward (psld_attn_fwd_split_f32) against the three-kernel path (batched limb GEMM, softmax, batched limb
GEMM), interleaved, random data.   python tools/bench_attn.py [--batch 128] [--c 480] [--products]

The three-kernel leg runs each product where the executor's bmm sends it: the full-tile batched limb kernel, the cut-tile one
(--c 480: P V) or the fp32 tile engine.  At a width with cut-tile products a further column times the three launches with
those products on the tile engine - the path before the cut-tile kernel and the C = 480 fused instances existed.
--products: the N = c products of a 16x16 block (P V, dV, dQ, dK), cut-tile kernel against the tile-engine launch."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from psld_amd import ops  # noqa: E402

DEV = "cuda"


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def bmm(ta, tb, m, n, k, a, lda, sa, bb, ldb, sb, cc, ldc, sc, batch, alpha=1.0, tail=True):
    """The executor's choice for one batched product (``tail`` False: cut-tile shapes go to the tile engine)."""
    if ops.bgemm_split_supported(ta, tb, m, n, k):
        ops.bgemm_split(ta, tb, m, n, k, a, lda, sa, bb, ldb, sb, cc, ldc, sc, batch, alpha)
    elif tail and ops.bgemm_split_tail_supported(ta, tb, m, n, k):
        ops.bgemm_split_tail(ta, tb, m, n, k, a, lda, sa, bb, ldb, sb, cc, ldc, sc, batch, alpha)
    else:
        ops.gemm_raw(ta, tb, m, n, k, a, lda, sa, bb, ldb, sb, cc, ldc, sc, batch, ops.epilogue(alpha=alpha) if alpha != 1.0 else None)


def products(b, c, rounds, iters, hw=256):
    """P V, dV = P^T dO, dQ = dS K, dK = dS^T Q of a 16x16 block as the backward tape sends them (q | k | v and their
    gradients as column slices of [b, hw, 3c] buffers): cut-tile limb kernel against the tile engine, interleaved."""
    qkv, dqkv = torch.randn(b, hw, 3 * c, device=DEV), torch.empty(b, hw, 3 * c, device=DEV)
    q, k, v, ld = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], 3 * c
    dq, dk, dv = dqkv[..., :c], dqkv[..., c:2 * c], dqkv[..., 2 * c:]
    p, ho = torch.randn(b, hw, hw, device=DEV), torch.randn(b, hw, c, device=DEV)
    o = torch.empty(b, hw, c, device=DEV)
    calls = {"P V": (0, 0, hw, c, hw, p, hw, hw * hw, v, ld, hw * ld, o, c, hw * c, b, 1.0),
             "dV": (1, 0, hw, c, hw, p, hw, hw * hw, ho, c, hw * c, dv, ld, hw * ld, b, 1.0),
             "dQ": (0, 0, hw, c, hw, p, hw, hw * hw, k, ld, hw * ld, dq, ld, hw * ld, b, c ** -0.5),
             "dK": (1, 0, hw, c, hw, p, hw, hw * hw, q, ld, hw * ld, dk, ld, hw * ld, b, c ** -0.5)}
    for name, a in calls.items():
        assert ops.bgemm_split_tail_supported(*a[:5]), (name, a[:5])
        fs = [lambda: bmm(*a, tail=True), lambda: bmm(*a, tail=False)]
        ts = [[], []]
        for _ in range(rounds):
            for i, f in enumerate(fs):
                ts[i].append(timeit(f, iters))
        m = [sorted(t)[len(t) // 2] * 1e6 for t in ts]
        fl = 2.0 * b * hw * hw * c
        print(f"{name:4s} B={b} HW={hw} C={c} (ta={a[0]} tb={a[1]}): cut-tile limb kernel {m[0]:7.1f} us ({fl / m[0] / 1e6:5.1f} TF)   "
              f"tile engine {m[1]:7.1f} us ({fl / m[1] / 1e6:5.1f} TF)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--c", type=int, default=256, help="channels (256, 128 or 480)")
    ap.add_argument("--products", action="store_true", help="time the N = c batched products of a 16x16 block instead")
    args = ap.parse_args()
    ops.lib()
    b, c = args.batch, args.c
    if args.products:
        return products(b, c, args.rounds, args.iters)
    for hw in (256, 64):
        qkv = torch.randn(b, hw, 3 * c, device=DEV)
        q, k, v, ld = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], 3 * c
        scale = c ** -0.5
        o0, o1, o2 = (torch.empty(b, hw, c, device=DEV) for _ in range(3))
        p0, p1 = torch.empty(b, hw, hw, device=DEV), torch.empty(b, hw, hw, device=DEV)

        def three(tail=True):
            bmm(0, 1, hw, hw, c, q, ld, hw * ld, k, ld, hw * ld, p0, hw, hw * hw, b, scale, tail)
            ops.softmax_rows(p0, p0, b * hw, hw)
            bmm(0, 0, hw, c, hw, p0, hw, hw * hw, v, ld, hw * ld, o0, c, hw * c, b, 1.0, tail)
        fs = [three, lambda: ops.attn_fwd(q, k, v, ld, b, hw, c, scale, o1, p1), lambda: ops.attn_fwd(q, k, v, ld, b, hw, c, scale, o2, None)]
        has_tail = ops.bgemm_split_tail_supported(0, 0, hw, c, hw)
        if has_tail:
            fs.append(lambda: three(False))
        ts = [[] for _ in fs]
        for _ in range(args.rounds):
            for i, f in enumerate(fs):
                ts[i].append(timeit(f, args.iters))
        m = [sorted(t)[len(t) // 2] * 1e6 for t in ts]
        fl = 2 * 2.0 * b * hw * hw * c
        err = float((o1 - o0).norm() / o0.norm())
        print(f"attention fwd B={b} HW={hw} C={c}: three kernels {m[0]:7.1f} us   fused + P {m[1]:7.1f} us ({fl / m[1] / 1e6:5.1f} TF)   "
              f"fused, no P {m[2]:7.1f} us ({fl / m[2] / 1e6:5.1f} TF)   rel diff {err:.1e}" +
              (f"   three kernels, cut-tile products on the tile engine {m[3]:7.1f} us" if has_tail else ""))


if __name__ == "__main__":
    main()

"""Timing of the AFHQv2-128 inpainting network (nf = 160) on the tree whose root is argv[1] (profiles/r07/afhq160.md).

    python tools/bench_afhq160.py ROOT eval 16       # eval forward (one EM step's network call), ms / images per s
    python tools/bench_afhq160.py ROOT train 8       # forward + loss + backward
    python tools/bench_afhq160.py ROOT kernels 16    # one 3x3 forward launch per level, as the executor sends it, and the
                                                     # same launch with cout zero-padded to a multiple of 128
    python tools/bench_afhq160.py ROOT pointwise 16  # one forward launch per distinct pointwise (m, k, n) of the network: the
                                                     # limb route (tail launch) against the fp32 tile engine's GEMM

ROOT may be another checkout of the project (built in place) so that two trees are timed on one box; the configuration is
built from ``afhqv2_128`` with the inpainting script's network keys, which older trees without ``afhqv2_128_inpaint`` have too.
"""
import json
import os
import sys
import time

root = sys.argv[1]
sys.path.insert(0, os.path.abspath(root))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # tests.synth of this tree
import torch  # noqa: E402

import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402
from tests.synth import synth_inputs, synth_state_dict  # noqa: E402

what = sys.argv[2]
B = int(sys.argv[3]) if len(sys.argv) > 3 else 16
DEV = "cuda"
assert os.path.abspath(psld_amd.__file__).startswith(os.path.abspath(root)), psld_amd.__file__


def cfg160():
    c = C.afhqv2_128()
    sf = c.model.score_fn
    sf.in_ch, sf.out_ch, sf.nf, sf.ch_mult, sf.num_res_blocks, sf.attn_resolutions, sf.dropout = 6, 3, 160, [1, 2, 2, 3, 3], 2, [8, 16], 0.2
    sde = c.model.sde
    sde.nu, sde.gamma, sde.kappa = 4.0, 0.0, 0.04
    return c


def ev(start, end):
    torch.cuda.synchronize()
    return start.elapsed_time(end)


if what in ("eval", "train"):
    psld_amd.import_modules_into_registry()
    cfg = cfg160()
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 6100)
    net.load_state_dict(sd)
    net = net.to(DEV)
    if what == "eval":
        net.eval()
        x = torch.randn(B, 6, 128, 128, device=DEV)
        t = torch.rand(B, device=DEV) * 0.9 + 0.05

        def step():
            with torch.no_grad():
                net(x, t)
        warm, iters = 5, 20
    else:
        net.train()
        sde = get_module("sde", "psld")(cfg)
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        x0, eps, t = synth_inputs(B, 3, 128, seed=5)
        x0, eps, t = x0.to(DEV), eps.to(DEV), t.to(DEV)

        def step():
            net.zero_grad(set_to_none=False)
            crit(x0, t, net, eps=eps).backward()
        warm, iters = 5, 15
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.time()
    s.record()
    for _ in range(iters):
        step()
    e.record()
    ms = ev(s, e) / iters
    print(json.dumps({"tree": root, "what": what, "B": B, "ms": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1),
                      "wall_s": round(time.time() - t0, 2)}), flush=True)
elif what == "pointwise":
    # (k, n, map side) of the network's pointwise contractions, forward and data gradient: 1x1 shortcuts, attention
    # projections (q|k|v as one N = 3c GEMM), stride-2 pyramid GEMMs.  Per shape: the launch the executor sends on this tree
    # (ops.gemm_split_tail, or ops.gemm_split where the old kernels take the shape) and the tile-engine GEMM the parent sent.
    shapes = [(160, 320, 64), (320, 160, 64), (320, 480, 16), (480, 320, 16),
              (960, 480, 8), (480, 960, 8), (960, 480, 16), (480, 960, 16), (800, 480, 16), (480, 800, 16), (800, 320, 32),
              (320, 800, 32), (640, 320, 32), (320, 640, 32), (640, 320, 64), (320, 640, 64), (480, 320, 64), (320, 480, 64),
              (480, 160, 128), (160, 480, 128), (320, 160, 128), (160, 320, 128),
              (480, 1440, 16), (480, 480, 16), (1440, 480, 16), (480, 1440, 8), (480, 480, 8), (1440, 480, 8),
              (1440, 320, 64), (320, 1440, 64), (2880, 320, 32), (320, 2880, 32), (2880, 480, 16), (480, 2880, 16),
              (4320, 480, 8), (480, 4320, 8)]
    tail = hasattr(ops, "gemm_split_tail")
    out = []
    for k, n, side in shapes:
        m = B * side * side
        a = torch.randn(m, k, device=DEV)
        w = torch.randn(n, k, device=DEV) * 0.05
        bias = torch.randn(n, device=DEV)
        y = torch.empty(m, n, device=DEV)
        epi = ops.epilogue(bias=bias)
        runs = {"tile": lambda: ops.gemm_raw(0, 1, m, n, k, a, k, 0, w, k, 0, y, n, 0, 1, epi)}
        if tail and ops.gemm_tail_supported(k, m, n):
            frag = ops.gemm_frag_tail(w, n, k, k, 1)
            runs["limb_tail"] = lambda: ops.gemm_split_tail(a, m, frag, n, y, epi)
        elif ops.gemm_split_supported(k, 0, m, n):
            frag = ops.gemm_frag(w, n, k, k, 1)
            runs["limb"] = lambda: ops.gemm_split(a, None, m, frag, n, y, epi)
        res = {}
        for tag, run in runs.items():
            for _ in range(3):
                run()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            for _ in range(20):
                run()
            en.record()
            us = ev(st, en) / 20 * 1e3
            res[tag] = {"us": round(us, 1), "tflops": round(2 * m * k * n / us / 1e6, 1)}
        out.append({"m": m, "k": k, "n": n, **res})
        del a, w, y
    print(json.dumps({"tree": root, "what": "pointwise", "B": B, "shapes": out}), flush=True)
else:
    # one 3x3 forward launch per level of the network at batch B, as the executor sends it (new tree: Winograd with tails;
    # parent: the tile engine), plus the zero-padded-to-128 alternative on the Winograd kernel where the tree takes it
    shapes = [(160, 160, 128), (320, 320, 64), (320, 320, 32), (480, 480, 16), (480, 480, 8)]
    out = []
    for ci, co, s in shapes:
        x = torch.randn(B, s, s, ci, device=DEV)
        w = torch.randn(co, ci, 3, 3, device=DEV) * 0.05
        res = {}
        for tag, cout in (("exec", co), ("pad128", -(-co // 128) * 128)):
            if tag == "pad128" and not ops.conv3x3_wino_supported(ci, 0, B, s, s, cout):
                continue
            wp = torch.zeros(cout, ci, 3, 3, device=DEV)
            wp[:co] = w
            y = torch.empty(B, s, s, cout, device=DEV)
            if ops.conv3x3_wino_supported(ci, 0, B, s, s, cout):
                uf = ops.conv3x3_wino_frag(wp, False)
                run = lambda: ops.conv3x3_wino(x, None, uf, cout, y, allow_split=True)  # noqa: E731
                kind = "wino"
            else:
                wohwi = wp.permute(0, 2, 3, 1).contiguous()
                run = lambda: ops.conv2d_nhwc(x, None, wohwi, cout, 3, 3, 1, 1, 1, s, s, y, None)  # noqa: E731
                kind = "tile"
            for _ in range(3):
                run()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 20
            st.record()
            for _ in range(n):
                run()
            en.record()
            us = ev(st, en) / n * 1e3
            res[tag] = {"kind": kind, "us": round(us, 1), "tflops_direct_eq": round(2 * B * s * s * ci * co * 9 / us / 1e6, 1)}
        out.append({"ci": ci, "co": co, "s": s, "B": B, **res})
    print(json.dumps({"tree": root, "what": "kernels", "levels": out}), flush=True)

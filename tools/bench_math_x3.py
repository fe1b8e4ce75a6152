"""Math mode 'bf16x3' (two bf16 limbs, three products) against 'bf16x6' (three limbs, six products), alternating
bf16x6, bf16x3, bf16x6, bf16x3, ... in ONE process:
  (a) one forward launch at B = 512: 3x3 convolutions 128->128 @32, 256->256 @32 / @16 / @8 (Winograd F(2x2,3x3)) and the
      pointwise 512->256 @32 (HIP events, --iters launches after a warm-up launch, --repeats rounds);
  (b) --steps Euler-Maruyama steps of the C10-SOTA network at B = 512 and B = 64 after --warmup steps, --repeats rounds,
      and the rel-L2 of the 'bf16x3' state against the 'bf16x6' state after those steps on the same noise.
Seeded synthetic weights; nothing is read from outside the tree.  The gate the project uses: the SLOWEST bf16x3 figure
against the FASTEST bf16x6 figure of a row.
    python tools/bench_math_x3.py [--iters 20] [--steps 20] [--warmup 5] [--repeats 3] [--batches 512,64]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402

DEV = "cuda"
MODES = ("bf16x6", "bf16x3")


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


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def report(name, t, unit=1e6, what="us"):
    slow3, fast6 = max(t["bf16x3"]), min(t["bf16x6"])
    med = {m: sorted(t[m])[len(t[m]) // 2] for m in MODES}
    print(f"{name}: bf16x6 {' '.join(f'{v * unit:8.1f}' for v in t['bf16x6'])} {what} | bf16x3 "
          f"{' '.join(f'{v * unit:8.1f}' for v in t['bf16x3'])} {what} | median x{med['bf16x6'] / med['bf16x3']:.3f}, "
          f"fastest bf16x6 / slowest bf16x3 x{fast6 / slow3:.3f}", flush=True)


def launches(args):
    B = 512
    for cin, cout, s in ((128, 128, 32), (256, 256, 32), (256, 256, 16), (256, 256, 8)):
        g = torch.Generator(device=DEV).manual_seed(cin + s)
        x = torch.randn(B, s, s, cin, device=DEV, generator=g)
        w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) * 0.05
        bias = torch.randn(cout, device=DEV, generator=g)
        res = torch.randn(B, s, s, cout, device=DEV, generator=g)
        epi = ops.epilogue(bias=bias, residual=res, ld_residual=cout, out_scale=0.7)
        f6, f3 = ops.conv3x3_wino_frag(w, False), ops.conv3x3_wino_frag_x3(w)
        y6, y3 = torch.empty(B, s, s, cout, device=DEV), torch.empty(B, s, s, cout, device=DEV)
        fn = {"bf16x6": lambda: ops.conv3x3_wino(x, None, f6, cout, y6, epi, allow_split=True),
              "bf16x3": lambda: ops.conv3x3_wino_x3(x, None, f3, cout, y3, epi, allow_split=True)}
        t = {m: [] for m in MODES}
        for _ in range(args.repeats):
            for m in MODES:
                t[m].append(timeit(fn[m], args.iters))
        report(f"conv3x3 {cin}->{cout} @{s} B={B} (rel-L2 x3 vs x6 {rel_l2(y3, y6):.2e})", t)
    k, n, m_ = 512, 256, B * 32 * 32
    g = torch.Generator(device=DEV).manual_seed(7)
    a = torch.randn(m_, k, device=DEV, generator=g)
    bm = torch.randn(n, k, device=DEV, generator=g) * 0.05
    bias = torch.randn(n, device=DEV, generator=g)
    f6, f3 = ops.gemm_frag(bm, n, k, k, 1), ops.gemm_frag_x3(bm, n, k, k, 1)
    y6, y3 = torch.empty(m_, n, device=DEV), torch.empty(m_, n, device=DEV)
    epi = ops.epilogue(bias=bias)
    fn = {"bf16x6": lambda: ops.gemm_split(a, None, m_, f6, n, y6, epi), "bf16x3": lambda: ops.gemm_split_x3(a, None, m_, f3, n, y3, epi)}
    t = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:
            t[m].append(timeit(fn[m], args.iters))
    report(f"pointwise {k}->{n} @32 B={B} (rel-L2 x3 vs x6 {rel_l2(y3, y6):.2e})", t)


def synthetic_net(cfg):
    net = get_module("score_fn", "ncsnpp")(cfg)
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() > 1:
                fan_in = p[0].numel() if p.dim() == 4 else p.shape[0] if name.endswith(".W") else p.shape[-1]
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(fan_in))
            elif "GroupNorm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return net.to(DEV).eval()


def em_steps(args):
    psld_amd.import_modules_into_registry()
    cfg = C.c10_sota()
    net = synthetic_net(cfg)
    sde = get_module("sde", "psld")(cfg)
    ng = torch.Generator(device=DEV)

    def noise(i, x):
        return torch.randn(x.shape, device=DEV, dtype=torch.float64, generator=ng.manual_seed(1000 + i))
    for B in (int(v) for v in args.batches.split(",")):
        g = torch.Generator(device=DEV).manual_seed(B)
        batch = torch.randn(B, 6, 32, 32, device=DEV, generator=g)
        batch[:, 3:] *= 0.5
        ts_w = torch.linspace(0, 0.2, args.warmup + 1, dtype=torch.float64, device=DEV)
        ts = torch.linspace(0, 0.8, args.steps + 1, dtype=torch.float64, device=DEV)
        t = {m: [] for m in MODES}
        state = {}
        for _ in range(args.repeats):
            for m in MODES:
                ops.set_math_mode(m)
                sampler = get_module("samplers", "em_sde")(cfg, sde, net)
                sampler.noise_fn = noise
                sampler.sample(batch, ts_w, args.warmup, denoise=False)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                state[m] = sampler.sample(batch, ts, args.steps, denoise=False)
                e.record()
                torch.cuda.synchronize()
                t[m].append(s.elapsed_time(e) / args.steps * 1e-3)
        report(f"EM step C10-SOTA B={B} ({args.steps} steps; rel-L2 of the bf16x3 state vs bf16x6 {rel_l2(state['bf16x3'], state['bf16x6']):.2e})",
               t, 1e3, "ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="512,64")
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--skip-em", action="store_true")
    args = ap.parse_args()
    ops.lib()
    old = ops.math_mode()
    try:
        if not args.skip_launches:
            launches(args)
        if not args.skip_em:
            em_steps(args)
    finally:
        ops.set_math_mode(old)


if __name__ == "__main__":
    main()

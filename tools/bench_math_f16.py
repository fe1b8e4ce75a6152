"""Eval math 'f16' (one fp16 product per accumulator) against math mode 'bf16x3' (two bf16 limbs, three products), alternating
bf16x3, f16, bf16x3, f16, ... in ONE process per part:
  launches  one forward launch at B = 512: 3x3 convolutions 128->128 @32, 256->256 @32 / @16 / @8 (Winograd F(2x2,3x3)) and the
            pointwise 512->256 @32 (HIP events, --iters launches after a warm-up launch, --repeats rounds);
  em        --steps Euler-Maruyama steps of the C10-SOTA network at one batch size after --warmup steps, --repeats rounds, and
            the rel-L2 of the 'f16' state against the 'bf16x3' state after those steps on the same noise.
Without --part the tool is a driver: it runs every part (launches, em at each of --batches) as a child process under a time
limit of its own (--limit seconds) and stops at the first part that fails or runs out of time.
Seeded synthetic weights; nothing is read from outside the tree.  The gate the project uses: the SLOWEST f16 figure against
the FASTEST bf16x3 figure of a row.
    python tools/bench_math_f16.py [--iters 20] [--steps 20] [--warmup 5] [--repeats 3] [--batches 512,64] [--limit 240]"""
import argparse
import math
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402

DEV = "cuda"
MODES = ("bf16x3", "f16")


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
    slow16, fast3 = max(t["f16"]), min(t["bf16x3"])
    med = {m: sorted(t[m])[len(t[m]) // 2] for m in MODES}
    print(f"{name}: bf16x3 {' '.join(f'{v * unit:8.1f}' for v in t['bf16x3'])} {what} | f16 "
          f"{' '.join(f'{v * unit:8.1f}' for v in t['f16'])} {what} | median x{med['bf16x3'] / med['f16']:.3f}, "
          f"fastest bf16x3 / slowest f16 x{fast3 / slow16:.3f} ({'PASS' if slow16 < fast3 else 'FAIL'})", flush=True)


def launches(args):
    B = 512
    for cin, cout, s in ((128, 128, 32), (256, 256, 32), (256, 256, 16), (256, 256, 8)):
        g = torch.Generator(device=DEV).manual_seed(cin + s)
        x = torch.randn(B, s, s, cin, device=DEV, generator=g)
        w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) * 0.05
        bias = torch.randn(cout, device=DEV, generator=g)
        res = torch.randn(B, s, s, cout, device=DEV, generator=g)
        epi = ops.epilogue(bias=bias, residual=res, ld_residual=cout, out_scale=0.7)
        f3, f1 = ops.conv3x3_wino_frag_x3(w), ops.conv3x3_wino_frag_f16(w)
        y3, y1 = torch.empty(B, s, s, cout, device=DEV), torch.empty(B, s, s, cout, device=DEV)
        fn = {"bf16x3": lambda: ops.conv3x3_wino_x3(x, None, f3, cout, y3, epi, allow_split=True),
              "f16": lambda: ops.conv3x3_wino_f16(x, None, f1, cout, y1, epi, allow_split=True)}
        t = {m: [] for m in MODES}
        for _ in range(args.repeats):
            for m in MODES:
                t[m].append(timeit(fn[m], args.iters))
        report(f"conv3x3 {cin}->{cout} @{s} B={B} (rel-L2 f16 vs x3 {rel_l2(y1, y3):.2e})", t)
    k, n, m_ = 512, 256, B * 32 * 32
    g = torch.Generator(device=DEV).manual_seed(7)
    a = torch.randn(m_, k, device=DEV, generator=g)
    bm = torch.randn(n, k, device=DEV, generator=g) * 0.05
    bias = torch.randn(n, device=DEV, generator=g)
    f3, f1 = ops.gemm_frag_x3(bm, n, k, k, 1), ops.gemm_frag_f16(bm, n, k, k, 1)
    y3, y1 = torch.empty(m_, n, device=DEV), torch.empty(m_, n, device=DEV)
    epi = ops.epilogue(bias=bias)
    fn = {"bf16x3": lambda: ops.gemm_split_x3(a, None, m_, f3, n, y3, epi), "f16": lambda: ops.gemm_split_f16(a, None, m_, f1, n, y1, epi)}
    t = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:
            t[m].append(timeit(fn[m], args.iters))
    report(f"pointwise {k}->{n} @32 B={B} (rel-L2 f16 vs x3 {rel_l2(y1, y3):.2e})", t)


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
                ops.set_eval_math("f16" if m == "f16" else "limb")
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
        report(f"EM step C10-SOTA B={B} ({args.steps} steps; rel-L2 of the f16 state vs bf16x3 {rel_l2(state['f16'], state['bf16x3']):.2e})",
               t, 1e3, "ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="512,64")
    ap.add_argument("--limit", type=int, default=240, help="driver: seconds a part may take")
    ap.add_argument("--part", default=None, choices=["launches", "em"], help="run one part in this process (em: --batches)")
    args = ap.parse_args()
    if args.part is None:
        common = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--steps", str(args.steps),
                  "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        parts = [["--part", "launches"]] + [["--part", "em", "--batches", b] for b in args.batches.split(",")]
        for part in parts:
            try:
                rc = subprocess.run(common + part, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:         # nothing more is started on the GPU after a part that failed or ran out of time
                print(f"part {' '.join(part)} ended with status {rc}: stopping", flush=True)
                sys.exit(rc if rc > 0 else 1)
        return
    ops.lib()
    old, old_eval = ops.math_mode(), ops.eval_math()
    try:
        ops.set_math_mode("bf16x3")
        if args.part == "launches":
            launches(args)
        else:
            em_steps(args)
    finally:
        ops.set_math_mode(old)
        ops.set_eval_math(old_eval)


if __name__ == "__main__":
    main()

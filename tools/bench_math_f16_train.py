"""Record f16 (``--train-math f16``: one fp16 product in the forward and data-gradient launches of a recording pass) against
record math 'bf16x3', alternating bf16x3, f16, bf16x3, f16, ... in ONE process per part:
  launches        one launch at B = 128 (HIP events, --iters launches after a warm-up launch, --repeats rounds): the Winograd data
                  gradient 256->256 @32 and the pointwise data gradient 512->256 @32 (dy of 256 channels to 512), dy ~ N(0, 1) *
                  2^-20 with shift 20 on the fp16 side;
  NAME:BATCH      --steps full HSM train steps (perturb + forward + loss + backward + clip + Adam + EMA) after --warmup steps,
                  --repeats rounds: c10_sota:128, celeba64_sota:128, c10_sota:16.
Without --part the tool is a driver: every part runs as a child process under its own ``timeout -k 10``, one after the other, and
the first part that fails ends the run (nothing more is started on the GPU).  Seeded synthetic inputs; nothing is read from outside
the tree.  The gate the project uses: the SLOWEST f16 figure against the FASTEST bf16x3 figure of a row.
    python tools/bench_math_f16_train.py [--iters 20] [--steps 10] [--warmup 5] [--repeats 3] [--parts launches,c10_sota:128,...]"""
import argparse
import copy
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("bf16x3", "f16")
PARTS = "launches,c10_sota:128,celeba64_sota:128,c10_sota:16"
DEV = "cuda"


def report(name, t, unit=1e6, what="us"):
    slow16, fast3 = max(t["f16"]), min(t["bf16x3"])
    med = {m: sorted(t[m])[len(t[m]) // 2] for m in MODES}
    print(f"{name}: bf16x3 {' '.join(f'{v * unit:8.1f}' for v in t['bf16x3'])} {what} | f16 "
          f"{' '.join(f'{v * unit:8.1f}' for v in t['f16'])} {what} | median x{med['bf16x3'] / med['f16']:.3f}, "
          f"fastest bf16x3 / slowest f16 x{fast3 / slow16:.3f}", flush=True)


def launches(args):
    import torch
    from psld_amd import ops
    from tools.bench_math_x3 import rel_l2, timeit
    B, s, shift = 128, 32, 20
    g = torch.Generator(device=DEV).manual_seed(11)
    cin = cout = 256
    dy = torch.randn(B, s, s, cout, device=DEV, generator=g) * 2.0 ** -shift
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) * 0.05
    f3, f16 = ops.conv3x3_wino_dgrad_frag_x3(w), ops.conv3x3_wino_dgrad_frag_f16(w)
    y3, y16 = (torch.empty(B, s, s, cin, device=DEV) for _ in range(2))
    fn = {"bf16x3": lambda: ops.conv3x3_wino_x3(dy, None, f3, cin, y3, None, allow_split=True),
          "f16": lambda: ops.conv3x3_wino_f16s(dy, None, f16, cin, y16, shift, None, allow_split=True)}
    t = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:
            t[m].append(timeit(fn[m], args.iters))
    report(f"dgrad {cout}->{cin} @{s} B={B} (rel-L2 f16 vs x3 {rel_l2(y16, y3):.2e})", t)
    k, n, m_ = 256, 512, B * s * s              # dy [m][256] W: the data gradient of a 1x1 weight stored [256 out][512 in]
    dyp = torch.randn(m_, k, device=DEV, generator=g) * 2.0 ** -shift
    wp = torch.randn(k, n, device=DEV, generator=g) * 0.05
    p3, p16 = ops.gemm_frag_x3(wp, n, k, 1, n), ops.gemm_frag_f16(wp, n, k, 1, n)
    z3, z16 = (torch.empty(m_, n, device=DEV) for _ in range(2))
    fn = {"bf16x3": lambda: ops.gemm_split_x3(dyp, None, m_, p3, n, z3, None),
          "f16": lambda: ops.gemm_split_f16s(dyp, None, m_, p16, n, z16, shift, None)}
    t = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:
            t[m].append(timeit(fn[m], args.iters))
    report(f"pointwise dgrad {n}->{k} @{s} B={B} (rel-L2 f16 vs x3 {rel_l2(z16, z3):.2e})", t)


def train_steps(args, row):
    import torch
    import psld_amd
    from psld_amd import config as C, ops
    from psld_amd.optim import EMAWeightUpdate
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    name, batch = row.split(":")
    batch = int(batch)
    cfg = getattr(C, name)()
    cfg.training.batch_size = batch
    size = cfg.data.image_size
    g = torch.Generator(device=DEV).manual_seed(0)
    data = [torch.rand(batch, 3, size, size, device=DEV, generator=g) * 2 - 1 for _ in range(2)]
    t = {m: [] for m in MODES}
    final = {}
    ops.set_record_math("bf16x3")
    for _ in range(args.repeats):
        for m in MODES:
            ops.set_record_f16(m == "f16")
            # a network of its own per measurement, from the same seed: both modes time the same steps of the same run
            torch.manual_seed(cfg.training.seed)
            net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
            ema = copy.deepcopy(net)
            for p in ema.parameters():
                p.requires_grad = False
            sde = get_module("sde", "psld")(cfg)
            crit = get_module("losses", "psld_score_loss")(cfg, sde)
            wrapper = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, criterion=crit)
            cb = EMAWeightUpdate(cfg.training.ema_decay)

            def run(n, first):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last = None
                for i in range(n):
                    last = wrapper.training_step(data[(first + i) % len(data)], first + i)
                    cb.on_train_batch_end(None, wrapper)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, last
            run(args.warmup, 0)
            dt, last = run(args.steps, args.warmup)
            t[m].append(dt / args.steps)
            final[m] = float(last.item())
            ops.check_device_errors(torch.device(DEV, torch.cuda.current_device()))
            del wrapper, net, ema
            torch.cuda.empty_cache()
    report(f"train step {name} B={batch} ({args.steps} steps after {args.warmup}; final loss bf16x3 {final['bf16x3']:.5f}, "
           f"f16 {final['f16']:.5f})", t, 1e3, "ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default=PARTS)
    ap.add_argument("--part", default=None, help="run this one part in this process (what the driver starts)")
    ap.add_argument("--part-timeout", type=int, default=240, help="seconds a part may take")
    args = ap.parse_args()
    if args.part is None:       # the driver: it never opens the GPU itself
        for part in args.parts.split(","):
            cmd = ["timeout", "-k", "10", str(args.part_timeout), sys.executable, os.path.abspath(__file__), "--part", part,
                   "--iters", str(args.iters), "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"part {part} ended with status {rc}: stopping", flush=True)
                sys.exit(rc)
        return
    from psld_amd import ops
    ops.lib()
    old = ops.record_math(), ops.record_f16()
    try:
        if args.part == "launches":
            launches(args)
        else:
            train_steps(args, args.part)
    finally:
        ops.set_record_math(old[0])
        ops.set_record_f16(old[1])


if __name__ == "__main__":
    main()

"""One Euler-Maruyama sampling step of C10-SOTA with and without classifier-free guidance, on the tree whose root is argv[1]
(profiles/r15/cfg.md).

    python tools/bench_cfg.py ROOT uncond 512 [steps]    # the unconditional network, batch 512
    python tools/bench_cfg.py ROOT cfg 256 [steps]       # label_classes = 10, CFGScoreFn at scale 2: network batch 512

ROOT may be another checkout of the project (built in place), so that the parent commit's unconditional step and this tree's
guided step are timed on one box, one process each, alternating.  Prints one JSON line: ms per EM step over ``steps`` steps
(HIP events around the whole run, after a warm-up run of 3 steps).
"""
import json
import os
import sys

root = sys.argv[1]
sys.path.insert(0, os.path.abspath(root))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # tests.synth of this tree
import torch  # noqa: E402

import psld_amd  # noqa: E402
from psld_amd import config as C  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

what = sys.argv[2]
B = int(sys.argv[3]) if len(sys.argv) > 3 else (512 if what == "uncond" else 256)
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
DEV = "cuda"
assert what in ("uncond", "cfg"), what
assert os.path.abspath(psld_amd.__file__).startswith(os.path.abspath(root)), psld_amd.__file__

psld_amd.import_modules_into_registry()
cfg = C.c10_sota()
keys = [(k, tuple(v.shape)) for k, v in get_module("score_fn", "ncsnpp")(cfg).state_dict().items()]
sd = synth_state_dict(keys, 7)
if what == "cfg":
    cfg.model.score_fn.label_classes = 10
    nf = cfg.model.score_fn.nf
    sd = {"label_emb": 0.1 * torch.randn(11, 4 * nf, generator=torch.Generator().manual_seed(21)), **sd}
net = get_module("score_fn", "ncsnpp")(cfg)
net.load_state_dict(sd)
net = net.to(DEV).eval()
fn = net
if what == "cfg":
    from psld_amd.guidance import CFGScoreFn
    fn = CFGScoreFn(net, torch.arange(B, device=DEV) % 10, 2.0)
sde = get_module("sde", "psld")(cfg)
sampler = get_module("samplers", "em_sde")(cfg, sde, fn)
batch = sde.prior_sampling((B, 3, 32, 32), device=DEV)


def run(n):
    ts = torch.linspace(0, sde.T - 1e-3, n + 1, dtype=torch.float64, device=DEV)
    return sampler.sample(batch, ts, n, denoise=False)


run(3)
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
x = run(steps)
e.record()
torch.cuda.synchronize()
ms = s.elapsed_time(e)
print(json.dumps({"tree": root, "what": what, "sampler_batch": B, "network_batch": 2 * B if what == "cfg" else B, "steps": steps,
                  "ms_per_em_step": ms / steps, "finite": bool(torch.isfinite(x).all())}), flush=True)

"""Static instruction counts of the ends of every wino_conv8s_kernel instantiation in a device assembly file of conv_wino.hip
(hipcc with the Makefile's flags plus -S --cuda-device-only): the set-up in front of the first barrier, what follows the last
MFMA (the epilogue; in builds whose loop ends on a transform, that transform too), runtime integer divisions (one
v_rcp_iflag_f32 each), scratch accesses, and the register metadata.
    python tools/wino_isa_regions.py conv_wino.s [kernel_substring]"""
import re
import sys

s = open(sys.argv[1]).read()
want = sys.argv[2] if len(sys.argv) > 2 else "wino_conv8s_kernel"


def count(seg):
    vec = sum(1 for o in seg if o.startswith("v_") and not o.startswith("v_mfma"))
    return (f"instructions={len(seg)} vector={vec} divisions={sum(1 for o in seg if o.startswith('v_rcp_iflag'))} "
            f"mfma={sum(1 for o in seg if o.startswith('v_mfma'))} scratch={sum(1 for o in seg if o.startswith('scratch_'))} "
            f"global_loads={sum(1 for o in seg if o.startswith('global_load'))}")


for f in re.split(r"\n(?=_Z\w+:)", s):
    name = f.split(":", 1)[0]
    if want not in name or "\n" in name:
        continue
    ins = []
    for ln in f.split(".Lfunc_end")[0].split("\n")[1:]:
        t = ln.strip()
        if t and t[0] not in ";." and not t.endswith(":"):
            ins.append(t.split()[0])
    first_bar = next(i for i, o in enumerate(ins) if o.startswith("s_barrier"))
    last_mfma = max(i for i, o in enumerate(ins) if o.startswith("v_mfma"))
    meta = s[s.find(".name:           " + name):][:700]
    print(name)
    print("  set-up (to the first barrier):", count(ins[:first_bar]))
    print("  between                      :", count(ins[first_bar:last_mfma + 1]))
    print("  after the last MFMA          :", count(ins[last_mfma + 1:]))
    print("  " + " ".join(x.strip() for x in meta.split("\n") if "vgpr" in x or "private_segment" in x))

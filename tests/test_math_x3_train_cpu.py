"""Record math 'bf16x3' (two bf16 limbs in the passes that record a backward pass) - what can be checked without a GPU: the
setting in the C ABI, Python and the environment, the CLI option, and the CPU reference of the arithmetic
(tests/x3_train_ref.py) against fp64 autograd and, routed through the oracle, against the fp32 oracle."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import _lib, config as C
from tests import x3_ref as X
from tests import x3_train_ref as XT
from tests.synth import synth_inputs, synth_state_dict
from tests.test_oracle_golden import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_math_setter_and_getter():
    from psld_amd import ops
    lib = _lib.load()
    before, mode = lib.psld_get_record_math(), lib.psld_get_math_mode()
    try:
        assert lib.psld_set_record_math(2) == 0 and lib.psld_get_record_math() == 2
        for bad in (0, 3, -1):          # f32 is no record math
            assert lib.psld_set_record_math(bad) != 0 and b"psld_set_record_math" in lib.psld_last_error()
            assert lib.psld_get_record_math() == 2
        assert lib.psld_get_math_mode() == mode             # the two settings are independent
        assert lib.psld_set_record_math(1) == 0 and ops.record_math() == "bf16x6"
        ops.set_record_math("bf16x3")
        assert ops.record_math() == "bf16x3" and lib.psld_get_record_math() == 2
        with pytest.raises(ValueError):
            ops.set_record_math("f32")
        assert ops.record_math() == "bf16x3"
        lib.psld_set_math_mode(mode)
        assert lib.psld_get_record_math() == 2
    finally:
        lib.psld_set_record_math(before)
    assert lib.psld_set_math_mode(3) != 0                   # still no fourth math mode
    lib.psld_set_math_mode(mode)


@pytest.mark.parametrize("value,mode,record", [(None, 1, 1), ("bf16x6", 1, 1), ("bf16x3", 2, 1), ("bf16x3_train", 2, 2),
                                               ("f32", 0, 1), ("bf16x3_training", 1, 1)])
def test_environment_spelling(value, mode, record):
    """PSLD_MATH is read once per process: each spelling in a child process, through either getter first."""
    env = {k: v for k, v in os.environ.items() if k != "PSLD_MATH"}
    if value is not None:
        env["PSLD_MATH"] = value
    for order in ("m, r = lib.psld_get_math_mode(), lib.psld_get_record_math()",
                  "r, m = lib.psld_get_record_math(), lib.psld_get_math_mode()"):
        code = f"from psld_amd import _lib; lib = _lib.load(); {order}; print(m, r)"
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split() == [str(mode), str(record)], (value, out.stdout)


def test_cli_train_math_option():
    from psld_amd import cli
    ap = cli.build_parser()
    for cmd in ("train", "train_clf"):
        for mode in ("bf16x6", "bf16x3"):
            assert ap.parse_args([cmd, "--train-math", mode]).train_math == mode
        assert ap.parse_args([cmd]).train_math is None        # default: the process's setting is left alone
        with pytest.raises(SystemExit):
            ap.parse_args([cmd, "--train-math", "f32"])
        with pytest.raises(SystemExit):
            ap.parse_args([cmd, "--math", "bf16x3"])          # no abbreviation reaches it
    for cmd in ("sample", "cc_sample", "inpaint"):
        with pytest.raises(SystemExit):
            ap.parse_args([cmd, "--train-math", "bf16x3"])


def test_two_limb_gradients_agree_with_fp64_autograd():
    """Weight gradient (Winograd domain) and data gradient of one 3x3 layer against fp64 autograd: near 2^-17, and away
    from fp32 (the arithmetic really is narrower)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 16, 16, generator=g)
    w = torch.randn(96, 64, 3, 3, generator=g) * 0.05
    dy = torch.randn(2, 96, 16, 16, generator=g)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    torch.nn.functional.conv2d(x64, w64, padding=1).backward(dy.double())
    ew, ed = rel_l2(XT.two_limb_wgrad3x3(x, dy), w64.grad), rel_l2(XT.two_limb_dgrad3x3(dy, w), x64.grad)
    print(f"two-limb gradients vs fp64: weight gradient {ew:.2e}, data gradient {ed:.2e}")
    assert 1e-6 < ew < 2e-5 and 1e-6 < ed < 2e-5
    # the transforms themselves are exact re-associations: in fp64, without the split, the Winograd-domain form is the gradient
    du = torch.einsum("pto,ptc->poc", XT.wino_m(dy).double().reshape(16, -1, 96), XT.wino_v_cols_first(x).double().reshape(16, -1, 64))
    exact = torch.einsum("ia,jb,ijoc->ocab", XT._G, XT._G, du.reshape(4, 4, 96, 64))
    assert rel_l2(exact, w64.grad) < 1e-6
    # and the column-first V is the row-first V of the forward reference up to fp32 rounding
    assert rel_l2(XT.wino_v_cols_first(x), X.wino_v(x)) < 1e-6


def test_routed_oracle_forward_and_backward_on_a_128_channel_net(monkeypatch):
    """The oracle's loss and parameter gradients with every contraction of forward, data gradient and weight gradient in
    two-limb arithmetic against the fp32 oracle on C.tiny(nf=128, ch_mult=(1, 1)): inside the 1e-4 contract (global
    rel-L2 over all parameter gradients), and measurably apart from fp32."""
    cfg = C.tiny(nf=128, ch_mult=(1, 1))
    from psld_amd.registry import get_module
    import psld_amd
    psld_amd.import_modules_into_registry()
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7)
    x0, eps, t = synth_inputs(2, 3, 16, seed=3)
    sde = O.PSLDOracle.from_config(cfg)

    def run():
        osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
        loss = O.psld_score_loss(sde, x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
        loss.backward()
        return loss.detach(), {k: v.grad for k, v in osd.items() if v.grad is not None}
    l32, g32 = run()
    XT.route_oracle_autograd(monkeypatch, O)
    l2, g2 = run()
    monkeypatch.undo()
    assert g2.keys() == g32.keys()
    num = torch.stack([(g2[k].double() - g32[k].double()).norm() for k in g32]).norm().item()
    den = torch.stack([g32[k].double().norm() for k in g32]).norm().item()
    print(f"two-limb routed oracle, tiny nf=128: loss {l2.item():.6f} vs {l32.item():.6f}, gradients global rel-L2 {num / den:.3e}")
    assert abs(l2.item() - l32.item()) < 1e-4 * abs(l32.item())
    assert 1e-7 < num / den < 1e-4

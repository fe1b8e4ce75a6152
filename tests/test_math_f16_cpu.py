"""Eval math 'f16' (one fp16 product; reference-GPU-equivalent, NOT fp32-equivalent inference) - what can be checked without a
GPU: the setting and the byte counts of the C ABI, the CLI option, the CPU reference of the arithmetic (tests/f16_ref.py)
that the GPU tests lean on, and its distance from the reference goldens against the yardstick the mode is offered on: the same
oracle with operands rounded to TF32, the reference's own default GPU convolution arithmetic."""
import json
import os

import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import _lib, config as C
from tests import f16_ref as H
from tests import x3_ref as X
from tests.conftest import GOLDEN
from tests.synth import synth_state_dict
from tests.test_oracle_golden import T, _net_cfg, _net_meta, rel_l2


def _f16_meta():
    with open(os.path.join(GOLDEN, "f16_meta.json")) as fh:
        return json.load(fh)


def test_setting_round_trip_and_byte_counts():
    from psld_amd import ops
    lib = _lib.load()
    before, mode = lib.psld_get_eval_math(), lib.psld_get_math_mode()
    try:
        assert lib.psld_set_eval_math(1) == 0 and lib.psld_get_eval_math() == 1
        assert lib.psld_set_eval_math(2) != 0 and b"psld_set_eval_math" in lib.psld_last_error()
        assert lib.psld_set_eval_math(-1) != 0 and lib.psld_get_eval_math() == 1        # a refusal leaves the setting alone
        assert lib.psld_get_math_mode() == mode                                        # a setting of its own
        assert lib.psld_set_math_mode(3) != 0 and b"psld_set_math_mode" in lib.psld_last_error()   # the enumeration did not grow
        assert lib.psld_set_eval_math(0) == 0 and lib.psld_get_eval_math() == 0
        ops.set_eval_math("f16")
        assert ops.eval_math() == "f16" and lib.psld_get_eval_math() == 1
        ops.set_eval_math("limb")
        assert ops.eval_math() == "limb"
        with pytest.raises(ValueError):
            ops.set_eval_math("bf16")
    finally:
        lib.psld_set_eval_math(before)
    for cout, cin in ((128, 128), (256, 512), (160, 320), (480, 320)):
        pad = 16384
        one = lib.psld_conv3x3_wino_frag_bytes_f16(cout, cin)
        assert one == cout * cin * 16 * 2 + pad
        assert 2 * (one - pad) == lib.psld_conv3x3_wino_frag_bytes_x3(cout, cin) - pad
        assert ops.conv3x3_wino_frag_bytes_f16(cout, cin) == one
        assert lib.psld_gemm_frag_bytes_f16(cout, cin) == cout * cin * 2
        assert 2 * lib.psld_gemm_frag_bytes_f16(cout, cin) == lib.psld_gemm_frag_bytes_x3(cout, cin)
    for row in ((512, 0, 8 * 32 * 32, 256), (512, 0, 16 * 32 * 32, 256), (256, 256, 16 * 32 * 32, 256),
                (256, 0, 16 * 32 * 32, 128), (160, 0, 64 * 32 * 32, 256)):
        assert lib.psld_gemm_split_f16_supported(*row) == lib.psld_gemm_split_x3_supported(*row)
        assert ops.gemm_split_f16_wanted(*row) == ops.gemm_split_x3_wanted(*row)
    assert lib.psld_gemm_split_f16_supported(512, 0, 16 * 32 * 32, 256) == 1


def test_environment_value_selects_both_settings():
    """PSLD_MATH=f16 is a value of the one existing variable: math mode bf16x3 + eval math f16, record math untouched."""
    import subprocess
    import sys
    code = "from psld_amd import ops; print(ops.math_mode(), ops.eval_math(), ops.record_math())"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("f16", "bf16x3 f16 bf16x6"), ("bf16x3", "bf16x3 limb bf16x6"), ("", "bf16x6 limb bf16x6")):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PSLD_MATH=value), cwd=root, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])


def test_cli_math_option():
    from psld_amd import cli
    ap = cli.build_parser()
    for cmd in ("sample", "cc_sample", "inpaint"):
        assert ap.parse_args([cmd, "--math", "f16"]).math == "f16"
        assert ap.parse_args([cmd]).math is None
    with pytest.raises(SystemExit):
        ap.parse_args(["train", "--math", "f16"])
    with pytest.raises(SystemExit):
        ap.parse_args(["sample", "--math", "bf16"])


def test_round_f16_clamps_and_rounds_to_nearest_even():
    x = torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.0, 65520.0, 7e4, 1e6, -1e6, 3e38, -3e38,
                      2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 1e-10])
    want = torch.tensor([0.0, 1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0,
                         2.0 ** -24, 0.0, 2.0 ** -24, 0.0])
    assert torch.equal(H.round_f16(x), want)
    g = torch.Generator().manual_seed(7)
    r = torch.randn(4096, generator=g)
    assert bool(((H.round_f16(r) - r).abs() <= r.abs() * 2.0 ** -11).all())
    assert bool(((H.round_tf32(r) - r).abs() <= r.abs() * 2.0 ** -11).all())
    assert torch.equal(H.round_tf32(r).view(torch.int32) & 0x1fff, torch.zeros(4096, dtype=torch.int32))


def test_f16_conv_forms_agree_with_fp64():
    """The Winograd form and the im2col form of the reference against a true fp64 convolution on tests/x3_ref.py's test shape:
    within a factor 2 of each other (one rounding per operand either way, near 2^-12), and strictly above the two-limb
    reference's error on the same data - the arithmetic really is narrower."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 16, 16, generator=g)
    w = torch.randn(96, 64, 3, 3, generator=g) * 0.05
    ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    ew = rel_l2(H.f16_conv3x3(x, w), ref)
    xo = x[:, :, :15, :15]
    refo = torch.nn.functional.conv2d(xo.double(), w.double(), padding=1)
    ed = rel_l2(H.f16_conv2d(xo, w, None, 1, 1).double(), refo)
    e2w = rel_l2(X.two_limb_conv3x3(x, w), ref)
    e2d = rel_l2(X.two_limb_conv2d(xo, w, None, 1, 1).double(), refo)
    print(f"f16 conv vs fp64: Winograd form {ew:.2e}, direct form {ed:.2e} (two-limb reference: {e2w:.2e}, {e2d:.2e})")
    assert 0.5 * ed <= ew <= 2 * ed
    assert ew > e2w and ed > e2d


def _forward_err(golden, monkeypatch, name, rnd):
    meta = _net_meta()[name]
    g_ = golden(f"net_{name}.npz")
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    with monkeypatch.context() as m:
        H.route_oracle(m, O, rnd)
        with torch.no_grad():
            y = O.ncsnpp_forward(sd, _net_cfg(name), T(g_["x"]), T(g_["t"]))
    return rel_l2(y, T(g_["y"]))


@pytest.mark.parametrize("name", ["c10_sota", "celeba64"])
def test_reference_forward_against_goldens(golden, monkeypatch, name):
    """The oracle with its contractions on operands rounded once to fp16 against the reference's own outputs: no farther
    (x1.25: tie handling and the clamp differ) than the same oracle on TF32-rounded operands, and the figure the GPU tests
    are bounded by (tests/golden/f16_meta.json) is this one."""
    e16 = _forward_err(golden, monkeypatch, name, H.round_f16)
    e32 = _forward_err(golden, monkeypatch, name, H.round_tf32)
    print(f"f16 reference forward {name}: rel-L2 {e16:.3e} vs the reference golden (TF32-rounded operands: {e32:.3e})")
    assert e16 <= 1.25 * e32
    assert e16 > 1e-4                      # outside the parity contract: what the documents say
    rec = _f16_meta()[name]
    assert abs(rec["f16"] - e16) <= 1e-3 * e16 and abs(rec["tf32"] - e32) <= 1e-3 * e32


@pytest.mark.parametrize("stride", ["uniform", "quadratic"])
def test_reference_em_sampler_against_goldens(golden, monkeypatch, stride):
    g = golden("em_c10_sota.npz")
    cfg = C.c10_sota()
    sde = O.PSLDOracle.from_config(cfg)
    meta = _net_meta()["c10_sota"]
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    ts, n = O.sampling_times(sde.T, cfg.evaluation.eval_eps, 4, True, stride)
    err = {}
    for tag, rnd in (("f16", H.round_f16), ("tf32", H.round_tf32)):
        with monkeypatch.context() as m:
            H.route_oracle(m, O, rnd)
            with torch.no_grad():
                x = O.em_sample(sde, lambda u, tt: O.ncsnpp_forward(sd, cfg, u, tt), T(g[f"batch_{stride}"]), ts, n, True,
                                cfg.evaluation.eval_eps, noise=list(T(g[f"noise_{stride}"])))
        err[tag] = rel_l2(x, T(g[f"x_{stride}"]))
    print(f"f16 reference EM sampler ({stride}): rel-L2 {err['f16']:.3e} vs the reference golden (TF32-rounded: {err['tf32']:.3e})")
    assert err["f16"] <= 1.25 * err["tf32"]
    rec = _f16_meta()[f"em_{stride}"]
    assert abs(rec["f16"] - err["f16"]) <= 1e-3 * err["f16"]


def test_fixture_lists_every_network_of_the_gpu_tests():
    m = _f16_meta()
    assert set(m) == {"c10_sota", "celeba64", "afhqv2_128", "afhqv2_128_inpaint", "em_uniform", "em_quadratic"}
    for name, rec in m.items():
        assert 1e-4 < rec["f16"] <= 1.25 * rec["tf32"], name

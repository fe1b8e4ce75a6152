"""Math mode 'bf16x3' (two bf16 limbs, three products; reduced-precision inference) - what can be checked without a GPU:
the mode switch and the two-limb byte counts of the C ABI, the CLI option, and the CPU reference of the arithmetic
(tests/x3_ref.py) that the GPU tests lean on, against the reference goldens."""
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import _lib, config as C
from tests import x3_ref as X
from tests.synth import synth_state_dict
from tests.test_oracle_golden import T, _net_cfg, _net_meta, rel_l2


def test_mode_switch_and_byte_counts():
    from psld_amd import ops
    lib = _lib.load()
    before = lib.psld_get_math_mode()
    try:
        assert lib.psld_set_math_mode(2) == 0 and lib.psld_get_math_mode() == 2
        assert lib.psld_set_math_mode(3) != 0 and b"psld_set_math_mode" in lib.psld_last_error()
        assert lib.psld_get_math_mode() == 2
        assert lib.psld_set_math_mode(1) == 0
        ops.set_math_mode("bf16x3")
        assert ops.math_mode() == "bf16x3" and lib.psld_get_math_mode() == 2
        ops.set_math_mode("bf16x6")
        assert ops.math_mode() == "bf16x6"
    finally:
        lib.psld_set_math_mode(before)
    for cout, cin in ((128, 128), (256, 512), (160, 320), (480, 320)):
        pad = lib.psld_conv3x3_wino_frag_bytes(cout, cin) - cout * cin * 16 * 6
        assert pad == 16384
        two = lib.psld_conv3x3_wino_frag_bytes_x3(cout, cin)
        assert two == cout * cin * 16 * 4 + pad
        assert 3 * (two - pad) == 2 * (lib.psld_conv3x3_wino_frag_bytes(cout, cin) - pad)
        assert ops.conv3x3_wino_frag_bytes_x3(cout, cin) == two
    for n, k in ((256, 256), (768, 256), (256, 512)):
        assert lib.psld_gemm_frag_bytes_x3(n, k) == n * k * 4
        assert 3 * lib.psld_gemm_frag_bytes_x3(n, k) == 2 * lib.psld_gemm_frag_bytes(n, k)
    # the two-limb pointwise GEMM is the eight-wave kernel of 128 x 256 tiles; the executor takes it from 128 tiles on
    assert lib.psld_gemm_split_x3_supported(512, 0, 8 * 32 * 32, 256) == 1
    assert not ops.gemm_split_x3_wanted(512, 0, 8 * 32 * 32, 256) and ops.gemm_split_x3_wanted(512, 0, 16 * 32 * 32, 256)
    assert lib.psld_gemm_split_x3_supported(256, 256, 16 * 32 * 32, 256) == 1
    assert lib.psld_gemm_split_x3_supported(256, 0, 16 * 32 * 32, 128) == 0           # n % 256
    assert lib.psld_gemm_split_x3_supported(160, 0, 64 * 32 * 32, 256) == 0           # what psld_gemm_split_supported refuses


def test_cli_math_option():
    from psld_amd import cli
    ap = cli.build_parser()
    for cmd in ("sample", "cc_sample", "inpaint"):
        for mode in ("bf16x6", "bf16x3", "f32"):
            assert ap.parse_args([cmd, "--math", mode]).math == mode
        assert ap.parse_args([cmd]).math is None          # default: the process's mode is left alone
    with pytest.raises(SystemExit):
        ap.parse_args(["sample", "--math", "bf16"])
    with pytest.raises(SystemExit):
        ap.parse_args(["train", "--math", "bf16x3"])      # training is fp32-equivalent: no such option


def test_split2_is_the_head_of_the_three_limb_split():
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.randn(4096, generator=g),
                   torch.randn(4096, generator=g) * 1e-38, torch.randn(4096, generator=g) * 1e-41,      # denormal range
                   torch.randn(4096, generator=g) * 1e30, torch.randn(4096, generator=g) * 3e38,
                   torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 2.0 ** -149, 65504.0, 3.0e38])])
    x = x[torch.isfinite(x)]
    hi2, lo2 = X.split2(x)
    hi3, mid3, lo3 = X.split3(x)
    assert torch.equal(hi2.view(torch.int32), hi3.view(torch.int32))
    assert torch.equal(lo2.view(torch.int32), mid3.view(torch.int32))
    # both are bf16 values; in the normal range the two limbs carry x to 2^-16 and the three limbs carry it exactly
    ok = torch.isfinite(hi2)              # rne_bf16 of the largest fp32 values is infinite
    for t in (hi2, lo2, lo3):
        assert torch.equal(t[ok], t[ok].to(torch.bfloat16).float())
    normal = ok & (x.abs() > 1e-30)
    assert bool(((hi2 + lo2 - x)[normal].abs() <= x[normal].abs() * 2.0 ** -16).all())
    assert torch.equal(((hi3 + mid3) + lo3)[normal], x[normal])


def test_two_limb_conv_forms_agree_with_fp64():
    """The Winograd form and the im2col form of the reference against a true fp64 convolution: both near 2^-17, and far
    from fp32 (the arithmetic really is narrower)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 16, 16, generator=g)
    w = torch.randn(96, 64, 3, 3, generator=g) * 0.05
    ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    ew = rel_l2(X.two_limb_conv3x3(x, w), ref)
    ed = rel_l2(X.two_limb_conv2d(x[:, :, :15, :15], w, None, 1, 1).double(),
                torch.nn.functional.conv2d(x[:, :, :15, :15].double(), w.double(), padding=1))
    print(f"two-limb conv vs fp64: Winograd form {ew:.2e}, direct form {ed:.2e}")
    assert 1e-6 < ew < 2e-5 and 1e-6 < ed < 2e-5


@pytest.mark.parametrize("name", ["c10_sota", "celeba64"])
def test_reference_forward_against_goldens(golden, monkeypatch, name):
    """The oracle with its contractions in two-limb arithmetic against the reference's own outputs: inside the 1e-4 parity
    contract, and measurably apart from the fp32 oracle (0 - 5e-7)."""
    meta = _net_meta()[name]
    g = golden(f"net_{name}.npz")
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    X.route_oracle(monkeypatch, O)
    with torch.no_grad():
        y = O.ncsnpp_forward(sd, _net_cfg(name), T(g["x"]), T(g["t"]))
    err = rel_l2(y, T(g["y"]))
    print(f"two-limb reference forward {name}: rel-L2 {err:.3e} vs the reference golden")
    assert 2e-6 < err < 1e-4


def test_reference_em_sampler_against_goldens(golden, monkeypatch):
    g = golden("em_c10_sota.npz")
    cfg = C.c10_sota()
    sde = O.PSLDOracle.from_config(cfg)
    meta = _net_meta()["c10_sota"]
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    X.route_oracle(monkeypatch, O)
    for stride in ("uniform", "quadratic"):
        ts, n = O.sampling_times(sde.T, cfg.evaluation.eval_eps, 4, True, stride)
        with torch.no_grad():
            x = O.em_sample(sde, lambda u, tt: O.ncsnpp_forward(sd, cfg, u, tt), T(g[f"batch_{stride}"]), ts, n, True,
                            cfg.evaluation.eval_eps, noise=list(T(g[f"noise_{stride}"])))
        err = rel_l2(x, T(g[f"x_{stride}"]))
        print(f"two-limb reference EM sampler ({stride}): rel-L2 {err:.3e} vs the reference golden")
        assert 2e-6 < err < 1e-4

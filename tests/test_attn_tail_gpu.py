"""Attention at 480 channels (the nf = 160 AFHQv2-128 inpainting network) on the GPU: the fused forward kernel's C = 480
instances and the cut-tile batched limb GEMM (ops.bgemm_split_tail) against fp64 within the limb kernels' 3e-6, bit for bit
against themselves and against the full-tile kernel on zero-padded operands, between guard bands, AttnBlockpp(480) against
the oracle, and the network - where no batched product of the 16x16 level may reach the fp32 tile engine any more."""
import functools

import pytest
import torch

from oracle import psld_oracle as O
from tests import guard as G
from tests.synth import synth_inputs, synth_state_dict
from tests.test_afhq160_gpu import S, _build, _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse here too)
from tests.test_blocks_gpu import Harness, _nchw, _nhwc
from tests.test_kernels_gpu import gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = 3e-6             # the project's gate for every limb kernel against fp64
C = 480


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# fused forward, C = 480
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attn_case(b, hw):
    """q | k | v (CPU, the recipe of test_fused_attention_forward) and the fp64 probabilities / output, once per shape."""
    g = torch.Generator().manual_seed(90)
    qkv = torch.randn(b, hw, 3 * C, generator=g) * 1.5
    scale = float(C) ** -0.5
    q64, k64, v64 = (t.double() for t in qkv.split(C, dim=-1))
    pref = torch.softmax(torch.einsum("bic,bjc->bij", q64, k64) * scale, dim=-1)
    return qkv, scale, pref, torch.einsum("bij,bjc->bic", pref, v64)


@pytest.mark.parametrize("fused_buf", [True, False], ids=["one-buffer", "three-tensors"])
@pytest.mark.parametrize("b,hw", [(1, 64), (3, 64), (1, 256), (3, 256)])
def test_fused_attention_forward_c480(ops, b, hw, fused_buf):
    """softmax(scale q k^T) v in one kernel at c = 480 against fp64; the run without p is bitwise the run with it; two runs
    are bitwise equal; at hw = 256 agreement with QK^T on bgemm_split + softmax_rows + PV on bgemm_split_tail."""
    assert ops.attn_fwd_supported(hw, C)
    qkv, scale, pref, oref = _attn_case(b, hw)
    dev = qkv.to(DEV)
    if fused_buf:
        q, k, v, ld = dev[..., :C], dev[..., C:2 * C], dev[..., 2 * C:], 3 * C
    else:
        q, k, v = (t.contiguous() for t in dev.split(C, dim=-1))
        ld = C

    def run(with_p):
        out, p = _nan(b, hw, C), _nan(b, hw, hw) if with_p else None
        ops.attn_fwd(q, k, v, ld, b, hw, C, scale, out, p)
        return out, p
    out, p = run(True)
    eo, ep = rel_l2(out, oref), rel_l2(p, pref)
    print(f"fused attention b={b} hw={hw} c={C} one buffer={fused_buf}: out rel-L2 {eo:.2e}  p rel-L2 {ep:.2e}")
    assert eo < GATE and ep < GATE
    assert torch.equal(out, run(False)[0])
    out2, p2 = run(True)
    assert torch.equal(out, out2) and torch.equal(p, p2)
    if hw != 256:
        return
    assert ops.bgemm_split_supported(0, 1, hw, hw, C) and ops.bgemm_split_tail_supported(0, 0, hw, C, hw)
    p3 = _nan(b, hw, hw)
    ops.bgemm_split(0, 1, hw, hw, C, q, ld, hw * ld, k, ld, hw * ld, p3, hw, hw * hw, b, scale)
    ops.softmax_rows(p3, p3, b * hw, hw)
    o3 = _nan(b, hw, C)
    ops.bgemm_split_tail(0, 0, hw, C, hw, p3, hw, hw * hw, v, ld, hw * ld, o3, C, hw * C, b)
    e3, ep3 = rel_l2(out, o3), rel_l2(p, p3)
    print(f"    against the three launches: out {e3:.2e}  p {ep3:.2e}")
    assert e3 < GATE and ep3 < GATE


# ---------------------------------------------------------------------------------------------------------------------
# cut-tile batched GEMM
# ---------------------------------------------------------------------------------------------------------------------
def _operands(ta, tb, m, n, k, batch, pad=0):
    """A, B as test_bgemm_split makes them (``pad`` leading columns that the launch must not use), their used parts."""
    A = gen(batch, *((k, m + pad) if ta else (m, k + pad)), seed=77)
    B = gen(batch, *((n, k + pad) if tb else (k, n + pad)), seed=78)
    return A, B, (A[:, :, pad:] if pad else A), (B[:, :, pad:] if pad else B)


def _tail(ops, ta, tb, m, n, k, batch, A, B, pad, alpha=0.25, launch=None):
    out = _nan(batch, m, n + pad)
    lda, ldb = A.shape[2], B.shape[2]
    (launch or ops.bgemm_split_tail)(ta, tb, m, n, k, A.view(-1)[pad:], lda, A.shape[1] * lda, B.view(-1)[pad:], ldb,
                                     B.shape[1] * ldb, out.view(-1)[pad:], n + pad, m * (n + pad), batch, alpha)
    return out


def _check_tail(ops, ta, tb, m, n, k, batch, pad):
    assert ops.bgemm_split_tail_supported(ta, tb, m, n, k) and not ops.bgemm_split_supported(ta, tb, m, n, k)
    A, B, a_use, b_use = _operands(ta, tb, m, n, k, batch, pad)
    opa = a_use.double().transpose(1, 2) if ta else a_use.double()
    opb = b_use.double().transpose(1, 2) if tb else b_use.double()
    ref = 0.25 * opa @ opb
    Ad, Bd = A.to(DEV), B.to(DEV)
    out = _tail(ops, ta, tb, m, n, k, batch, Ad, Bd, pad)
    err = rel_l2(out[:, :, pad:], ref)
    print(f"bgemm tail ta={ta} tb={tb} m={m} n={n} k={k} batch={batch} pad={pad}: rel-L2 {err:.2e}")
    assert err < GATE
    if pad:
        assert bool(torch.isnan(out[:, :, :pad]).all())
    assert torch.equal(out[:, :, pad:], _tail(ops, ta, tb, m, n, k, batch, Ad, Bd, pad)[:, :, pad:])
    # the full-tile kernel on B zero-padded to whole tiles (its own buffers: the tail launch above never saw them)
    npad = -(-n // 128) * 128
    Bp = torch.zeros(batch, *((npad, k) if tb else (k, npad)), device=DEV)
    if tb:
        Bp[:, :n] = b_use.to(DEV)
    else:
        Bp[:, :, :n] = b_use.to(DEV)
    full = _tail(ops, ta, tb, m, npad, k, batch, a_use.contiguous().to(DEV), Bp, 0, launch=ops.bgemm_split)
    assert torch.equal(out[:, :, pad:], full[:, :, :n])


@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("k", [32, 96, 256])
@pytest.mark.parametrize("n", [160, 192, 480])
@pytest.mark.parametrize("m", [128, 256])
def test_bgemm_split_tail(ops, ta, tb, m, n, k, batch):
    """NT / NN / TN with 32, 64 and 96 live columns in the cut tile (half a wave's columns, exactly one wave's, one and a
    half): fp64 within 3e-6; bit for bit the live columns of bgemm_split on B zero-padded to the next multiple of 128; twice
    bitwise."""
    _check_tail(ops, ta, tb, m, n, k, batch, 0)


@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0)])
def test_bgemm_split_tail_strided(ops, ta, tb):
    """Operands that are column slices (64 leading columns the launch must not use) and the output behind 64 columns of a
    wider NaN-filled buffer, which stay NaN - as test_bgemm_split does with ``pad``."""
    _check_tail(ops, ta, tb, 256, 480, 96, 3, 64)


def test_bgemm_split_tail_writes_nothing_beyond_n(ops):
    """ldc wider than n, no padding in front: the columns behind n of every row stay NaN in all three forms."""
    m, n, k, batch = 128, 160, 32, 2
    for ta, tb in ((0, 1), (0, 0), (1, 0)):
        A, B, _, _ = _operands(ta, tb, m, n, k, batch)
        out = _nan(batch, m, 256)
        ops.bgemm_split_tail(ta, tb, m, n, k, A.to(DEV), A.shape[2], A.shape[1] * A.shape[2], B.to(DEV), B.shape[2],
                             B.shape[1] * B.shape[2], out, 256, m * 256, batch)
        assert bool(torch.isfinite(out[:, :, :n]).all()) and bool(torch.isnan(out[:, :, n:]).all())


def test_bgemm_split_tail_predicate(ops):
    for ta, tb in ((0, 1), (0, 0), (1, 0)):
        assert ops.bgemm_split_tail_supported(ta, tb, 256, 480, 256)
        assert not ops.bgemm_split_tail_supported(ta, tb, 64, 480, 256)
        assert not ops.bgemm_split_tail_supported(ta, tb, 256, 96, 256)
        assert not ops.bgemm_split_tail_supported(ta, tb, 256, 256, 256)         # the full-tile kernel's
        assert not ops.bgemm_split_tail_supported(ta, tb, 256, 480, 48)
    assert not ops.bgemm_split_tail_supported(1, 1, 256, 480, 256)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 64 << 20)
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.fixture
def guard(ops, pool, monkeypatch):
    if pool.regions:
        pool.check()
        pool.release()
    return G.Guard(ops, pool).install(monkeypatch)


@pytest.mark.parametrize("with_p", [True, False], ids=["p", "no-p"])
@pytest.mark.parametrize("b,hw", [(2, 64), (1, 256)])
def test_guarded_fused_attention_c480(ops, guard, b, hw, with_p):
    """q | k | v in one [b, hw, 3c] buffer that ends flush against the band (v's last row is the buffer's last bytes)."""
    qkv, scale, pref, oref = _attn_case(b, hw)

    def fn(qkv, out, p=None):
        ops.attn_fwd(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], 3 * C, b, hw, C, scale, out, p)
    tensors = dict(qkv=qkv.to(DEV), out=torch.zeros(b, hw, C, device=DEV))
    if with_p:
        tensors["p"] = torch.zeros(b, hw, hw, device=DEV)
    plain, _ = G.run_guarded(guard, fn, tensors, ["out", "p"] if with_p else ["out"])
    assert rel_l2(plain["out"], oref) < GATE
    if with_p:
        assert rel_l2(plain["p"], pref) < GATE


@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0)])
def test_guarded_bgemm_split_tail(ops, guard, ta, tb):
    """Operands of exactly batch x rows x columns floats: the last row of the last batch ends at the band."""
    m, n, k, batch = 128, 160, 32, 2
    A, B, _, _ = _operands(ta, tb, m, n, k, batch)

    def fn(a, b, c):
        ops.bgemm_split_tail(ta, tb, m, n, k, a, a.shape[2], a.shape[1] * a.shape[2], b, b.shape[2], b.shape[1] * b.shape[2],
                             c, n, m * n, batch)
    plain, _ = G.run_guarded(guard, fn, dict(a=A.to(DEV), b=B.to(DEV), c=torch.zeros(batch, m, n, device=DEV)), ["c"])
    opa = A.double().transpose(1, 2) if ta else A.double()
    opb = B.double().transpose(1, 2) if tb else B.double()
    assert rel_l2(plain["c"], opa @ opb) < GATE


# ---------------------------------------------------------------------------------------------------------------------
# the block and the network
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_case(hw):
    """Parameters, input, output gradient and the fp64 oracle's results of AttnBlockpp(480) on a [2, 480, hw, hw] map."""
    from psld_amd import score_fn as SF
    mod = SF.AttnBlockpp(C)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in mod.state_dict().items()], 78)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, C, hw, hw, generator=g)
    osd = {f"m.{k}": v.double().requires_grad_(True) for k, v in sd.items()}
    xo = x.double().requires_grad_(True)
    yo = O.attn_block(xo, osd, "m")
    gy = torch.randn(*yo.shape, generator=g)
    yo.backward(gy.double())
    return sd, x, gy, yo.detach(), xo.grad, {k: osd[f"m.{k}"].grad for k in sd}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "three-launches"])
@pytest.mark.parametrize("hw", [16, 8])
def test_attention_block_c480_against_the_oracle(monkeypatch, hw, fused):
    """AttnBlockpp(480) through _Exec.attn, forward within 5e-6 and gradients within 1e-5 of oracle.attn_block in fp64 (the
    gates of test_wide_attention_against_the_oracle) - with the fused forward kernel and with ``fused_attn`` off (16x16: QK^T
    on the full-tile batched kernel, softmax, PV on the cut-tile one)."""
    from psld_amd import ops, score_fn as SF
    sd, x, gy, yo, gx, gw = _block_case(hw)
    h = Harness(SF.AttnBlockpp(C), sd)
    h.ex.fused_attn = fused
    calls = []
    fwd, tail = ops.attn_fwd, ops.bgemm_split_tail
    monkeypatch.setattr(ops, "attn_fwd", lambda *a, **k: (calls.append("attn_fwd"), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "bgemm_split_tail", lambda *a, **k: (calls.append("tail"), tail(*a, **k))[1])
    xn = h.S._Node(_nhwc(x))
    with h.ops.stream_scope():
        out = h.ex.attn(xn, h.mod)
    ef = rel_l2(_nchw(out.v), yo)
    h.backward(out, _nhwc(gy))
    eg = rel_l2(_nchw(xn.g), gx)
    print(f"AttnBlockpp(480) @{hw}x{hw} fused={fused}: forward {ef:.2e}  grad_x {eg:.2e}  launches {calls}")
    assert calls.count("attn_fwd") == (1 if fused else 0)
    assert calls.count("tail") == (0 if hw == 8 else (3 if fused else 4))
    assert ef < 5e-6
    assert eg < 1e-5
    for k in sd:
        if k == "NIN_1.b":      # the softmax is invariant to k's bias: the gradient is rounding noise around zero
            assert float(h.grad(k).abs().max()) < 1e-4 * float(h.grad("NIN_0.b").abs().max())
            continue
        e = rel_l2(h.grad(k), gw[k])
        print(f"    {k}: {e:.2e}")
        assert e < 1e-5, k


def test_afhq160_dispatch_keeps_the_16x16_attention_off_the_tile_engine(monkeypatch):
    """One training step and one eval forward at B = 4 with recording wrappers on ops.gemm_raw, ops.attn_fwd and
    ops.bgemm_split_tail.  Eval: no batched tile-engine GEMM at all, the fused kernel once per AttnBlockpp and without p.
    Training: the only batched tile-engine GEMMs are the 8x8 level's (M = 64 or N = 64, none with 256 rows or columns), and
    the cut-tile kernel runs dV, dQ and dK of every 16x16 block."""
    from psld_amd import ops
    from psld_amd import score_fn as SF
    from psld_amd.registry import get_module
    raw, fused, tails = [], [], []
    gemm, fwd, tail = ops.gemm_raw, ops.attn_fwd, ops.bgemm_split_tail

    def rec_gemm(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, Cc, ldc, sc, batch=1, *a, **k):
        if batch > 1:
            raw.append((ta, tb, M, N, K))
        return gemm(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, Cc, ldc, sc, batch, *a, **k)

    def rec_fwd(q, k, v, ld, batch, hw, c, scale, out, p=None):
        fused.append((hw, c, p is not None))
        return fwd(q, k, v, ld, batch, hw, c, scale, out, p)

    def rec_tail(ta, tb, M, N, K, *a, **k):
        tails.append((ta, tb, M, N, K))
        return tail(ta, tb, M, N, K, *a, **k)
    monkeypatch.setattr(ops, "gemm_raw", rec_gemm)
    monkeypatch.setattr(ops, "attn_fwd", rec_fwd)
    monkeypatch.setattr(ops, "bgemm_split_tail", rec_tail)
    net, cfg, _ = _build(train=True)
    n_attn = sum(isinstance(m, SF.AttnBlockpp) for m in net.all_modules)
    assert n_attn >= 2
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    x0, eps, t = synth_inputs(4, 3, S, seed=5)
    loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    train_raw, train_fused, train_tails = list(raw), list(fused), list(tails)
    del raw[:], fused[:], tails[:]
    net.eval()
    with torch.no_grad():
        net(torch.randn(4, 6, S, S, device=DEV), torch.rand(4, device=DEV) * 0.9 + 0.05)
    torch.cuda.synchronize()
    print("eval: fused", fused, "batched tile-engine GEMMs", raw)
    print("train: fused", train_fused, "tail", train_tails, "batched tile-engine GEMMs", sorted(set(train_raw)))
    assert not raw
    assert len(fused) == n_attn and all(c == C and not with_p for _, c, with_p in fused)
    assert all((M == 64 or N == 64) and 256 not in (M, N, K) for _, _, M, N, K in train_raw), sorted(set(train_raw))
    assert len(train_fused) == n_attn and all(with_p for _, _, with_p in train_fused)
    n16 = sum(hw == 256 for hw, _, _ in train_fused)
    assert n16 >= 1
    assert len(train_tails) == 3 * n16 and all(M == 256 and N == C and K == 256 for _, _, M, N, K in train_tails)

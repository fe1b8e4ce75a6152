"""Pointwise limb GEMMs for channel widths in steps of 32 on the GPU (ops.gemm_split_tail / gemm_tn_split_tail and the tail
fragment packers): forward / data gradient and weight gradient against fp64 within the limb kernels' 3e-6, bit for bit
against the full-tile kernels on zero-padded operands, between guard bands, and in the nf = 160 AFHQv2-128 inpainting
network - where no limb-width pointwise contraction may reach the fp32 tile engine any more."""
import functools

import pytest
import torch

from psld_amd import score_routes as R
from tests import guard as G
from tests.synth import synth_inputs
from tests.test_afhq160_gpu import S, T, _build, _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse here too)
from tests.test_kernels_gpu import gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = 3e-6             # the project's gate for every limb kernel against fp64

KN = [(160, 160), (320, 480), (480, 320), (800, 160), (480, 1440)]


@functools.lru_cache(maxsize=None)
def _fwd_case(m, k, n):
    """Operands (CPU) and the fp64 product, computed once per shape."""
    a, w = gen(m, k, seed=11), gen(n, k, seed=12, scale=0.1)
    bias, res, prev = gen(n, seed=13), gen(m, n, seed=14), gen(m, n, seed=15)
    return a, w, bias, res, prev, a.double() @ w.double().t()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("m", [130, 1000])
@pytest.mark.parametrize("k,n", KN)
def test_gemm_split_tail_against_fp64(ops, m, k, n):
    """bias + residual + out_scale; alpha + accumulate; ldy = 3n into the middle third of a NaN-filled buffer - from an
    [n][k] and from a [k][n] (NIN.W) matrix; every launch twice, bit for bit."""
    a, w, bias, res, prev, ref = _fwd_case(m, k, n)
    assert ops.gemm_tail_supported(k, m, n) and not ops.gemm_split_supported(k, 0, m, n)
    ad, biasd, resd, prevd = a.to(DEV), bias.to(DEV), res.to(DEV), prev.to(DEV)
    frag = ops.gemm_frag_tail(w.to(DEV), n, k, k, 1)
    assert frag.numel() == ops.gemm_frag_bytes_tail(n, k)
    frag_t = ops.gemm_frag_tail(w.t().contiguous().to(DEV), n, k, 1, n)
    assert torch.equal(frag, frag_t)

    def run(epi, init, ldy=None, split=True):
        y = init.clone()
        ops.gemm_split_tail(ad, m, frag, n, y if ldy is None else y.view(-1)[n:], epi, ldy=ldy, allow_split=split)
        return y
    for split in (True, False):             # the executor's call (K split through the workspace where the grid is small), and one launch
        epi = ops.epilogue(bias=biasd, residual=resd, ld_residual=n, out_scale=0.5)
        y = run(epi, _nan(m, n), split=split)
        err = rel_l2(y, (ref + bias.double() + res.double()) * 0.5)
        print(f"tail forward m={m} k={k} n={n} split={split}: rel-L2 {err:.2e}")
        assert err < GATE
        assert torch.equal(y, run(epi, _nan(m, n), split=split))
        epi = ops.epilogue(alpha=0.25, accumulate=True)
        acc = run(epi, prevd, split=split)
        err = rel_l2(acc, ref * 0.25 + prev.double())
        print(f"tail accumulate m={m} k={k} n={n} split={split}: rel-L2 {err:.2e}")
        assert err < GATE
        assert torch.equal(acc, run(epi, prevd, split=split))
        wide = run(ops.epilogue(bias=biasd), _nan(m, 3 * n), ldy=3 * n, split=split)
        err = rel_l2(wide[:, n:2 * n], ref + bias.double())
        print(f"tail ldy=3n m={m} k={k} n={n} split={split}: rel-L2 {err:.2e}")
        assert err < GATE
        assert bool(torch.isnan(wide[:, :n]).all()) and bool(torch.isnan(wide[:, 2 * n:]).all())
        again = run(ops.epilogue(bias=biasd), _nan(m, 3 * n), ldy=3 * n, split=split)
        assert torch.equal(wide[:, n:2 * n], again[:, n:2 * n])


def test_gemm_split_tail_split_k(ops):
    """m = 128, (k, n) = (960, 480): four tiles - the K range is cut over workgroups and reduced with the epilogue."""
    m, k, n = 128, 960, 480
    a, w, bias, res, prev, ref = _fwd_case(m, k, n)
    ad, frag = a.to(DEV), ops.gemm_frag_tail(w.to(DEV), n, k, k, 1)
    epi = ops.epilogue(bias=bias.to(DEV), residual=res.to(DEV), ld_residual=n, out_scale=0.5)
    ys = []
    for split in (True, True, False):
        y = _nan(m, n)
        ops.gemm_split_tail(ad, m, frag, n, y, epi, allow_split=split)
        ys.append(y)
        err = rel_l2(y, (ref + bias.double() + res.double()) * 0.5)
        print(f"tail split-K={split}: rel-L2 {err:.2e}")
        assert err < GATE
    assert torch.equal(ys[0], ys[1])
    assert not torch.equal(ys[0], ys[2]), "the workspace launch did not split K"


def test_gemm_split_tail_refuses_gn_part(ops):
    m, k, n = 128, 160, 160
    a, w, *_ = _fwd_case(m, k, n)
    frag = ops.gemm_frag_tail(w.to(DEV), n, k, k, 1)
    y = _nan(m, n)
    part = torch.zeros(2 * 2 * (n // 4) * 2, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="psld_gemm_split_tail_f32"):
        ops.gemm_split_tail(a.to(DEV), m, frag, n, y, ops.epilogue(gn_part=part, gn_hw=64))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and not bool(part.any())


@pytest.mark.parametrize("k,n", KN)
def test_gemm_split_tail_width_independence(ops, k, n):
    """The tail launch equals, bit for bit, the leading n columns of ops.gemm_split on the same data zero-padded to whole
    tiles (n -> 128s, k -> 64s): per output element the same chunks in the same order and the same six limb products (both
    launches take the same K split: the same tile count, the same chunk count, workspaces for eight slabs)."""
    m = 1000
    a, w, bias, res, prev, _ = _fwd_case(m, k, n)
    npad, kpad = -(-n // 128) * 128, -(-k // 64) * 64
    ap, wp = torch.zeros(m, kpad), torch.zeros(npad, kpad)
    ap[:, :k], wp[:n, :k] = a, w
    biasp, resp = torch.zeros(npad), torch.zeros(m, npad)
    biasp[:n], resp[:, :n] = bias, res
    assert ops.gemm_split_supported(kpad, 0, m, npad)
    y = _nan(m, n)
    ops.gemm_split_tail(a.to(DEV), m, ops.gemm_frag_tail(w.to(DEV), n, k, k, 1), n, y,
                        ops.epilogue(bias=bias.to(DEV), residual=res.to(DEV), ld_residual=n, out_scale=0.5))
    yp = _nan(m, npad)
    ops.gemm_split(ap.to(DEV), None, m, ops.gemm_frag(wp.to(DEV), npad, kpad, kpad, 1), npad, yp,
                   ops.epilogue(bias=biasp.to(DEV), residual=resp.to(DEV), ld_residual=npad, out_scale=0.5))
    assert torch.equal(y, yp[:, :n].contiguous())
    # the padded fragment set IS the full-tile packer's on the zero-padded matrix
    assert torch.equal(ops.gemm_frag_tail(w.to(DEV), n, k, k, 1), ops.gemm_frag(wp.to(DEV), npad, kpad, kpad, 1))


def test_pack_frag_batch_tail_placements(ops):
    """q | k | v as ONE fragment set: three [c][c] tensors as row ranges of an N = 3c set and as K ranges of a K = 3c set,
    packed in one launch into NaN-pattern buffers, equal the single packer on the concatenated matrix."""
    c = 160
    ws = [gen(c, c, seed=20 + i, scale=0.1).to(DEV) for i in range(3)]          # NIN.W layout [in][out]
    pf = torch.full((ops.gemm_frag_bytes_tail(3 * c, c),), 0xFF, dtype=torch.uint8, device=DEV)
    pd = torch.full((ops.gemm_frag_bytes_tail(c, 3 * c),), 0xFF, dtype=torch.uint8, device=DEV)
    rows, total = [], 0
    for i, w in enumerate(ws):
        for row, items in (ops.gemm_frag_tail_entry(w, pf, c, c, 1, c, n0=i * c, n_total=3 * c),
                           ops.gemm_frag_tail_entry(w, pd, c, c, c, 1, chunk0=i * 5, chunks_total=15)):
            rows.append(row + [total])
            total += items
    ops.pack_frag_batch_tail(torch.tensor(rows, dtype=torch.int64, device=DEV), len(rows), total)
    wcat = torch.cat(ws, dim=1)                                                     # [c][3c]
    assert torch.equal(pf, ops.gemm_frag_tail(wcat, 3 * c, c, 1, 3 * c))            # B[n][k] = wcat[k][n]
    assert torch.equal(pd, ops.gemm_frag_tail(wcat, c, 3 * c, 3 * c, 1))            # B[n][k] = wcat[n][k]


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [128, 2048])
@pytest.mark.parametrize("m,n", [(160, 160), (320, 480), (480, 160), (480, 1440)])
def test_gemm_tn_split_tail_against_fp64(ops, m, n, k):
    """slabs reduced by reduce_slabs against A^T B in fp64; B a column slice of a wider buffer; nsplit default and 3;
    repeatable; zero-padding the operands to 128s and running the full-tile kernel gives the same bits."""
    ldb = n + 64
    a, bw = gen(k, m, seed=31), gen(k, ldb, seed=32)
    ref = a.double().t() @ bw[:, 32:32 + n].double()
    assert ops.gemm_tn_split_tail_supported(m, n, k) and not ops.gemm_tn_split_supported(m, n, k)
    ad, bd = a.to(DEV), bw.to(DEV).view(-1)[32:]
    for want in (R._tn_split(m, n, k), 3):
        kt = k // 32
        per = -(-kt // want)
        nsplit = -(-kt // per)

        def run():
            slabs = _nan(nsplit, m, n)
            ops.gemm_tn_split_tail(m, n, k, ad, m, bd, ldb, slabs, n, nsplit)
            out = _nan(m, n)
            ops.reduce_slabs(slabs, nsplit, m * n, out)
            return out
        out = run()
        err = rel_l2(out, ref)
        print(f"tail wgrad m={m} n={n} k={k} nsplit={nsplit}: rel-L2 {err:.2e}")
        assert err < GATE
        assert torch.equal(out, run())
    mp, np_ = -(-m // 128) * 128, -(-n // 128) * 128
    ap, bp = torch.zeros(k, mp, device=DEV), torch.zeros(k, np_, device=DEV)
    ap[:, :m], bp[:, :n] = ad, bw[:, 32:32 + n].to(DEV)
    slabs_p = _nan(nsplit, mp, np_)
    ops.gemm_tn_split(mp, np_, k, ap, mp, bp, np_, slabs_p, np_, nsplit)
    slabs = _nan(nsplit, m, n)
    ops.gemm_tn_split_tail(m, n, k, ad, m, bd, ldb, slabs, n, nsplit)
    assert torch.equal(slabs, slabs_p[:, :m, :n].contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# guard bands: no tail wave, padded chunk or masked load reaches past a buffer
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


@pytest.mark.parametrize("m,k,n,ld,split", [(130, 160, 160, None, False), (130, 480, 320, None, False),
                                            (130, 160, 160, 3 * 160, False), (128, 960, 480, None, True)],
                         ids=["130x160x160", "130x480x320", "ldy=3n", "split-K"])
def test_guarded_forward(ops, guard, m, k, n, ld, split):
    """Packer and forward launch on buffers of exactly the documented size between 0xFF (NaN) bands: no band byte changes,
    results bitwise those on ordinary buffers."""
    a, w, bias, res, prev, ref = _fwd_case(m, k, n)

    def fn(a, w, bias, res, y):
        frag = ops.gemm_frag_tail(w, n, k, k, 1)            # exactly gemm_frag_bytes_tail bytes, from the pool
        epi = ops.epilogue(bias=bias, residual=res, ld_residual=n, out_scale=0.5)
        ops.gemm_split_tail(a, m, frag, n, y if ld is None else y.view(-1)[n:], epi, ldy=ld, allow_split=split)
        return frag
    y0 = torch.zeros(m, n if ld is None else ld)
    plain, _ = G.run_guarded(guard, fn, dict(a=a.to(DEV), w=w.to(DEV), bias=bias.to(DEV), res=res.to(DEV), y=y0.to(DEV)),
                             {"y": None if ld is None else (n, 2 * n)})
    assert guard.workspace_calls == (1 if split else 0)
    y = plain["y"] if ld is None else plain["y"][:, n:2 * n]
    assert rel_l2(y, (ref + bias.double() + res.double()) * 0.5) < GATE


def test_guarded_weight_gradient(ops, guard):
    m, n, k = 160, 160, 128
    a, bm = gen(k, m, seed=41), gen(k, n, seed=42)

    def fn(a, b, slabs):
        ops.gemm_tn_split_tail(m, n, k, a, m, b, n, slabs, n, 2)
    plain, _ = G.run_guarded(guard, fn, dict(a=a.to(DEV), b=bm.to(DEV), slabs=torch.zeros(2, m, n, device=DEV)), ["slabs"])
    assert rel_l2(plain["slabs"].sum(0), a.double().t() @ bm.double()) < GATE


# ---------------------------------------------------------------------------------------------------------------------
# the AFHQv2-128 inpainting network (nf = 160)
# ---------------------------------------------------------------------------------------------------------------------
def test_afhq160_dispatch_keeps_limb_width_pointwise_off_the_tile_engine(monkeypatch):
    """One training step and one eval forward at B = 4 with recording wrappers on the fp32 tile engine's entry points: no
    unbatched 1x1 convolution / GEMM whose two channel dimensions are multiples of 32 from 128 up and whose pixel dimension
    is at least 64 reaches it - forward, data gradient or weight gradient.  (Batched attention products, the time-embedding
    GEMMs (pixel dimension = batch) and the few-channel K = 64 GEMMs fall outside that definition.)"""
    from psld_amd import ops
    from psld_amd.registry import get_module
    calls = []
    conv, wgrad, gemm = ops.conv2d_nhwc, ops.conv2d_wgrad_nhwc, ops.gemm_raw

    def rec_conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k):
        if kh == 1 and kw == 1:
            cin = x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
            calls.append(("conv1x1", cin, cout, x1.numel() // x1.shape[-1]))
        return conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k)

    def rec_wgrad(dy, cout, x, kh, kw, stride, *a, **k):
        if kh == 1 and kw == 1:
            calls.append(("wgrad1x1", x.shape[-1], cout, x.numel() // x.shape[-1]))
        return wgrad(dy, cout, x, kh, kw, stride, *a, **k)

    def rec_gemm(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, Cc, ldc, sc, batch=1, *a, **k):
        if batch == 1:
            # A stored [K][M] (ta): a weight gradient, K = pixels; else M = pixels
            calls.append(("gemm_tn", M, N, K) if ta else ("gemm", K, N, M))
        return gemm(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, Cc, ldc, sc, batch, *a, **k)
    monkeypatch.setattr(ops, "conv2d_nhwc", rec_conv)
    monkeypatch.setattr(ops, "conv2d_wgrad_nhwc", rec_wgrad)
    monkeypatch.setattr(ops, "gemm_raw", rec_gemm)
    net, cfg, _ = _build(train=True)
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    x0, eps, t = synth_inputs(4, 3, S, seed=5)
    loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
    loss.backward()
    n_train = len(calls)
    net.eval()
    with torch.no_grad():
        net(torch.randn(4, 6, S, S, device=DEV), torch.rand(4, device=DEV) * 0.9 + 0.05)
    torch.cuda.synchronize()

    def limb(kind, c_a, c_b, pixels):
        return c_a % 32 == 0 and c_b % 32 == 0 and c_a >= 128 and c_b >= 128 and pixels >= 64
    print("tile engine, unbatched pointwise:", sorted(set(calls)), "train calls:", n_train)
    assert not [c for c in calls if limb(*c)], sorted(set(c for c in calls if limb(*c)))


def test_afhq160_forward_modes_and_repeatability(golden):
    """Eval forward against the reference's (net_afhq160.npz) within 2e-5 in the default mode; 'bf16x3' within 1e-4 of it
    (tail shapes run the three-limb launch there too); two forwards bitwise equal, and bitwise equal after the visit to
    'bf16x3'."""
    from psld_amd import ops
    net, cfg, _ = _build()
    g = golden("net_afhq160.npz")
    x, t = T(g["x"]).to(DEV), T(g["t"]).to(DEV)
    old = ops.math_mode()
    assert old == "bf16x6"
    with torch.no_grad():
        y1 = net(x, t).clone()
        y2 = net(x, t).clone()
        try:
            ops.set_math_mode("bf16x3")
            y3 = net(x, t).clone()
        finally:
            ops.set_math_mode(old)
        y4 = net(x, t).clone()
    err, err3 = rel_l2(y1, T(g["y"])), rel_l2(y3, y1)
    print(f"afhq160 pointwise tail: rel-L2 vs reference {err:.3e}; bf16x3 vs bf16x6 {err3:.3e}")
    assert err < 2e-5
    assert err3 < 1e-4
    assert torch.equal(y1, y2) and torch.equal(y1, y4)

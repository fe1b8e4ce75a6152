"""The bf16 contraction kernels against the exact limb probes of tests/limb_probe.py, in the default arithmetic ('bf16x6').

Part 1 - probes.  Operands on which every limb product and every fp32 partial sum is exactly representable (one product per
output element; admissibility, coverage and sensitivity are asserted on the CPU by tests/test_limb_probe_cpu.py), so a
launch's output must EQUAL the six-product model, element by element, into a NaN-filled buffer.  A mismatch is decoded:
family, case, launch, how many elements, the first coordinates and which limb product is missing / doubled there.  Two
baselines keep the harness honest: the fp32 tile engine (full fp32 products) matches the same probes, and the two-limb
``*_x3`` launches match the model of {hi*hi, hi*mid, mid*hi} - class 2 WITHOUT its mid*mid bit.

Part 2 - dense random operands against ``limb_probe.six_limb_einsum`` (the Winograd kernels: on the fp32-transformed
operands), rel-L2 over the whole tensor, per output column and per band of 16 output rows, each measured against the same
statistic of the same contraction in plain fp32 on the CPU (against fp64).  Cap: cond_ref.YARD_FACTOR (4) x that yardstick,
no floor - and below what the model with any one product dropped reaches (asserted).  attn_fwd (a softmax between its two
products: no exact probe, no limb model) is measured against fp64 with its fp32 twin as the yardstick.

Largest quotient kernel / yardstick measured on the MI355X, whole tensor / worst column / worst 16-row band (the smallest
quotient of a one-product-dropped model in brackets):
    conv3x3_split (forward = dgrad) ......... 1.11 / 1.56 / 1.19   [11.5 / 8.0 / 10.5]
    conv3x3_wino (forward = dgrad) .......... 0.83 / 1.13 / 0.93   [20.2 / 15.0 / 18.8]
    gemm_split / gemm_split_tail ............ 0.64 / 0.89 / 0.70   [16.6 / 9.4 / 14.8]    0.41 / 0.56 / 0.43   [10.7 / 6.5 / 9.6]
    gemm_tn_split / gemm_tn_split_tail ...... 0.39 / 0.61 / 0.42   [9.8 / 5.7 / 9.4]      0.40 / 0.55 / 0.42   [9.6 / 6.1 / 9.2]
    bgemm_split / bgemm_split_tail .......... 0.71 / 0.83 / 0.76   [13.8 / 9.8 / 12.7]    0.71 / 0.86 / 0.75   [13.8 / 10.8 / 12.7]
    conv3x3_wgrad_split (fp32 x = limb x) ... 0.51 / 0.94 / 0.52   [13.1 / 6.9 / 12.5]
    conv3x3_wgrad_wino ...................... 0.30 / 0.60 / 0.31   [11.1 / 4.5 / 10.7]
    attn_fwd (against fp64) ................. 0.71 / 1.75 / 0.91
Every probe launch of part 1 equalled its model on the MI355X.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import cond_ref as R
from tests import limb_probe as P
from tests import x3_ref as X
from tests import x3_train_ref as XT

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    assert _ops.math_mode() == "bf16x6"
    return _ops


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _must_equal(tag, y, launch, products=P.PRODUCTS):
    """torch.equal(y, model) - or the decoded failure."""
    want = launch.expected(products)
    y = y.detach().double().cpu().reshape(want.shape)
    if not torch.equal(y, want):
        pytest.fail(P.explain(tag, y, launch, products), pytrace=False)


def _sources(x, c1):
    """NCHW -> the one or two NHWC sources of a concatenation, on the device."""
    xh = _nhwc(x)
    return xh[..., :c1].contiguous().to(DEV), (xh[..., c1:].contiguous().to(DEV) if c1 < x.shape[1] else None)


def _real_weights(w_eff, dgrad):
    """The layer's OIHW weights whose forward (dgrad False) or data-gradient (True) fragments hold B[n][k][tap] = w_eff."""
    return (w_eff.flip(2, 3).transpose(0, 1).contiguous() if dgrad else w_eff).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# part 1: probes
# ---------------------------------------------------------------------------------------------------------------------
def _conv_probe(ops, key, dgrad, packer, launcher, products=P.PRODUCTS, supported=None):
    case = P.case(key)
    b, c1, c2, co, h, w = case.params["shape"]
    assert (supported or ops.conv3x3_split_supported)(c1, c2, b, h, w, co)
    frags = {}
    for i, la in enumerate(case.launches):
        wk = la.inp.get("wkey", ("launch", i))
        if wk not in frags:
            frags = {wk: packer(_real_weights(la.inp["w"], dgrad))}        # dense weights: one set per class
        x1, x2 = _sources(la.inp["x"], c1)
        for form, y in launcher(x1, x2, frags[wk], co, (b, h, w, co)):
            _must_equal(f"{case} {'data gradient' if dgrad else 'forward'} [{form}] launch {i}", y, la, products)


@pytest.mark.parametrize("dgrad", [False, True], ids=["forward", "dgrad"])
@pytest.mark.parametrize("key", P.case_ids("conv"))
def test_conv3x3_split_probe(ops, key, dgrad):
    """psld_conv3x3_split_f32 (fp32 input, split in the kernel) and psld_conv3x3_limb_f32 (LimbPlanes input) on forward and
    data-gradient fragments: two images per tile, two sources, four images per tile, the K split over channel chunks."""
    def launch(x1, x2, wf, co, shape):
        y = _nan(*shape)
        ops.conv3x3_split(x1, x2, wf, co, y)
        yield "fp32 input", y
        y = _nan(*shape)
        ops.conv3x3_split(ops.f32_to_limb(x1), ops.f32_to_limb(x2) if x2 is not None else None, wf, co, y)
        yield "limb planes", y
    _conv_probe(ops, key, dgrad, lambda w: ops.conv3x3_frag(w, dgrad), launch)


@pytest.mark.parametrize("key", ["conv:2x64x0x128x8x8-dense_x", "conv:1x256x256x256x8x8-dense_x", "conv:1x256x256x256x8x8-dense_w"])
def test_conv3x3_split_probe_without_workspace(ops, key):
    """workspace=False: no K split, the kernel's own epilogue on the small grids too."""
    def launch(x1, x2, wf, co, shape):
        y = _nan(*shape)
        ops.conv3x3_split(x1, x2, wf, co, y, workspace=False)
        yield "no workspace", y
    _conv_probe(ops, key, False, lambda w: ops.conv3x3_frag(w, False), launch)


@pytest.mark.parametrize("dgrad", [False, True], ids=["forward", "dgrad"])
@pytest.mark.parametrize("key", P.case_ids("wino"))
def test_conv3x3_wino_probe(ops, key, dgrad):
    """psld_conv3x3_wino_f32 / _ws_f32 (the 1x256->256 at 16x16 case asks for the split over channel chunks, as
    tests/test_math_x3_gpu.py does): the lattice input and single-tap weights pass the fp32 transforms as scaled copies."""
    case = P.case(key)
    b, c1, c2, co, h, w = case.params["shape"]
    split = case.params["split"]
    if split and not ops.conv3x3_wino_ws_bytes(c1, c2, b, h, w, co):
        pytest.skip("this device's CU count fills the grid without a split")

    def launch(x1, x2, uf, co, shape):
        y = _nan(*shape)
        ops.conv3x3_wino(x1, x2, uf, co, y, allow_split=split)
        yield "split chunks" if split else "one launch", y
    _conv_probe(ops, key, dgrad, lambda w: ops.conv3x3_wino_frag(w, dgrad), launch, supported=ops.conv3x3_wino_supported)


@pytest.mark.parametrize("key", P.case_ids("gemm"))
def test_gemm_split_probe(ops, key):
    """psld_gemm_split_f32: four waves (256 x 128, k = 64; 640 x 128, k = 96 + 32 from two sources) and eight waves (128
    tiles of 128 x 256), fragments from an [n][k] and from a [k][n] matrix."""
    case = P.case(key)
    m, n, k1, k2 = (case.params[v] for v in ("m", "n", "k1", "k2"))
    k = k1 + k2
    assert ops.gemm_split_supported(k1, k2, m, n)
    if m >= 16384:
        assert -(-m // 128) * (n // 256) >= 128             # the eight-wave kernel's grid
    for i, la in enumerate(case.launches):
        a, bm = la.a, la.b
        a1 = a[:, :k1].contiguous().to(DEV)
        a2 = a[:, k1:].contiguous().to(DEV) if k2 else None
        for form, frag in (("[n][k]", ops.gemm_frag(bm.to(DEV), n, k, k, 1)),
                           ("[k][n]", ops.gemm_frag(bm.t().contiguous().to(DEV), n, k, 1, n))):
            y = _nan(m, n)
            ops.gemm_split(a1, a2, m, frag, n, y)
            _must_equal(f"gemm_split {case} B {form} launch {i}", y, la)


@pytest.mark.parametrize("key", P.case_ids("gemm_tail"))
def test_gemm_split_tail_probe(ops, key):
    """psld_gemm_split_tail_f32 at 130 x 160 x 160, into a plain buffer and into the middle third of one with ldy = 3n."""
    case = P.case(key)
    m, n, k = (case.params[v] for v in ("m", "n", "k"))
    assert ops.gemm_tail_supported(k, m, n) and not ops.gemm_split_supported(k, 0, m, n)
    for i, la in enumerate(case.launches):
        a, frag = la.a.to(DEV), ops.gemm_frag_tail(la.b.to(DEV), n, k, k, 1)
        for split in (True, False):
            y = _nan(m, n)
            ops.gemm_split_tail(a, m, frag, n, y, allow_split=split)
            _must_equal(f"gemm_split_tail {case} allow_split={split} launch {i}", y, la)
        wide = _nan(m, 3 * n)
        ops.gemm_split_tail(a, m, frag, n, wide.view(-1)[n:], ldy=3 * n)
        _must_equal(f"gemm_split_tail {case} ldy=3n launch {i}", wide[:, n:2 * n], la)
        assert bool(torch.isnan(wide[:, :n]).all()) and bool(torch.isnan(wide[:, 2 * n:]).all())


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("key", P.case_ids("tn", "tn_tail"))
def test_gemm_tn_split_probe(ops, key, nsplit):
    """psld_gemm_tn_split_f32 / _tail_f32 (A^T B into per-K-range slabs): one range and three ranges of two K tiles."""
    case = P.case(key)
    m, n, k = (case.params[v] for v in ("m", "n", "k"))
    tail = case.family == "tn_tail"
    assert (ops.gemm_tn_split_tail_supported if tail else ops.gemm_tn_split_supported)(m, n, k)
    assert -(-(k // 32) // nsplit) * nsplit == k // 32
    for i, la in enumerate(case.launches):
        ad, bd = la.a.t().contiguous().to(DEV), la.b.t().contiguous().to(DEV)          # [k][m], [k][n]
        slabs = _nan(nsplit, m, n)
        (ops.gemm_tn_split_tail if tail else ops.gemm_tn_split)(m, n, k, ad, m, bd, n, slabs, n, nsplit)
        assert bool(torch.isfinite(slabs).all())
        _must_equal(f"gemm_tn_split{'_tail' if tail else ''} {case} nsplit={nsplit} launch {i}", slabs.double().sum(0), la)


@pytest.mark.parametrize("ta,tb", P.BGEMM_LAYOUTS, ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("key", P.case_ids("bgemm", "bgemm_tail"))
def test_bgemm_split_probe(ops, key, ta, tb):
    """psld_bgemm_split_f32 / _tail_f32 (both operands split in the kernel), batch 3, in the three layouts."""
    case = P.case(key)
    m, n, k, batch = (case.params[v] for v in ("m", "n", "k", "batch"))
    tail = case.family == "bgemm_tail"
    assert (ops.bgemm_split_tail_supported if tail else ops.bgemm_split_supported)(ta, tb, m, n, k)
    for i, la in enumerate(case.launches):
        a, bm = torch.stack(la.a, 0), torch.stack(la.b, 0)                             # [batch][m][k], [batch][n][k]
        ad = (a.transpose(1, 2) if ta else a).contiguous().to(DEV)
        bd = (bm if tb else bm.transpose(1, 2)).contiguous().to(DEV)
        out = _nan(batch, m, n)
        (ops.bgemm_split_tail if tail else ops.bgemm_split)(ta, tb, m, n, k, ad, ad.shape[2], ad.shape[1] * ad.shape[2], bd,
                                                            bd.shape[2], bd.shape[1] * bd.shape[2], out, n, m * n, batch)
        _must_equal(f"bgemm_split{'_tail' if tail else ''} {case} ta={ta} tb={tb} launch {i}", out, la)


@pytest.mark.parametrize("key", P.case_ids("wgrad"))
def test_conv3x3_wgrad_split_probe(ops, key):
    """psld_conv3x3_wgrad_split_f32 (fp32 x; 128-channel c_out tiles: the wave-specialised kernel) and
    psld_conv3x3_wgrad_xlimb_f32 (x as limb planes), slabs over K ranges at a column offset of a wider block."""
    case = P.case(key)
    b, ci, co, h, w = case.params["shape"]
    assert ops.conv3x3_wgrad_split_supported(co, ci, b, h, w)
    ktiles = b * h * w // 32
    per = -(-ktiles // min(3, ktiles))
    nsplit = -(-ktiles // per)
    cin_total, col0 = ci + 64, 64
    for i, la in enumerate(case.launches):
        gy, x = _nhwc(la.inp["dy"]).to(DEV), _nhwc(la.inp["x"]).to(DEV)
        for form, xin in (("fp32 x", x), ("limb-plane x", ops.f32_to_limb(x))):
            slabs = _nan(nsplit, co, 9, cin_total)
            ops.conv3x3_wgrad_split(gy, co, xin, slabs, cin_total, col0, nsplit)
            assert bool(torch.isnan(slabs[..., :col0]).all()) and bool(torch.isfinite(slabs[..., col0:]).all())
            dw = slabs[..., col0:].double().sum(0).permute(0, 2, 1)                     # [co][ci][tap]
            _must_equal(f"conv3x3_wgrad_split {case} [{form}] launch {i}", dw, la)


@pytest.mark.parametrize("nsplit", [None, 2], ids=["planned-split", "nsplit=2"])
@pytest.mark.parametrize("key", P.case_ids("wwino"))
def test_conv3x3_wgrad_wino_probe(ops, key, nsplit):
    """psld_conv3x3_wgrad_wino_f32 at the two smallest shapes of test_conv3x3_wgrad_winograd_domain (one and two sources)."""
    case = P.case(key)
    b, c1, c2, co, h, w = case.params["shape"]
    assert ops.conv3x3_wgrad_wino_supported(co, c1, c2, b, h, w)
    for i, la in enumerate(case.launches):
        x1, x2 = _sources(la.inp["x"], c1)
        dw = _nan(co, c1 + c2, 3, 3)
        ops.conv3x3_wgrad_wino(_nhwc(la.inp["dy"]).to(DEV), co, x1, dw, x2=x2, nsplit=nsplit)
        _must_equal(f"conv3x3_wgrad_wino {case} nsplit={nsplit} launch {i}", dw, la)


# ---- baselines: the harness itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["gemm:256x128x64+0-dense_a", "gemm:640x128x96+32-dense_b"])
def test_fp32_tile_engine_gemm_matches_the_probes(ops, key):
    """gemm_raw forms full fp32 products: on the probes that is the six-product model."""
    case = P.case(key)
    m, n, k = case.params["m"], case.params["n"], case.params["k1"] + case.params["k2"]
    for i, la in enumerate(case.launches):
        y = _nan(m, n)
        ops.gemm_raw(0, 1, m, n, k, la.a.to(DEV), k, 0, la.b.to(DEV), k, 0, y, n, 0)
        _must_equal(f"gemm_raw (fp32) {case} launch {i}", y, la)


@pytest.mark.parametrize("key", ["conv:2x64x0x128x8x8-dense_x", "conv:2x64x0x128x8x8-dense_w", "conv:2x64x32x128x16x16-dense_x"])
def test_fp32_tile_engine_conv_matches_the_probes(ops, key):
    def pack(w):
        wp = torch.empty(w.shape[0], 9, w.shape[1], device=DEV)
        ops.pack_ohwi(w, wp)
        return wp

    def launch(x1, x2, wp, co, shape):
        y = _nan(*shape)
        ops.conv2d_nhwc(x1, x2, wp, co, 3, 3, 1, 1, 1, shape[1], shape[2], y)
        yield "fp32 tile engine", y
    _conv_probe(ops, key, False, pack, launch)


def test_two_limb_launches_come_out_without_the_small_products(ops):
    """The ``*_x3`` launches against the model of {hi*hi, hi*mid, mid*hi}: class 2 without its mid*mid bit, classes 0 and 1
    without lo*hi / hi*lo - and NOT equal to the six-product model, so the probes tell the arithmetics apart."""
    case = P.case("gemm:16384x256x128+0-dense_a")
    m, n, k = 16384, 256, 128
    assert ops.gemm_split_x3_supported(k, 0, m, n)
    for i, la in enumerate(case.launches):
        y = _nan(m, n)
        ops.gemm_split_x3(la.a.to(DEV), None, m, ops.gemm_frag_x3(la.b.to(DEV), n, k, k, 1), n, y)
        _must_equal(f"gemm_split_x3 {case} launch {i}", y, la, P.X3_PRODUCTS)
        assert not torch.equal(y.double().cpu(), la.expected())

    def launch(x1, x2, uf, co, shape):
        y = _nan(*shape)
        ops.conv3x3_wino_x3(x1, x2, uf, co, y)
        yield "two limbs", y
    _conv_probe(ops, "wino:2x64x0x128x8x8", False, ops.conv3x3_wino_frag_x3, launch, P.X3_PRODUCTS, ops.conv3x3_wino_supported)
    case = P.case("wwino:8x128x0x256x8x8-dy_pixel")
    b, c1, c2, co, h, w = case.params["shape"]
    for i, la in enumerate(case.launches[:9]):
        dw = _nan(co, c1, 3, 3)
        ops.conv3x3_wgrad_wino_x3(_nhwc(la.inp["dy"]).to(DEV), co, _nhwc(la.inp["x"]).to(DEV), dw)
        _must_equal(f"conv3x3_wgrad_wino_x3 {case} launch {i}", dw, la, P.X3_PRODUCTS)


# ---------------------------------------------------------------------------------------------------------------------
# part 2: dense random operands against the limb model
# ---------------------------------------------------------------------------------------------------------------------
def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _quotients(tag, y, model, yard, ref64, drops):
    """Print and assert the three statistics of ``y`` against ``model`` under YARD_FACTOR x those of ``yard`` against
    ``ref64`` - and that every ``drops`` model (one product missing) lies above that cap in every statistic."""
    k = P.rel_l2_stats(y.detach().cpu(), model)
    f = P.rel_l2_stats(yard, ref64)
    names = ("whole", "column", "band16")
    q = [k[0] / f[0], float((k[1] / f[1]).max()), float((k[2] / f[2]).max())]
    qd = [min(d[0] for d in drops) / f[0] if drops else float("inf")]
    qd += [min(float((d[j] / f[j]).min()) for d in drops) if drops else float("inf") for j in (1, 2)]
    print(f"{tag}: kernel {k[0]:.2e} yardstick {f[0]:.2e}; quotient " +
          ", ".join(f"{n} {v:.2f} (one product dropped: {d:.1f})" for n, v, d in zip(names, q, qd)))
    for n, v, d in zip(names, q, qd):
        assert R.YARD_FACTOR < d, (tag, n, d)          # the cap separates the kernel from every one-product-dropped model
        assert v <= R.YARD_FACTOR, (tag, n, v)


def _drop_stats(prods_to_out, prods, model):
    return [P.rel_l2_stats(prods_to_out(P.sum_products(prods, drop=p)), model) for p in P.PRODUCTS]


def _conv_dense(b, c, co, h, w):
    x, wt = gen(b, c, h, w, seed=40), gen(co, c, 3, 3, seed=41, scale=0.1)
    ref64 = _nhwc(F.conv2d(x.double(), wt.double(), padding=1)).reshape(-1, co)
    yard = _nhwc(F.conv2d(x, wt, padding=1)).reshape(-1, co)
    return x, wt, yard, ref64


def test_dense_conv3x3_split_against_the_limb_model(ops):
    b, c, co, h, w = 2, 64, 128, 8, 8
    x, wt, yard, ref64 = _conv_dense(b, c, co, h, w)
    prods = P.limb_products("mk,nk->mn", P._cols(x), wt.reshape(co, -1))
    model = P.sum_products(prods)
    drops = _drop_stats(lambda t: t, prods, model)
    for dgrad in (False, True):
        y = _nan(b, h, w, co)
        ops.conv3x3_split(_nhwc(x).to(DEV), None, ops.conv3x3_frag(_real_weights(wt, dgrad), dgrad), co, y)
        _quotients(f"conv3x3_split {'dgrad' if dgrad else 'forward'} {b}x{c}->{co}@{h}x{w}", y.reshape(-1, co), model, yard, ref64, drops)


def test_dense_conv3x3_wino_against_the_limb_model(ops):
    b, c, co, h, w = 2, 64, 128, 8, 8
    x, wt, yard, ref64 = _conv_dense(b, c, co, h, w)
    v = X.wino_v(x)
    prods = P.limb_products("ptc,poc->pto", v.reshape(16, -1, c), X.wino_u(wt))

    def out(m):
        return P._wino_output(m, v.shape[1], v.shape[2], v.shape[3])
    model = out(P.sum_products(prods))
    drops = _drop_stats(out, prods, model)
    for dgrad in (False, True):
        y = _nan(b, h, w, co)
        ops.conv3x3_wino(_nhwc(x).to(DEV), None, ops.conv3x3_wino_frag(_real_weights(wt, dgrad), dgrad), co, y)
        _quotients(f"conv3x3_wino {'dgrad' if dgrad else 'forward'} {b}x{c}->{co}@{h}x{w}", y.reshape(-1, co), model, yard, ref64, drops)


@pytest.mark.parametrize("m,n,k,tail", [(256, 128, 64, False), (130, 160, 160, True)], ids=["gemm_split", "gemm_split_tail"])
def test_dense_gemm_split_against_the_limb_model(ops, m, n, k, tail):
    a, bm = gen(m, k, seed=70), gen(n, k, seed=71, scale=0.1)
    prods = P.limb_products("mk,nk->mn", a, bm)
    model = P.sum_products(prods)
    y = _nan(m, n)
    if tail:
        ops.gemm_split_tail(a.to(DEV), m, ops.gemm_frag_tail(bm.to(DEV), n, k, k, 1), n, y)
    else:
        ops.gemm_split(a.to(DEV), None, m, ops.gemm_frag(bm.to(DEV), n, k, k, 1), n, y)
    _quotients(f"gemm_split{'_tail' if tail else ''} {m}x{n}x{k}", y, model, a @ bm.t(), a.double() @ bm.double().t(),
               _drop_stats(lambda t: t, prods, model))


@pytest.mark.parametrize("m,n,k,tail", [(128, 128, 192, False), (160, 160, 192, True)], ids=["gemm_tn_split", "gemm_tn_split_tail"])
def test_dense_gemm_tn_split_against_the_limb_model(ops, m, n, k, tail):
    a, bm = gen(k, m, seed=75), gen(k, n, seed=76)
    prods = P.limb_products("km,kn->mn", a, bm)
    model = P.sum_products(prods)
    slabs = _nan(3, m, n)
    (ops.gemm_tn_split_tail if tail else ops.gemm_tn_split)(m, n, k, a.to(DEV), m, bm.to(DEV), n, slabs, n, 3)
    out = _nan(m, n)
    ops.reduce_slabs(slabs, 3, m * n, out)
    _quotients(f"gemm_tn_split{'_tail' if tail else ''} {m}x{n}x{k}", out, model, a.t() @ bm, a.double().t() @ bm.double(),
               _drop_stats(lambda t: t, prods, model))


@pytest.mark.parametrize("n", [128, 160], ids=["bgemm_split", "bgemm_split_tail"])
def test_dense_bgemm_split_against_the_limb_model(ops, n):
    m, k, batch = 256, 96, 3
    a, bm = gen(batch, m, k, seed=77), gen(batch, n, k, seed=78)
    prods = P.limb_products("bmk,bnk->bmn", a, bm)
    model = P.sum_products(prods).reshape(-1, n)
    out = _nan(batch, m, n)
    (ops.bgemm_split_tail if n % 128 else ops.bgemm_split)(0, 1, m, n, k, a.to(DEV), k, m * k, bm.to(DEV), k, n * k, out, n, m * n, batch)
    _quotients(f"bgemm_split{'_tail' if n % 128 else ''} {batch}x{m}x{n}x{k}", out.reshape(-1, n), model,
               (a @ bm.transpose(1, 2)).reshape(-1, n), (a.double() @ bm.double().transpose(1, 2)).reshape(-1, n),
               _drop_stats(lambda t: t.reshape(-1, n), prods, model))


def _wgrad_dense(b, ci, co, h, w):
    x, dy = gen(b, ci, h, w, seed=83) + 0.25, gen(b, co, h, w, seed=84)
    refs = []
    for dt in (torch.float32, torch.float64):
        wz = torch.zeros(co, ci, 3, 3, dtype=dt, requires_grad=True)
        F.conv2d(x.to(dt), wz, padding=1).backward(dy.to(dt))
        refs.append(wz.grad.reshape(co, -1))
    return x, dy, refs[0], refs[1]


def test_dense_conv3x3_wgrad_split_against_the_limb_model(ops):
    b, ci, co, h, w = 2, 128, 64, 8, 8
    x, dy, yard, ref64 = _wgrad_dense(b, ci, co, h, w)
    prods = P.limb_products("mk,nk->mn", dy.permute(1, 0, 2, 3).reshape(co, -1), P._cols(x).t().contiguous())
    model = P.sum_products(prods)
    drops = _drop_stats(lambda t: t, prods, model)
    for form in ("fp32 x", "limb-plane x"):
        xd = _nhwc(x).to(DEV)
        slabs = _nan(2, co, 9, ci)
        ops.conv3x3_wgrad_split(_nhwc(dy).to(DEV), co, xd if form == "fp32 x" else ops.f32_to_limb(xd), slabs, ci, 0, 2)
        dw = _nan(co, ci, 3, 3)
        ops.reduce_slabs(slabs, 2, co * 9 * ci, dw, layout=1, cout=co, taps=9, cin=ci)
        _quotients(f"conv3x3_wgrad_split [{form}] {b}x{ci}->{co}@{h}x{w}", dw.reshape(co, -1), model, yard, ref64, drops)


def test_dense_conv3x3_wgrad_wino_against_the_limb_model(ops):
    b, ci, co, h, w = 8, 128, 256, 8, 8
    x, dy, yard, ref64 = _wgrad_dense(b, ci, co, h, w)
    prods = P.limb_products("pto,ptc->poc", XT.wino_m(dy).reshape(16, -1, co), XT.wino_v_cols_first(x).reshape(16, -1, ci))

    def out(du):
        return torch.einsum("ia,jb,ijoc->ocab", XT._G, XT._G, du.reshape(4, 4, co, ci)).reshape(co, -1)
    model = out(P.sum_products(prods))
    dw = _nan(co, ci, 3, 3)
    ops.conv3x3_wgrad_wino(_nhwc(dy).to(DEV), co, _nhwc(x).to(DEV), dw)
    _quotients(f"conv3x3_wgrad_wino {b}x{ci}->{co}@{h}x{w}", dw.reshape(co, -1), model, yard, ref64, _drop_stats(out, prods, model))


def test_dense_attn_fwd_against_fp64(ops):
    """softmax(scale q k^T) v: no limb model (a softmax sits between the two products) - fp64 is the reference and its fp32
    twin the yardstick, as in tests/test_conditioning_gpu.py; the cap has no floor here."""
    b, hw, c = 1, 64, 128
    assert ops.attn_fwd_supported(hw, c)
    q, k, v = gen(b, hw, c, seed=70), gen(b, hw, c, seed=71), gen(b, hw, c, seed=72)
    scale = float(c) ** -0.5

    def ref(dt):
        p = torch.softmax(torch.einsum("bic,bjc->bij", q.to(dt), k.to(dt)) * scale, dim=-1)
        return torch.einsum("bij,bjc->bic", p, v.to(dt)).reshape(-1, c)
    out = _nan(b, hw, c)
    ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), c, b, hw, c, scale, out, None)
    _quotients(f"attn_fwd {b}x{hw}x{c}", out.reshape(-1, c), ref(torch.float64), ref(torch.float32), ref(torch.float64), [])

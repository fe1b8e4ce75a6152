"""Every launch form of the fp32 MFMA tile engine (psld_amd/csrc/tile_engine.hip) against fp64, on the case table of
tests/tile_cases.py: psld_gemm_f32, psld_gemm_tn_splitk_f32, psld_conv2d_nhwc_ws_f32 (with its split-K reduction pass) and
psld_conv2d_wgrad_nhwc_f32.

Part 1 - equality.  Small-integer operands on which every product, partial sum and epilogue step is exact in fp32 in any
order (admissibility, the form every case reaches, coverage of all forms and sensitivity of the references are asserted
without a GPU by tests/test_tile_engine_cpu.py): the launch's output must EQUAL the fp64 reference (torch.equal), written
into a NaN-filled buffer whose every other float - row padding behind ldc / ldy, the outer thirds of a 3 x cout row, the
columns of a weight-gradient slab outside [col0, col0 + cin) - must still be NaN.  The plan query is asked again on the
device pointers, so the kernel that ran is the one the case names.  Row biases come from a guard pool: exactly
ceil(M / rows_per_img) rows between NaN bands.  A mismatch reports case, form, count and the first coordinates.

Part 2 - one dense randn case per form against fp64: rel-L2 over the whole tensor, the worst output column and the worst band
of 16 output rows, each as a quotient over the same statistic of the same contraction accumulated in fp32 sequentially in k
order on the CPU (tile_cases.yardstick32; not a blocked sum: the kernel's chain is k-ordered).  Cap: cond_ref.YARD_FACTOR (4)
x the yardstick, no floor.

Largest quotient kernel / yardstick measured on the MI355X over the dense cases of a kernel kind (whole tensor / worst column /
worst 16-row band; the kernel's chain is one fmaf per k, the yardstick rounds the product and the sum):
    psld_gemm_f32 ................ generic 1.01 / 1.77 / 1.18   fast64 0.93 / 1.38 / 0.94   fast128 0.98 / 1.25 / 1.01   fast256 0.95 / 0.97 / 1.04
    psld_gemm_tn_splitk_f32 ...... generic 0.97 / 1.40 / 1.06   fast128 0.98 / 1.27 / 1.00
    psld_conv2d_nhwc_ws_f32 ...... generic 0.99 / 1.28 / 1.15   fast64 0.97 / 1.16 / 1.00   fast128 0.99 / 1.00 / 1.09   fast256 0.95 / 0.99 / 1.03
                                   fast64 + split-K (3 ranges) 0.58 / 0.84 / 0.62
    psld_conv2d_wgrad_nhwc_f32 ... generic 0.99 / 1.83 / 1.01   fast128 0.97 / 1.25 / 1.00
Every equality case of part 1 equalled its reference on the MI355X.
"""
import pytest
import torch

from tests import cond_ref as R
from tests import guard as G
from tests import limb_probe as P
from tests import tile_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def pool():
    return G.GuardPool(DEV, 3 * G.BAND)


def _planned(cl):
    case = cl.case
    form, ns = cl.plan()
    assert (T.form_name(form), ns) == (T.form_name(case.form), case.nsplit), f"{case}: the launch would take another form"
    return form


@pytest.mark.parametrize("key", T.case_ids())
def test_equals_fp64(ops, pool, key):
    o = T.operands(key)
    want = T.reference(o)
    w32 = want.float()
    assert torch.equal(w32.double(), want)
    cl = T.Call(ops, o, DEV, pool)
    form = _planned(cl)
    y = cl.launch()
    torch.cuda.synchronize()
    pool.check()
    pool.release()
    got = cl.written(y).reshape(want.shape)
    if not torch.equal(got, w32.to(DEV)):
        pytest.fail(T.explain(cl.case, form, got.double().cpu(), want), pytrace=False)
    outside = y[cl.outside_mask().to(DEV)]
    n_written = int((~torch.isnan(outside)).sum())
    assert n_written == 0, f"{cl.case} [{T.form_name(form)}]: {n_written} floats outside the output region were written"


@pytest.mark.parametrize("key,mutation", [("gemm:nt-fast64-epilogue-rpi32", "shift_rowbias"), ("conv:splitk3-epilogue", "swap_sources"),
                                          ("conv:splitk7-1x1-49steps", "drop_k4"), ("wgrad:fast-132x36", "transpose_taps")])
def test_comparison_notices_a_wrong_reference(ops, key, mutation):
    """The harness is honest: against the reference of a kernel that made one of the mistakes of tile_cases.MUTATIONS the
    same launch does NOT compare equal, and the message names the case, the form and coordinates."""
    o = T.operands(key)
    cl = T.Call(ops, o, DEV)
    form = _planned(cl)
    got = cl.written(cl.launch()).reshape(T.reference(o).shape).double().cpu()
    assert T.explain(cl.case, form, got, T.reference(o)) is None
    msg = T.explain(cl.case, form, got, T.reference(o, mutation))
    assert msg is not None and str(cl.case) in msg and T.form_name(form) in msg and "at (" in msg


# ---------------------------------------------------------------------------------------------------------------------
# part 2: dense random operands
# ---------------------------------------------------------------------------------------------------------------------
def _rows(case, t):
    """The 2-D [output rows][output columns] layout of the statistics."""
    if case.entry == "wgrad":
        return t.reshape(-1, t.shape[-2] * t.shape[-1])
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize("key", T.dense_ids())
def test_dense_against_fp64(ops, key):
    o = T.operands(key, dense=True)
    ref, yard = T.reference(o), T.yardstick32(o)
    cl = T.Call(ops, o, DEV)
    form = _planned(cl)
    y = cl.launch()
    torch.cuda.synchronize()
    got = _rows(cl.case, cl.written(y).reshape(ref.shape).cpu())
    ref, yard = _rows(cl.case, ref), _rows(cl.case, yard)
    live = ref.abs().sum(1) > 0                 # the slab of an empty K range is all zero - exactly, never NaN
    assert bool((got[~live] == 0).all())
    k = P.rel_l2_stats(got[live], ref[live])
    f = P.rel_l2_stats(yard[live], ref[live])
    q = [k[0] / f[0], float((k[1] / f[1]).max()), float((k[2] / f[2]).max())]
    print(f"{cl.case} [{T.form_name(form)}]: kernel {k[0]:.2e} yardstick {f[0]:.2e}; quotient whole {q[0]:.2f}, "
          f"column {q[1]:.2f}, band16 {q[2]:.2f}")
    for n, v in zip(("whole", "column", "band16"), q):
        assert v <= R.YARD_FACTOR, (str(cl.case), n, v)

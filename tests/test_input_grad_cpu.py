"""The input-gradient-only backward (``_Exec.input_grad_only``, ``NCSNpp.vjp_input``) as a launch sequence, dry-run on the CPU
with the stand-in library of ``tools/launch_trace.py``: one recorded forward + backward with ``want_dx``, once full and once
input-gradient-only, of three tiny networks at B = 2 in eval mode.

The input-only pass must launch nothing that serves a parameter gradient - no pointer into the flat gradient buffer, none of
the weight-gradient / slab / parameter-reduction entry points - and must launch every data-gradient kernel of the full pass
with the very same arguments, in the same order: its rows are a subsequence of the full pass's rows, and the rows it leaves
out are parameter-only.  Parameter-only rows of a full backward are, from the full trace alone:

  * a row with a ``["g", offset]`` pointer (it writes a gradient);
  * a row of an entry point that exists for weight gradients and their reductions alone (``_PARAM_ONLY``: split-K producers
    write slabs, not the gradient, so they carry no ``"g"`` pointer themselves);
  * ``psld_colsum_f32``: column sums are bias gradients (the two-pass form parks per-image sums in a temporary first);
  * the backward of the time-embedding MLP: the last tape entry, i.e. what follows the stem's data gradient (the last
    ``psld_nhwc_to_nchw_f32`` and the accumulation of its result into dx).  ``t`` gets no gradient, so the whole chain -
    d act(temb), the SiLU backwards, the Dense weight gradients - ends in parameters."""
import pytest
import torch

from tools import launch_trace as LT

CASES = {"nf128_bf16x6": (dict(nf=128), "bf16x6"), "nf160_bf16x6": (dict(nf=160), "bf16x6"), "nf32_f32": (dict(nf=32), "f32")}
# entry points whose only products are parameter gradients (or their partial sums)
_PARAM_ONLY = ("wgrad", "psld_gemm_tn_split", "psld_reduce_slabs", "psld_param_reduce", "psld_bias_grad")
# general-purpose entry points that ALSO write gradients in a full pass (time-MLP GEMMs, bias copies, few-channel repacks)
_SHARED = {"psld_gemm_f32", "psld_axpby_f32", "psld_colsum_f32", "psld_scale_copy2d_f32", "psld_copy_batch_f32"}
_TRACES = {}


def _param_only_name(name):
    return any(s in name for s in _PARAM_ONLY)


def _has_g(row):
    return any(isinstance(v, list) and v and v[0] == "g" for v in row[1:])


def _trace(name, igo, monkeypatch):
    """(forward rows, backward rows) of one recorded eval-mode pass with want_dx."""
    key = (name, igo)
    if key in _TRACES:
        return _TRACES[key]
    import psld_amd
    from psld_amd import _lib, config as cfgs, ops
    from psld_amd.registry import get_module
    from psld_amd.score_exec import _Exec
    ops.lib()
    for obj, attr, val in LT.patches():
        monkeypatch.setattr(obj, attr, val)
    psld_amd.import_modules_into_registry()
    tiny, mode = CASES[name]
    cfg = cfgs.tiny(**tiny)
    rec = LT._Recorder(_lib.load_real())
    saved = ops.math_mode()
    _lib.set_proxy(rec)
    try:
        ops.set_math_mode(mode)
        torch.manual_seed(0)
        net = get_module("score_fn", "ncsnpp")(cfg)
        net.overlap_wgrad = False
        flat, grad = net.flatten_parameters(), net.flat_grad()
        rec.spans = [("p", flat.data_ptr(), 4 * flat.numel()), ("g", grad.data_ptr(), 4 * grad.numel())]
        size, sf = cfg.data.image_size, cfg.model.score_fn
        x, t = torch.zeros(2, sf.in_ch, size, size), torch.zeros(2)
        with torch.no_grad():
            net.eval()
            ex = _Exec(net, record=True, input_grad_only=igo)
            assert ex.input_grad_only == igo
            ex.want_dx = True
            y = ex.run(x, t)
            n_fwd = len(rec.rows)
            if not igo:
                net._begin_backward()
            ex.backward(torch.zeros_like(y))
            assert ex.dx_nchw is not None and ex.dx_nchw.shape == x.shape
    finally:
        ops.set_math_mode(saved)
        _lib.set_proxy(None)
    _TRACES[key] = rec.rows[:n_fwd], rec.rows[n_fwd:]
    return _TRACES[key]


def _is_subsequence(short, long):
    it = iter(long)
    return all(any(r == q for q in it) for r in short)


def _data_gradient_rows(full_bwd):
    last = max(i for i, r in enumerate(full_bwd) if r[0] == "psld_nhwc_to_nchw_f32")
    if last + 1 < len(full_bwd) and full_bwd[last + 1][0] == "psld_axpby_f32" and not _has_g(full_bwd[last + 1]):
        last += 1       # dx of the stem added to the pyramid's
    return [r for r in full_bwd[:last + 1] if not _has_g(r) and not _param_only_name(r[0]) and r[0] != "psld_colsum_f32"]


@pytest.mark.parametrize("name", list(CASES))
def test_input_only_trace(name, monkeypatch):
    full_fwd, full_bwd = _trace(name, False, monkeypatch)
    fwd, bwd = _trace(name, True, monkeypatch)
    # the full pass does what this test assumes of it
    g_names = {r[0] for r in full_bwd if _has_g(r)}
    assert g_names, "the full backward writes no gradient?"
    unknown = {n for n in g_names if not _param_only_name(n)} - _SHARED
    assert not unknown, f"entry points that write gradients and are in neither list of this test: {sorted(unknown)}"
    assert any(_param_only_name(r[0]) and not _has_g(r) for r in full_bwd)      # split-K producers: slabs, no "g"
    # no pointer into the flat gradient buffer, no weight-gradient or parameter-reduction entry point - in either half
    assert not [r[0] for r in fwd + bwd if _has_g(r)]
    assert not sorted({r[0] for r in fwd + bwd if _param_only_name(r[0])})
    # the same launches with the same arguments, in order
    assert _is_subsequence(fwd, full_fwd)
    assert _is_subsequence(bwd, full_bwd)
    # every data-gradient row of the full backward is there - and nothing else
    assert bwd == _data_gradient_rows(full_bwd)
    assert len(bwd) < len(full_bwd)


def test_flag_is_off_by_default():
    import inspect

    from psld_amd.score_tape import _ExecBase
    sig = inspect.signature(_ExecBase.__init__)
    assert sig.parameters["input_grad_only"].default is False

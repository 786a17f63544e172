"""The NCF entry points alone (csrc/ncf.hip: clsr_ncf_score, clsr_ncf_train) against the float64 reference of
tests/ncf_cases.py.  Logits and model_output are held within the propagated fp32 bound of the reference
(tests/ncf_oracle.py); dlogit, the four slice sets, the reduced dense gradient block and the slices' sums of squares to the
relative tolerances and floor of tests/test_caser_gpu.py (the case of identical lines, whose dense gradients cancel to an
exact zero, to the propagated error of the cancelling terms instead: tests/ncf_cases.py).  tests/test_ncf_cpu.py holds that no tower unit of any case is
undecidable, so no comparison hangs on a ReLU gate."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ncf_cases as K  # noqa: E402
from clsr_amd import _lib, ops  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402

DEV = "cuda:0"


def _within(got, exp, bound, name):
    got = got.detach().double().cpu().reshape(-1)
    err = (got - exp.reshape(-1)).abs()
    excess = float((err - bound.reshape(-1)).max())
    print("%s: max err %.3e, bound there %.3e" % (name, float(err.max()), float(bound.reshape(-1)[err.argmax()])))
    assert excess <= 0, "%s: error exceeds the propagated fp32 bound by %.3e" % (name, excess)


def _close(got, exp, rtol, atol, name):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    err = (got - exp).abs()
    excess = float((err - (atol + rtol * exp.abs())).max())
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


def _device_inputs(c):
    inp = K.make_inputs(c)
    tabs = [t.to(DEV) for t in inp["tabs"]]
    return inp, tabs, K.block(inp).to(DEV), inp["users"].to(DEV), inp["items"].to(DEV), inp["labels"].to(DEV)


def _train(c, poison=0.0):
    """One clsr_ncf_train call + the partial-sum reduction the caller owes.  Outputs start from ``poison`` so that an
    element nobody wrote shows."""
    inp, tabs, blk, users, items, labels = _device_inputs(c)
    shape = (c.Du, len(c.widths)) + K.w4(c.widths)
    P = query("clsr_ncf_param_floats", *shape)
    assert P == blk.numel()
    parts = query("clsr_ncf_parts", c.B, c.G)
    full = lambda *s: torch.full(s, poison, device=DEV)
    out = dict(logit=full(c.B), mo=full(c.B, c.Du + c.widths[-1]), dlogit=full(c.B), sl=[full(c.B, c.Du) for _ in range(4)],
               uid=torch.full((c.B,), -1, dtype=torch.int32, device=DEV),
               ws=full(query("clsr_ncf_workspace_floats", c.B, c.G, *shape)),
               loss=torch.zeros(8, dtype=torch.float64, device=DEV), ss=torch.zeros(4, dtype=torch.float64, device=DEV),
               dblock=full(P))
    call("clsr_ncf_train", users, 1, items, labels, *tabs, blk, *shape, c.B, c.G, 1.0 / (c.B // c.G), out["logit"], out["mo"],
         out["dlogit"], *out["sl"], out["uid"], out["ws"], out["loss"], out["ss"])
    ops.multi("clsr_reduce_parts_multi", ops.RpDesc,
              [ops.RpDesc.row(partial=out["ws"][10 * parts:], out=out["dblock"], scale=1.0, nparts=parts, stride=P, n=P)])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_train_matches_reference(c):
    ref, out = K.reference(c), _train(c, poison=float("nan"))
    _within(out["logit"], ref["logit"], ref["e_logit"], "logit")
    _within(out["mo"], ref["model_output"], ref["e_model_output"], "model_output")
    assert torch.equal(out["uid"].cpu(), K.make_inputs(c)["users"])
    _close([float(out["loss"][0])], [ref["loss"]], 1e-5, 1e-7, "loss")
    floor = 4e-6 * float(ref["dblock"].abs().max())
    _close(out["dlogit"], ref["dlogit"], 2e-3, 2e-4 * float(ref["dlogit"].abs().max()), "dlogit")
    for k, (got, exp) in enumerate(zip(out["sl"], ref["slices"])):
        _close(got, exp, 2e-3, 2e-4 * float(exp.abs().max()) + floor, "slices %d" % k)
        _close([float(out["ss"][k]) ** 0.5], [ref["sumsq"][k] ** 0.5], 1e-3, 1e-7, "slice norm %d" % k)
    if ref["cancel_bound"] is not None:      # identical lines: an exact cancellation, held to the error of its terms
        assert float(ref["dblock"].abs().max()) < 1e-15
        _within(out["dblock"], ref["dblock"], ref["cancel_bound"], "dense gradient block (cancelling)")
    else:
        _close(out["dblock"], ref["dblock"], 2e-3, 2e-4 * float(ref["dblock"].abs().max()) + floor, "dense gradient block")


@pytest.mark.parametrize("c", K.SCORE + [K.CASES[4]], ids=K.case_id)
def test_score_matches_reference(c):
    ref = K.reference(c)
    inp, tabs, blk, users, items, _ = _device_inputs(c)
    shape = (c.Du, len(c.widths)) + K.w4(c.widths)
    logit = torch.full((c.B,), float("nan"), device=DEV)
    mo = torch.full((c.B, c.Du + c.widths[-1]), float("nan"), device=DEV)
    call("clsr_ncf_score", users, 1, items, *tabs, blk, *shape, c.B, logit, mo)
    torch.cuda.synchronize()
    _within(logit, ref["logit"], ref["e_logit"], "logit")
    _within(mo, ref["model_output"], ref["e_model_output"], "model_output")
    logit2 = torch.full((c.B,), float("nan"), device=DEV)
    call("clsr_ncf_score", users, 1, items, *tabs, blk, *shape, c.B, logit2, None)      # model_output is optional
    torch.cuda.synchronize()
    assert torch.equal(logit, logit2)


def test_shared_user_rows():
    """``user_div`` = G: one user id per group of G lines (the compact feed of de-duplicated histories)."""
    c = K.CASES[2]
    inp, tabs, blk, users, items, _ = _device_inputs(c)
    shape = (c.Du, len(c.widths)) + K.w4(c.widths)
    per_group = users[::c.G].contiguous()
    a, b = torch.empty(c.B, device=DEV), torch.empty(c.B, device=DEV)
    call("clsr_ncf_score", per_group.repeat_interleave(c.G), 1, items, *tabs, blk, *shape, c.B, a, None)
    call("clsr_ncf_score", per_group, c.G, items, *tabs, blk, *shape, c.B, b, None)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_two_launches_are_bit_identical():
    a, b = _train(K.MULTI), _train(K.MULTI, poison=7.0)
    for k in ("logit", "mo", "dlogit", "uid", "loss", "ss", "dblock"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["sl"], b["sl"]):
        assert torch.equal(x, y)


def test_shape_past_the_lds_limit_is_refused():
    Du, widths = K.PAST_LDS
    shape = (Du, len(widths)) + K.w4(widths)
    assert query("clsr_ncf_supported", *shape, 5) == 0
    assert query("clsr_ncf_lds_floats", *shape) > query("clsr_ncf_lds_budget_floats")
    c = K.Case(10, 5, Du, widths, "edge", 0, "")
    inp, tabs, blk, users, items, labels = _device_inputs(c)
    lib = _lib.load()
    logit = torch.zeros(c.B, device=DEV)
    s = ops.stream_ptr()
    rc = lib.clsr_ncf_score(users.data_ptr(), 1, items.data_ptr(), *[t.data_ptr() for t in tabs], blk.data_ptr(), *shape,
                            c.B, logit.data_ptr(), None, s)
    assert rc == -1 and "ncf" in _lib.last_error()
    with pytest.raises(_lib.ClsrLibraryError):
        call("clsr_ncf_score", users, 1, items, *tabs, blk, *shape, c.B, logit, None)
    # a group the tile cannot hold, rows that are no whole groups: -1 as well
    ok = K.CASES[0]
    inp, tabs, blk, users, items, labels = _device_inputs(ok)
    shape = (ok.Du, len(ok.widths)) + K.w4(ok.widths)
    gmax = query("clsr_ncf_max_group")
    assert query("clsr_ncf_supported", *shape, gmax) == 1 and query("clsr_ncf_supported", *shape, gmax + 1) == 0
    out = _train(ok)
    for B, G in ((gmax + 1, gmax + 1), (ok.B - 1, ok.G)):
        with pytest.raises(_lib.ClsrLibraryError):
            call("clsr_ncf_train", users, 1, items, labels, *tabs, blk, *shape, B, G, 1.0, out["logit"], out["mo"], out["dlogit"],
                 *out["sl"], out["uid"], out["ws"], out["loss"], out["ss"])

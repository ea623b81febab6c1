"""``ops.loco.loco_linear`` (``loco_linear_kernels.hip``) against ``loco_linear_reference`` at the smallest shapes that
reach each path: 1 / 63 / 64 / 65 / 130 columns (the 64-column chunk and its tail), 2100 (the row is read again, not
kept in LDS), 1 / 5 / 9 records over four waves a workgroup, 1 / 3 / 16 margin columns.
Integer cases (integer ``X`` and ``W``; identity and step links) are exact in fp64, so values, order and the tie rule
must match the reference cell for cell. Real cases stay within ``d * 2^-52 * (1 + sum_j |W_j x_j|)`` times the slope
bound of the link, and their selection is compared where the reference keys are more than twice that apart. With one
column that bound is below the rounding of ``exp`` itself, so ``d = 1`` runs the links that are exact there."""
import numpy as np
import pytest
import torch

import loco_linear_reference as R
from transmogrifai_amd.ops.loco import loco_linear

pytestmark = pytest.mark.gpu

# a group across the 64-column boundary, two interleaved in one chunk, one whose cells are all zero
GROUPS = {130: [list(range(60, 70)), [70, 72, 74], [71, 73, 75], [100, 101]], 65: [[62, 63, 64]], 2100: [[5, 2090]]}
#        d, n, Cm, link, top_k, fp64, abs, leave_out
INTEGER = [(1, 1, 1, "identity", 1, False, True, False), (1, 5, 1, "identity", 20, True, False, False),
           (63, 5, 1, "identity", 3, True, False, False), (64, 9, 1, "step", 20, False, True, True),
           (65, 5, 1, "identity", 20, False, False, True), (130, 9, 1, "identity", 3, True, True, False),
           (130, 9, 1, "identity", 20, False, False, True), (130, 5, 1, "identity", 64, True, False, False),
           (2100, 2, 1, "identity", 20, False, True, False)]
REAL = [(1, 9, 1, "identity", 3, True, True, False), (63, 5, 1, "binary", 3, False, True, False),
        (64, 9, 3, "softmax", 20, True, False, False), (65, 5, 16, "softmax", 1, False, True, True),
        (130, 9, 1, "exp", 20, True, False, True), (130, 5, 3, "softmax", 3, False, False, False),
        (130, 9, 16, "softmax", 20, True, True, True), (130, 5, 1, "sigmoid", 3, True, True, False),
        (130, 5, 1, "square", 3, False, True, True), (130, 5, 1, "inverse", 3, True, False, False),
        (130, 5, 1, "power", 3, True, True, False)]


def _case(d, n, Cm, link, integer, fp64):
    rng = np.random.default_rng(d * 131 + n * 17 + Cm)
    if integer:                                      # small integers: equal keys and zero coefficients occur
        X = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
        W = rng.integers(-2, 3, size=(d, Cm)).astype(np.float64)
        b, param = np.ones(Cm), 0.5
    else:
        X = rng.normal(size=(n, d)).astype(np.float32).astype(np.float64) * (rng.random((n, d)) < 0.6)
        W = rng.normal(size=(d, Cm)) / np.sqrt(d)
        b, param = rng.normal(size=Cm), 2.0
        if link in ("square", "inverse", "power"):   # margins in [1, ...): away from the links' singular points
            X, W, b = np.abs(X), np.abs(W), np.ones(Cm) + np.abs(W).T @ np.abs(X).max(0)
            W = -W
    groups = GROUPS.get(d, [])
    if d == 130:
        X[:, groups[3]] = 0
    if n > 1:
        X[-1] = 0                                    # an all-zero record
    dev = torch.device("cuda")
    cand = np.empty(d, np.int64)
    plain = [j for j in range(d) if not any(j in g for g in groups)]
    cand[plain] = np.arange(len(plain))
    for g, cols in enumerate(groups):
        cand[cols] = len(plain) + g
    args = (torch.as_tensor(X, dtype=torch.float64 if fp64 else torch.float32, device=dev), torch.as_tensor(W),
            torch.as_tensor(b), link, param, torch.as_tensor(cand, device=dev), len(plain),
            torch.as_tensor([float(len(g)) for g in groups], dtype=torch.float64, device=dev))
    return X, W, b, param, groups, args


@pytest.mark.parametrize("integer,d,n,Cm,link,top_k,fp64,abs_mode,leave_out",
                         [(True,) + c for c in INTEGER] + [(False,) + c for c in REAL])
def test_kernel_matches_the_reference(integer, d, n, Cm, link, top_k, fp64, abs_mode, leave_out):
    X, W, b, param, groups, args = _case(d, n, Cm, link, integer, fp64)
    wcols, wdiffs, vals, unit, L = R.loco(X, W, b, link, param, groups, top_k, abs_mode, leave_out)
    K, C = wdiffs.shape[1:]                       # sentinel-filled outputs with a guard behind them
    cbuf = torch.full((n * K + 64,), -7, dtype=torch.long, device="cuda")
    dbuf = torch.full((n * K * C + 64,), -7.5, dtype=torch.float64, device="cuda")
    loco_linear(*args, top_k, abs_mode, leave_out, out=(cbuf[:n * K].view(n, K), dbuf[:n * K * C].view(n, K, C)))
    assert (cbuf[n * K:] == -7).all() and (dbuf[n * K * C:] == -7.5).all() and not (dbuf[:n * K * C] == -7.5).any()
    again = loco_linear(*args, top_k, abs_mode, leave_out)
    cols, diffs = cbuf[:n * K].view(n, K), dbuf[:n * K * C].view(n, K, C)
    assert torch.equal(cols, again[0]) and torch.equal(diffs, again[1])         # bitwise repeatable
    assert (diffs[cols < 0] == 0).all() and (n == 1 or (cols[-1] == -1).all())   # the all-zero record: no insight
    cols, diffs = cols.cpu().numpy(), diffs.cpu().numpy()
    bound = np.zeros(n) if integer else d * 2.0 ** -52 * (L + unit)
    ok = R.separated(vals, abs_mode, 2 * bound) | integer
    assert ok.sum() >= n - 1 and ((wcols[ok] >= 0).any() or d == 1)
    assert np.array_equal(cols[ok], wcols[ok])
    assert (np.abs(diffs[ok] - wdiffs[ok]).max((1, 2)) <= bound[ok]).all(), (np.abs(diffs - wdiffs).max((1, 2)), bound)


def test_public_path_on_a_device_vector_equals_the_host_formula():
    from test_record_insights_loco_margins import HIST, _fit
    from transmogrifai_amd.data.columns import VectorColumn
    from transmogrifai_amd.stages.insights.record_insights import RecordInsightsLOCO
    X, model = _fit("lr2")
    st = RecordInsightsLOCO(model, top_k=3, perturbation="margins", vector_aggregation_strategy="LeaveOutVector")
    st.histories = HIST
    host, dev = st.transform_columns(VectorColumn(X)), st.transform_columns(VectorColumn(X.cuda()))
    assert dev.cols.is_cuda and torch.equal(dev.cols.cpu(), host.cols)
    W, b, link, param = model.learner.linear_margins(model.state)
    unit, L = R.loco(X.numpy(), W.numpy(), b.numpy(), link, param, [[6, 7, 8, 9]], 3, True, True)[3:]
    assert ((dev.diffs.cpu() - host.diffs).abs().amax((1, 2)).numpy() <= 10 * 2.0 ** -52 * (L + unit)).all()

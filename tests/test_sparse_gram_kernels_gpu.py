"""``SparseDesign.wgram`` / ``mm64`` (``ops/csrc/hip/sparse_gram_kernels.hip``) against numpy fp64 of the definition on the
designs of tests/multiclass_oracle.py, and the two regression learners that take them on the public path. Integer cases
({+-1, +-2} values, weights {0, 1, 2}, ``|y| <= 3``) have integer products and sums far below 2^53: the Gram must equal
numpy's in any summation order. Real cases: ``|G - G_ref| <= N U64 (|A|^T |w| |A|)``, the bound of an fp64 sum of N
exact-product terms."""
import functools

import numpy as np
import pytest
import torch

import multiclass_oracle as O
from transmogrifai_amd.models.base import FitJob, learner_class
from transmogrifai_amd.ops import _native as N_
from transmogrifai_amd.ops import linear as LK
from transmogrifai_amd.ops.stats import weighted_gram

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = -1.5e300
DESIGNS = (("segs70", True), ("segs70", False), ("seg4096_two_segments", True), ("n1", True), ("n5", True),
           ("no_dense", True), ("no_sparse", True))


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _design(name, integer):
    X = O.design(name, integer)
    with pytest.MonkeyPatch.context() as mp:
        if name != "seg4096_two_segments":          # that one cuts its column at the segment length as shipped
            mp.setattr(LK, "_SEG_NNZ", O.SEG_SMALL)
        return X, LK.SparseDesign(_cuda(X))


def _case(N, K, ymode, integer):
    """Weights ``[N, K]`` and the response (None, ``[N]`` or ``[N, K]``) in fp64."""
    rng = np.random.default_rng(1000 * K + len(ymode) + int(integer))
    if integer:
        W = rng.integers(0, 3, (N, K)).astype(F64)
        W[rng.random(N) < 0.3] = 0                  # whole rows without weight: a fold mask
        Y = rng.integers(-3, 4, (N, K)).astype(F64)
    else:
        W, Y = O._weights(rng, (N, K)).astype(F64), rng.standard_normal((N, K))
    return W, {"none": None, "shared": Y[:, 0].copy(), "per_weight": Y}[ymode]


def _definition(X, W, Y):
    """``A_k^T diag(w_k) A_k`` with ``A_k = [X | 1 | y_k]`` and the real-case bound, ``[K, D, D]`` each."""
    N, K = W.shape
    G, B = [], []
    for k in range(K):
        yk = [] if Y is None else [(Y if Y.ndim == 1 else Y[:, k])[:, None]]
        A = np.concatenate([X.astype(F64), np.ones((N, 1))] + yk, 1)
        G.append(A.T @ (W[:, k:k + 1] * A))
        B.append(N * O.U64 * (np.abs(A).T @ (np.abs(W[:, k:k + 1]) * np.abs(A))))
    return np.stack(G), np.stack(B)


def _check_wgram(D, X, W, Y, integer):
    ref, bound = _definition(X, W, Y)
    out = torch.full(ref.shape, SENT, dtype=torch.float64, device="cuda")       # every element must be overwritten
    g = D.wgram(_cuda(W), _cuda(Y), out=out).cpu().numpy()
    dense = weighted_gram(_cuda(X), _cuda(W), _cuda(Y)).cpu().numpy()
    assert np.array_equal(g, g.transpose(0, 2, 1))
    if integer:
        assert np.array_equal(g, ref) and np.array_equal(dense, ref)
    else:
        assert (np.abs(g - ref) <= bound).all() and (np.abs(g - dense) <= bound).all()


@pytest.mark.parametrize("ymode", ("none", "shared", "per_weight"))
@pytest.mark.parametrize("kk", ("1", "KW", "KW+1"))
@pytest.mark.parametrize("name,integer", DESIGNS, ids=[f"{n}-{'int' if i else 'real'}" for n, i in DESIGNS])
def test_wgram_against_the_definition(name, integer, kk, ymode):
    X, D = _design(name, integer)
    kw = int(N_.hip().tmog_hip_sparse_wgram_kw())
    W, Y = _case(X.shape[0], {"1": 1, "KW": kw, "KW+1": kw + 1}[kk], ymode, integer)
    _check_wgram(D, X, W, Y, integer)


def _narrow_rows(n_dense, n_sparse):
    """67 rows: ``n_dense`` full integer columns, then sparse columns of 2 to 4 non-zeros each."""
    rng = np.random.default_rng(n_dense * 7 + n_sparse)
    X = np.zeros((67, n_dense + n_sparse), F32)
    X[:, :n_dense] = O._fill(rng, (67, n_dense), True)
    for t in range(4):
        hit = rng.random(n_sparse) < (1.0 if t < 2 else 0.5)
        X[rng.integers(0, 67, n_sparse)[hit], n_dense + np.flatnonzero(hit)] = O._fill(rng, int(hit.sum()), True)
    return X


@pytest.mark.parametrize("over", (-1, 0, 1))
def test_wgram_width_pass_boundary(over):
    """``ds + De`` one below, at and one above the width of one pass; above it the launch makes two column ranges."""
    width = int(N_.hip().tmog_hip_sparse_wgram_width_max()) + over
    X = _narrow_rows(2, width - 4)                  # De = 2 dense + 1 + y
    D = LK.SparseDesign(_cuda(X))
    assert D.ds + int(D.idx_d.numel()) + 2 == width and LK.sparse_wgram_supported(D)
    W, Y = _case(67, 2, "shared", True)
    _check_wgram(D, X, W, Y, True)


def test_wgram_dense_block_cap():
    cap = int(N_.hip().tmog_hip_sparse_wgram_dd_max())
    X = _narrow_rows(cap, 6)
    D = LK.SparseDesign(_cuda(X))
    assert int(D.idx_d.numel()) == cap and LK.sparse_wgram_supported(D)
    _check_wgram(D, X, *_case(67, 2, "per_weight", True), True)
    assert not LK.sparse_wgram_supported(LK.SparseDesign(_cuda(_narrow_rows(cap + 1, 6))))


@pytest.mark.parametrize("P", (1, 17, 65))
def test_mm64_against_numpy(P):
    X, D = _design("segs70", False)
    S = O.Sparse(X, O.SEG_SMALL)
    rng = np.random.default_rng(P)
    B, b0 = rng.standard_normal((X.shape[1], P)), rng.standard_normal(P)
    got = D.mm64(_cuda(B), _cuda(b0))
    assert torch.equal(got, D.mm64(_cuda(B), _cuda(b0)))                         # a fixed order: the same bits
    ref = X.astype(F64) @ B + b0
    bound = (S.row_nnz[:, None] + len(S.idx_d) + 2) * O.U64 * (np.abs(X).astype(F64) @ np.abs(B) + np.abs(b0))
    assert (np.abs(got.cpu().numpy() - ref) <= bound).all()
    c = int(S.idx_s[5])                             # a NaN row of B reaches the rows that hold its column, no other
    B[c] = np.nan
    bad = D.mm64(_cuda(B), _cuda(b0)).cpu().numpy()
    holds = X[:, c] != 0
    assert holds.any() and np.isnan(bad[holds]).all() and np.array_equal(bad[~holds], got.cpu().numpy()[~holds])


def test_wgram_repeatable():
    X, D = _design("segs70", False)
    W, Y = _case(X.shape[0], 5, "per_weight", False)
    assert torch.equal(D.wgram(_cuda(W), _cuda(Y)), D.wgram(_cuda(W), _cuda(Y)))


@functools.lru_cache(maxsize=None)
def _table():
    """4096 x 256 integers, ~3 % non-zeros and 2 dense columns; an integer and a Poisson response; 2 folds."""
    rng = np.random.default_rng(5)
    X = np.zeros((4096, 256), F32)
    hit = rng.random(X.shape) < 0.03
    X[hit] = O._fill(rng, int(hit.sum()), True)
    X[:, :2] = O._fill(rng, (4096, 2), True)
    beta = np.zeros(256)
    beta[:24] = rng.integers(-2, 3, 24)
    y_int = np.clip(np.rint(X @ beta / 4 + rng.integers(-1, 2, 4096)), -3, 3).astype(F32)
    y_poi = rng.poisson(np.exp(0.5 + 0.05 * (X @ beta))).astype(F32)
    fold = rng.integers(0, 2, 4096)
    return X, y_int, y_poi, [np.flatnonzero(fold != f) for f in range(2)]


def _fit(monkeypatch, learner, y, params, switch):
    """``fit_batch`` of one job per fold and parameter set; the states and the number of ``SparseDesign.wgram`` calls."""
    X, _, _, folds = _table()
    monkeypatch.setenv("TMOG_LINREG_SPARSE", switch)
    calls, orig = [], LK.SparseDesign.wgram
    monkeypatch.setattr(LK.SparseDesign, "wgram", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    lr = learner_class(learner)()
    rows = [_cuda(f) for f in folds]
    jobs = [FitJob(dict(lr.defaults, **p), r) for p in params for r in rows]
    return lr.fit_batch(_cuda(X), _cuda(y), jobs), len(calls)


def test_linear_regression_public_path(monkeypatch):
    params = [dict(reg_param=0.1), dict(reg_param=0.1, elastic_net_param=0.5)]
    on, n_on = _fit(monkeypatch, "OpLinearRegression", _table()[1], params, "1")
    off, n_off = _fit(monkeypatch, "OpLinearRegression", _table()[1], params, "0")
    assert n_on == 1 and n_off == 0
    for a, b in zip(on, off):                       # exact Grams on both paths, shared code after them
        assert np.array_equal(a["coefficients"], b["coefficients"]) and a["intercept"] == b["intercept"]


def _irls_numpy(X, y, rows, fam, reg, tol, max_iter):
    """The update of ``GeneralizedLinearRegressionLearner._irls`` in numpy fp64 for one problem: ``[coef | intercept]``."""
    N, d = X.shape
    Xa = np.concatenate([X.astype(F64), np.ones((N, 1))], 1)
    w0, y = np.zeros(N), y.astype(F64)
    w0[rows] = 1.0
    mean = (w0 @ Xa[:, :d]) / w0.sum()
    var_x = (w0 @ Xa[:, :d] ** 2) / w0.sum() - mean * mean
    pen = np.diag(np.append(reg * w0.sum() * np.maximum(var_x, 0), 0.0)) + 1e-12 * np.eye(d + 1)
    mu, beta = (np.where(y > 0, y, 0.1) if fam == "poisson" else y.copy()), np.zeros(d + 1)
    for _ in range(max_iter):
        eta, gp, var = (np.log(mu), 1.0 / mu, mu) if fam == "poisson" else (mu, np.ones(N), np.ones(N))
        z, w = eta + (y - mu) * gp, w0 / np.maximum(gp * gp * var, 1e-300)
        nb = np.linalg.solve(Xa.T @ (w[:, None] * Xa) + pen, Xa.T @ (w * z))
        delta, beta = np.abs(nb - beta).max(), nb
        mu = np.maximum(np.exp(Xa @ beta), 1e-12) if fam == "poisson" else Xa @ beta
        if delta < tol:
            break
    return beta


@pytest.mark.parametrize("fam", ("gaussian", "poisson"))
def test_glm_public_path(monkeypatch, fam):
    """Gaussian / identity, ``max_iter`` 1: one WLS step on an exact Gram, compared with numpy's solve of the same
    system at 1e-9 relative (ridge 0.1: the system's 2-norm condition number is 78, so a solve loses ~2 digits of
    fp64's 16). Poisson / log, ``tol`` 1e-8: both iterations stop after a step below ``tol`` and IRLS converges
    quadratically, so each is within ``tol`` of the fixed point: ``4 tol`` absolute. The dense path on the host
    meets the same bound against the same reference (6 iterations, largest difference 5.6e-16)."""
    X, y_int, y_poi, folds = _table()
    y, tol, iters = (y_int, 1e-6, 1) if fam == "gaussian" else (y_poi, 1e-8, 25)
    params = [dict(family=fam, reg_param=0.1, tol=tol, max_iter=iters)]
    on, n_on = _fit(monkeypatch, "OpGeneralizedLinearRegression", y, params, "1")
    off, n_off = _fit(monkeypatch, "OpGeneralizedLinearRegression", y, params, "0")
    assert n_on >= 2 and n_off == 0                 # G0 and every iteration's Gram
    for f, rows in enumerate(folds):
        ref = _irls_numpy(X, y, rows, fam, 0.1, tol, iters)
        for got in (on[f], off[f]):
            err = np.abs(np.append(got["coefficients"], got["intercept"]) - ref)
            assert (err <= (1e-9 * np.abs(ref).max() if fam == "gaussian" else 4 * tol)).all()

"""``sparse_lr_kernel`` (``ops/csrc/hip/sparse_lr_kernels.hip``, ``ops/linear.py`` ``sparse_lr_pass``) against numpy fp64 of
the definition on the designs of tests/multiclass_oracle.py. Bounds are derived (``u = 2^-24``): integer designs give
margins exact in fp32; the intrinsics get ``8 e32`` -- ``e32`` the largest difference of the kernel's formula in numpy
``float32`` and fp64 on the case's own fp32 margins, the loss divided by ``max(1, |l|)`` -- times ``w`` for R (plus one ``u``
for the product) and ``w max(1, |l|)`` for the loss; ``f`` and ``r`` add ``n 2^-52 sum |x|`` (their products are exact in
fp64); real designs add ``mm_bound`` and the bias through ``|l'| <= 1`` (squared: ``|r| + bound``; hinge: its step)."""
import functools

import numpy as np
import pytest
import torch

import multiclass_oracle as O
from transmogrifai_amd.ops import linear as LK

pytestmark = pytest.mark.gpu

U, U64, F32, F64 = O.U, O.U64, np.float32, np.float64
PS = (1, 16, 17, 24, 33, 65)            # chunk widths 16 / 16 / 32 / 32 / 64 and a second chunk of 64
DESIGNS = (("segs70", True), ("segs70", False), ("n1", True), ("n5", True), ("no_dense", True), ("no_sparse", True),
           ("nd128", True), ("nd129", True))
SENT = F32(-1.5e30)


@functools.lru_cache(maxsize=None)
def _design(name, integer):
    if name.startswith("nd"):           # N = 67: the last wave's row slots are partly filled at every chunk width
        nd = int(name[2:])
        X = np.zeros((67, nd + 6), F32)
        X[:, :nd] = O._fill(np.random.default_rng(nd), (67, nd), True)
        X[9 * np.arange(6), nd + np.arange(6)] = 2.0
    else:
        X = O.design(name, integer)
    return X, O.Sparse(X, 4096), LK.SparseDesign(torch.from_numpy(X).cuda())


def _case(X, P, loss, integer):
    (N, d), rng = X.shape, np.random.default_rng(P * 131 + len(loss))
    # integer V, every third row times 40: margins 0, +-1 and far beyond +-88; many-to-one wmap, a spare W column
    V = (rng.integers(-1, 2, (d, P)) * np.where(np.arange(d) % 3 == 0, 40, 1)[:, None]).astype(F32)
    if not integer:
        V = rng.standard_normal((d, P)).astype(F32)
    nw = max(1, (P + 1) // 2)
    return dict(V=V, bias=rng.integers(-2, 3, P).astype(F32), y=(rng.random(N) < 0.5).astype(F32),
                wmap=((np.arange(P) * 5) % nw).astype(np.int32), W=O._weights(rng, (N, nw + 1)),
                ysc=(0.5 + rng.random(P)).astype(F32) if loss == "squared" else None)


def _definition(loss, m, y, ysc):
    if loss != "logistic":              # the hinge and squared formulas are their definitions
        return _formula(loss, m, y, ysc, F64)
    y = y.astype(F64)[:, None]
    return np.maximum(m, 0) + np.log1p(np.exp(-np.abs(m))) - y * m, O.sigmoid(m) - y


def _formula(loss, m, y, ysc, t):
    """The kernel's formula (``loss_and_grad``) in numpy dtype ``t``, every operation rounded once."""
    m, y, one = m.astype(t), y.astype(t)[:, None], t(1)
    if loss == "logistic":
        with np.errstate(all="ignore"):
            e = np.exp(-np.abs(m))
            u = one + e
            lp = np.where(u == one, e, np.log(u) * (e / (u - one)))
        return np.maximum(m, 0) + lp - y * m, np.where(m >= 0, one / u, e * (one / u)) - y
    if loss == "hinge":
        ys = 2 * y - one
        return np.maximum(one - ys * m, 0), np.where(ys * m < one, -ys, t(0))
    r = m - y / ysc.astype(t)[None, :]
    return t(0.5) * r * r, r


def _run(D, c, loss, grad):
    # R inside a sentinel border with a spare column: only [N, P] may be written, and nothing with grad == 0
    N, P = D.shape[0], c["V"].shape[1]
    big = torch.full((N + 2, P + 3), float(SENT), dtype=torch.float32, device="cuda")
    t = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in c.items()}
    f, r, _ = LK.sparse_lr_pass(D, t["y"], t["W"], t["V"], t["bias"], loss, t["ysc"], grad, t["wmap"],
                                R=big[1:N + 1, 1:P + 1])
    got = big.cpu().numpy()
    inner = got[1:N + 1, 1:P + 1].copy()
    got[1:N + 1, 1:P + 1] = SENT
    assert (got == SENT).all(), "written outside R [N, P]"
    assert (inner != SENT).all() if grad else (inner == SENT).all()
    return f.cpu().numpy(), r.cpu().numpy(), inner


@pytest.mark.parametrize("grad", (True, False), ids=("grad1", "grad0"))
@pytest.mark.parametrize("loss", ("logistic", "hinge", "squared"))
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("name,integer", DESIGNS, ids=[f"{n}-{'int' if i else 'real'}" for n, i in DESIGNS])
def test_kernel_matches_fp64(name, integer, P, loss, grad):
    from transmogrifai_amd.ops import _native
    assert _native.hip().tmog_hip_sparse_lr_nd_max() == 128          # nd128 / nd129 stand on each side of it
    X, S, D = _design(name, integer)
    c = _case(X, P, loss, integer)
    m, mb = O.mm_bound(S, c["V"])
    m, mb = m + c["bias"].astype(F64), (mb + U * np.abs(c["bias"])) * (not integer)
    if integer and name == "segs70" and P >= 16:
        assert (np.abs(m) > 88).any() and (m == 0).any() and ((2 * c["y"][:, None] - 1) * m == 1).any()
    w = c["W"][:, c["wmap"]].astype(F64)
    l, g = _definition(loss, m, c["y"], c["ysc"])
    m32 = m.astype(F32)
    (l32, g32), (l64, g64) = (_formula(loss, m32, c["y"], c["ysc"], t) for t in (F32, F64))
    el = 8 * float((np.abs(l32 - l64) / np.maximum(1.0, np.abs(l64))).max())
    eg = 8 * float(np.abs(g32 - g64).max())
    step = {"logistic": mb, "squared": mb, "hinge": 1.0 * (np.abs((2 * c["y"][:, None] - 1) * m - 1) < mb)}[loss]
    tol_l = w * (el * np.maximum(1.0, np.abs(l)) + mb * (np.abs(g) + mb if loss == "squared" else 1.0))
    tol_g = w * (eg + step)
    f, r, R = _run(D, c, loss, grad)
    assert (np.abs(f - (w * l).sum(0)) <= tol_l.sum(0) + len(X) * U64 * np.abs(w * l).sum(0)).all()
    assert (np.abs(r - (w * g).sum(0)) <= tol_g.sum(0) + len(X) * U64 * np.abs(w * g).sum(0)).all()
    if grad:
        assert (np.abs(R - w * g) <= tol_g + U * np.abs(w * g)).all()
        if integer and loss != "logistic":
            assert (O.bits(R) == O.bits(g32 * c["W"][:, c["wmap"]])).all()


def test_a_nan_row_of_v_reaches_only_the_rows_that_hold_its_column():
    X, S, D = _design("segs70", True)           # rows of 0 to 130 non-zeros share waves: short rows are padded
    c = _case(X, 24, "logistic", True)
    base = _run(D, c, "logistic", True)[2]
    j = int(S.idx_s[0])
    c["V"][j] = np.nan
    R, hit = _run(D, c, "logistic", True)[2], X[:, j] != 0
    assert hit.any() and np.isnan(R[hit]).all() and (O.bits(R[~hit]) == O.bits(base[~hit])).all()


@pytest.mark.parametrize("P", (24, 65))
def test_two_calls_are_bitwise_equal(P):
    X, S, D = _design("segs70", False)
    a, b = (_run(D, _case(X, P, "logistic", False), "logistic", True) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _sparse_x(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.where(torch.rand(N, d, generator=g) < 0.03, torch.rand(N, d, generator=g) * 3, torch.zeros(N, d))
    X[:, :5] = torch.randn(N, 5, generator=g)
    return X, g


@pytest.mark.parametrize("loss", ("logistic", "hinge"))
def test_batched_objective_on_sparse_design_matches_fp64(loss):
    from transmogrifai_amd.models.linear import BatchedObjective
    N, d, P = 4096, 300, 4
    X, g = _sparse_x(N, d, 5)
    y = (torch.rand(N, generator=g) < 0.4).double()
    W = (torch.rand(N, P, generator=g) < 0.7).double()
    inv_std = torch.rand(d, P, generator=g, dtype=torch.float64) + 0.5
    l2, fi = torch.tensor([0.0, 0.01, 0.1, 1.0], dtype=torch.float64), torch.tensor([True, True, False, True])
    Uc = 0.05 * torch.randn(d + 1, P, generator=g, dtype=torch.float64)
    ref = BatchedObjective(X.double(), y, W, inv_std, loss, l2, fi)
    ob = BatchedObjective(LK.SparseDesign(X.cuda()), y.cuda(), W.cuda().float(), inv_std.cuda(), loss, l2.cuda(),
                          fi.cuda())
    assert ob.fused
    (f0, g0), (f1, g1) = ref.value_grad(Uc), ob.value_grad(Uc.cuda())
    torch.testing.assert_close(f1.cpu(), f0, rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(ob.value(Uc.cuda()).cpu(), ref.value(Uc), rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(g1.cpu(), g0, rtol=2e-4, atol=2e-6)


def test_linear_svc_fit_on_sparse_design_matches_dense_fit(monkeypatch):
    from transmogrifai_amd.models.base import FitJob, learner_class
    X, g = _sparse_x(8192, 320, 3)
    beta = torch.tensor([1.0, -1.0, 0.5, 0.0, 0.3, 0.8, -0.6, 1.5])
    X, y = X.cuda(), (torch.rand(8192, generator=g) < torch.sigmoid(X[:, :8] @ beta)).float().cuda()
    svc = learner_class("OpLinearSVC")()
    jobs = [FitJob(dict(svc.defaults, reg_param=0.1, max_iter=60), r)
            for r in (torch.arange(0, 6000, device="cuda"), torch.arange(2000, 8192, device="cuda"))]
    assert LK.SparseDesign.worthwhile(X)
    a = svc.fit_batch(X, y, jobs)
    monkeypatch.setenv("TMOG_LR_SPARSE", "0")
    b = svc.fit_batch(X, y, jobs)
    for s1, s2 in zip(a, b):
        np.testing.assert_allclose(s1["coefficients"], s2["coefficients"], atol=2e-3)

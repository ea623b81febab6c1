"""``sparse_mnl_kernel`` (``ops/csrc/hip/sparse_mnl_kernels.hip``, ``ops/linear.py`` ``sparse_mnl_pass``) against numpy fp64
of the definition (``O.softmax_loss_residual`` on ``O.mm_bound(S, V)[0] + bias``) on the designs of
tests/multiclass_oracle.py. The tolerance is the model of tests/test_multiclass_kernels_gpu.py ``_softmax_expect``
(``u = 2^-24``): ``O.allow_e32`` of the case's own ``e32`` times ``w`` for R and ``w max(1, |lse|)`` for the loss, ``u |x|`` for
the product with ``w``, ``n 2^-52 sum |x|`` for the fp64 sums. ``e32`` is evaluated here with the kernel's order of addition: the
exponentials of a problem are added as a balanced tree over its group of ``KP`` lanes (``_e32``), not in class order.

Integer designs give margins exact in fp32, so that is all the slack. Real designs add the margin error ``b = max_k
(mm_bound + u |bias|)`` through the softmax's Lipschitz constants in the max norm: ``d p_k / d m_j = p_k ([j == k] - p_j)``
has absolute row sum ``2 p_k (1 - p_k) <= 1/2``, so ``|dp_k| <= b / 2``; ``d (lse - m_y) / d m_j = p_j - [j == y]`` has
absolute sum ``2 (1 - p_y) <= 2``, so ``|dl| <= 2 b``.

The ``E32`` caps of the oracle (4.5e-7 / 4.7e-7) are left as they are. Evaluating ``_e32`` with numpy ``float32`` on the
host over every case of this file gave at most 2.30e-7 for the probabilities (below its cap) and 2.91e-5 for the loss
(above: the cap binds). The large loss figures come from saturated rows whose label's margin lies far below ``lse`` (``m_y =
-83`` under ``lse = 3``): they are the one rounding of ``lse - m_y`` at the size of ``|m_y|`` measured against ``|lse|``, which
the ``u |loss|`` term already grants."""
import functools

import numpy as np
import pytest
import torch

import multiclass_oracle as O
from transmogrifai_amd.ops import linear as LK

pytestmark = pytest.mark.gpu

U, U64, F32, F64 = O.U, O.U64, np.float32, np.float64
DESIGNS = (("segs70", True), ("segs70", False), ("n1", True), ("n5", True), ("no_dense", True), ("no_sparse", True),
           ("nd128", True), ("nd129", True))


def _kp(K):
    return 4 if K <= 4 else 8 if K <= 8 else 16


# each KP = 4 / 8 / 16 from both sides; per K, (P, rows a wave): a partly filled slot of 16 lanes, the 32-lane slot, a
# full chunk of 64 lanes, a second chunk (in the same lanes; on blockIdx.y where the dense block leaves no room), three
# and four chunks a lane, and six chunks as two workgroup columns of three
KPS = [(K, P, rows) for K in (2, 3, 4, 5, 8, 9, 16) for pw in (64 // _kp(K),)
       for P, rows in ((1, 4), (pw // 2, 2), (pw, 1), (pw + 1, 1), (3 * pw, 1), (4 * pw, 1), (5 * pw + 1, 1))]
SENT = F32(-1.5e30)


@functools.lru_cache(maxsize=None)
def _design(name, integer):
    if name.startswith("nd"):           # N = 67: the last wave's row slots are partly filled at every slot width
        nd = int(name[2:])
        X = np.zeros((67, nd + 6), F32)
        X[:, :nd] = O._fill(np.random.default_rng(nd), (67, nd), True)
        X[9 * np.arange(6), nd + np.arange(6)] = 2.0
    else:
        X = O.design(name, integer)
    return X, O.Sparse(X, 4096), LK.SparseDesign(torch.from_numpy(X).cuda())


def _e32(m32, y, kp):
    """``O.softmax_e32`` with the kernel's sum: classes padded to ``kp`` with -inf, added by xor butterfly."""
    N, P, K = m32.shape
    mp = np.full((N, P, kp), -np.inf, F32)
    mp[:, :, :K] = m32
    mx = mp.max(2, keepdims=True)
    e = np.exp((mp - mx).astype(F32)).astype(F32)
    se, s = e, 1
    while s < kp:
        se, s = (se + se[:, :, np.arange(kp) ^ s]).astype(F32), 2 * s
    se = se[:, :, :1]
    p32, lse32 = (e * (F32(1) / se).astype(F32)).astype(F32)[:, :, :K], (mx + np.log(se).astype(F32)).astype(F32)[:, :, 0]
    loss64, R64, lse64 = O.softmax_loss_residual(m32, y, np.ones((N, P)))
    yi = y.astype(np.int64)
    ok = (yi >= 0) & (yi < K)
    my32 = np.take_along_axis(m32, np.clip(yi, 0, K - 1)[:, None, None].repeat(P, 1), 2)[:, :, 0]
    loss32 = np.where(ok[:, None], (lse32 - my32).astype(F32), F32(0))
    oh = np.zeros((N, 1, K))
    oh[np.flatnonzero(ok), 0, yi[ok]] = 1.0
    return (float(np.abs(p32 - (R64 + oh)).max()),
            float((np.abs(loss32 - loss64) / np.maximum(1.0, np.abs(lse64))).max()))


@functools.lru_cache(maxsize=None)
def _case(name, integer, K, P):
    """Operands, the fp64 reference and the tolerances, computed once for both ``grad`` settings."""
    X, S, _ = _design(name, integer)
    (N, d), rng, C = X.shape, np.random.default_rng(K * 1009 + P), P * K
    # integer V, every third row times 40: rows where one class takes all the mass and rows where classes tie
    V = (rng.integers(-1, 2, (d, C)) * np.where(np.arange(d) % 3 == 0, 40, 1)[:, None]).astype(F32)
    if not integer:
        V = rng.standard_normal((d, C)).astype(F32)
    bias = rng.integers(-1, 2, C).astype(F32)
    nw = max(1, (P + 1) // 2)           # a many-to-one wmap and a spare W column
    c = dict(V=V, bias=bias, y=O._labels(rng, N, K), wmap=((np.arange(P) * 5) % nw).astype(np.int32),
             W=O._weights(rng, (N, nw + 1)))
    m, mb = O.mm_bound(S, V)
    m = (m + bias.astype(F64)).reshape(N, P, K)
    b = ((mb + U * np.abs(bias)) * (not integer)).reshape(N, P, K).max(2)
    w = c["W"][:, c["wmap"]].astype(F64)
    loss, R, lse = O.softmax_loss_residual(m, c["y"], w)
    ep, el = _e32(m.astype(F32), c["y"], _kp(K))
    tolL = w * (O.allow_e32("softmax_loss", el) * np.maximum(1.0, np.abs(lse)) + 2 * b) + U * np.abs(loss)
    tolR = w[:, :, None] * (O.allow_e32("softmax_p", ep) + 0.5 * b[:, :, None]) + U * np.abs(R)
    return c, m, loss, R.reshape(N, C), tolL, tolR.reshape(N, C)


def _run(D, c, P, K, grad):
    # R inside a sentinel border with spare columns: only [N, P*K] may be written, and nothing with grad == 0
    N, C = D.shape[0], P * K
    big = torch.full((N + 2, C + 3), float(SENT), dtype=torch.float32, device="cuda")
    t = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    f, rs, _ = LK.sparse_mnl_pass(D, t["y"], t["W"], t["V"], t["bias"], P, K, grad, t["wmap"], R=big[1:N + 1, 1:C + 1])
    got = big.cpu().numpy()
    inner = got[1:N + 1, 1:C + 1].copy()
    got[1:N + 1, 1:C + 1] = SENT
    assert (got == SENT).all(), "written outside R [N, P*K]"
    assert (inner != SENT).all() if grad else (inner == SENT).all()
    return f.cpu().numpy(), rs.cpu().numpy(), inner


@pytest.mark.parametrize("grad", (True, False), ids=("grad1", "grad0"))
@pytest.mark.parametrize("K,P,rows", KPS)
@pytest.mark.parametrize("name,integer", DESIGNS, ids=[f"{n}-{'int' if i else 'real'}" for n, i in DESIGNS])
def test_kernel_matches_fp64(name, integer, K, P, rows, grad):
    from transmogrifai_amd.ops import _native
    assert _native.hip().tmog_hip_sparse_mnl_nd_max() == 128         # nd128 / nd129 stand on each side of it
    assert _native.hip().tmog_hip_sparse_mnl_rows(P, K) == rows
    X, S, D = _design(name, integer)
    c, m, loss, R, tolL, tolR = _case(name, integer, K, P)
    if integer and name == "segs70" and P > 1:
        top = np.sort(m, 2)[:, :, -2:]
        assert (top[:, :, 1] - top[:, :, 0] > 120).any() and (top[:, :, 1] == top[:, :, 0]).any()
        assert ((c["y"] < 0) | (c["y"] >= K)).any() and (c["W"] == 0).any()
    f, rs, Rg = _run(D, c, P, K, grad)
    assert (np.abs(f - loss.sum(0)) <= tolL.sum(0) + len(X) * U64 * np.abs(loss).sum(0)).all()
    assert (np.abs(rs - R.sum(0)) <= tolR.sum(0) + len(X) * U64 * np.abs(R).sum(0)).all()
    if grad:
        assert (np.abs(Rg - R) <= tolR).all(), float((np.abs(Rg - R) - tolR).max())


@pytest.mark.parametrize("K,P", ((6, 24), (3, 2)))
def test_two_calls_are_bitwise_equal(K, P):
    D = _design("segs70", False)[2]
    a, b = (_run(D, _case("segs70", False, K, P)[0], P, K, True) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_seventeen_classes_are_not_served():
    D = _design("n5", True)[2]
    assert LK.sparse_mnl_supported(D, 16) and not LK.sparse_mnl_supported(D, 17) and not LK.sparse_mnl_supported(D, 1)


def test_multinomial_fit_takes_the_sparse_pass_and_matches_the_unfused_fit(monkeypatch):
    from transmogrifai_amd.models import linear as ML
    from transmogrifai_amd.models.base import FitJob, learner_class
    g = torch.Generator().manual_seed(0)
    X = torch.where(torch.rand(12000, 400, generator=g) < 0.03, torch.rand(12000, 400, generator=g) * 3,
                    torch.zeros(12000, 400))
    X[:, :5] = torch.randn(12000, 5, generator=g)
    y = torch.multinomial(torch.softmax(X[:, :3], 1), 1, generator=g).reshape(-1).float().cuda()
    X = X.cuda()
    made, init = [], ML.MultinomialObjective.__init__
    monkeypatch.setattr(ML.MultinomialObjective, "__init__", lambda self, *a, **k: (init(self, *a, **k), made.append(self))[0])
    lr = learner_class("OpLogisticRegression")()
    jobs = [FitJob(dict(lr.defaults, reg_param=0.01, max_iter=60), r)
            for r in (torch.arange(0, 8000, device="cuda"), torch.arange(4000, 12000, device="cuda"))]
    monkeypatch.setenv("TMOG_MNL_SPARSE_FUSED", "1")
    a = lr.fit_batch(X, y, jobs)
    monkeypatch.setenv("TMOG_MNL_SPARSE_FUSED", "0")
    b = lr.fit_batch(X, y, jobs)
    assert [o.sparse for o in made] == [True, False] and all(isinstance(o.X, LK.SparseDesign) for o in made)
    for s1, s2 in zip(a, b):
        np.testing.assert_allclose(s1["coefficient_matrix"], s2["coefficient_matrix"], atol=2e-3)

"""The sparse LDA E-step and topic-statistics kernels (``ops/csrc/hip/lda_kernels.hip``) against a per-document
numpy fp64 oracle that uses no project code (digamma from ``torch.digamma`` on CPU fp64 tensors).

Tolerance. The oracle and the dense ``lda_e_step`` are two fp64 evaluations of the same arithmetic that differ
only in summation order. Over the cases below, on the CPU, the largest elementwise relative difference between
them in what ``lda_e_step`` returns (``theta``, ``sstats``) is 4.8e-12: ``sstats`` of the capacity corpus at
K = 17 run to convergence (up to 100 iterations carry a difference forward). The fixed three-iteration cases stay
below 3.6e-14, ``theta`` of the convergence cases below 4.3e-13, the stage-level fit below 8.4e-13. The kernels add
their own ``digamma`` and ``exp`` to the reordering and are allowed 64x the largest: ``REL = 3.1e-10``.

``n_iter`` must equal the oracle's for every document whose convergence measure never comes within a relative
1e-9 of ``tol`` in the oracle; the others are left out of the comparison and may be at most 1 % of a corpus.
``sstats`` sums over every document, so it is compared only where no document is left out.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 300
REL = 64 * 4.8e-12
CYCLE = (65, 130, 0, 1, 5, 63, 64)          # empty document, single term, the wave boundary


def corpus(lengths, n_cols=V, seed=0):              # dense fp32 counts 1..5, lengths[i] distinct terms in row i
    rng = np.random.default_rng(seed)
    X = np.zeros((len(lengths), n_cols), np.float32)
    for i, n in enumerate(lengths):
        X[i, rng.choice(n_cols, n, replace=False)] = rng.integers(1, 6, n)
    return X


def tables(K, n_cols=V, seed=0):
    lam = torch.from_numpy(np.random.default_rng(100 + seed).gamma(100.0, 0.01, (K, n_cols)))
    return torch.digamma(lam) - torch.digamma(lam.sum(1, keepdim=True)), np.full(K, 1.0 / K)


def oracle(X, Elogbeta, alpha, iters, tol):
    """``gamma, n_iter, expEt, r (CSR order), sstats, near`` document by document."""
    expEb = np.exp(Elogbeta.numpy())
    K = expEb.shape[0]

    def exp_elog_theta(g):
        return np.exp((torch.digamma(torch.from_numpy(g)) - torch.digamma(torch.tensor(g.sum()))).numpy())

    gamma, n_iter, expEt, r, near = [], [], [], [], []
    sstats = np.zeros_like(expEb)
    for x in X.astype(np.float64):
        cols = np.nonzero(x)[0]
        cnt, B = x[cols], expEb[:, cols]
        g, n, at_tol = 1.0 + cnt.sum() / K + np.zeros(K), 0, False
        for _ in range(iters):
            e = exp_elog_theta(g)
            new = alpha + e * (B @ (cnt / (e @ B + 1e-100)))
            change = np.abs(new - g).mean()
            at_tol |= abs(change - tol) <= 1e-9 * tol
            g, n = new, n + 1
            if change < tol:
                break
        e = exp_elog_theta(g)
        rd = cnt / (e @ B + 1e-100)
        sstats[:, cols] += np.outer(e, rd) * B
        gamma.append(g), n_iter.append(n), expEt.append(e), r.append(rd), near.append(at_tol)
    return np.array(gamma), np.array(n_iter), np.array(expEt), np.concatenate(r), sstats, np.array(near)


def close(got, want):
    return bool((np.abs(got.cpu().numpy() - want) <= REL * np.abs(want)).all())


# (document lengths or "cap", K, N, iters); tol = 0: every document runs exactly iters iterations
FIXED = [(CYCLE, K, 257, 3) for K in (1, 2, 3, 10, 16, 17, 64)] + \
        [(CYCLE, 10, N, 3) for N in (1, 5)] + [(CYCLE, 10, 257, it) for it in (1, 20)] + \
        [("cap", K, 6, 3) for K in (10, 17, 64)]


def run_case(lengths, K, N, iters, tol, seed=0):
    from transmogrifai_amd.ops import lda as L
    if lengths == "cap":                            # the LDS boundary and a multi-chunk spill
        cap = L.lds_terms(K)
        assert 0 < cap and 2 * cap + 3 <= V
        lengths = (cap - 1, cap, cap + 1, 2 * cap + 3, 0, cap + 1)
    X = corpus([lengths[i % len(lengths)] for i in range(N)], seed=seed)
    Elogbeta, alpha = tables(K, seed=seed)
    want = oracle(X, Elogbeta, alpha, iters, tol)
    csr = L.DocTermCSR(torch.from_numpy(X).cuda())
    expEbT = torch.exp(Elogbeta).t().contiguous().cuda()
    gamma, n_iter, expEt, r = L.doc_fixed_point(csr, expEbT, torch.from_numpy(alpha).cuda(), iters, tol)
    sstats = L.topic_stats(csr, expEt, r, expEbT)
    torch.cuda.synchronize()
    return (gamma, n_iter, expEt, r, sstats), want


@pytest.mark.parametrize("lengths,K,N,iters", FIXED, ids=lambda v: "cycle" if v is CYCLE else str(v))
def test_fixed_iterations(lengths, K, N, iters):
    (gamma, n_iter, expEt, r, sstats), (w_gamma, w_n, w_expEt, w_r, w_sstats, _) = run_case(lengths, K, N, iters, 0.0)
    assert (n_iter.cpu().numpy() == iters).all() and (w_n == iters).all()
    assert close(gamma, w_gamma) and close(expEt, w_expEt) and close(r, w_r) and close(sstats, w_sstats)


@pytest.mark.parametrize("lengths,K,seed", [(CYCLE, 10, 0), (CYCLE, 10, 1), (CYCLE, 3, 2), ("cap", 17, 0)],
                         ids=lambda v: "cycle" if v is CYCLE else str(v))
def test_per_document_convergence(lengths, K, seed):
    N = 257 if lengths is CYCLE else 6
    (gamma, n_iter, _, _, sstats), (w_gamma, w_n, _, _, w_sstats, near) = run_case(lengths, K, N, 100, 1e-3, seed)
    keep = ~near
    assert near.mean() <= 0.01 and w_n.min() < 10 and w_n.max() == 100
    assert (n_iter.cpu().numpy()[keep] == w_n[keep]).all()
    assert close(gamma[torch.from_numpy(keep).cuda()], w_gamma[keep]) and (near.any() or close(sstats, w_sstats))


def test_topic_statistics_over_segments():
    """An empty column, a column with one document, and a column of 4100 documents (two CSC segments)."""
    from transmogrifai_amd.ops import lda as L
    N, K = 4100, 10
    X = np.zeros((N, V), np.float32)
    X[:, 2] = np.random.default_rng(5).integers(1, 6, N)
    X[7, 1] = 3
    X[np.arange(0, N, 41), 3 + np.arange(0, N, 41) % 90] = 2
    Elogbeta, alpha = tables(K)
    _, _, w_expEt, w_r, w_sstats, _ = oracle(X, Elogbeta, alpha, 3, 0.0)
    csr = L.DocTermCSR(torch.from_numpy(X).cuda())
    assert csr.n_seg == int((X != 0).any(0).sum()) + 1
    expEbT = torch.exp(Elogbeta).t().contiguous().cuda()
    _, _, expEt, r = L.doc_fixed_point(csr, expEbT, torch.from_numpy(alpha).cuda(), 3, 0.0)
    sstats = L.topic_stats(csr, expEt, r, expEbT)
    assert close(expEt, w_expEt) and close(r, w_r) and close(sstats, w_sstats)
    assert (sstats[:, 0] == 0).all() and (sstats[:, 1] > 0).all()


def oracle_fit(X, lam, K, em_steps=5):
    """The stage's fit and transform with the oracle as its E-step: ``topics, theta, near``."""
    a, near = np.full(K, 1.0 / K), np.zeros(len(X), bool)
    for _ in range(em_steps):
        *_, sstats, at_tol = oracle(X, torch.digamma(lam) - torch.digamma(lam.sum(1, keepdim=True)), a, 50, 1e-3)
        lam, near = 1.0 / K + torch.from_numpy(sstats), near | at_tol
    topics = (lam / lam.sum(1, keepdim=True)).numpy()
    gamma, *_, at_tol = oracle(X, torch.log(torch.from_numpy(topics).clamp_min(1e-100)), a, 100, 1e-3)
    return topics, gamma / gamma.sum(1, keepdims=True), near | at_tol


def test_stage_fit_and_transform(monkeypatch):
    """``OpLDA(k=3, max_iter=5)`` through the sparse path against the oracle's full fit; with the variable unset
    the same corpus takes the dense path and gives bitwise the dense model."""
    from transmogrifai_amd.data.columns import VectorColumn
    from transmogrifai_amd.data.dataset import Dataset
    from transmogrifai_amd.features import types as T
    from transmogrifai_amd.stages.feature import nlp_stages as S
    from transmogrifai_amd.testkit.feature_builder import TestFeatureBuilder
    N, W, K = 300, 64, 3
    X = corpus([3 + i % 20 for i in range(N)], n_cols=W, seed=4)
    ds, (v,) = TestFeatureBuilder.of(("v", T.OPVector, [list(map(float, row)) for row in X]))
    dev_ds = Dataset({v.name: VectorColumn(torch.from_numpy(X).cuda(), ds[v.name].metadata)})

    def fit_transform():
        model = S.OpLDA(k=K, max_iter=5, seed=0).set_input(v).fit(dev_ds)
        return model, model.transform(dev_ds)[model.get_output().name].values, model._infer(dev_ds[v.name].values)

    dense_model = fit_transform()[0]
    monkeypatch.setenv("TMOG_LDA_SPARSE", "1")
    model, out, theta = fit_transform()
    assert torch.equal(out, theta.to(out.dtype))
    Xd = torch.from_numpy(X).cuda().to(torch.float64)
    alpha = torch.full((K,), 1.0 / K, dtype=torch.float64, device="cuda")
    lam0 = torch.rand(K, W, generator=torch.Generator(device="cpu").manual_seed(0), dtype=torch.float64) * 0.5 + 0.75
    lam = lam0.cuda()
    for _ in range(5):
        lam = 1.0 / K + S.lda_e_step(Xd, torch.digamma(lam) - torch.digamma(lam.sum(1, keepdim=True)), alpha, 50)[1]
    assert np.array_equal(dense_model.topics, (lam / lam.sum(1, keepdim=True)).cpu().numpy())
    topics, want, near = oracle_fit(X, lam0, K)
    assert near.mean() <= 0.01
    assert close(torch.from_numpy(model.topics), topics) and close(theta[torch.from_numpy(~near).cuda()], want[~near])

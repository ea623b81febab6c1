"""Multiclass XGBoost on the device: the two round-epilogue kernels (ops/csrc/hip/boost_multi_kernels.hip) against
torch fp64, and whole fits on the fused path against the torch path."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARRAYS = ("tree_off", "nodes", "default_left", "value", "gain", "cover")


def _native_loaded():
    from transmogrifai_amd.ops import _native
    return _native.hip_loaded()


@pytest.mark.parametrize("K", [3, 7])
def test_epilogue_kernels_match_torch_fp64(K):
    from transmogrifai_amd.ops import _native as NV
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(10 + K)
    N, P = 1000, 2
    Q = P * K
    rows = [torch.arange(0, N, 2), torch.arange(1, N, 3)]
    F = torch.rand(Q, N, generator=g, dtype=torch.float64) * 6.0 - 3.0
    for p in range(P):
        for r in range(20):                      # one class far ahead: saturated softmax, hessian floor
            F[p * K + r % K, r] = 40.0
        F[p * K:(p + 1) * K, 20:40] = -40.0      # all classes equal: the uniform case
    y = torch.randint(0, K, (N,), generator=g)

    # ---- boost_margin_add: one tree per pseudo-job, 4 leaves (and one unused root id) per tree
    ent, gid = [], []
    for q in range(Q):
        r = rows[q // K]
        ent.append(r | (1 << 24))                                    # packed entry: row | weight << 24
        gid.append(q * 5 + 1 + torch.randint(0, 4, (r.numel(),), generator=g))
    ent, gid = torch.cat(ent).to(torch.int32), torch.cat(gid).to(torch.int32)
    n_gid = Q * 5
    val = torch.randn(n_gid, generator=g, dtype=torch.float32)
    gid_tree = torch.arange(n_gid) // 5
    # tree t belongs to pseudo-job tree_job[t]; its rows are its model's, so permute inside each model only
    tree_job = torch.cat([p * K + torch.randperm(K, generator=g) for p in range(P)])
    F_ref = F.clone()
    q_of = tree_job[gid_tree[gid.long()]]
    F_ref.view(-1)[q_of * N + (ent.long() & 0xFFFFFF)] += val[gid.long()].double()
    Fd = F.to(dev)
    d = [t.to(dev) for t in (ent, gid, val, gid_tree, tree_job)]
    NV.check(NV.hip().tmog_hip_boost_margin_add(NV.ptr(d[0]), NV.ptr(d[1]), int(ent.numel()), NV.ptr(d[2]),
                                                NV.ptr(d[3]), NV.ptr(d[4]), N, NV.ptr(Fd), n_gid, Q, Q, 0,
                                                NV.stream(dev)), "boost_margin_add")
    assert torch.equal(Fd.cpu(), F_ref)          # an fp64 add of an exactly converted fp32

    # ---- softmax_grad on the constructed margins (saturated / uniform rows intact)
    Fd = F.to(dev)
    cat = torch.cat(rows).to(dev)
    off = torch.tensor([0, rows[0].numel(), rows[0].numel() + rows[1].numel()], device=dev)
    models = torch.arange(P, device=dev)
    G = torch.full((Q, N), 7.0, dtype=torch.float32, device=dev)
    H = torch.full((Q, N), 7.0, dtype=torch.float32, device=dev)
    tam = torch.zeros(64, Q, 2, dtype=torch.int32, device=dev)
    err = torch.zeros(P, dtype=torch.int32, device=dev)
    yf = y.to(torch.float32).to(dev)
    NV.check(NV.hip().tmog_hip_softmax_grad(NV.ptr(cat), NV.ptr(off), NV.ptr(models), P,
                                            max(int(r.numel()) for r in rows), K, N, P, NV.ptr(Fd), NV.ptr(yf),
                                            NV.ptr(G), NV.ptr(H), NV.ptr(tam), NV.ptr(err), NV.stream(dev)),
             "softmax_grad")
    G, H, tam, err = G.cpu(), H.cpu(), tam.cpu(), err.cpu()
    amax = tam.view(torch.float32).amax(0)
    ulp = 2.0 ** -23
    cls = torch.arange(K)[:, None]
    for p in range(P):
        r = rows[p]
        m = F[p * K:(p + 1) * K][:, r]
        pr = torch.softmax(m, 0)
        g_ref = (pr - (y[r][None, :] == cls).double()).float()
        h_ref = (2.0 * pr * (1.0 - pr)).clamp_min(1e-16).float()
        Gp, Hp = G[p * K:(p + 1) * K][:, r], H[p * K:(p + 1) * K][:, r]
        for got, ref in ((Gp, g_ref), (Hp, h_ref)):
            dif = (got.double() - ref.double()).abs()
            assert bool((dif <= 2 * ulp * ref.double().abs() + 1e-12).all()), float(dif.max())
        assert torch.equal(amax[p * K:(p + 1) * K, 0], Gp.abs().amax(1))
        assert torch.equal(amax[p * K:(p + 1) * K, 1], Hp.amax(1))
        assert int(err[p]) == int((m.argmax(0) != y[r]).sum())
        out = torch.ones(N, dtype=torch.bool)
        out[r] = False
        assert bool((G[p * K:(p + 1) * K][:, out] == 7.0).all()) and bool((H[p * K:(p + 1) * K][:, out] == 7.0).all())
    assert bool((H == np.float32(1e-16)).any())                      # the saturated rows sit on the hessian floor
    assert _native_loaded()


@functools.lru_cache(maxsize=None)
def _data():
    g = torch.Generator().manual_seed(5)
    n, d = 6000, 8
    X = torch.randn(n, d, generator=g)
    X[:, :2] = (X[:, :2] > 0.8).float()               # two 0/1 columns exercise the missing bin
    s = X[:, 3] + X[:, 0] - 0.5 * X[:, 5] + 0.3 * torch.randn(n, generator=g)
    y = ((s > -0.4).long() + (s > 0.6).long()).float()
    return X.cuda(), y.cuda()


def _jobs(three=False):
    from transmogrifai_amd.models.base import FitJob
    from transmogrifai_amd.models.trees import XGBoostClassifierLearner
    params = dict(XGBoostClassifierLearner.defaults, objective="multi:softprob", num_round=8, max_depth=3, eta=0.3,
                  missing=0.0, num_early_stopping_rounds=3)
    n = 6000
    jobs = [FitJob(params, torch.arange(0, n, 2, device="cuda")),
            FitJob(dict(params, max_depth=5), torch.arange(1, n, 3, device="cuda"))]
    if three:
        jobs.append(FitJob(dict(params, eta=0.1), torch.arange(0, n, 2, device="cuda")))
    return jobs


def _fit(three=False):
    from transmogrifai_amd.models.trees import XGBoostClassifierLearner
    X, y = _data()
    return XGBoostClassifierLearner().fit_batch(X, y, _jobs(three))


def _same_states(a, b):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        assert sa["num_trees"] == sb["num_trees"]
        for k in ARRAYS:
            np.testing.assert_array_equal(np.asarray(sa["forest"][k]), np.asarray(sb["forest"][k]), err_msg=k)


def test_fused_fit_matches_torch_path(monkeypatch):
    from transmogrifai_amd.models.trees import XGBoostClassifierLearner
    X, _ = _data()
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("TMOG_XGB_FUSED", flag)
        sts = _fit()
        assert all(s["n_classes"] == 3 and s["num_trees"] % 3 == 0 and s["num_trees"] > 0 for s in sts)
        outs.append((sts, [XGBoostClassifierLearner().predict(s, X)[2].cpu() for s in sts]))
    for sa, sb in zip(outs[0][0], outs[1][0]):
        assert sa["num_trees"] == sb["num_trees"]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert a.shape == (6000, 3)
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    assert _native_loaded()


def test_kernel_maxima_give_the_scanned_scales(monkeypatch):
    """Trees grown with the softmax kernel's maxima as ``quant_amax`` equal the trees grown with the grower's
    per-round scan of (g, h) (``TMOG_XGB_AMAX=0``) bit for bit."""
    monkeypatch.setenv("TMOG_XGB_AMAX", "1")
    a = _fit()
    monkeypatch.setenv("TMOG_XGB_AMAX", "0")
    b = _fit()
    _same_states(a, b)
    assert any(len(np.asarray(s["forest"]["nodes"])) > 3 * s["num_trees"] for s in a)      # trees not trivial


def test_pipelined_parts_keep_a_models_classes_together(monkeypatch):
    monkeypatch.setenv("TMOG_XGB_PIPE", "1")
    a = _fit(three=True)
    monkeypatch.setenv("TMOG_XGB_PIPE", "2")
    b = _fit(three=True)
    _same_states(a, b)

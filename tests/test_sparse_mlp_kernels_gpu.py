"""``sparse_mlp_kernel`` (``ops/csrc/hip/sparse_mlp_kernels.hip``, ``ops/linear.py`` ``sparse_mlp_pass``) against a plain numpy
fp64 network on the designs of tests/multiclass_oracle.py. The tolerance is not a constant: every case also runs the
unfused device pass (``MLPObjective`` on the densified fp32 matrix) and requires, per quantity and element,
``err_fused <= 4 max(err_unfused, 16 * 2^-24 * scale)``: ``scale`` the fp64 sum of the absolute terms of the element (the
same products with every factor replaced by its absolute value), ``err_unfused`` the largest error of the unfused pass
over the quantity. The factor 4 covers another summation order and the fast ``exp`` / reciprocal; the floor keeps a
lucky exact unfused result from failing the new path. The unfused ``dZ1`` is what ``_sigmoid_backprop_`` leaves at
the first layer. Largest observed ratios err_fused / bound: profiles/sparse_mlp.txt."""
import functools

import numpy as np
import pytest
import torch

import multiclass_oracle as O
from transmogrifai_amd.models import mlp as M
from transmogrifai_amd.ops import linear as LK

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = F32(-1.5e30)
DESIGNS = ("segs70", "n1", "no_dense", "no_sparse", "nd128", "nd129")
TAILS = ((1, 2), (16, 3), (17, 16), (64, 64, 6), (33, 5, 16))      # every chunk width, padding in both MFMA dimensions


@functools.lru_cache(maxsize=None)
def _design(name, integer=False):
    if name.startswith("nd"):           # N = 67 rows, a dense block on each side of the kernel's 128 columns
        nd = int(name[2:])
        X = np.zeros((67, nd + 6), F32)
        X[:, :nd] = O._fill(np.random.default_rng(nd), (67, nd), True)
        X[9 * np.arange(6), nd + np.arange(6)] = 2.0
    else:
        X = O.design(name, integer)
    return X, LK.SparseDesign(torch.from_numpy(X).cuda())


def _network(X, y, W, params):
    """fp64 forward, softmax cross-entropy and backward of every problem: per problem ``(values, scales)`` in the
    order f, (dW, db) from the last layer to the first, dZ1."""
    X, out = X.astype(F64), []
    for p in range(W.shape[1]):
        w = W[:, p].astype(F64)
        ws = w.sum()
        acts = [X]
        for Wl, bl in params[:-1]:
            acts.append(O.sigmoid(acts[-1] @ Wl[p].astype(F64) + bl[p]))
        z = acts[-1] @ params[-1][0][p].astype(F64) + params[-1][1][p]
        loss, R, _ = O.softmax_loss_residual(z[:, None, :], y, w[:, None])
        dZ = R[:, 0] / ws
        dA = np.abs(dZ)
        val, sc = [loss.sum() / ws], [np.abs(loss).sum() / ws]
        for l in range(len(params) - 1, -1, -1):
            val += [acts[l].T @ dZ, dZ.sum(0)]
            sc += [np.abs(acts[l]).T @ dA, dA.sum(0)]
            if l:
                d, Wl = acts[l] * (1 - acts[l]), params[l][0][p].astype(F64)
                dZ, dA = (dZ @ Wl.T) * d, (dA @ np.abs(Wl).T) * d
        out.append((val + [dZ], sc + [dA]))
    return out


def _blocks(f, grads, dZ1, p, h1):
    """One problem's results in ``_network`` order (``grads`` first layer first)."""
    out = [f[p]]
    for dW, db in reversed(grads):
        out += [dW[p], db[p]]
    return [np.asarray(v, F64) for v in out + [dZ1[:, p * h1:(p + 1) * h1]]]


def _fused(D, y, W, params, grad):
    # dZ1 inside a sentinel border with a spare column: only [N, P * h1] may be written, and nothing without grad
    N, (P, _, h1) = D.shape[0], params[0][0].shape
    big = torch.full((N + 2, P * h1 + 3), float(SENT), dtype=torch.float32, device="cuda")
    t = [tuple(torch.from_numpy(a).cuda() for a in l) for l in params]
    Wt = torch.from_numpy(W).cuda()
    f, tail, db1, dW1, _ = LK.sparse_mlp_pass(D, torch.from_numpy(y).cuda(), Wt, t, Wt.sum(0, dtype=torch.float64), grad,
                                              dZ1=big[1:N + 1, 1:P * h1 + 1])
    got = big.cpu().numpy()
    inner = got[1:N + 1, 1:P * h1 + 1].copy()
    got[1:N + 1, 1:P * h1 + 1] = SENT
    assert (got == SENT).all(), "written outside dZ1 [N, P * h1]"
    if not grad:
        assert (inner == SENT).all() and tail is None
        return [f.cpu().numpy()]
    assert (inner != SENT).all() and (inner.reshape(N, P, h1)[W == 0] == 0).all()
    grads = [(dW1.cpu().numpy(), db1.cpu().numpy())] + [(a.cpu().numpy(), b.cpu().numpy()) for a, b in tail]
    return [f.cpu().numpy(), grads, inner]


def _unfused(X, y, W, params, layers, monkeypatch):
    """The dense device pass on the same case; its dZ1 ``[P, N, h1]`` is the array ``_sigmoid_backprop_`` last leaves."""
    kept, inner = [], M._sigmoid_backprop_
    monkeypatch.setattr(M, "_sigmoid_backprop_", lambda Dh, A: (inner(Dh, A), kept.append(Dh))[0])
    P = W.shape[1]
    U = torch.from_numpy(np.concatenate([np.concatenate([Wl.reshape(P, -1).T, bl.T]) for Wl, bl in params])).double()
    ob = M.MLPObjective(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(W).cuda(), layers)
    f, g = ob.value_grad(U.cuda())
    g = g.cpu().numpy()
    grads = [(g[o:o + a * b].T.reshape(P, a, b), g[ob_:ob_ + b].T) for o, a, b, ob_ in ob.slices]
    return f.cpu().numpy(), grads, np.concatenate(list(kept[-1].cpu().numpy()), 1)


def _check(X, D, tail, params, y, W, grad, monkeypatch):
    layers, h1 = (X.shape[1],) + tuple(tail), tail[0]
    ref = _network(X, y, W, params)
    fu = _unfused(X, y, W, params, layers, monkeypatch)
    ff = _fused(D, y, W, params, grad)
    worst = 0.0
    for p, (val, sc) in enumerate(ref):
        got = _blocks(*ff, p, h1) if grad else [ff[0][p]]
        for v, s, a, b in zip(val, sc, got, _blocks(*fu, p, h1)):
            bound = 4 * np.maximum(np.abs(b - v).max(), 16 * O.U * s)
            assert np.isfinite(a).all()
            worst = max(worst, float((np.abs(a - v) / np.maximum(bound, 1e-300)).max()))
    print(f"err_fused / bound = {worst:.3f}")
    assert worst <= 1.0
    return ff


def _case(X, tail, P):
    (N, d), rng = X.shape, np.random.default_rng(X.shape[0] * 31 + sum(tail) + P)
    layers = (d,) + tuple(tail)
    params = [((rng.standard_normal((P, a, b)) * 2 / np.sqrt(min(a, 40))).astype(F32),
               rng.standard_normal((P, b)).astype(F32)) for a, b in zip(layers[:-1], layers[1:])]
    W = O._weights(rng, (N, P))
    W[(np.arange(N)[:, None] + np.arange(P)) % 3 == 1] = 0          # rows outside the fold
    if N == 1:
        W[:] = 1.5
    return params, O._labels(rng, N, tail[-1]), W


@pytest.mark.parametrize("grad", (True, False), ids=("grad1", "grad0"))
@pytest.mark.parametrize("P", (1, 3))
@pytest.mark.parametrize("tail", TAILS, ids=["-".join(map(str, t)) for t in TAILS])
@pytest.mark.parametrize("name", DESIGNS)
def test_pass_matches_fp64(name, tail, P, grad, monkeypatch):
    from transmogrifai_amd.ops import _native
    assert _native.hip().tmog_hip_sparse_mlp_nd_max() == 128         # nd128 / nd129 stand on each side of it
    X, D = _design(name)
    if name == "nd129":
        assert not LK.sparse_mlp_supported(D, (X.shape[1],) + tail)
        return
    assert LK.sparse_mlp_supported(D, (X.shape[1],) + tail)
    _check(X, D, tail, *_case(X, tail, P), grad, monkeypatch)


def test_saturated_units_and_logits(monkeypatch):
    X, D = _design("segs70", True)
    d, tail, P, rng = X.shape[1], (16, 3), 2, np.random.default_rng(7)
    # integer first-layer weights, every third row times 40: pre-activations 0, +-1 and far beyond +-88; logits 40 apart
    params = [((rng.integers(-1, 2, (P, d, 16)) * np.where(np.arange(d) % 3 == 0, 40, 1)[None, :, None]).astype(F32),
               rng.integers(-2, 3, (P, 16)).astype(F32)),
              ((rng.integers(-1, 2, (P, 16, 3)) * 40).astype(F32), rng.integers(-2, 3, (P, 3)).astype(F32))]
    y, W = O._labels(rng, len(X), 3), O._weights(rng, (len(X), P))
    assert ((y < 0) | (y >= 3)).any()                                # loss 0, no one-hot term: _network's rule
    dZ1 = _check(X, D, tail, params, y, W, True, monkeypatch)[2]
    for p in range(P):
        z1 = X.astype(F64) @ params[0][0][p].astype(F64) + params[0][1][p]
        a32 = O.sigmoid_f32(z1.astype(F32))
        flat = (a32 == 0) | (a32 == 1)
        assert (np.abs(z1) > 88).any() and flat.any() and (dZ1[:, p * 16:(p + 1) * 16][flat] == 0).all()


@pytest.mark.parametrize("tail", ((32, 6), (64, 16, 6)))
def test_two_calls_are_bitwise_equal(tail):
    X, D = _design("segs70")
    params, y, W = _case(X, tail, 3)
    a, b = (_fused(D, y, W, params, True) for _ in range(2))
    flat = lambda r: [r[0], r[2]] + [t for pair in r[1] for t in pair]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat(a), flat(b)))


def test_fit_batch_takes_the_fused_pass(monkeypatch):
    from transmogrifai_amd.models.base import FitJob, learner_class
    g = torch.Generator().manual_seed(11)
    N, d, layers = 4096, 256, [256, 16, 3]
    cols = torch.randint(0, d, (N, 8), generator=g)
    X = torch.zeros(N, d).scatter_(1, cols, torch.rand(N, 8, generator=g) + 0.5)
    y = (X[:, :90].sum(1) < X[:, 90:170].sum(1)).long() + (X[:, 170:].sum(1) > X[:, :170].sum(1) / 2).long()
    lr = learner_class("OpMultilayerPerceptronClassifier")()
    folds = (torch.arange(0, 3000), torch.arange(1000, N))
    jobs = [FitJob(dict(lr.defaults, layers=layers, max_iter=30, seed=3), r.cuda()) for r in folds]
    calls, inner = [], LK.sparse_mlp_pass
    monkeypatch.setattr(LK, "sparse_mlp_pass", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])

    def losses(states):
        out = []
        for s, r in zip(states, folds):
            w = [np.asarray(t)[None] for t in s["weights"]]
            Wr = np.zeros((N, 1), F32)
            Wr[r.numpy()] = 1
            out.append(_network(X.numpy(), y.numpy().astype(F32), Wr, list(zip(w[::2], w[1::2])))[0][0][0])
        return np.array(out)

    fits = {}
    for key, env in (("off", {"TMOG_MLP_SPARSE_FUSED": "0"}), ("mfma", {"TMOG_MLP_SPARSE_FUSED": "0", "TMOG_DENSE_MFMA": "1"}),
                     ("fused", {"TMOG_MLP_SPARSE_FUSED": "1", "TMOG_DENSE_MFMA": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fits[key] = losses(lr.fit_batch(X.cuda(), y.double().cuda(), jobs))
        assert bool(calls) == (key == "fused")
    init = losses([{"weights": [p.reshape(s) for p, s in zip(
        np.split(M._init_params(layers, 3), [4096, 4112, 4160]), ((256, 16), (16,), (16, 3), (3,)))]}] * 2)
    spread = np.abs(fits["off"] - fits["mfma"])
    print("fused", fits["fused"], "unfused", fits["off"], "mfma", fits["mfma"], "initial", init)
    assert (fits["fused"] < init).all()
    assert (np.abs(fits["fused"] - fits["off"]) <= 4 * spread).all()

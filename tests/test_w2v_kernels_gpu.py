"""The window-batched skip-gram kernels (``ops/csrc/hip/w2v_kernels.hip``) against a numpy fp64 oracle that uses no
project code: a direct loop over windows, slots and columns.

Tolerance. An entry may differ from the oracle by ``C * n * 2**-24 *`` (the oracle's sum of the absolute values of
the terms that entered it), ``n`` the longest accumulation chain behind it: ``Dp + 16`` for a slab entry, plus the
number of slab rows keyed to the table row for a table entry (summed over the steps of a chain of steps). ``C`` is
8x the largest such ratio that an fp32 numpy evaluation of the same oracle shows against the fp64 one on the CPU
over ``CASES`` and the three chained steps: 0.669 (``gout`` of the saturated case; 0.156 without it), so
``C = 5.352``. The largest ratios are the saturated case's, where the rounding of a logit near 30 is multiplied
by the logit's sensitivity; the kernel forms ``1 - sigmoid`` without cancellation, as the oracle does, and gets no
further allowance for its ``expf``.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 8 * 0.669
#        w   S  dim    B    V  peak |logit| (0: as drawn)
CASES = [(1, 1, 4, 1, 1, 0), (5, 5, 20, 5, 7, 0), (8, 15, 100, 257, 7, 0), (5, 15, 256, 5, 300, 0),
         (8, 5, 256, 257, 300, 0), (1, 5, 100, 257, 300, 0), (5, 5, 20, 257, 7, 30)]


def inputs(w, S, dim, B, V, peak, seed=0):
    """Documents of 0, 1, 2, 2w, 2w + 1 and 40 tokens; positions at the single-token document (an all-invalid
    window) and at document ends first; negatives that include the centre word and repeat themselves."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum([0, 1, 2, 2 * w, 2 * w + 1, 40])])
    T, Dp = int(ptr[-1]), (dim + 15) // 16 * 16
    tok = rng.integers(0, V, T).astype(np.int32)
    pos = np.concatenate([[0, ptr[5], T - 1, ptr[3], ptr[5] - 1, 1, 2], rng.integers(0, T, B)])[:B].astype(np.int32)
    neg = rng.integers(0, V, (B, S)).astype(np.int32)
    neg[::2, 0] = tok[pos[::2]]
    neg[:, S - 1] = neg[:, 0]
    ein, eout = np.zeros((V, Dp), np.float32), np.zeros((V, Dp), np.float32)
    ein[:, :dim] = rng.uniform(-0.5, 0.5, (V, dim))
    eout[:, :dim] = rng.normal(0, 0.5, (V, dim))
    if peak:
        eout *= np.float32(peak / np.abs(ein.astype(np.float64) @ eout.T.astype(np.float64)).max())
    return ein, eout, tok, ptr, pos, neg


def oracle(ein, eout, tok, ptr, pos, neg, w, lr, dt=np.float64, mag=None):
    """One step: slabs, keys, updated tables, then the absolute-term sums of the slabs and the tables and the
    chain lengths of the tables. ``mag``: the tables' absolute-term sums and chain lengths so far (a chain of steps)."""
    (V, Dp), (B, S) = ein.shape, neg.shape
    ein, eout = ein.astype(dt), eout.astype(dt)
    kin, kout = np.full((B, 16), V, np.int32), np.full((B, 16), V, np.int32)
    for b, t in enumerate(pos):
        d = np.searchsorted(ptr, t, side="right") - 1
        for i, o in enumerate(list(range(-w, 0)) + list(range(1, w + 1))):
            if ptr[d] <= t + o < ptr[d + 1]:
                kin[b, i] = tok[t + o]
        kout[b, 0], kout[b, 1:S + 1] = tok[t], neg[b]
    n_pos = int((kin < V).sum())
    a_pos = dt(lr) / dt(n_pos) if n_pos else dt(0)
    a_neg = a_pos / dt(S)
    g = [np.zeros((B, 16, Dp), dt), np.zeros((B, 16, Dp), dt)]
    ga = [np.zeros((B, 16, Dp)), np.zeros((B, 16, Dp))]
    for b in range(B):
        for i in np.nonzero(kin[b] < V)[0]:
            for j in range(S + 1):
                x, y = ein[kin[b, i]], eout[kout[b, j]]
                L = np.dot(x, y)
                e = a_pos / (1 + np.exp(L)) if j == 0 else -a_neg / (1 + np.exp(-L))
                g[0][b, i] += e * y
                g[1][b, j] += e * x
                ga[0][b, i] += np.abs(np.float64(e) * y)
                ga[1][b, j] += np.abs(np.float64(e) * x)
    new = [ein.copy(), eout.copy()]
    mag = mag or [np.abs(ein, dtype=np.float64), np.abs(eout, dtype=np.float64), np.zeros(V), np.zeros(V)]
    mag = [m.copy() for m in mag]
    for s, keys in enumerate((kin, kout)):
        for b, i in zip(*np.nonzero(keys < V)):
            new[s][keys[b, i]] += g[s][b, i]
            mag[s][keys[b, i]] += ga[s][b, i]
        mag[2 + s] += Dp + 16 + np.bincount(keys[keys < V], minlength=V)
    return g, (kin, kout), new, ga, mag, n_pos


def ratio(got, ref, mag, n):
    """The largest error in units of ``n * 2**-24 * mag``; an entry no term entered must be exactly zero."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(err[mag == 0] == 0)
    return float((err[mag > 0] / (n * 2.0**-24 * mag)[mag > 0]).max(initial=0.0))


def device_state(ein, eout, tok, ptr):
    from transmogrifai_amd.ops import word2vec as W2V
    return W2V, torch.from_numpy(ein).cuda(), torch.from_numpy(eout).cuda(), W2V.TokenCorpus(tok, ptr, "cuda")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_window_and_step(case):
    w, S, dim, B, V, peak = case
    ein, eout, tok, ptr, pos, neg = inputs(*case)
    g, keys, new, ga, mag, n_pos = oracle(ein, eout, tok, ptr, pos, neg, w, 1.0)
    W2V, din, dout, corpus = device_state(ein, eout, tok, ptr)
    tpos, tneg = torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda()
    if (B, V) == (257, 7):
        assert min(np.bincount(k[k < V], minlength=V).min() for k in keys) > W2V.seg_cap()
    out = W2V.window_grads(din, dout, corpus, tpos, tneg, w, torch.tensor([n_pos], dtype=torch.int32), 1.0)
    assert np.array_equal(out[2].cpu().numpy(), keys[0]) and np.array_equal(out[3].cpu().numpy(), keys[1])
    worst = [ratio(out[s].cpu().numpy(), g[s], ga[s], ein.shape[1] + 16) for s in (0, 1)]
    W2V.step(din, dout, corpus, tpos, tneg, w, 0.025)
    worst += [ratio(t.cpu().numpy(), new[s], mag[s], mag[2 + s][:, None]) for s, t in enumerate((din, dout))]
    print("error ratios (gin, gout, emb_in, emb_out):", worst)
    assert max(worst) <= C


def test_three_steps_keep_the_pad_zero():
    w, S, dim, B, V, _ = case = CASES[1]
    ein, eout, tok, ptr, _, _ = inputs(*case)
    W2V, din, dout, corpus = device_state(ein, eout, tok, ptr)
    new, mag = [ein, eout], None
    for seed in (1, 2, 3):
        _, _, _, _, pos, neg = inputs(*case, seed=seed)
        new, mag = oracle(new[0], new[1], tok, ptr, pos, neg, w, 1.0, mag=mag)[2::2]
        W2V.step(din, dout, corpus, torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), w, 0.025)
    for s, t in enumerate((din, dout)):
        assert bool((t[:, dim:] == 0).all())
        assert ratio(t.cpu().numpy(), new[s], mag[s], mag[2 + s][:, None]) <= C


def test_reproducible():
    case = CASES[2]
    ein, eout, tok, ptr, pos, neg = inputs(*case)
    runs = []
    for _ in range(2):
        W2V, din, dout, corpus = device_state(ein, eout, tok, ptr)
        W2V.step(din, dout, corpus, torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), case[0], 0.025)
        runs.append((din, dout))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("dim", [5, 16, 100])
def test_doc_mean(dim):
    from transmogrifai_amd.ops import word2vec as W2V
    rng = np.random.default_rng(dim)
    ptr = np.concatenate([[0], np.cumsum([0, 1, 63, 64, 65, 300])])
    tok, vec = rng.integers(0, 50, ptr[-1]), rng.normal(0, 1, (50, dim)).astype(np.float32)
    got = W2V.doc_mean(W2V.TokenCorpus(tok, ptr, "cuda"), torch.from_numpy(vec)).cpu().numpy()
    for d in range(6):
        rows = vec[tok[ptr[d]:ptr[d + 1]]].astype(np.float64)
        ref = rows.mean(0) if len(rows) else np.zeros(dim)
        # the fp64 sum's own rounding, then one rounding to the fp32 output
        assert np.all(np.abs(got[d] - ref) <= 2.0**-24 * np.abs(ref) + 300 * 2.0**-53 * np.abs(rows).sum(0).max(initial=0))


def two_clusters(device):
    from transmogrifai_amd.features import types as T
    from transmogrifai_amd.testkit.feature_builder import TestFeatureBuilder
    rng = np.random.default_rng(0)
    words = (["cat", "dog", "pet", "fur"], ["car", "road", "wheel", "engine"])
    docs = [list(rng.choice(words[int(rng.random() >= 0.5)], 6)) for _ in range(300)]
    return TestFeatureBuilder.of(("t", T.TextList, docs), ("x", T.Real, [0.0] * 300), device=device)


@pytest.mark.parametrize("device,kw", [("cpu", {}), ("cuda", {"window_size": 9})])
def test_windows_trainer_refuses(device, kw):
    from transmogrifai_amd.stages.feature import nlp_stages as N
    ds, (t, _) = two_clusters(device)
    with pytest.raises(ValueError, match="windows"):
        N.OpWord2Vec(vector_size=16, min_count=1, trainer="windows", **kw).set_input(t).fit(ds)


def test_windows_trainer_synonyms():
    """``max_iter``: the smallest of 20, 40, ... at which the oracle's arithmetic, trained in numpy fp64 on the CPU
    on this corpus with these parameters (one step of 1800 windows per epoch), meets the criterion below for all of
    the seeds 0..4: 20 (five of five; so did every later multiple up to 400)."""
    from transmogrifai_amd.stages.feature import nlp_stages as N
    ds, (t, _) = two_clusters("cuda")
    m = N.OpWord2Vec(vector_size=16, min_count=1, max_iter=20, trainer="windows", seed=1).set_input(t).fit(ds)
    syn = [w for w, _ in m.find_synonyms("cat", 3)]
    assert set(syn) <= {"dog", "pet", "fur", "car", "road", "wheel", "engine"}
    assert len(set(syn) & {"dog", "pet", "fur"}) >= 2

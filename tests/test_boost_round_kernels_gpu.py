"""The XGBoost boosting-round kernels (ops/csrc/hip/boost_kernels.hip: boost_epilogue_kernel and
boost_prologue_kernel) against fp64 / numpy oracles computed from the same hand-built inputs, and whole fits on
the squared-error path with the fused round on and off."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARRAYS = ("tree_off", "nodes", "default_left", "value", "gain", "cover")
ULP = 2.0 ** -23
SENT = 7.0                      # pre-fill of cells a launch must not touch
PATTERN = 0x12345678            # pre-fill of the inactive jobs' maxima words
COPIES = 64                     # boost_kernels.hip kAmaxCopies


def _native_loaded():
    from transmogrifai_amd.ops import _native
    return _native.hip_loaded()


# ------------------------------------------------------------------------------------------------ boost_epilogue

EPI_N, EPI_P = 1500, 5
EPI_ACT = (0, 2, 3, 4)                                  # job 1 is inactive
EPI_TREE_JOB = np.array([3, 0, 4, 2], np.int64)         # tree t belongs to job EPI_TREE_JOB[t]: not the identity
EPI_EDGES = (800.0, -800.0, 40.0, -40.0, 0.0)           # exp overflows / underflows, the hessian floor, p = 1/2


@functools.lru_cache(maxsize=None)
def _epi_case(layout, wide, objective, bins):
    """Hand-built inputs of one epilogue launch and their expected outputs (numpy, fp64). ``bins`` only shapes the
    binary:logistic margins (every score in the middle of a bin); read-only once built."""
    rng = np.random.default_rng(1000 + 10 * objective + (layout == "perm") + 100 * (bins % 97))
    N, P = EPI_N, EPI_P
    rows = {0: np.sort(rng.choice(N, 37, replace=False)), 2: np.sort(rng.choice(N, 5, replace=False)),
            3: np.arange(1, N, 3), 4: np.arange(N)}
    n_gid = 5 * len(EPI_TREE_JOB)                       # five leaf ids a tree, the first one (the root's) unused
    val = rng.standard_normal(n_gid).astype(np.float32)
    gid_tree = (np.arange(n_gid) // 5).astype(np.int64)
    tree_of = {int(p): t for t, p in enumerate(EPI_TREE_JOB)}
    if objective == 0:
        y = rng.integers(0, 2, N).astype(np.float32)
        y[rows[2]] = np.array([1, 0, 1, 0, 1], np.float32)          # the five-row job sees both labels
    else:
        y = (rng.standard_normal(N) * 10.0).astype(np.float32)
    y64 = y.astype(np.float64)

    job, row, gid, m = [], [], [], []
    for p in EPI_ACT:
        r = rows[p]
        n = r.size
        if objective == 0:
            k = rng.integers(0, bins - 1, n)                        # target bins 0 .. bins - 2
            if p == 4:      # half the rows share three bins (many lanes a slot), the rest spread (> 8 slots a wave)
                k[: n // 2] = rng.choice(rng.integers(0, bins - 1, 3), n // 2)
            q = (k + 0.5) / (bins - 1)
            mp = np.log(q / (1.0 - q))
            if p == 2:                                              # five rows: one edge each, labels 1 0 1 0 1
                mp[:] = EPI_EDGES
            else:                                                   # every edge with both labels
                used = set()
                for lab in (0.0, 1.0):
                    for edge in EPI_EDGES:
                        i = next(i for i in range(n) if y[r[i]] == lab and i not in used)
                        used.add(i)
                        mp[i] = edge
        else:
            mp = rng.standard_normal(n) * 10.0
            e = min(n, 6) // 3
            mp[:e] = y64[r[:e]] + 1e6                               # |F - y| around 1e6, both signs
            mp[e:2 * e] = y64[r[e:2 * e]] - 1e6
            mp[2 * e:3 * e] = y64[r[2 * e:3 * e]]                   # F == y exactly (see F0 below)
            if p == 2:
                mp[3:] = y64[r[3:]]
        job.append(np.full(n, p, np.int64))
        row.append(r.astype(np.int64))
        gid.append(tree_of[p] * 5 + 1 + rng.integers(0, 4, n))
        m.append(mp)
    job, row, gid, m = (np.concatenate(a) for a in (job, row, gid, m))
    if layout == "perm":                                            # every wave holds all four jobs
        o = rng.permutation(job.size)
        job, row, gid, m = job[o], row[o], gid[o], m[o]
    n_entries = job.size
    assert n_entries % 64 != 0
    if layout == "contig":
        assert set(job[:64].tolist()) == {0, 2, 3}                  # three jobs in the first wave
    w = rng.choice(np.array([1, 2, 255], np.int64), n_entries)
    ent = row if wide else row | (w << 24)                          # the weight byte must be masked off
    ent = ent.astype(np.uint32).view(np.int32)

    v64 = val.astype(np.float64)[gid]
    F0 = m - v64                    # y - val and its sum with val are exact in fp64 for two fp32 of this range
    F_init = np.full((P, N), SENT, np.float64)
    F_init[job, row] = F0
    F_ref = F_init.copy()
    F_ref[job, row] = F0 + v64                                      # an fp64 add of an exactly converted fp32
    Fe = F_ref[job, row]
    ye = y64[row]
    touched = np.zeros((P, N), bool)
    touched[job, row] = True
    G_ref = np.full((P, N), SENT, np.float32)
    H_ref = np.full((P, N), SENT, np.float32)
    counts = None
    if objective == 0:
        with np.errstate(over="ignore"):
            pr = 1.0 / (1.0 + np.exp(-Fe))
        G_ref[job, row] = (pr - ye).astype(np.float32)
        H_ref[job, row] = np.maximum(pr * (1.0 - pr), 1e-16).astype(np.float32)
        # metrics.binned_aupr_multi: b = int(float32 score clamped to [0, 1] * float32(bins - 1)), descending slots
        t = np.clip(pr.astype(np.float32), np.float32(0), np.float32(1)) * np.float32(bins - 1)
        assert t.dtype == np.float32
        b = t.astype(np.int64)
        t64 = t.astype(np.float64)
        # every score is at least 0.25 from an edge between two bins. Two ends are not such edges: below bin 0
        # there is none (the score is clamped at 0 and the conversion truncates), and a score of exactly 1.0 sits
        # on the last bin by construction -- it comes from margins >= 40, where 1 + exp(-m) rounds to 1 whatever
        # the last bits of exp are (exp(-40) is 26 times below 2^-53).
        mid = (np.abs(t64 - np.rint(t64)) >= 0.25) | (t64 <= 0.75) | ((pr == 1.0) & (Fe >= 39.0))
        assert bool(mid.all())
        lab = (ye > 0.5).astype(np.int64)
        slot = (job * 2 + lab) * bins + (bins - 1 - b)
        counts = np.bincount(slot, minlength=P * 2 * bins).reshape(P, 2, bins).astype(np.int32)
        for p in EPI_ACT:
            for c in (0, 1):
                assert counts[p, c].sum() == int(((job == p) & (lab == c)).sum())
    else:
        G_ref[job, row] = (Fe - ye).astype(np.float32)
        H_ref[job, row] = np.float32(1.0)
    return dict(N=N, P=P, rows=rows, n_gid=n_gid, n_entries=n_entries, wide=int(wide), objective=objective,
                ent=torch.from_numpy(ent.copy()), gid=torch.from_numpy(gid.astype(np.int32)),
                val=torch.from_numpy(val), gid_tree=torch.from_numpy(gid_tree),
                tree_job=torch.from_numpy(EPI_TREE_JOB.copy()), y=torch.from_numpy(y),
                F_init=torch.from_numpy(F_init), F_ref=torch.from_numpy(F_ref), G_ref=torch.from_numpy(G_ref),
                H_ref=torch.from_numpy(H_ref), touched=torch.from_numpy(touched),
                counts=None if counts is None else torch.from_numpy(counts))


def _run_epilogue(c, bins, with_amax=True, with_counts=True):
    """One launch on fresh buffers: (F, G, H, tam, counts) on the host."""
    from transmogrifai_amd.ops import _native as NV
    dev = torch.device("cuda")
    P, N = c["P"], c["N"]
    d = {k: c[k].to(dev) for k in ("ent", "gid", "val", "gid_tree", "tree_job", "y")}
    F = c["F_init"].to(dev)
    G = torch.full((P, N), SENT, dtype=torch.float32, device=dev)
    H = torch.full((P, N), SENT, dtype=torch.float32, device=dev)
    tam = torch.zeros(COPIES, P, 2, dtype=torch.int32, device=dev)
    tam[:, 1, :] = PATTERN
    counts = torch.zeros(P, 2, bins, dtype=torch.int32, device=dev) if (bins and with_counts) else None
    NV.check(NV.hip().tmog_hip_boost_epilogue(
        NV.ptr(d["ent"]), NV.ptr(d["gid"]), c["n_entries"], NV.ptr(d["val"]), NV.ptr(d["gid_tree"]),
        NV.ptr(d["tree_job"]), N, NV.ptr(F), NV.ptr(G), NV.ptr(H), NV.ptr(d["y"]), c["objective"], NV.ptr(counts),
        bins if counts is not None else 0, c["n_gid"], len(EPI_TREE_JOB), P, NV.stream(dev),
        NV.ptr(tam) if with_amax else None, c["wide"]), "boost_epilogue")
    torch.cuda.synchronize()
    return F.cpu(), G.cpu(), H.cpu(), tam.cpu(), None if counts is None else counts.cpu()


def _check_fgh(c, F, G, H):
    assert torch.equal(F, c["F_ref"])                               # touched cells exact, the others keep SENT
    tch = c["touched"]
    assert bool((G[~tch] == SENT).all()) and bool((H[~tch] == SENT).all())
    assert not bool(tch[1].any())
    if c["objective"] == 0:
        for got, ref in ((G, c["G_ref"]), (H, c["H_ref"])):
            dif = (got.double() - ref.double()).abs()[tch]
            assert bool((dif <= 2 * ULP * ref.double().abs()[tch] + 1e-12).all()), float(dif.max())
        assert bool((H[tch] == np.float32(1e-16)).any())            # saturated rows sit on the hessian floor
    else:
        assert torch.equal(G, c["G_ref"])                           # one fp64 subtraction, one rounding
        assert torch.equal(H, c["H_ref"])


def _check_maxima(c, G, H, tam):
    amax = tam.view(torch.float32).amax(0)
    for p in EPI_ACT:
        r = torch.from_numpy(c["rows"][p])
        assert torch.equal(amax[p], torch.stack([G[p, r].abs().max(), H[p, r].max()]))
    assert bool((tam[:, 1, :] == PATTERN).all())                    # the inactive job's 128 words


@pytest.mark.parametrize("bins", [1 << 16, 1000, 2])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout", ["contig", "perm"])
def test_epilogue_logistic_matches_fp64(layout, wide, bins):
    """binary:logistic: margins bit for bit, (g, h) within two fp32 ulp of the fp64 sigmoid, the per-job maxima and
    the whole (job, label, score-bin) count table exactly. Every active job holds the margins +-800, +-40 and 0;
    the jobs with ten rows or more hold each of them with both labels."""
    c = _epi_case(layout, wide, 0, bins)
    F, G, H, tam, counts = _run_epilogue(c, bins)
    _check_fgh(c, F, G, H)
    _check_maxima(c, G, H, tam)
    assert torch.equal(counts, c["counts"])
    assert int(counts[1].sum()) == 0
    assert _native_loaded()


@pytest.mark.parametrize("layout", ["contig", "perm"])
def test_epilogue_logistic_optional_outputs(layout):
    """Without the maxima buffer, and without the count table (``bins = 0``: no early stopping), F, G and H are
    the same values."""
    c = _epi_case(layout, 0, 0, 1000)
    F, G, H, tam, counts = _run_epilogue(c, 1000, with_amax=False)
    _check_fgh(c, F, G, H)
    assert torch.equal(counts, c["counts"])
    assert bool((tam[:, list(EPI_ACT), :] == 0).all()) and bool((tam[:, 1, :] == PATTERN).all())
    F, G, H, tam, counts = _run_epilogue(c, 0)
    assert counts is None
    _check_fgh(c, F, G, H)
    _check_maxima(c, G, H, tam)
    assert _native_loaded()


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("layout", ["contig", "perm"])
def test_epilogue_squared_error_exact(layout, wide):
    """``objective = 1``: g = float32(F - y) bit for bit (|F - y| up to 1e6, and F == y), h = 1, the maxima exact,
    and a count table passed along stays empty."""
    c = _epi_case(layout, wide, 1, 1000)
    F, G, H, tam, counts = _run_epilogue(c, 1000)
    _check_fgh(c, F, G, H)
    _check_maxima(c, G, H, tam)
    tch = c["touched"]
    assert bool((G[tch] == 0.0).any()) and float(G[tch].abs().max()) > 9e5
    assert bool((tam.view(torch.float32).amax(0)[list(EPI_ACT), 1] == 1.0).all())
    assert int(counts.abs().sum()) == 0
    F, G, H, tam, counts = _run_epilogue(c, 0)                      # the regressor's call: no table
    _check_fgh(c, F, G, H)
    _check_maxima(c, G, H, tam)
    assert _native_loaded()


def test_epilogue_rejects_packed_entries_beyond_24_bit_rows():
    """Packed entries hold 24 row bits: ``N = 2^24`` without ``wide_rows`` is refused before any launch."""
    from transmogrifai_amd.ops import _native as NV
    dev = torch.device("cuda")
    z32 = torch.zeros(4, dtype=torch.int32, device=dev)
    z64 = torch.zeros(4, dtype=torch.int64, device=dev)
    f32 = torch.zeros(4, dtype=torch.float32, device=dev)
    f64 = torch.zeros(4, dtype=torch.float64, device=dev)
    rc = NV.hip().tmog_hip_boost_epilogue(NV.ptr(z32), NV.ptr(z32), 1, NV.ptr(f32), NV.ptr(z64), NV.ptr(z64),
                                          1 << 24, NV.ptr(f64), NV.ptr(f32), NV.ptr(f32), NV.ptr(f32), 0, None, 0,
                                          1, 1, 1, NV.stream(dev), None, 0)
    assert rc == -2
    torch.cuda.synchronize()
    assert float(f64.abs().sum()) == 0.0 and float(f32.abs().sum()) == 0.0
    assert _native_loaded()


# ------------------------------------------------------------------------------------------------ boost_prologue

def _qmax():
    from transmogrifai_amd.models import tree_engine as TE
    return TE.quant_qmax()


def _bits(x):
    """The bit patterns of an fp32 / fp64 array: equal bits, not merely equal values."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _pow2_scale(a):
    """2^clip(floor(log2(qmax / max(a, 1e-30))), -60, 60) of fp32 maxima, the exponent read from the bits of the
    fp32 quotient (a zero quotient gives -127, which clips to -60)."""
    a = np.asarray(a, np.float32)
    with np.errstate(divide="ignore", over="ignore"):
        x = np.float32(_qmax()) / np.maximum(a, np.float32(1e-30))
    assert x.dtype == np.float32
    e = ((x.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
    return np.exp2(np.clip(e, -60, 60).astype(np.float64)).astype(np.float32)


def _boundary():
    """A maximum ``a`` with qmax / a an exact power of two (qmax < 2^24, so a = qmax / 1024 is an fp32), between
    its two fp32 neighbours: the scale halves from ``a`` to the next value up."""
    a = np.float32(_qmax() / 1024.0)
    assert float(a) * 1024.0 == _qmax()
    lo, hi = np.nextafter(a, np.float32(0)), np.nextafter(a, np.float32(np.inf))
    assert _pow2_scale([lo, a, hi]).tolist() == [1024.0, 1024.0, 512.0]
    return lo, a, hi


def _pro_build(P, act, counts, a_exp, wide, seed, stride=2000):
    """Root entries, (g, h) tables and the oracle's outputs for jobs ``act`` with ``counts`` entries and the
    final maxima ``a_exp`` ([T, 2] fp32). The statistics are drawn so that a staged value stays below qmax;
    every fourth entry of a job has weight 1 and statistics on an exact rounding tie, with both signs."""
    from transmogrifai_amd.models import tree_engine as TE
    rng = np.random.default_rng(seed)
    T = len(act)
    a_exp = np.asarray(a_exp, np.float32).reshape(T, 2)
    q = _pow2_scale(a_exp)                                          # [T, 2]
    qmax = _qmax()
    G = (rng.standard_normal((P, stride)) * 3.0).astype(np.float32)   # cells no entry reads: arbitrary
    H = np.abs(rng.standard_normal((P, stride)) * 3.0).astype(np.float32)
    tjobs, ws = [], []
    for t, (p, n) in enumerate(zip(act, counts)):
        r = rng.choice(stride - 3, n, replace=False).astype(np.int64)
        w = np.ones(n, np.int64) if wide else rng.choice(np.array([1, 2, 255], np.int64), n)
        tie = np.arange(n) % 4 == 0
        w[tie] = 1
        k = rng.integers(0, 1000, n) + 0.5
        sg = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        g = np.where(tie, sg * k / float(q[t, 0]), rng.uniform(-0.99, 0.99, n) * qmax / (w * float(q[t, 0])))
        h = np.where(tie, k / float(q[t, 1]), rng.uniform(0.0, 0.99, n) * qmax / (w * float(q[t, 1])))
        G[p, r], H[p, r] = g.astype(np.float32), h.astype(np.float32)
        if n:
            assert bool((G[p, r][tie].astype(np.float64) == g[tie]).all())      # the ties are exact fp32
        tjobs.append(TE.TreeJob(int(p), TE.TreeParams(), torch.from_numpy(r),
                                None if wide else torch.from_numpy(w)))
        ws.append(w)
    root, cnts = TE._root_rows(tjobs, torch.device("cpu"), bool(wide))
    assert list(cnts) == list(counts)
    # the oracle: rint(float32(float32(w * g) * q_g)), half to even, from the packed entries themselves
    e = root.numpy().view(np.uint32).astype(np.int64)
    er = e if wide else e & 0xFFFFFF
    ew = np.ones(e.size, np.float32) if wide else (e >> 24).astype(np.float32)
    assert wide or bool((ew == np.concatenate(ws).astype(np.float32)).all())
    et = np.repeat(np.arange(T), counts)
    ep = np.asarray(act, np.int64)[et]
    wg = ew * G[ep, er]
    wh = ew * H[ep, er]
    assert wg.dtype == np.float32
    sg, sh = wg * q[et, 0], wh * q[et, 1]
    assert sg.dtype == np.float32 and float(np.abs(sg).max(initial=0)) < 2.0 ** 30
    gh = np.stack([np.rint(sg), np.rint(sh)], 1).astype(np.int32)
    frac = np.abs(sg.astype(np.float64)) % 1.0
    assert e.size < 4 or bool((frac == 0.5).any())
    return dict(P=P, act=list(act), counts=list(counts), T=T, wide=int(wide), stride=stride, tjobs=tjobs,
                root=root, G=torch.from_numpy(G), H=torch.from_numpy(H), a_exp=a_exp, q=q,
                qinv=1.0 / q.astype(np.float64), gh=torch.from_numpy(gh), total=int(e.size))


def _pro_mode(c, later, seed):
    """Inputs that make the kernel arrive at ``a_exp``. First round: ``amax`` holds it. Later round: the maximum of
    ``comp`` and of the 64 copies of ``tam_prev``; the winning copy is 0, 17 or 63 by job, and ``comp`` wins the
    hessian of the first job."""
    rng = np.random.default_rng(seed)
    P, act, a = c["P"], c["act"], c["a_exp"]
    amax = np.full((P, 2), 123.0, np.float32)
    comp = tam_prev = None
    if not later:
        amax[act] = a
    else:
        comp = np.full((P, 2), 5e37, np.float32)                    # inactive jobs: anything
        tamf = np.full((COPIES, P, 2), 9e37, np.float32)
        for t, p in enumerate(act):
            for s in range(2):
                v = a[t, s]
                small = np.float32(0.0) if v == 0 else np.nextafter(v, np.float32(0))
                lower = (rng.random(COPIES).astype(np.float32) * (small if np.isfinite(small) else np.float32(1e30)))
                tamf[:, p, s] = np.minimum(lower, small)
                if t == 0 and s == 1:
                    comp[p, s] = v                                  # comp wins
                else:
                    comp[p, s] = tamf[3, p, s]
                    tamf[(0, 17, 63)[t % 3], p, s] = v
        tam_prev = tamf.view(np.int32).copy()
        assert bool((tam_prev >= 0).all())                          # non-negative floats, no NaN
        want = np.maximum(comp[act], tamf[:, act, :].max(0))
        np.testing.assert_array_equal(_bits(want), _bits(a))
    return amax, comp, tam_prev


def _run_prologue(c, amax, comp, tam_prev):
    from transmogrifai_amd.models import tree_engine as TE
    from transmogrifai_amd.ops import _native as NV
    dev = torch.device("cuda")
    P, T, total = c["P"], c["T"], c["total"]
    amax_d = torch.from_numpy(amax.copy()).to(dev)
    comp_d = None if comp is None else torch.from_numpy(comp).to(dev)
    prev_d = None if tam_prev is None else torch.from_numpy(tam_prev).to(dev)
    next_d = torch.full((COPIES, P, 2), PATTERN, dtype=torch.int32, device=dev)
    act_d = torch.tensor(c["act"], dtype=torch.int32, device=dev)
    off_d = torch.from_numpy(np.concatenate([[0], np.cumsum(c["counts"])]).astype(np.int64)).to(dev)
    root_d = c["root"].to(dev)
    rows_d = torch.full((max(total, 1),), -1, dtype=torch.int32, device=dev)
    gh_d = torch.full((max(total, 1), 2), -1, dtype=torch.int32, device=dev)
    G_d, H_d = c["G"].to(dev), c["H"].to(dev)
    qs_d = torch.full((P, 2), -SENT, dtype=torch.float32, device=dev)
    qi_d = torch.full((P, 2), -SENT, dtype=torch.float64, device=dev)
    rc = NV.hip().tmog_hip_boost_prologue(
        NV.ptr(prev_d), NV.ptr(next_d), NV.ptr(comp_d), NV.ptr(amax_d), P, NV.ptr(act_d), T, NV.ptr(off_d),
        NV.ptr(root_d), NV.ptr(rows_d), total, NV.ptr(G_d), NV.ptr(H_d), c["stride"], NV.ptr(gh_d), NV.ptr(qs_d),
        NV.ptr(qi_d), TE.quant_qmax(), c["wide"], NV.stream(dev))
    torch.cuda.synchronize()
    out = dict(rc=rc, amax=amax_d.cpu(), tam_next=next_d.cpu(), rows=rows_d.cpu()[:total], gh=gh_d.cpu()[:total],
               qscale=qs_d.cpu(), qinv=qi_d.cpu(), tam_prev=None if prev_d is None else prev_d.cpu())
    return out


def _check_prologue(c, out, amax_in, tam_prev):
    from transmogrifai_amd.models import tree_engine as TE
    assert out["rc"] == 0
    P, act = c["P"], c["act"]
    idle = [p for p in range(P) if p not in act]
    assert torch.equal(out["rows"], c["root"])
    assert torch.equal(out["gh"], c["gh"])
    np.testing.assert_array_equal(_bits(out["qscale"].numpy()[act]), _bits(c["q"]))
    np.testing.assert_array_equal(_bits(out["qinv"].numpy()[act]), _bits(c["qinv"]))
    np.testing.assert_array_equal(_bits(out["amax"].numpy()[act]), _bits(c["a_exp"]))
    assert bool((out["qscale"][idle] == -SENT).all()) and bool((out["qinv"][idle] == -SENT).all())
    np.testing.assert_array_equal(_bits(out["amax"].numpy()[idle]), _bits(amax_in[idle]))
    assert bool((out["tam_next"][:, act, :] == 0).all())
    assert bool((out["tam_next"][:, idle, :] == PATTERN).all())
    if tam_prev is not None:
        assert np.array_equal(out["tam_prev"].numpy(), tam_prev)
    # the project's torch path on CPU copies of the same tensors: the two must not drift apart
    hint = torch.full((P, 2), 123.0, dtype=torch.float32)
    hint[act] = torch.from_numpy(c["a_exp"])
    cpu = torch.device("cpu")
    sc, inv = TE._quant_scales(TE.MODE_GH, 2, c["tjobs"], c["G"], c["H"], c["root"], 4096, cpu, amax_hint=hint,
                               wmax_hint=1.0)
    if c["total"]:
        staged = TE._stage_gh(c["root"], c["counts"], c["tjobs"], c["G"], c["H"], sc, c["stride"], bool(c["wide"]))
        assert torch.equal(out["gh"], staged)
        assert torch.equal(out["qscale"][act], sc[act])
        assert torch.equal(out["qinv"][act], inv[act])


def _pro_values():
    lo, a, hi = _boundary()
    f = np.float32
    return {
        # job 1: (0 -> the 1e-30 clamp, exponent capped at +60; 1e-38), job 3: (a, next up), job 4: (next down, 1)
        "first": [(f(0.0), f(1e-38)), (a, hi), (lo, f(1.0))],
        # job 1: (3e38, comp-won 1.0), job 3 (empty): (inf -> exponent capped at -60, a), job 4: (next up, next down)
        "later": [(f(3e38), f(1.0)), (f(np.inf), a), (hi, lo)],
        "wide": [(f(1.0), f(0.0)), (hi, f(3e38)), (a, f(np.inf))],
    }


@pytest.mark.parametrize("name,counts,later,wide", [("first", (1, 70, 600), False, 0),
                                                    ("later", (5, 0, 300), True, 0),
                                                    ("wide", (1, 70, 600), True, 1)])
def test_prologue_matches_numpy_oracle(name, counts, later, wide):
    """Maxima, power-of-two scales (zero, denormal, floor-boundary, huge and infinite maxima), the root copy and
    the staged (g, h) with exact ties, bit for bit; the side effects on the maxima buffers; and the torch path
    (``_quant_scales`` + ``_stage_gh``) on the same inputs."""
    c = _pro_build(6, [1, 3, 4], counts, _pro_values()[name], wide, seed=31 + len(name))
    amax, comp, tam_prev = _pro_mode(c, later, seed=5)
    out = _run_prologue(c, amax, comp, tam_prev)
    _check_prologue(c, out, amax, tam_prev)
    q = c["q"]
    if name == "first":
        assert q[0].tolist() == [2.0 ** 60, 2.0 ** 60] and q[1].tolist() == [1024.0, 512.0]
    if name == "later":
        assert q[0, 0] == np.float32(2.0 ** -60) and q[1, 0] == np.float32(2.0 ** -60)
    assert _native_loaded()


def test_prologue_grid_stride_second_trip():
    """More entries than the 2048 blocks of 256 threads cover in one trip: rows and staged values in full."""
    n = 2048 * 256 + 1000
    c = _pro_build(1, [0], [n], [(np.float32(0.75), np.float32(0.25))], 0, seed=77, stride=n + 5)
    amax, comp, tam_prev = _pro_mode(c, False, seed=6)
    out = _run_prologue(c, amax, comp, tam_prev)
    assert out["rc"] == 0
    assert torch.equal(out["rows"], c["root"])
    assert torch.equal(out["gh"], c["gh"])
    np.testing.assert_array_equal(_bits(out["qscale"].numpy()), _bits(c["q"]))
    assert _native_loaded()


def test_prologue_job_count_boundary():
    """64 active jobs fill the kernel's shared tables and match the oracle; 65 are refused before any launch."""
    rng = np.random.default_rng(8)
    act = rng.permutation(64).tolist()
    a = np.exp(rng.uniform(-20.0, 20.0, (64, 2))).astype(np.float32)
    c = _pro_build(64, act, [3] * 64, a, 0, seed=9, stride=50)
    amax, comp, tam_prev = _pro_mode(c, True, seed=10)
    out = _run_prologue(c, amax, comp, tam_prev)
    _check_prologue(c, out, amax, tam_prev)
    a = np.exp(rng.uniform(-20.0, 20.0, (65, 2))).astype(np.float32)
    c = _pro_build(65, list(range(65)), [3] * 65, a, 0, seed=11, stride=50)
    amax, comp, tam_prev = _pro_mode(c, False, seed=12)
    out = _run_prologue(c, amax, comp, tam_prev)
    assert out["rc"] == -2
    assert bool((out["gh"] == -1).all()) and bool((out["qscale"] == -SENT).all())
    assert _native_loaded()


# ------------------------------------------------------------------------- whole fits on the squared-error path

@functools.lru_cache(maxsize=None)
def _fit_data():
    g = torch.Generator().manual_seed(5)
    n, d = 6000, 8
    X = torch.randn(n, d, generator=g)
    X[:, :2] = (X[:, :2] > 0.8).float()               # two 0/1 columns exercise the missing bin
    s = X[:, 3] + X[:, 0] - 0.5 * X[:, 5] + 0.3 * torch.randn(n, generator=g)
    return X.cuda(), s.cuda(), (s > 0.2).float().cuda()


def _fit_jobs(defaults, **over):
    from transmogrifai_amd.models.base import FitJob
    params = dict(defaults, num_round=8, max_depth=3, eta=0.3, missing=0.0, num_early_stopping_rounds=3, **over)
    n = 6000
    return [FitJob(params, torch.arange(0, n, 2, device="cuda")),
            FitJob(dict(params, max_depth=5), torch.arange(1, n, 3, device="cuda"))]


def _same_states(a, b):
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        assert sa["num_trees"] == sb["num_trees"]
        for k in ARRAYS:
            np.testing.assert_array_equal(np.asarray(sa["forest"][k]), np.asarray(sb["forest"][k]), err_msg=k)


def _fused_on_off(monkeypatch, learner, y, jobs):
    X = _fit_data()[0]
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("TMOG_XGB_FUSED", flag)
        outs.append(learner().fit_batch(X, y, jobs))
    return outs


def test_regressor_fused_round_identical_forests(monkeypatch):
    """``OpXGBoostRegressor``: the fused round (prologue + epilogue kernels, ``objective = 1``) grows exactly the
    forests of the torch path -- both add double(value) to the same fp64 margin, take float32(F - y) and h = 1,
    and scale by exact powers of two from the same maxima."""
    from transmogrifai_amd.models.trees import XGBoostRegressorLearner
    a, b = _fused_on_off(monkeypatch, XGBoostRegressorLearner, _fit_data()[1],
                         _fit_jobs(XGBoostRegressorLearner.defaults))
    _same_states(a, b)
    assert all(s["num_trees"] == 8 for s in a)
    assert any(len(np.asarray(s["forest"]["nodes"])) > 3 * s["num_trees"] for s in a)      # trees not trivial
    assert _native_loaded()


def test_squared_error_classifier_fused_round_identical_forests(monkeypatch):
    """``OpXGBoostClassifier(objective="reg:squarederror")`` with early stopping: identical forests and the same
    number of kept trees with the fused round on and off.

    The epilogue kernel fills the early-stopping count table for binary:logistic only. The fused path used to hand
    the squared-error classifier's (empty) table to the AuPR kernel all the same: the metric read 0 every round, the
    job "stopped" after ``num_early_stopping_rounds`` rounds and kept one tree, where the torch path kept the
    rounds its training AuPR asked for. The fused path now takes that metric from the margins, as the torch
    path does."""
    from transmogrifai_amd.models.trees import XGBoostClassifierLearner
    a, b = _fused_on_off(monkeypatch, XGBoostClassifierLearner, _fit_data()[2],
                         _fit_jobs(XGBoostClassifierLearner.defaults, objective="reg:squarederror"))
    _same_states(a, b)
    assert all(s.get("objective") == "reg:squarederror" for s in a)
    assert any(s["num_trees"] > 1 for s in a)
    assert any(len(np.asarray(s["forest"]["nodes"])) > 3 * s["num_trees"] for s in a)
    assert _native_loaded()

"""``staged_eval_kernel`` (ops/csrc/hip/staged_eval_kernels.hip) against the NumPy oracle of tests/staged_eval_oracle.py
in its exact regime, against the host twin bit for bit in the margins, and against itself from launch to launch; one
write-guard case through the C entry point; the held-out early stopping of tests/test_staged_eval.py on the device."""
import numpy as np
import pytest
import torch

import staged_eval_oracle as SO
import test_staged_eval as TS
from transmogrifai_amd.models import tree_engine as te
from transmogrifai_amd.ops._native import ABI_CONSTS

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 257, 1000)             # one lane, around a wave, more than one workgroup, a ragged last one
FS = (5, 600)


def _cases():
    out = []
    k = 0
    for metric in SO.BINARY + SO.REGRESSION:
        for shape in TS.SHAPES:
            out.append((metric, shape, NS[k % len(NS)], FS[k % len(FS)], 1))
            k += 1
    for metric in SO.MULTI:
        for K in (1, 3, 9, 64):
            for shape in TS.SHAPES:
                out.append((metric, shape, NS[k % len(NS)], FS[(k // 2) % len(FS)], K))
                k += 1
    return out


@pytest.mark.parametrize("metric,shape,n,F,K", _cases())
def test_kernel_matches_oracle_and_host_twin(metric, shape, n, F, K):
    c = SO.case(1000 + n + F + K, metric, n=n, F=F, K=K, **TS.SHAPES[shape])
    got, margins = TS.check_case(c, "cuda")
    again, margins2 = TS.run_case(c, "cuda")
    assert torch.equal(got, again) and torch.equal(margins, margins2)           # bitwise, floating sums included
    host, host_margins = TS.run_case(c, "cpu")
    assert torch.equal(margins.cpu(), host_margins)
    if metric in SO.EXACT:
        assert torch.equal(got.cpu(), host)
    from transmogrifai_amd.ops import _native
    assert _native.hip_loaded()


def test_every_row_count_in_one_workgroup_and_two():
    """The row counts around the wave and workgroup sizes, on the metric with a barrier per stage."""
    for n in NS + (256, 512, 513):
        TS.check_case(SO.case(n, "logloss", n=n, F=5, stages=(1, 2, 1), missing=True), "cuda")


def test_no_rows_and_no_stages_launch_nothing():
    for metric in ("logloss", "error", "aucpr", "mlogloss"):
        K = 3 if metric in SO.MULTI else 1
        TS.check_case(SO.case(3, metric, n=0, F=5, K=K, stages=(2, 1)), "cuda")
        TS.check_case(SO.case(4, metric, n=20, F=5, K=K, stages=()), "cuda")


SENT = -1.5e300
ISENT = -(1 << 60)


@pytest.mark.parametrize("metric", ["logloss", "error"])
def test_entry_point_writes_exactly_its_outputs(metric):
    """tmog_hip_forest_staged_eval with sentinel-filled ``values``, ``counts`` and ``slab`` buffers one element longer
    than the call needs: a floating metric fills exactly ``values[:S]`` and ``slab[:nblk * S]`` and leaves the counts
    alone, a counted one adds into exactly ``counts[:S]`` and leaves the other two alone."""
    from transmogrifai_amd.ops import _native as N
    n, F = 300, 12
    c = SO.case(77, metric, n=n, F=F, stages=(2, 1, 3), missing=True, row_list=True)
    m, want, bound = SO.expect(c)
    S, f = 3, c["forest"]
    nblk = (n + ABI_CONSTS["TMOG_EVAL_BLOCK"] - 1) // ABI_CONSTS["TMOG_EVAL_BLOCK"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    X, rows, y = d(c["X"]), d(c["rows"].astype(np.int32)), d(c["y"])
    nodes, dl, lv = d(f.nodes), d(f.default_left), d(f.value[:, 0])
    toff, tw, so, tc = d(f.tree_off[:-1].astype(np.int64)), d(c["weights"]), d(c["stage_off"]), d(c["tree_col"])
    margins = torch.full((n + 1, 1), float(c["base"]), dtype=torch.float64, device="cuda")
    margins[n] = SENT
    values = torch.full((S + 1,), SENT, dtype=torch.float64, device="cuda")
    slab = torch.full((nblk * S + 1,), SENT, dtype=torch.float64, device="cuda")
    counts = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    counts[S] = ISENT
    rc = N.hip().tmog_hip_forest_staged_eval(
        X.data_ptr(), F, rows.data_ptr(), n, y.data_ptr(), nodes.data_ptr(), dl.data_ptr(), lv.data_ptr(),
        toff.data_ptr(), tw.data_ptr(), f.missing_bin, so.data_ptr(), S, tc.data_ptr(), 1,
        ABI_CONSTS["TMOG_EVAL_" + metric.upper()], c["scale"], 1 << 16, margins.data_ptr(), values.data_ptr(),
        counts.data_ptr(), None, slab.data_ptr(), N.stream())
    torch.cuda.synchronize()
    assert rc == 0
    values, slab, counts, margins = values.cpu().numpy(), slab.cpu().numpy(), counts.cpu().numpy(), margins.cpu().numpy()
    assert values[S] == SENT and slab[-1] == SENT and counts[S] == ISENT and margins[n, 0] == SENT
    np.testing.assert_array_equal(margins[:n], m[-1])
    if metric == "logloss":
        SO.assert_raw(values[:S], want, bound, metric)
        assert (slab[:-1] != SENT).all() and (counts[:S] == 0).all()
        assert (np.abs(slab[:-1].reshape(nblk, S).sum(0) - want) <= bound).all()
    else:
        SO.assert_raw(counts[:S], want, bound, metric)
        assert (values == SENT).all() and (slab == SENT).all()
    # an unknown metric code and a binary metric over K margins are refused without a launch
    for code, K in ((7, 1), (-1, 1), (ABI_CONSTS["TMOG_EVAL_LOGLOSS"], 3)):
        assert N.hip().tmog_hip_forest_staged_eval(None, F, None, n, None, None, None, None, None, None, -1, None, S,
                                                   None, K, code, 1.0, 16, None, None, None, None, None,
                                                   N.stream()) != 0


@pytest.mark.parametrize("resident", ["1", "0"], ids=["resident", "host_planned"])
def test_watch_early_stopping_on_the_device(monkeypatch, resident):
    """The held-out early stopping of test_staged_eval.py at n = 3000, on the device-planned path (the chunk's trees
    come from ``resident_forests``) and on the host-planned one: the CPU backend's model, the same history."""
    monkeypatch.setenv("TMOG_TREE_RESIDENT", resident)
    copies = []
    real = te.resident_forests
    monkeypatch.setattr(te, "resident_forests", lambda trees: copies.append(len(trees)) or real(trees))
    st = TS._watched_fit("binary", device="cuda")[5]
    monkeypatch.setenv("TMOG_TREE_RESIDENT", "1")
    L, X, y, params, rows, cpu, metric, K = TS._watched_fit("binary")
    TS._same_model(st, cpu)
    assert st["num_trees"] < 40 and st["best_iteration"] == cpu["best_iteration"]
    assert st["eval_metric"] == "logloss" and st["eval_history"].shape == cpu["eval_history"].shape
    np.testing.assert_allclose(st["eval_history"], cpu["eval_history"], rtol=1e-12, atol=0)
    chunks = [k for k in copies if k]               # device-planned rounds per copy (the CPU fit has none)
    if resident == "1":
        assert len(chunks) >= 2 and max(chunks) <= 3        # one copy per chunk of min(patience, 16) = 3 rounds
    else:
        assert not any(copies)

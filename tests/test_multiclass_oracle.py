"""tests/multiclass_oracle.py against hand-computed cases and against the host torch paths of the multi-class linear and
MLP learners, on the case tables that tests/test_multiclass_kernels_gpu.py runs on the device: ``SparseDesign`` built on
the CPU (field by field, at the real segment length and at a small one), ``MultinomialObjective`` with the fused path off
on fp64 input, ``MLPObjective._output``, ``_bias_sigmoid_`` and ``_sigmoid_backprop_`` on CPU tensors. Also the recorded
ceilings of the float32 re-evaluation (``E32``). No GPU."""
import numpy as np
import pytest
import torch

import multiclass_oracle as O
from transmogrifai_amd.models.linear import MultinomialObjective
from transmogrifai_amd.models.mlp import MLPObjective, _bias_sigmoid_, _sigmoid_backprop_
from transmogrifai_amd.ops import linear as LK


# ================================================================================================= sparse design
def test_sparse_builder_by_hand():
    X = np.array([[0, 5, 0, 1],
                  [2, 6, 0, 0],
                  [0, 7, 0, 0],
                  [3, 8, 0, 0],
                  [4, 9, 0, 0],
                  [0, 0, 0, 0],
                  [0, 1, 0, 0],
                  [0, 2, 0, 0]], np.float32)         # column 1: 7 of 8 rows (dense); column 0: 3 of 8 is > 0.25 * 8 too
    S = O.Sparse(X, seg=2, dense_frac=0.5)           # at 0.5: dense = {1}; sparse = {0, 2, 3}
    assert S.idx_d.tolist() == [1] and S.idx_s.tolist() == [0, 2, 3]
    assert S.row_ptr.tolist() == [0, 1, 2, 2, 3, 4, 4, 4, 4]
    assert S.col.tolist() == [2, 0, 0, 0] and S.val.tolist() == [1, 2, 3, 4]
    assert S.csc_row.tolist() == [1, 3, 4, 0] and S.csc_val.tolist() == [2, 3, 4, 1]
    assert S.seg_begin.tolist() == [0, 2, 3, 4]      # column 0: pairs 0-1 and 2; column 2: none; column 3: pair 3
    assert S.col_seg.tolist() == [0, 2, 2, 3] and S.n_seg == 3
    assert [S.segments_of(j) for j in range(3)] == [2, 0, 1]


def test_segs70_design_reaches_the_named_paths():
    S = O.Sparse(O.design("segs70", True), O.SEG_SMALL)
    assert S.row_nnz[:len(O.ROW_NNZ)].tolist() == list(O.ROW_NNZ)
    assert len(S.idx_d) == 3
    special = S.col_cnt[-len(O.SPECIAL_COL_NNZ):]
    assert special.tolist() == list(O.SPECIAL_COL_NNZ)
    assert [S.segments_of(S.ds - 6 + i) for i in range(6)] == [0, 1, 1, 2, 2, 5]
    last5 = S.col_seg[S.ds] - 1                       # the 5-segment column's last segment holds exactly one pair
    assert S.seg_begin[last5 + 1] - S.seg_begin[last5] == 1
    S2 = O.Sparse(O.design("seg4096_two_segments", False), 4096)
    assert S2.idx_d.tolist() == [0, 1] and S2.segments_of(0) == 2 and 4096 < S2.col_cnt[0] < 0.25 * 20000
    assert O.Sparse(O.design("no_dense", False), 70).idx_d.size == 0
    assert O.Sparse(O.design("no_sparse", False), 70).ds == 0
    S5 = O.Sparse(O.design("n5", False), 70)
    assert S5.idx_d.tolist() == [0] and S5.col_cnt.tolist() == [1] * 7 + [0]
    S1 = O.Sparse(O.design("n1", False), 70)
    assert S1.idx_d.tolist() == [1, 4] and S1.nnz == 0 and S1.n_seg == 0 and S1.ds == 4


@pytest.mark.parametrize("seg", [None, O.SEG_SMALL], ids=["seg4096", "seg70"])
@pytest.mark.parametrize("name", ("segs70", "seg4096_two_segments") + O.DESIGNS_SMALL)
def test_sparse_builder_matches_sparse_design(name, seg, monkeypatch):
    if seg is not None:
        monkeypatch.setattr(LK, "_SEG_NNZ", seg)
    for integer in (True, False):
        X = O.design(name, integer)
        S = O.Sparse(X, LK._SEG_NNZ, LK.SparseDesign.DENSE_FRAC)
        D = LK.SparseDesign(torch.from_numpy(X))
        assert D.ds == S.ds and D.nnz == S.nnz and D.n_seg == S.n_seg
        for field in ("row_ptr", "col", "csc_row", "seg_begin", "col_seg", "idx_d", "idx_s"):
            got = getattr(D, field)
            assert got.dtype == torch.from_numpy(getattr(S, field)).dtype, field
            assert got.tolist() == getattr(S, field).tolist(), field
        assert np.array_equal(O.bits(D.val.numpy()), O.bits(S.val))
        assert np.array_equal(O.bits(D.csc_val.numpy()), O.bits(S.csc_val))
        assert np.array_equal(O.bits(D.csc_val_sq.numpy()), O.bits(S.csc_val * S.csc_val))
        assert np.array_equal(O.bits(D.Xd.numpy()), O.bits(S.Xd))


def test_product_bounds_hold_for_an_fp32_row_loop():
    """The derived bounds against a literal fp32 evaluation in the kernels' order (numpy float32, pair by pair)."""
    X = O.design("no_dense", False)
    S = O.Sparse(X, 8)
    V, R = O.operands(X, 3, False)
    ref, bound = O.mm_bound(S, V)
    Vs = V[S.idx_s]
    for r in range(S.N):
        acc = np.zeros(3, np.float32)
        for t in range(S.row_ptr[r], S.row_ptr[r + 1]):
            acc = (acc + S.val[t] * Vs[S.col[t]]).astype(np.float32)
        assert (np.abs(acc - ref[r]) <= bound[r]).all()
    ref, bound = O.tmm_bound(S, R, False)
    for j in range(S.ds):
        tot = np.zeros(3)
        for s in range(S.col_seg[j], S.col_seg[j + 1]):
            acc = np.zeros(3, np.float32)
            for t in range(S.seg_begin[s], S.seg_begin[s + 1]):
                acc = (acc + S.csc_val[t] * R[S.csc_row[t]]).astype(np.float32)
            tot += acc
        assert (np.abs(tot - ref[S.idx_s[j]]) <= bound[S.idx_s[j]]).all()


# ======================================================================================================== bf16
def test_bf16_rounding_by_hand_and_against_torch():
    x = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -1 - 2.0 ** -8, 0.0], np.float32)
    assert O.bf16_round(x).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, 0.0]        # ties go to even
    rng = np.random.default_rng(0)
    r = (rng.standard_normal(20000) * np.exp(rng.standard_normal(20000) * 5)).astype(np.float32)
    t = torch.from_numpy(r)
    hi_t = t.to(torch.bfloat16)
    lo_t = (t - hi_t.float()).to(torch.bfloat16)
    hi, lo = O.bf16_split(r)
    assert np.array_equal(hi, hi_t.float().numpy()) and np.array_equal(lo, lo_t.float().numpy())
    assert np.array_equal(O.bf16_from_bits(O.bf16_bits(hi)), hi)
    assert np.array_equal(O.bf16_bits(hi).view(np.int16), hi_t.view(torch.int16).numpy())
    assert (np.abs(lo) <= 2.0 ** -8 * np.abs(hi)).all()
    assert (np.abs(r.astype(np.float64) - hi - lo) <= 2.0 ** -17 * np.abs(r)).all()
    assert O.bf16_ulp(np.array([1.0, 1.5, 2.0, 0.75])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]


# ======================================================================================================= softmax
def test_softmax_oracle_by_hand():
    m = np.log(np.array([[[1.0, 2.0, 5.0]], [[1.0, 1.0, 2.0]], [[3.0, 1.0, 4.0]]]))          # N = 3, P = 1, K = 3
    loss, R, lse = O.softmax_loss_residual(m, np.array([2.0, -1.0, 3.0]), np.array([[2.0], [3.0], [0.5]]))
    np.testing.assert_allclose(lse[:, 0], np.log([8.0, 4.0, 8.0]), rtol=1e-15)
    np.testing.assert_allclose(loss[:, 0], [2 * np.log(8 / 5), 0.0, 0.0], rtol=1e-15)        # labels -1 and K: loss 0
    np.testing.assert_allclose(R[0, 0], [2 / 8, 4 / 8, 2 * (5 / 8 - 1)], rtol=1e-15)
    np.testing.assert_allclose(R[1, 0], [3 / 4, 3 / 4, 6 / 4], rtol=1e-15)                   # ... and no one-hot term
    np.testing.assert_allclose(R[2, 0], [1.5 / 8, 0.5 / 8, 2 / 8], rtol=1e-15)


@pytest.mark.parametrize("margins", O.SOFTMAX_MARGINS)
@pytest.mark.parametrize("N", O.SOFTMAX_N)
@pytest.mark.parametrize("P,K", O.SOFTMAX_PK, ids=O.SOFTMAX_PK_IDS)
def test_softmax_oracle_matches_mlp_output(P, K, N, margins):
    """``MLPObjective._output`` on the CPU, fp64 logits, in-range labels (its clamp of other labels is never reached
    from ``fit_batch``, see the oracle's docstring)."""
    M, bias, y, W = O.softmax_case(P, K, N, margins, out_of_range=False)
    obj = MLPObjective(torch.zeros(N, 1), torch.from_numpy(y), torch.from_numpy(W), [1, K])
    logits = torch.from_numpy(M.astype(np.float64)).view(N, P, K).permute(1, 0, 2)
    f, R = obj._output(logits, torch.from_numpy(bias.astype(np.float64)).view(P, K), True)
    m = M.astype(np.float64).reshape(N, P, K) + bias.astype(np.float64).reshape(1, P, K)
    loss, Rr, _ = O.softmax_loss_residual(m, y, W)
    np.testing.assert_allclose(f.numpy(), loss.sum(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.permute(1, 0, 2).numpy(), Rr, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_oracle_matches_host_multinomial_objective(K):
    """``MultinomialObjective`` with the fused path off (CPU), fp64: margins, loss, ``X^T R`` and the intercept sums from
    the oracle's product and softmax references."""
    X = O.design("no_dense", False).astype(np.float64)
    N, d = X.shape
    P = 3
    rng = np.random.default_rng(K)
    y = rng.integers(0, K, N).astype(np.float64)
    W = O._weights(rng, (N, P)).astype(np.float64)
    U = rng.standard_normal(((d + 1) * K, P)) * 0.5
    ob = MultinomialObjective(torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(W), torch.ones(d, P).double(),
                              torch.zeros(P).double(), torch.ones(P, dtype=torch.bool), K)
    assert not ob.fused
    f, g = ob.value_grad(torch.from_numpy(U))
    B = U.reshape(d + 1, K, P)
    V = B[:d].transpose(0, 2, 1).reshape(d, P * K)
    m = O.xv(X, V)[0].reshape(N, P, K) + B[d].T[None]
    loss, R, _ = O.softmax_loss_residual(m, y, W)
    wsum = W.sum(0)
    np.testing.assert_allclose(f.numpy(), loss.sum(0) / wsum, rtol=1e-12)
    np.testing.assert_allclose(ob.value(torch.from_numpy(U)).numpy(), loss.sum(0) / wsum, rtol=1e-12)
    G = O.xtr(X, R.reshape(N, P * K))[0].reshape(d, P, K).transpose(0, 2, 1) / wsum
    gr = np.concatenate([G, (R.sum(0).T / wsum)[None]], 0).reshape(U.shape)
    np.testing.assert_allclose(g.numpy(), gr, rtol=1e-10, atol=1e-13)


# =========================================================================================================== mlp
@pytest.mark.parametrize("N", O.MLP_N)
@pytest.mark.parametrize("B", O.MLP_B)
@pytest.mark.parametrize("P", O.MLP_P)
def test_mlp_oracles_match_host_paths(P, B, N):
    Z, b = O.sigmoid_case(P, N, B)
    ref, e32 = O.bias_sigmoid(Z, b)
    assert e32 <= O.E32["sigmoid"]
    got = _bias_sigmoid_(torch.from_numpy(Z.copy()), torch.from_numpy(b)).numpy()
    assert (np.abs(got - ref) <= O.allow_e32("sigmoid", e32)).all()
    D, A = O.backprop_case(P, N, B)
    want, _ = O.sigmoid_backprop(D, A)
    Dt = torch.from_numpy(D.copy())
    sums = _sigmoid_backprop_(Dt, torch.from_numpy(A)).numpy()
    assert (np.abs(Dt.numpy() - want) <= 4 * O.U * np.abs(want) + 2.0 ** -149).all()
    own = Dt.numpy().astype(np.float64)
    assert (np.abs(sums - own.sum(1)) <= N * O.U64 * np.abs(own).sum(1)).all()


def test_sigmoid_oracle_at_the_saturation_list():
    z = np.array(O.SIGMOID_Z)
    s = O.sigmoid(z)
    assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all() and (np.diff(s) >= 0).all()
    assert s[5] == s[6] == 0.5 and s[0] == 0.0 and s[-1] == 1.0
    np.testing.assert_allclose(s[4], 1 / (1 + np.exp(20.0)), rtol=1e-15)
    s32 = O.sigmoid_f32(z.astype(np.float32))
    assert np.isfinite(s32).all() and (np.diff(s32) >= 0).all()


# =========================================================================================== the recorded ceilings
def test_e32_ceilings_cover_every_case():
    """Every case's float32-against-fp64 figure is at or below its entry of the table in the oracle's docstring."""
    worst = dict.fromkeys(O.E32, 0.0)
    for P, K in O.SOFTMAX_PK:
        for N in O.SOFTMAX_N:
            for margins in O.SOFTMAX_MARGINS:
                M, bias, y, _ = O.softmax_case(P, K, N, margins)
                ep, el = O.softmax_e32(O.margins_f32(M, bias, P, K), y)
                worst["softmax_p"], worst["softmax_loss"] = max(worst["softmax_p"], ep), max(worst["softmax_loss"], el)
    for P in O.MNL_P:
        for K in O.MNL_K:
            for N in O.MNL_N:
                M2, bias, y, _, _ = O.mnl_case(P, K, N)
                ep, el = O.softmax_e32(O.mnl_margins_f32(M2, bias, P, K), y)
                worst["mnl_p"], worst["mnl_loss"] = max(worst["mnl_p"], ep), max(worst["mnl_loss"], el)
    for _, K, pc, N, dpad, _, _ in O.MNL_BF16_CASES:
        for integer in (False, True):
            X, Vhi, Vlo, bias, y, _, _ = O.mnl_bf16_case(K, pc, N, dpad, integer)
            m, _ = O.mnl_bf16_reference(X, Vhi, Vlo, bias, N, K)
            ep, el = O.softmax_e32(m.astype(np.float32), y)
            worst["bf16_p"], worst["bf16_loss"] = max(worst["bf16_p"], ep), max(worst["bf16_loss"], el)
    for k in ("softmax_p", "softmax_loss", "mnl_p", "mnl_loss", "bf16_p", "bf16_loss"):
        assert 0 < worst[k] <= O.E32[k], (k, worst[k])


def test_empty_tail_blocks():
    for N in (1, 2, 3, 5, 257, 2047, 2048, 2049, 5000):
        nblk = O.empty_tail_blocks(N)
        rpb = -(-N // nblk)
        assert (nblk - 1) * rpb >= N and ((nblk - 2) * (-(-N // (nblk - 1))) < N or nblk == 2)

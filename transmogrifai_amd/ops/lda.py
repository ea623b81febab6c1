"""Sparse variational E-step of LDA on the device (``ops/csrc/hip/lda_kernels.hip``).

The dense E-step (``stages/feature/nlp_stages.py lda_e_step``) works on the whole ``[N, V]`` term-count matrix in
fp64; a document holds a few dozen of the ``V`` terms. Here the corpus is a CSR built once per fit or transform,
the per-document fixed point runs in one kernel whose work is ``nnz * K``, and the topic statistics are a
deterministic segmented reduction over the CSC of the same non-zeros.
"""
from __future__ import annotations

import os

import torch

_SEG_NNZ = 4096        # non-zeros per CSC segment (one wave each), as SparseDesign
MAX_K = 64             # lda_kernels.hip kMaxK: one lane per topic


class DocTermCSR:
    """The non-zeros of a dense term-count matrix ``X [N, V]``: CSR (``row_ptr`` int64, ``col`` int32 sorted per
    row, ``val`` fp32), their segmented CSC (``csc_row`` int32, ``seg_begin`` / ``col_seg`` int64, segments of at
    most 4096 non-zeros of one column), ``csc_pos`` (the CSR position of every CSC entry) and ``row_sum`` (fp64).
    Built on the device of ``X``: by ``ops.linear.csr_csc_build`` (``ops/csrc/hip/sparse_build_kernels.hip``; an fp32 or
    fp64 device matrix of at most 16384 columns, ``row_sum`` added in column order), otherwise, or with
    ``TMOG_SPARSE_BUILD=0``, in row chunks with torch ops. Values are kept as fp32: term counts are exact, an fp64
    column of other values (tf-idf weights, counts above 2**24) is rounded where the dense path is not."""

    def __init__(self, X: torch.Tensor, chunk: int = 1 << 16):
        from .linear import csr_csc_build, sparse_build_enabled, sparse_build_supported
        dev = X.device
        N, V = X.shape
        self.shape = (N, V)
        self.device = dev
        if sparse_build_enabled() and sparse_build_supported(X):
            B = csr_csc_build(X, None, _SEG_NNZ, want_pos=True, want_row_sum=True, want_val=False)
            for name in ("nnz", "row_ptr", "col", "val", "row_sum", "csc_pos", "csc_row", "col_seg", "n_seg",
                         "seg_begin"):
                setattr(self, name, B[name])
            return
        rows, cols, vals = [], [], []
        for a in range(0, N, chunk):
            Xc = X[a:a + chunk]
            ij = torch.nonzero(Xc)                  # row-major: columns ascending within a row
            rows.append(ij[:, 0] + a)
            cols.append(ij[:, 1])
            vals.append(Xc[ij[:, 0], ij[:, 1]].to(torch.float32))
        r = torch.cat(rows) if rows else torch.zeros(0, dtype=torch.int64, device=dev)
        c = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.int64, device=dev)
        v = torch.cat(vals) if vals else torch.zeros(0, dtype=torch.float32, device=dev)
        self.nnz = int(r.numel())
        self.row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.row_ptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0)
        self.col = c.to(torch.int32).contiguous()
        self.val = v.contiguous()
        self.row_sum = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, r, v.to(torch.float64))
        self.csc_pos = torch.argsort(c * max(N, 1) + r).contiguous()
        self.csc_row = r[self.csc_pos].to(torch.int32).contiguous()
        cnt = torch.bincount(c, minlength=V)
        col_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        col_start[1:] = torch.cumsum(cnt, 0)
        nseg = (cnt + _SEG_NNZ - 1) // _SEG_NNZ
        self.col_seg = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        self.col_seg[1:] = torch.cumsum(nseg, 0)
        self.n_seg = int(self.col_seg[-1].item()) if V else 0
        seg_col = torch.repeat_interleave(torch.arange(V, device=dev), nseg)
        within = torch.arange(self.n_seg, device=dev) - self.col_seg[seg_col]
        self.seg_begin = torch.cat([col_start[seg_col] + within * _SEG_NNZ,
                                    torch.tensor([self.nnz], dtype=torch.int64, device=dev)]).contiguous()


def worthwhile(X: torch.Tensor, K: int) -> bool:
    """The sparse path serves a device matrix with at most 64 topics; it is taken for a wide, long and mostly zero
    one (the rule of ``SparseDesign.worthwhile``, on a row sample). ``TMOG_LDA_SPARSE=1`` / ``0`` force the choice.
    Such a matrix needs the HIP library: if it cannot be built or loaded this raises, it does not run dense."""
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dim() == 2 and 1 <= K <= MAX_K):
        return False
    force = os.environ.get("TMOG_LDA_SPARSE")
    if force == "0":
        return False
    if force != "1":
        if X.shape[1] < 256 or X.shape[0] < 4096:
            return False
        samp = X[:: max(1, X.shape[0] // 8192)]
        if float((samp != 0).float().mean()) >= 0.1:
            return False
    from . import _native as N_
    N_.hip()                                        # a library that cannot be loaded is an error, not a dense run
    return True


def lds_terms(K: int) -> int:
    """Terms of one document that the E-step kernel keeps in LDS; longer documents re-read the rest from L2."""
    from . import _native as N_
    return int(N_.hip().tmog_hip_lda_lds_terms(int(K)))


def doc_fixed_point(csr: DocTermCSR, expEbT: torch.Tensor, alpha: torch.Tensor, iters: int, tol: float):
    """``lda_estep_kernel``: ``(gamma [N, K], n_iter [N] int32, expEt [N, K], r [nnz])`` for ``expEbT [V, K]`` fp64;
    ``expEt`` and ``r = count / phinorm`` (CSR order) are taken at the final ``gamma``."""
    from . import _native as N_
    N, V = csr.shape
    K = int(expEbT.shape[1])
    dev = csr.device
    if tuple(expEbT.shape) != (V, K) or expEbT.dtype != torch.float64 or not expEbT.is_contiguous():
        raise ValueError(f"expEbT must be a contiguous fp64 [{V}, K] tensor")
    alpha = alpha.to(device=dev, dtype=torch.float64).contiguous()
    gamma = torch.empty(N, K, dtype=torch.float64, device=dev)
    expEt = torch.empty(N, K, dtype=torch.float64, device=dev)
    n_iter = torch.empty(N, dtype=torch.int32, device=dev)
    r = torch.empty(csr.nnz, dtype=torch.float64, device=dev)
    queue = torch.empty(1, dtype=torch.int32, device=dev)
    N_.check(N_.hip().tmog_hip_lda_estep(N_.ptr(csr.row_ptr), N_.ptr(csr.col), N_.ptr(csr.val), N, N_.ptr(expEbT), K,
                                         N_.ptr(alpha), int(iters), float(tol), N_.ptr(queue), N_.ptr(gamma),
                                         N_.ptr(n_iter), N_.ptr(expEt), N_.ptr(r), N_.stream(dev)), "lda_estep")
    return gamma, n_iter, expEt, r


def topic_stats(csr: DocTermCSR, expEt: torch.Tensor, r: torch.Tensor, expEbT: torch.Tensor) -> torch.Tensor:
    """``lda_sstats_kernel``: ``sstats[k, v] = expEb[k, v] * sum_d expEt[d, k] r[d, v]``, ``[K, V]`` fp64."""
    from . import _native as N_
    V = csr.shape[1]
    K = int(expEbT.shape[1])
    dev = csr.device
    partial = torch.empty(max(csr.n_seg, 1), K, dtype=torch.float64, device=dev)
    sstats = torch.empty(K, V, dtype=torch.float64, device=dev)
    N_.check(N_.hip().tmog_hip_lda_sstats(N_.ptr(csr.seg_begin), N_.ptr(csr.csc_row), N_.ptr(csr.csc_pos), csr.n_seg,
                                          N_.ptr(csr.col_seg), V, N_.ptr(expEt), N_.ptr(r), N_.ptr(expEbT), K,
                                          N_.ptr(partial), N_.ptr(sstats), N_.stream(dev)), "lda_sstats")
    return sstats


def e_step(csr: DocTermCSR, Elogbeta: torch.Tensor, alpha: torch.Tensor, iters: int = 100, tol: float = 1e-3,
           sstats: bool = True):
    """The E-step of ``lda_e_step`` over a :class:`DocTermCSR`: ``(theta [N, K], sstats [K, V] or None, n_iter)``."""
    expEbT = torch.exp(Elogbeta.to(device=csr.device, dtype=torch.float64)).t().contiguous()
    gamma, n_iter, expEt, r = doc_fixed_point(csr, expEbT, alpha, iters, tol)
    ss = topic_stats(csr, expEt, r, expEbT) if sstats else None
    return gamma / gamma.sum(1, keepdim=True), ss, n_iter

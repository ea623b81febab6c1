"""Exact LOCO insights of the linear-margin learners on the device (``csrc/hip/loco_linear_kernels.hip``).

A margin model is ``score = link(b + W^T x)`` (``Learner.linear_margins``); zeroing column ``j`` moves the margin by
``-W[j, :] x_j``, so one pass over a record's non-zeros gives every candidate's score change and the kernel selects
the top-K on the spot."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native as N

# link codes of the kernel (enum Link), in order
LINKS = ("identity", "exp", "inverse", "sigmoid", "square", "power", "binary", "step", "softmax")
MAX_TOP_K = 64
MAX_MARGINS = 16


def n_scores(link: str, Cm: int) -> int:
    return 2 if link == "binary" else Cm


def loco_linear(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor, link: str, param: float,
                cand_of_col: torch.Tensor, n_plain: int, group_size: torch.Tensor, top_k: int, abs_mode: bool,
                leave_out: bool, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                ) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """Top-K LOCO insights of the records ``X [n, d]`` (device, fp32 or fp64, unit column stride) under the margin
    model ``link(b + W^T x)`` with ``W [d, Cm]``, ``b [Cm]`` (fp64): ``(cols int64 [n, K] (-1 = no insight), diffs
    fp64 [n, K, C])`` as ``RecordInsightsLOCO._loco_block`` returns them, with zeros where there is no insight.
    ``cand_of_col [d]`` maps a column to its candidate -- plain columns ``0 .. n_plain - 1`` in column order, group
    ``g`` to ``n_plain + g`` -- and ``group_size [G]`` holds the group sizes. A group is aggregated by ``Avg`` (the
    mean of its members' changes over the group size) or, with ``leave_out``, zeroed as a whole, and is reported
    under its first active column. Ties keep the earlier candidate; a run is bitwise repeatable. ``out``: contiguous
    ``(cols, diffs)`` of those shapes to write into; every cell of both is written.

    Returns ``None`` for a shape outside the kernel's limits (``top_k <= 64``, ``Cm <= 16``, the group state within
    the LDS, fp32 / fp64 with unit column stride); the caller then uses its host formula. A NaN or infinite cell
    keeps whatever the arithmetic gives and reads or writes nothing out of bounds."""
    n, d = X.shape
    Cm = int(W.shape[1])
    G = int(group_size.numel())
    m = n_plain + G
    if not X.is_cuda or X.dtype not in (torch.float32, torch.float64) or (d > 0 and X.stride(1) != 1) \
            or not 1 <= top_k <= MAX_TOP_K or not 1 <= Cm <= MAX_MARGINS or (n > 1 and X.stride(0) < d):
        return None
    if tuple(W.shape) != (d, Cm) or b.numel() != Cm or cand_of_col.numel() != d or (Cm > 1 and link != "softmax"):
        raise ValueError("loco_linear: inconsistent margin model")
    if d > 0 and (int(cand_of_col.min()) < 0 or int(cand_of_col.max()) >= m):
        raise ValueError("loco_linear: cand_of_col names a candidate outside the plan")
    dev = X.device
    C = n_scores(link, Cm)
    kk = min(top_k, m)
    K = min(top_k if abs_mode else 2 * top_k, 2 * kk)
    if out is None:
        out = (torch.empty(n, K, dtype=torch.long, device=dev), torch.empty(n, K, C, dtype=torch.float64, device=dev))
    cols, diffs = out
    if (tuple(cols.shape), cols.dtype, tuple(diffs.shape), diffs.dtype) != ((n, K), torch.long, (n, K, C), torch.float64) \
            or not (cols.is_contiguous() and diffs.is_contiguous() and cols.device == diffs.device == dev):
        raise ValueError("loco_linear: out must be contiguous device (int64 [n, K], float64 [n, K, C])")
    if n == 0 or m == 0 or K == 0:
        return cols.fill_(-1), diffs.zero_()
    Wd = W.to(dev, torch.float64).contiguous()
    bd = b.to(dev, torch.float64).contiguous()
    cd = cand_of_col.to(dev, torch.int32).contiguous()
    gs = group_size.to(dev, torch.float64).contiguous()
    rc = N.hip().tmog_hip_loco_linear(
        N.ptr(X), int(X.dtype == torch.float64), n, d, X.stride(0) if n > 1 else max(d, 1), N.ptr(Wd), N.ptr(bd), Cm,
        LINKS.index(link), float(param), N.ptr(cd), n_plain, G, N.ptr(gs), top_k, int(abs_mode), int(leave_out),
        N.ptr(cols), N.ptr(diffs), N.stream(dev))
    if rc == -3:                     # the group accumulators do not fit the LDS
        return None
    N.check(rc, "loco_linear")
    return cols, diffs

"""Plain numpy fp64 LOCO of a margin model ``s(b + W^T x)`` by the definition ``s(m) - s(m - sum t)``, with the
candidate layout of ``RecordInsightsLOCO`` (plain columns in column order, then one candidate per group) and a
selection that is two stable sorts (ties keep the earlier candidate, positives before negatives). No project code."""
import numpy as np


def scores(m, link, param=0.0):
    m = np.asarray(m, np.float64)
    if link == "softmax":
        e = np.exp(m - m.max())
        return e / e.sum()
    e = m[0]
    if link == "binary":
        p = 1.0 / (1.0 + np.exp(-e))
        return np.array([1.0 - p, p])
    return np.array([{"identity": lambda: e, "exp": lambda: np.exp(e), "inverse": lambda: 1.0 / e,
                      "sigmoid": lambda: 1.0 / (1.0 + np.exp(-e)), "square": lambda: e * e,
                      "power": lambda: max(e, 1e-12) ** (1.0 / param), "step": lambda: float(e > param)}[link]()])


def slope(link, param, lo, hi):
    """A bound of the link's slope on the margins [lo, hi] a record visits (the derivative at the worse end)."""
    return {"identity": lambda: 1.0, "binary": lambda: 0.25, "sigmoid": lambda: 0.25, "softmax": lambda: 0.5,
            "step": lambda: 0.0, "exp": lambda: np.exp(hi), "square": lambda: 2 * max(abs(lo), abs(hi)),
            "inverse": lambda: 1.0 / min(abs(lo), abs(hi)) ** 2,
            "power": lambda: max(lo ** (1 / param - 1), hi ** (1 / param - 1)) / abs(param)}[link]()


def loco(X, W, b, link, param, groups, top_k, abs_mode, leave_out):
    """``(cols [n, K], diffs [n, K, C], vals [n, m], unit [n], L [n])``: the insights, every candidate's value in
    the explained score column, per record ``L * sum_j max_c |W_jc x_j|`` (what one relative rounding of the margin
    terms moves a score by) and the slope bound ``L`` itself."""
    X, W, b = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    n, d = X.shape
    grouped = {c for g in groups for c in g}
    cands = [[j] for j in range(d) if j not in grouped] + [list(g) for g in groups]
    m = len(cands)
    kk = min(top_k, m)
    K = min(top_k if abs_mode else 2 * top_k, 2 * kk)
    C = len(scores(b, link, param))
    cols, diffs = np.full((n, K), -1, np.int64), np.zeros((n, K, C))
    vals, unit, L = np.zeros((n, m)), np.zeros(n), np.zeros(n)
    for i in range(n):
        T = W * X[i][:, None]
        M = b + T.sum(0)
        s0 = scores(M, link, param)
        ex = 0 if C == 1 else 1 if C == 2 else int(np.argmax(M))
        V, rep, seen = np.zeros((m, C)), np.full(m, -1), [M]
        for c, members in enumerate(cands):
            act = [j for j in members if X[i, j] != 0]
            if not act:
                continue
            rep[c] = act[0]
            if leave_out or len(members) == 1:
                seen.append(M - T[act].sum(0))
                V[c] = s0 - scores(seen[-1], link, param)
            else:
                seen += [M - T[j] for j in act]
                V[c] = sum(s0 - scores(M - T[j], link, param) for j in act) / len(members)
        v = vals[i] = V[:, ex]
        order = lambda idx, key: [idx[k] for k in np.argsort(-key[idx], kind="stable")]
        pos = order(np.flatnonzero((v > 0) & (rep >= 0)), v)[:kk]
        neg = order(np.flatnonzero((v < 0) & (rep >= 0)), -v)[:kk]
        merged = np.array(pos + neg, np.int64)
        sel = order(merged, np.abs(v) if abs_mode else v)[:K] if merged.size else []
        cols[i, :len(sel)], diffs[i, :len(sel)] = rep[sel], V[sel]
        seen = np.array(seen)
        L[i] = slope(link, param, seen.min(), seen.max())
        unit[i] = L[i] * np.abs(T).max(1).sum()
    return cols, diffs, vals, unit, L


def separated(vals, abs_mode, gap):
    """Records whose candidate keys (and 0) are pairwise more than ``gap[i]`` apart: their selection is decided."""
    keys = np.abs(vals) if abs_mode else vals
    keys = np.sort(np.concatenate([keys, np.zeros((len(keys), 1))], 1), 1)
    steps = np.diff(keys, axis=1)
    exact_zero = (keys[:, 1:] == 0) & (keys[:, :-1] == 0)                # inactive candidates are exactly 0
    return np.where(exact_zero, np.inf, steps).min(1) > gap

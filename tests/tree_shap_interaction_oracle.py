"""Brute-force SHAP interaction values, straight from the definition, on the ``Forest`` node arrays (NumPy only).

With ``g(S)`` the forest's path-dependent game of ``tree_shap_oracle`` (``_game``) over the ``U`` used features,
the interaction value of two features ``i != j`` is half the Shapley interaction index,

    Phi_ij = sum over S within N - {i, j} of |S|! (U - |S| - 2)! / (2 (U - 1)!)
             * (g(S + i + j) - g(S + i) - g(S + j) + g(S)),

the main effect is ``Phi_ii = phi_i - sum_{j != i} Phi_ij`` with ``phi`` the Shapley values of
``tree_shap_oracle.shap_oracle``, the bias cell ``Phi_UU = g(empty)`` and the rest of row and column ``U`` is 0.
All ``2^U`` subsets are evaluated at once as a bitmask vector. Shares no code with the implementation."""
import math

import numpy as np

import tree_shap_oracle as O


def interaction_oracle(forest, Xb, rows=None, tree_weight=None, tree_out=None, n_out=None):
    """``(Phi float64 [n, U + 1, U + 1, C], used int64 [U])`` by enumeration of all feature subsets."""
    Xb = np.asarray(Xb)
    rows = np.arange(Xb.shape[0]) if rows is None else np.asarray(rows)
    T, K = forest.n_trees, forest.K
    w = np.ones(T) if tree_weight is None else np.asarray(tree_weight, np.float64)
    tout = np.zeros(T, np.int64) if tree_out is None else np.asarray(tree_out, np.int64)
    C = int(n_out) if n_out is not None else (int(tout.max()) if T else 0) + K
    used = O.used_features(forest)
    U = used.size
    phi = O.shap_oracle(forest, Xb, rows, tree_weight, tree_out, n_out)[0]
    masks = np.arange(1 << U, dtype=np.int64)
    pop = np.zeros(masks.size, np.int64)
    for u in range(U):
        pop += (masks >> u) & 1
    fact = [math.factorial(i) for i in range(U + 1)]
    Phi = np.zeros((rows.size, U + 1, U + 1, C))
    for n, r in enumerate(rows):
        g = np.zeros((masks.size, C))
        for t in range(T):
            g[:, tout[t]:tout[t] + K] += w[t] * O._game(forest, t, Xb[r], used, masks)
        for i in range(U):
            for j in range(i + 1, U):
                bi, bj = 1 << i, 1 << j
                rest = masks[(masks & (bi | bj)) == 0]
                sw = np.asarray([fact[s] * fact[U - s - 2] / (2.0 * fact[U - 1]) for s in range(U - 1)])[pop[rest]]
                d = g[rest | bi | bj] - g[rest | bi] - g[rest | bj] + g[rest]
                Phi[n, i, j] = Phi[n, j, i] = (sw[:, None] * d).sum(0)
        for i in range(U):
            Phi[n, i, i] = phi[n, i] - Phi[n, i, :U].sum(0)
        Phi[n, U, U] = phi[n, U]
    return Phi, used


_CASES = {}


def case(name):
    """``(forest, Xb, kwargs, oracle Phi)`` of a named ``tree_shap_oracle`` case; the enumeration runs once per
    process and is shared by the CPU and the GPU tests."""
    if name not in _CASES:
        forest, Xb, kw, _ = O.case(name)
        _CASES[name] = (forest, Xb, kw, interaction_oracle(forest, Xb, **kw)[0])
    return _CASES[name]

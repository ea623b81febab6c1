"""Exact partial dependence (PDP) and individual conditional expectation (ICE) curves of a fitted workflow's tree
model: how the score moves as one column of the feature vector moves over the model's own bin grid, every other
column as the records have it. Beyond the reference (it has ``ModelInsights``' one number per column, no curves).

:func:`partial_dependence` scores the data up to the model's feature vector, samples rows, resolves the requested
features to vector columns and asks the learner (``Learner.partial_dependence`` -> ``tree_engine``'s
``forest_partial_dependence``: one step function per tree path, no rescoring). The grid of a column is the complete
set of its bins, so the curve is exact for the model -- there is no grid resolution to choose.

:func:`partial_dependence_pairs` does the same for pairs of columns: the surface of the score over the product of
the two columns' bin grids (``forest_partial_dependence_pairs``: rectangles of one leaf below the tree paths), and
Friedman and Popescu's H-statistic per pair, the share of the surface's variance that the two 1-D curves do not
explain."""
from __future__ import annotations

import itertools
import json
from dataclasses import asdict, dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .model_insights import _NONFINITE, _clean


@dataclass
class GridPoint:
    """One bin of a column: the values in ``(lower, upper]`` (the missing bin: ``missing``, no edges)."""
    bin: int
    lower: Optional[float]
    upper: Optional[float]
    missing: bool
    count: int                      # rows of the sample that sit in this bin
    values: List[float]             # the averaged score per output column


@dataclass
class ColumnDependence:
    index: int                      # column of the feature vector
    name: str
    parentFeature: List[str]
    indicatorValue: Optional[str]
    descriptorValue: Optional[str]
    grid: List[GridPoint]


@dataclass
class PartialDependence:
    learner: str
    scale: str                      # "response": probabilities / prediction; "raw": what shap_values attributes
    rows: int                       # sampled rows the curves average over
    seed: int
    columns: List[ColumnDependence]
    ice: Optional[torch.Tensor] = field(default=None, repr=False)           # [rows, Q, NB, C'], not in the JSON
    ice_valid: Optional[torch.Tensor] = field(default=None, repr=False)     # [Q, NB]: the grid points of `columns`
    row_ids: Optional[torch.Tensor] = field(default=None, repr=False)       # the sampled rows (None: all)

    def to_json_dict(self) -> Dict[str, Any]:
        return _clean({"learner": self.learner, "scale": self.scale, "rows": self.rows, "seed": self.seed,
                       "columns": [asdict(c) for c in self.columns]})

    def to_json(self, pretty: bool = True) -> str:
        return json.dumps(self.to_json_dict(), indent=2 if pretty else None)

    @staticmethod
    def from_json(s: Union[str, Dict]) -> "PartialDependence":
        d = json.loads(s) if isinstance(s, str) else s

        return PartialDependence(d["learner"], d["scale"], int(d["rows"]), int(d["seed"]),
                                 [_column_from_json(c) for c in d["columns"]])


def _column_from_json(c) -> ColumnDependence:
    def num(v):
        return _NONFINITE[v] if isinstance(v, str) and v in _NONFINITE else v

    return ColumnDependence(c["index"], c["name"], list(c["parentFeature"]), c.get("indicatorValue"),
                            c.get("descriptorValue"),
                            [GridPoint(g["bin"], num(g["lower"]), num(g["upper"]), bool(g["missing"]),
                                       int(g["count"]), [num(v) for v in g["values"]]) for g in c["grid"]])


@dataclass
class PairSurface:
    """The surface of one pair of columns over the product of their grids. ``a`` and ``b`` carry the axes (valid
    bins only) with the columns' own 1-D curves; ``values[i][j]`` is the averaged score per output column with ``a``
    at its ``i``-th grid point and ``b`` at its ``j``-th, ``counts[i][j]`` the rows of the sample in that cell."""
    a: ColumnDependence
    b: ColumnDependence
    values: List[List[List[float]]]
    counts: List[List[int]]
    h_statistic: List[float]        # Friedman's H per output column: 0 additive, 1 pure interaction


@dataclass
class PairDependence:
    learner: str
    scale: str                      # "response": probabilities / prediction; "raw": what shap_values attributes
    rows: int                       # sampled rows the surfaces average over
    seed: int
    pairs: List[PairSurface]
    row_ids: Optional[torch.Tensor] = field(default=None, repr=False)       # the sampled rows (None: all)

    def to_json_dict(self) -> Dict[str, Any]:
        return _clean({"learner": self.learner, "scale": self.scale, "rows": self.rows, "seed": self.seed,
                       "pairs": [asdict(p) for p in self.pairs]})

    def to_json(self, pretty: bool = True) -> str:
        return json.dumps(self.to_json_dict(), indent=2 if pretty else None)

    @staticmethod
    def from_json(s: Union[str, Dict]) -> "PairDependence":
        d = json.loads(s) if isinstance(s, str) else s

        def num(v):
            return _NONFINITE[v] if isinstance(v, str) and v in _NONFINITE else v

        pairs = [PairSurface(_column_from_json(p["a"]), _column_from_json(p["b"]),
                             [[[num(v) for v in cell] for cell in line] for line in p["values"]],
                             [[int(c) for c in line] for line in p["counts"]], [num(v) for v in p["h_statistic"]])
                 for p in d["pairs"]]
        return PairDependence(d["learner"], d["scale"], int(d["rows"]), int(d["seed"]), pairs)


def _prediction_stage(model, feature):
    if feature is None:
        feature = next((f for f in model.result_features if f.wtype.__name__ == "Prediction"), None)
    if feature is None:
        raise ValueError("No prediction feature in the workflow model: name the feature to explain")
    st = next((s for s in model.stages if feature.origin_stage is not None and s.uid == feature.origin_stage.uid),
              None)
    if st is None:
        raise ValueError(f"Feature '{feature.name}' is either a raw feature or not part of this workflow model")
    return st


def resolve_columns(features: Sequence, history: List[dict]) -> List[int]:
    """Vector columns of ``features``: an int is a column index, a string a raw feature's name (every column derived
    from it, by the column history's origins) or a column's own name. Order kept, duplicates dropped."""
    out: List[int] = []
    for f in features:
        if isinstance(f, (int, np.integer)):
            if not 0 <= int(f) < len(history):
                raise ValueError(f"column {int(f)} is outside the feature vector of {len(history)} columns")
            hit = [int(f)]
        else:
            name = getattr(f, "name", f)
            hit = [h["index"] for h in history
                   if name in h["parentFeatureOrigins"] or name in h["parentFeatureName"] or name == h["columnName"]]
            if not hit:
                raise ValueError(f"no column of the feature vector derives from '{name}'")
        out += [c for c in hit if c not in out]
    return out


def partial_dependence(model, data=None, features: Optional[Sequence] = None, top_k: int = 10,
                       scale: str = "response", sample: Optional[int] = 10_000, seed: int = 0, ice: bool = False,
                       feature=None) -> PartialDependence:
    """Partial dependence of the selected tree model of a fitted workflow ``model`` on ``data`` (None: the model's
    own input). ``features``: raw feature names (every vector column derived from them) and / or vector column
    indices; None takes the ``top_k`` columns by the learner's ``feature_contributions``. ``scale``: ``"response"``
    (probabilities, a regressor's prediction) or ``"raw"`` (margins / vote sums, as ``shap_values`` attributes them).
    At most ``sample`` rows are used, drawn with a generator seeded by ``seed`` (None: every row). ``ice=True`` keeps
    the per-record curves in ``result.ice`` (``rows * Q * NB * C' * 8`` bytes). ``feature``: the prediction feature
    to explain when the model has several. A model that is not a tree learner is a ``ValueError``."""
    learner, state, name, X, history, rows, n = _sampled_input(model, data, sample, seed, feature)
    cols = _top_columns(learner, state, name, int(X.shape[1]), top_k) if features is None else \
        resolve_columns(features, history)
    if not cols:
        raise ValueError("no column to compute the partial dependence of")
    values, valid, counts, curves = learner.partial_dependence(state, X, cols, rows, None, scale, ice)
    spec = learner._forest(state)[1]
    values, valid_c, counts = values.cpu().numpy(), valid.cpu().numpy(), counts.cpu().numpy()
    out = [_column_dependence(c, history, spec, valid_c[q], counts[q], values[q]) for q, c in enumerate(cols)]
    return PartialDependence(str(name), scale, n if rows is None else int(rows.numel()), int(seed), out,
                             curves, valid if ice else None, rows)


def _sampled_input(model, data, sample, seed, feature):
    """What both public functions start from: ``(learner, state, its name, the feature vector X, its column
    history, the sampled rows or None, n rows of X)``. A model that is not a tree learner is a ``ValueError``."""
    from ..models.base import Learner
    st = _prediction_stage(model, feature)
    learner, state = getattr(st, "learner", None), getattr(st, "state", None)
    name = getattr(learner, "name", None) or getattr(st, "learner_name", None) or type(st).__name__
    if learner is None or state is None or \
            getattr(type(learner), "partial_dependence", Learner.partial_dependence) is Learner.partial_dependence:
        raise ValueError(f"partial dependence needs a tree learner; the selected model is {name}")
    vec = st._inputs[-1]
    scored = model.score(data, keep_intermediate_features=True)
    col = scored[vec.name]
    X, history = col.values, col.metadata.column_history()
    n = int(X.shape[0])
    rows = None
    if sample is not None and n > int(sample):
        g = torch.Generator().manual_seed(int(seed))
        rows = torch.sort(torch.randperm(n, generator=g)[:int(sample)]).values
    return learner, state, name, X, history, rows, n


def _top_columns(learner, state, name, d: int, top_k: int) -> List[int]:
    contrib = learner.feature_contributions(state, d)
    if contrib is None:
        raise ValueError(f"{name} has no feature contributions: name the features")
    c = np.abs(np.asarray(contrib, np.float64))
    c = c.sum(0) if c.ndim > 1 else c
    order = np.argsort(-c, kind="stable")
    return [int(i) for i in order[:max(0, int(top_k))] if c[i] > 0]


def _column_dependence(c: int, history, spec, valid, counts, values) -> ColumnDependence:
    """Column ``c`` with its valid grid points: ``valid`` / ``counts`` ``[NB]``, ``values`` ``[NB, C']`` (numpy)."""
    h, nt = history[c], int(spec.n_thresh[c])
    grid = []
    for b in np.nonzero(valid)[0]:
        b = int(b)
        missing = spec.missing_bin >= 0 and b == spec.missing_bin
        lower = None if missing else (float("-inf") if b == 0 else float(spec.thresholds[c, b - 1]))
        upper = None if missing else (float("inf") if b >= nt else float(spec.thresholds[c, b]))
        grid.append(GridPoint(b, lower, upper, bool(missing), int(counts[b]), [float(v) for v in values[b]]))
    return ColumnDependence(c, h["columnName"], list(h["parentFeatureName"]), h["indicatorValue"],
                            h["descriptorValue"], grid)


def h_statistic(surface: torch.Tensor, counts: torch.Tensor, curve_a: torch.Tensor, curve_b: torch.Tensor,
                counts_a: torch.Tensor, counts_b: torch.Tensor) -> torch.Tensor:
    """Friedman and Popescu's H of one pair, per output column ``[C']``: with the cell counts ``w_ij`` of the sample,
    ``F_ab`` the surface ``[NB, NB, C']`` centred by its ``w``-weighted mean and ``F_a`` / ``F_b`` the 1-D curves
    ``[NB, C']`` centred by their count-weighted means, ``H^2 = sum w (F_ab - F_a - F_b)^2 / sum w F_ab^2``;
    0.0 where the denominator is 0 (a flat surface)."""
    def centred(f, w):
        w = w.to(torch.float64).reshape(w.shape + (1,))
        return f - (w * f).sum(tuple(range(w.dim() - 1))) / w.sum(), w

    f_ab, w = centred(surface, counts)
    f_a, f_b = centred(curve_a, counts_a)[0], centred(curve_b, counts_b)[0]
    num = (w * (f_ab - f_a[:, None, :] - f_b[None, :, :]) ** 2).sum((0, 1))
    den = (w * f_ab ** 2).sum((0, 1))
    return torch.where(den > 0, torch.sqrt(num / den.clamp_min(torch.finfo(torch.float64).tiny)), torch.zeros_like(den))


def resolve_pairs(pairs: Sequence, history: List[dict]) -> List[tuple]:
    """``[(a, b)]`` vector columns of ``pairs``, 2-tuples of column indices and / or raw feature names; a name must
    stand for exactly one column here."""
    def one(f):
        hit = resolve_columns([f], history)
        if len(hit) != 1:
            raise ValueError(f"'{getattr(f, 'name', f)}' stands for the columns {hit} of the feature vector: name "
                             "one of them by its index")
        return hit[0]

    out = []
    for p in pairs:
        if not isinstance(p, (tuple, list)) or len(p) != 2:
            raise ValueError(f"a pair is a 2-tuple of columns or feature names, got {p!r}")
        a, b = one(p[0]), one(p[1])
        if a == b:
            raise ValueError(f"the two columns of a pair must be different, got column {a} twice")
        out.append((a, b))
    return out


def partial_dependence_pairs(model, data=None, pairs: Optional[Sequence] = None, top_k: int = 4,
                             scale: str = "response", sample: Optional[int] = 10_000, seed: int = 0,
                             feature=None) -> PairDependence:
    """Two-way partial dependence of the selected tree model of a fitted workflow ``model`` on ``data`` (None: the
    model's own input): per pair of columns the surface of the averaged score over the product of the two bin grids,
    the cell counts of the sample and Friedman's H-statistic (:func:`h_statistic`, on the scale of the result, from
    the same rows). ``pairs``: 2-tuples of vector column indices and / or raw feature names that stand for one
    column each; None takes every unordered pair of the ``top_k`` columns by the learner's
    ``feature_contributions``. ``scale``, ``sample``, ``seed`` and ``feature`` are those of
    :func:`partial_dependence`. A model that is not a tree learner is a ``ValueError``."""
    learner, state, name, X, history, rows, n = _sampled_input(model, data, sample, seed, feature)
    if pairs is None:
        pq = list(itertools.combinations(_top_columns(learner, state, name, int(X.shape[1]), top_k), 2))
    else:
        pq = resolve_pairs(pairs, history)
    if not pq:
        raise ValueError("no pair of columns to compute the partial dependence of")
    cols = sorted({c for p in pq for c in p})
    values, valid, counts = learner.partial_dependence_pairs(state, X, np.asarray(pq, np.int64), rows, None, scale)
    curves, valid1, counts1, _ = learner.partial_dependence(state, X, cols, rows, None, scale)
    h = torch.stack([h_statistic(values[p], counts[p], curves[cols.index(a)], curves[cols.index(b)],
                                 counts1[cols.index(a)], counts1[cols.index(b)]) for p, (a, b) in enumerate(pq)])
    spec = learner._forest(state)[1]
    values, counts, h = values.cpu().numpy(), counts.cpu().numpy(), h.cpu().numpy()
    curves, valid1, counts1 = curves.cpu().numpy(), valid1.cpu().numpy(), counts1.cpu().numpy()
    out = []
    for p, (a, b) in enumerate(pq):
        qa, qb = cols.index(a), cols.index(b)
        ia, ib = np.nonzero(valid1[qa])[0], np.nonzero(valid1[qb])[0]
        out.append(PairSurface(_column_dependence(a, history, spec, valid1[qa], counts1[qa], curves[qa]),
                               _column_dependence(b, history, spec, valid1[qb], counts1[qb], curves[qb]),
                               [[[float(v) for v in values[p, i, j]] for j in ib] for i in ia],
                               [[int(counts[p, i, j]) for j in ib] for i in ia], [float(v) for v in h[p]]))
    return PairDependence(str(name), scale, n if rows is None else int(rows.numel()), int(seed), out, rows)

"""Exact partial dependence (PDP) and individual conditional expectation (ICE) curves of a fitted workflow's tree
model: how the score moves as one column of the feature vector moves over the model's own bin grid, every other
column as the records have it. Beyond the reference (it has ``ModelInsights``' one number per column, no curves).

:func:`partial_dependence` scores the data up to the model's feature vector, samples rows, resolves the requested
features to vector columns and asks the learner (``Learner.partial_dependence`` -> ``tree_engine``'s
``forest_partial_dependence``: one step function per tree path, no rescoring). The grid of a column is the complete
set of its bins, so the curve is exact for the model -- there is no grid resolution to choose."""
from __future__ import annotations

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

        def num(v):
            return _NONFINITE[v] if isinstance(v, str) and v in _NONFINITE else v

        cols = [ColumnDependence(c["index"], c["name"], list(c["parentFeature"]), c.get("indicatorValue"),
                                 c.get("descriptorValue"),
                                 [GridPoint(g["bin"], num(g["lower"]), num(g["upper"]), bool(g["missing"]),
                                            int(g["count"]), [num(v) for v in g["values"]]) for g in c["grid"]])
                for c in d["columns"]]
        return PartialDependence(d["learner"], d["scale"], int(d["rows"]), int(d["seed"]), cols)


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
    n, d = int(X.shape[0]), int(X.shape[1])
    rows = None
    if sample is not None and n > int(sample):
        g = torch.Generator().manual_seed(int(seed))
        rows = torch.sort(torch.randperm(n, generator=g)[:int(sample)]).values
    if features is None:
        contrib = learner.feature_contributions(state, d)
        if contrib is None:
            raise ValueError(f"{name} has no feature contributions: name the features")
        c = np.abs(np.asarray(contrib, np.float64))
        c = c.sum(0) if c.ndim > 1 else c
        order = np.argsort(-c, kind="stable")
        cols = [int(i) for i in order[:max(0, int(top_k))] if c[i] > 0]
    else:
        cols = resolve_columns(features, history)
    if not cols:
        raise ValueError("no column to compute the partial dependence of")
    values, valid, counts, curves = learner.partial_dependence(state, X, cols, rows, None, scale, ice)
    spec = learner._forest(state)[1]
    values, valid_c, counts = values.cpu().numpy(), valid.cpu().numpy(), counts.cpu().numpy()
    out = []
    for q, c in enumerate(cols):
        h, nt = history[c], int(spec.n_thresh[c])
        grid = []
        for b in np.nonzero(valid_c[q])[0]:
            b = int(b)
            missing = spec.missing_bin >= 0 and b == spec.missing_bin
            lower = None if missing else (float("-inf") if b == 0 else float(spec.thresholds[c, b - 1]))
            upper = None if missing else (float("inf") if b >= nt else float(spec.thresholds[c, b]))
            grid.append(GridPoint(b, lower, upper, bool(missing), int(counts[q, b]), [float(v) for v in values[q, b]]))
        out.append(ColumnDependence(c, h["columnName"], list(h["parentFeatureName"]), h["indicatorValue"],
                                    h["descriptorValue"], grid))
    return PartialDependence(str(name), scale, n if rows is None else int(rows.numel()), int(seed), out,
                             curves, valid if ice else None, rows)

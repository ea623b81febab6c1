"""Per-record explanations: leave-one-column-out (LOCO) and score/feature correlation insights.

Reference: ``RecordInsightsLOCO`` (``core/.../stages/impl/insights/RecordInsightsLOCO.scala:100-347``: top-K
by |score change| or top-K positive + negative, text / date column groups aggregated by ``Avg`` or
``LeaveOutVector``), ``RecordInsightsCorr`` (``RecordInsightsCorr.scala:55-220``: per-feature
correlation with each score column times the normalized feature value) and ``RecordInsightsParser``
(``insightToText`` / ``parseInsights``). SURVEY.md K30.

Device design: LOCO is computed for a whole block of records at once. Every (record, non-zero
column) perturbation becomes one row of a perturbed batch scored by the model's vectorized predict
(for linear models the batch is never materialized: the perturbed margin is ``m_i - w_j x_ij``, an
elementwise [rows, d] tensor op); top-K selection per record is ``torch.topk`` over the
[rows, candidates] score-change matrix. Only the final ``TextMap`` strings are built on the host.
For tree models ``perturbation="paths"`` replaces the perturbed batches by exact path perturbation
(``tree_engine.forest_loco``, HIP kernel ``ops/csrc/hip/loco_kernels.hip``): a zeroed column can change a tree's
answer only where it is tested on the record's own path, so only those path suffixes are walked again.

Beyond the reference: ``RecordInsightsSHAP`` explains tree models with exact path-dependent TreeSHAP
(``tree_engine.forest_shap``, HIP kernel ``ops/csrc/hip/shap_kernels.hip``) instead of perturbing columns, and
``RecordInsightsSHAPInteractions`` splits those attributions into main effects and pair effects (exact SHAP
interaction values, ``tree_engine.forest_shap_interactions``, the second kernel of the same file).
"""
from __future__ import annotations

import json
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...data.columns import ObjectColumn, PredictionColumn, VectorColumn
from ...features import types as T
from ..base import BinaryEstimator, BinaryTransformer, UnaryTransformer, register_stage

TEXT_TYPES = {"Text", "TextArea", "TextList", "TextMap", "TextAreaMap"}
DATE_TYPES = {"Date", "DateTime", "DateMap", "DateTimeMap"}
TIME_PERIODS = ("DayOfMonth", "DayOfWeek", "DayOfYear", "HourOfDay", "MonthOfYear", "WeekOfMonth", "WeekOfYear")


# ------------------------------------------------------------------------------------------- parser
def insight_to_text(column_info: str, score_diffs) -> Tuple[str, str]:
    scores = [[i, float(s)] for i, s in enumerate(score_diffs)]
    return column_info, json.dumps(scores, separators=(",", ":"))


def parse_insights(insights: Dict[str, str]) -> Dict[str, List[Tuple[int, float]]]:
    """``RecordInsightsParser.parseInsights``: column-history JSON -> [(score index, value)]."""
    out = {}
    for k, v in (insights or {}).items():
        hist = json.loads(k)
        key = hist.get("columnName", k)
        out[key] = [(int(a), float(b)) for a, b in json.loads(v)]
    return out


def _short(t: str) -> str:
    return t.rsplit(".", 1)[-1]


def _history_json(h: dict) -> str:
    return json.dumps(h, separators=(",", ":"), sort_keys=False)


def _jf(x: float) -> str:
    """A float as ``json.dumps`` writes it (repr; NaN / Infinity for the non-finite)."""
    return repr(x) if math.isfinite(x) else json.dumps(x)


class InsightsColumn(ObjectColumn):
    """``TextMap`` column of record insights kept as device tensors -- column index [n, K] (-1 = none),
    score changes [n, K, C] and the vector's column-history keys -- and rendered to the reference's
    ``{columnHistory JSON: "[[scoreIndex, diff], ...]"}`` maps only when rows are read on the host."""

    def __init__(self, cols: torch.Tensor, diffs: torch.Tensor, keys: Sequence[str]):
        self.ftype = T.TextMap
        self.cols, self.diffs, self.keys = cols, diffs, list(keys)
        self._values = None

    @property
    def values(self):
        if self._values is None:
            cols = self.cols.cpu().numpy()
            diffs = self.diffs.cpu().numpy()
            arr = np.empty(cols.shape[0], dtype=object)
            for i in range(cols.shape[0]):
                arr[i] = self._render(cols[i], diffs[i])
            self._values = arr
        return self._values

    @values.setter
    def values(self, v):
        self._values = v

    def _render(self, cols, diffs) -> Dict[str, str]:
        return {self.keys[c]: "[" + ",".join(f"[{j},{_jf(x)}]" for j, x in enumerate(dv)) + "]"
                for c, dv in zip(cols.tolist(), diffs.tolist()) if c >= 0}

    def __len__(self):
        return int(self.cols.shape[0])

    @property
    def device(self):
        return self.cols.device

    def take(self, idx):
        i = idx.to(self.cols.device, torch.long) if isinstance(idx, torch.Tensor) else \
            torch.as_tensor(np.asarray(idx, np.int64), device=self.cols.device)
        return InsightsColumn(self.cols.index_select(0, i), self.diffs.index_select(0, i), self.keys)

    def to(self, device):
        return InsightsColumn(self.cols.to(device), self.diffs.to(device), self.keys)

    def row(self, i):
        if self._values is not None:
            return self._values[i]
        return self._render(self.cols[i].cpu().numpy(), self.diffs[i].cpu().numpy())

    def null_mask(self):
        return ~(self.cols >= 0).any(1).cpu()

    @classmethod
    def _concat(cls, cols):
        if all(isinstance(c, InsightsColumn) and c.keys == cols[0].keys and c.diffs.shape[1:] == cols[0].diffs.shape[1:]
               for c in cols):
            return InsightsColumn(torch.cat([c.cols for c in cols]), torch.cat([c.diffs for c in cols]), cols[0].keys)
        return ObjectColumn(T.TextMap, np.concatenate([c.values for c in cols]))


class PairInsightsColumn(InsightsColumn):
    """``InsightsColumn`` whose insights are column pairs: column indices ``[n, K, 2]`` (smaller first, -1 = none),
    pair effects ``[n, K, C]``; a key is the JSON array of the two columns' history objects."""

    def _render(self, cols, diffs) -> Dict[str, str]:
        return {"[" + self.keys[a] + "," + self.keys[b] + "]":
                "[" + ",".join(f"[{j},{_jf(x)}]" for j, x in enumerate(dv)) + "]"
                for (a, b), dv in zip(cols.tolist(), diffs.tolist()) if a >= 0}

    def take(self, idx):
        i = idx.to(self.cols.device, torch.long) if isinstance(idx, torch.Tensor) else \
            torch.as_tensor(np.asarray(idx, np.int64), device=self.cols.device)
        return PairInsightsColumn(self.cols.index_select(0, i), self.diffs.index_select(0, i), self.keys)

    def to(self, device):
        return PairInsightsColumn(self.cols.to(device), self.diffs.to(device), self.keys)

    def null_mask(self):
        return ~(self.cols[:, :, 0] >= 0).any(1).cpu()

    @classmethod
    def _concat(cls, cols):
        if all(isinstance(c, PairInsightsColumn) and c.keys == cols[0].keys
               and c.diffs.shape[1:] == cols[0].diffs.shape[1:] for c in cols):
            return PairInsightsColumn(torch.cat([c.cols for c in cols]), torch.cat([c.diffs for c in cols]),
                                      cols[0].keys)
        return ObjectColumn(T.TextMap, np.concatenate([c.values for c in cols]))


def parse_interaction_insights(insights: Dict[str, str]) -> Dict[Tuple[str, str], List[Tuple[int, float]]]:
    """The inverse of ``RecordInsightsSHAPInteractions``' rendering: [history A, history B] JSON ->
    ``{(column name A, column name B): [(score index, value)]}``."""
    out = {}
    for k, v in (insights or {}).items():
        a, b = json.loads(k)
        out[a.get("columnName"), b.get("columnName")] = [(int(i), float(x)) for i, x in json.loads(v)]
    return out


# ---------------------------------------------------------------------------------------------- LOCO
@register_stage
class RecordInsightsLOCO(UnaryTransformer):
    """Unary (OPVector -> TextMap) transformer wrapping a fitted prediction model stage."""
    operation_name = "recordInsightsLOCO"
    output_type = T.TextMap
    _defaults = {"top_k": 20, "top_k_strategy": "abs", "vector_aggregation_strategy": "Avg",
                 "perturbation": "rescore"}
    PERTURBATIONS = ("rescore", "paths", "auto")

    def __init__(self, model=None, uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.model = model
        self.histories: Optional[List[dict]] = None
        self.chunk_elems = 1 << 22

    # -- model access
    def _learner_state(self):
        m = self.model
        return m.learner, m.state

    def _scores(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(score matrix [n, C], predicted class [n])."""
        learner, state = self._learner_state()
        pred, raw, prob = learner.predict(state, X)
        if prob.shape[1] > 0:
            s = prob
        else:
            s = pred.reshape(-1, 1)
        return s.to(torch.float64), pred.reshape(-1)

    def _use_paths(self) -> bool:
        """``perturbation``: ``rescore`` (default) scores one perturbed copy of the record per non-zero column;
        ``paths`` asks the learner for exact LOCO scores by tree-path perturbation (``Learner.loco_scores``, tree
        learners: ``tree_engine.forest_loco``) and is an error for a learner without them; ``auto`` takes paths
        where the learner has them and rescores otherwise."""
        mode = self.params.get("perturbation", "rescore")
        if mode not in self.PERTURBATIONS:
            raise ValueError(f"perturbation must be one of {self.PERTURBATIONS}, got {mode!r}")
        if mode == "rescore":
            return False
        from ...models.base import Learner
        learner = self._learner_state()[0]
        has = getattr(type(learner), "loco_scores", Learner.loco_scores) is not Learner.loco_scores
        if mode == "paths" and not has:
            raise ValueError(f"perturbation='paths' needs a tree learner with loco_scores, "
                             f"{getattr(learner, 'name', type(learner).__name__)} has none (use 'rescore' or 'auto')")
        return has

    def _paths_diffs(self, X: torch.Tensor, gcols):
        """Score changes from the learner's path-perturbation LOCO: (per used column [n, U, C], per column group
        [n, G, C], used columns [U])."""
        learner, state = self._learner_state()
        base, pert, used = learner.loco_scores(state, X, groups=[g.cpu().numpy() for g in gcols])
        diff = base[:, None, :] - pert
        U = len(used)
        return diff[:, :U], diff[:, U:], torch.as_tensor(np.asarray(used, np.int64), device=X.device)

    # -- groups of columns aggregated as one insight (text hashes, date unit circles)
    def _groups(self, hist: List[dict]):
        groups: Dict[str, List[int]] = {}
        for j, h in enumerate(hist):
            types = {_short(t) for t in h.get("parentFeatureType", [])}
            is_text = bool(types & TEXT_TYPES) and h.get("indicatorValue") is None and h.get("descriptorValue") is None
            is_date = bool(types & DATE_TYPES) and h.get("descriptorValue") is not None
            if not (is_text or is_date):
                continue
            origins = h.get("parentFeatureOrigins") or h.get("parentFeatureName") or [""]
            name = origins[0] + ("_" + h["grouping"] if h.get("grouping") else "")
            if is_date:
                tp = str(h.get("descriptorValue")).split("_")[-1]
                if tp.lower() in {p.lower() for p in TIME_PERIODS}:
                    name += "_" + next(p for p in TIME_PERIODS if p.lower() == tp.lower())
            groups.setdefault(name, []).append(j)
        return groups

    def _plan(self, hist: List[dict], d: int, device):
        """Candidate layout of one vector width: plain columns first (in column order), then one
        candidate per column group. Returns (cand_of_col [d], group size per candidate [m], plain
        column per candidate (-1 for groups) [m], group column tensors)."""
        groups = self._groups(hist)
        in_group = torch.zeros(d, dtype=torch.bool)
        for cols in groups.values():
            in_group[cols] = True
        plain = torch.nonzero(~in_group).flatten()
        n_plain = int(plain.numel())
        cand_of_col = torch.empty(d, dtype=torch.long)
        cand_of_col[plain] = torch.arange(n_plain)
        gsize = [1.0] * n_plain
        gcols = []
        for g, cols in enumerate(groups.values()):
            cand_of_col[torch.as_tensor(cols)] = n_plain + g
            gsize.append(float(len(cols)))
            gcols.append(torch.as_tensor(cols, device=device))
        plain_col = torch.cat([plain, torch.full((len(gcols),), -1, dtype=torch.long)])
        return (cand_of_col.to(device), torch.as_tensor(gsize, dtype=torch.float64, device=device),
                plain_col.to(device), gcols)

    def _rescore_changes(self, X, nz, base, cand_of_col, gsize):
        """``[n * m, C]`` score changes of the rescore mode: one perturbed copy per (record, non-zero column),
        scored in bounded chunks, its change added to the column's candidate (divided by the group size)."""
        n, d = X.shape
        dev = X.device
        m, C = int(gsize.numel()), base.shape[1]
        rows, cols = torch.nonzero(nz, as_tuple=True)
        V = torch.zeros(n * m, C, dtype=torch.float64, device=dev)
        cand = cand_of_col[cols]
        step = max(1, self.chunk_elems // max(d, 1))
        ar = torch.arange(min(step, rows.numel()), device=dev)
        for a in range(0, rows.numel(), step):
            r, c = rows[a:a + step], cols[a:a + step]
            Xp = X.index_select(0, r)
            Xp[ar[:r.numel()], c] = 0
            s, _ = self._scores(Xp)
            ca = cand[a:a + step]
            V.index_add_(0, r * m + ca, (base.index_select(0, r) - s) / gsize[ca][:, None])
        return V

    def _loco_block(self, X: torch.Tensor, hist: List[dict], plan=None):
        """Top-K score changes of one block of records, all on the device: (column [n, K] (-1 = no
        insight), diffs [n, K, C]). Every (record, non-zero column) perturbation is one row of a perturbed
        batch; its score change is scattered into the record's candidate (the column itself, or its
        text / date group: ``Avg`` divides the group sum by the group size, ``LeaveOutVector`` re-scores
        the record with the whole group zeroed), then the top-K positive and negative candidates are
        merged and ordered per record by one stable sort (``RecordInsightsLOCO.scala:246-273``). In paths mode
        (:meth:`_use_paths`) the score changes come from ``Learner.loco_scores`` instead of perturbed batches --
        a column the trees do not split on changes nothing -- and everything after them is the same code."""
        n, d = X.shape
        dev = X.device
        paths = self._use_paths()
        base, pred_cls = self._scores(X)
        C = base.shape[1]
        if C == 0:
            raise RuntimeError("model does not produce scores for insights")
        if C == 1:
            ex = torch.zeros(n, dtype=torch.long, device=dev)
        elif C == 2:
            ex = torch.ones(n, dtype=torch.long, device=dev)
        else:
            ex = pred_cls.to(torch.long)
        cand_of_col, gsize, plain_col, gcols = plan if plan is not None else self._plan(hist, d, dev)
        m = int(gsize.numel())
        k = int(self.params["top_k"])
        abs_mode = self.params["top_k_strategy"] == "abs"
        kk = min(k, m)
        K = min(k if abs_mode else 2 * k, 2 * kk)
        if m == 0 or n == 0:
            return (torch.full((n, K), -1, dtype=torch.long, device=dev),
                    torch.zeros(n, K, C, dtype=torch.float64, device=dev))
        nz = X != 0
        if paths:
            col_diff, group_diff, used = self._paths_diffs(X, gcols)
            cu = cand_of_col[used]
            V = torch.zeros(n, m, C, dtype=torch.float64, device=dev)
            V.index_add_(1, cu, col_diff / gsize[cu][None, :, None])
        else:
            V = self._rescore_changes(X, nz, base, cand_of_col, gsize).view(n, m, C)
        Cc = plain_col[None, :].expand(n, m).clone()
        n_plain = m - len(gcols)
        leave_out = self.params["vector_aggregation_strategy"] != "Avg"
        for g, gct in enumerate(gcols):
            active = nz[:, gct]
            has = active.any(1)
            Cc[:, n_plain + g] = torch.where(has, gct[active.to(torch.int8).argmax(1)], torch.full_like(has, -1,
                                                                                                    dtype=torch.long))
            if leave_out and paths:
                V[:, n_plain + g] = torch.where(has[:, None], group_diff[:, g], torch.zeros_like(base))
            elif leave_out:     # LeaveOutVector: zero every active column of the group at once
                Xp = X.clone()
                Xp[:, gct] = 0
                s, _ = self._scores(Xp)
                V[:, n_plain + g] = torch.where(has[:, None], base - s, torch.zeros_like(base))
        val = V.gather(2, ex.view(n, 1, 1).expand(n, m, 1)).squeeze(2)
        valid = (Cc >= 0) & (val != 0)
        ninf = torch.full_like(val, -float("inf"))
        pv, pi = torch.topk(torch.where(valid & (val > 0), val, ninf), kk, dim=1)
        nv, ni = torch.topk(torch.where(valid & (val < 0), -val, ninf), kk, dim=1)
        idx = torch.cat([pi, ni], 1)                                   # positives first, then negatives
        ok = torch.cat([pv, nv], 1) != -float("inf")
        v = val.gather(1, idx)
        key = torch.where(ok, v.abs() if abs_mode else v, torch.full_like(v, -float("inf")))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :K]
        sel = idx.gather(1, order)
        okK = ok.gather(1, order)
        colsK = torch.where(okK, Cc.gather(1, sel), torch.full_like(sel, -1))
        diffsK = V.gather(1, sel[:, :, None].expand(n, K, C))
        return colsK, diffsK

    def _run(self, X: torch.Tensor, hist: List[dict]):
        n, d = X.shape
        plan = self._plan(hist, d, X.device)
        m, C = max(int(plan[1].numel()), 1), 2
        block = max(64, (1 << 23) // (m * C))
        parts = [self._loco_block(X[a:a + block], hist, plan) for a in range(0, n, block)] or \
            [self._loco_block(X[:0], hist, plan)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def transform_columns(self, *cols, ds=None):
        vec: VectorColumn = cols[0]
        if vec.metadata is not None:
            self.histories = vec.metadata.column_history()
        hist = self.histories
        if hist is None:
            raise ValueError("RecordInsightsLOCO needs the input vector metadata (column histories)")
        cidx, diffs = self._run(vec.values, hist)
        return InsightsColumn(cidx, diffs, [_history_json(h) for h in hist])

    def transform_row(self, *values):
        x = torch.as_tensor(np.asarray(values[0], np.float64))[None, :]
        if self.histories is None:
            raise ValueError("RecordInsightsLOCO has not seen vector metadata yet")
        cidx, diffs = self._loco_block(x, self.histories)
        return InsightsColumn(cidx, diffs, [_history_json(h) for h in self.histories]).row(0)

    def ctor_args(self):
        from ...workflow.io import stage_to_json
        return {"model": stage_to_json(self.model) if self.model is not None else None,
                "histories": self.histories, "perturbation": self.params.get("perturbation", "rescore")}

    def load_ctor_args(self, a):
        from ...workflow.io import _build_stage
        self.model = _build_stage(a["model"]) if a.get("model") else None
        self.histories = a.get("histories")
        if a.get("perturbation") is not None:
            self.params["perturbation"] = a["perturbation"]


# ---------------------------------------------------------------------------------------------- SHAP
@register_stage
class RecordInsightsSHAP(RecordInsightsLOCO):
    """Unary (OPVector -> TextMap) transformer wrapping a fitted tree model stage: exact path-dependent
    TreeSHAP attributions of the model's additive score (the raw class-vote sums of a forest, the margin
    of a boosted model; beyond the reference, which only has LOCO). The insights of a record plus the bias
    add up to its raw prediction. Candidates come from the columns the trees split on; a text / date
    column group (the grouping of ``RecordInsightsLOCO``) is one candidate worth the sum of its members --
    SHAP is additive, so there is no aggregation strategy -- reported under its first active column (its
    first split column when the record has none). Top-K selection is LOCO's, by the same score column."""
    operation_name = "recordInsightsSHAP"
    _defaults = {"top_k": 20, "top_k_strategy": "abs", "perturbation": "rescore"}    # perturbation: ignored

    def _shap(self, X: torch.Tensor, context=None):
        learner, state = self._learner_state()
        try:
            return learner.shap_values(state, X, None, context)
        except NotImplementedError as e:
            raise ValueError(f"RecordInsightsSHAP needs a tree model: {e}") from e

    def _shap_plan(self, hist: List[dict], used: np.ndarray, device):
        """Candidates over the used columns: plain used columns first (in column order), then one per column
        group with a used member. Returns (candidate of used slot [U], plain column per candidate (-1 for
        groups) [m], per group (all its columns, its first used column))."""
        member = {}
        for g, cols in enumerate(self._groups(hist).values()):
            for c in cols:
                member[c] = (g, cols)
        plain = [int(c) for c in used if int(c) not in member]
        gids: Dict[int, int] = {}
        gcols = []
        cand = np.empty(len(used), np.int64)
        k = 0
        for u, c in enumerate(int(c) for c in used):
            if c not in member:
                cand[u] = k
                k += 1
                continue
            g, cols = member[c]
            if g not in gids:
                gids[g] = len(plain) + len(gcols)
                gcols.append((torch.as_tensor(cols, device=device), c))
            cand[u] = gids[g]
        plain_col = torch.as_tensor(plain + [-1] * len(gcols), dtype=torch.long, device=device)
        return torch.as_tensor(cand, device=device), plain_col, gcols

    def _shap_block(self, X: torch.Tensor, hist: List[dict]):
        """Top-K attributions of one block of records: (column [n, K] (-1 = no insight), phi [n, K, C]).
        The selection is ``_loco_block``'s -- top-K positive and negative candidates by the selecting score
        column, merged by one stable sort -- except that a candidate whose attribution is 0 in the selecting
        column but not in another one (a column only another class's trees split on) counts as a positive
        of strength 0, so that all insights of a record still add up to its score."""
        n = X.shape[0]
        dev = X.device
        phi, used = self._shap(X)
        U, C = phi.shape[1] - 1, phi.shape[2]
        ex = self._score_column(X, C)
        cand, plain_col, gcols = self._shap_plan(hist, used, dev)
        m = int(plain_col.numel())
        K = self._top_width(m)
        if m == 0 or n == 0:
            return (torch.full((n, K), -1, dtype=torch.long, device=dev),
                    torch.zeros(n, K, C, dtype=torch.float64, device=dev))
        V = torch.zeros(n, m, C, dtype=torch.float64, device=dev)
        V.index_add_(1, cand, phi[:, :U])
        Cc = self._reported_columns(X, plain_col, gcols)
        sel, okK = self._top_candidates(V, ex)
        colsK = torch.where(okK, Cc.gather(1, sel), torch.full_like(sel, -1))
        diffsK = V.gather(1, sel[:, :, None].expand(n, K, C))
        return colsK, diffsK

    def _score_column(self, X: torch.Tensor, C: int) -> torch.Tensor:
        """The score column candidates are ranked by, per record ``[n]`` (LOCO's choice: the only one, the
        positive class, the predicted class)."""
        n, dev = X.shape[0], X.device
        if C == 1:
            return torch.zeros(n, dtype=torch.long, device=dev)
        if C == 2:
            return torch.ones(n, dtype=torch.long, device=dev)
        learner, state = self._learner_state()
        return learner.predict(state, X)[0].reshape(-1).to(torch.long)

    def _top_width(self, m: int) -> int:
        """Insights per record when there are ``m`` candidates."""
        k = int(self.params["top_k"])
        return min(k if self.params["top_k_strategy"] == "abs" else 2 * k, 2 * min(k, m))

    def _reported_columns(self, X: torch.Tensor, plain_col: torch.Tensor, gcols) -> torch.Tensor:
        """The column every candidate is reported under, per record ``[n, m]``: a plain candidate's own column,
        a group's first active column (its first split column when the record has none)."""
        n, m, dev = X.shape[0], int(plain_col.numel()), X.device
        Cc = plain_col[None, :].expand(n, m).clone()
        n_plain = m - len(gcols)
        for g, (gct, first_used) in enumerate(gcols):
            active = X[:, gct] != 0
            Cc[:, n_plain + g] = torch.where(active.any(1), gct[active.to(torch.int8).argmax(1)],
                                             torch.full((n,), first_used, dtype=torch.long, device=dev))
        return Cc

    def _top_candidates(self, V: torch.Tensor, ex: torch.Tensor):
        """The selection of :meth:`_shap_block` over the attributions ``V [n, m, C]`` by the score column ``ex``:
        (selected candidate [n, K], whether the slot holds one [n, K])."""
        n, m, C = V.shape
        kk = min(int(self.params["top_k"]), m)
        K = self._top_width(m)
        abs_mode = self.params["top_k_strategy"] == "abs"
        val = V.gather(2, ex.view(n, 1, 1).expand(n, m, 1)).squeeze(2)
        valid = (V != 0).any(2)
        ninf = torch.full_like(val, -float("inf"))
        pv, pi = torch.topk(torch.where(valid & (val >= 0), val, ninf), kk, dim=1)
        nv, ni = torch.topk(torch.where(valid & (val < 0), -val, ninf), kk, dim=1)
        idx = torch.cat([pi, ni], 1)                                   # positives first, then negatives
        ok = torch.cat([pv, nv], 1) != -float("inf")
        v = val.gather(1, idx)
        key = torch.where(ok, v.abs() if abs_mode else v, torch.full_like(v, -float("inf")))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :K]
        return idx.gather(1, order), ok.gather(1, order)

    def bias(self, X: torch.Tensor) -> torch.Tensor:
        """The attribution's bias per score column, ``[C]``: what the insights of a record add up from."""
        return self._shap(X[:1])[0][0, -1]

    def _run(self, X: torch.Tensor, hist: List[dict]):
        n, d = X.shape
        learner, state = self._learner_state()
        # [block, U + 1, C] stays bounded: U <= d, C <= the class count (2 score columns for a binary model)
        block = max(64, (1 << 23) // ((d + 1) * max(2, int(learner.n_classes(state)))))
        parts = [self._shap_block(X[a:a + block], hist) for a in range(0, n, block)] or \
            [self._shap_block(X[:0], hist)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def transform_columns(self, *cols, ds=None):
        vec: VectorColumn = cols[0]
        if vec.metadata is not None:
            self.histories = vec.metadata.column_history()
        hist = self.histories
        if hist is None:
            raise ValueError("RecordInsightsSHAP needs the input vector metadata (column histories)")
        cidx, diffs = self._run(vec.values, hist)
        return InsightsColumn(cidx, diffs, [_history_json(h) for h in hist])

    def transform_row(self, *values):
        x = torch.as_tensor(np.asarray(values[0], np.float64))[None, :]
        if self.histories is None:
            raise ValueError("RecordInsightsSHAP has not seen vector metadata yet")
        cidx, diffs = self._shap_block(x, self.histories)
        return InsightsColumn(cidx, diffs, [_history_json(h) for h in self.histories]).row(0)


@register_stage
class RecordInsightsSHAPInteractions(RecordInsightsSHAP):
    """Unary (OPVector -> TextMap) transformer wrapping a fitted tree model stage: exact SHAP interaction values
    (``tree_engine.forest_shap_interactions``, the second kernel of ``ops/csrc/hip/shap_kernels.hip``). They split
    the attribution of every candidate of ``RecordInsightsSHAP`` into a main effect and its pair effects with
    every other candidate. The interaction matrix is folded onto the candidates on both axes, so a pair inside
    one text / date group lands in that group's main effect. Per record the stage reports the top ``top_k``
    candidate pairs by the pair effect ``Phi_ab + Phi_ba`` of the selecting score column (the selection of
    ``RecordInsightsSHAP``, both strategies); the key of an insight is the JSON array of the two candidates'
    column histories in column order. :meth:`main_effects` plus all pair effects plus :meth:`bias` add up to the
    record's raw score."""
    operation_name = "recordInsightsSHAPInteractions"
    BLOCK_BYTES = 1 << 29            # one block's interaction matrix stays below about 512 MB

    def _interactions(self, X: torch.Tensor, context=None):
        learner, state = self._learner_state()
        try:
            return learner.shap_interaction_values(state, X, None, context)
        except NotImplementedError as e:
            raise ValueError(f"RecordInsightsSHAPInteractions needs a tree model: {e}") from e

    def _folded(self, X: torch.Tensor, hist: List[dict]):
        """The interaction matrix of one block folded onto the candidates: (V [n, m, m, C], plan)."""
        Phi, used = self._interactions(X)
        n, U, C = Phi.shape[0], Phi.shape[1] - 1, Phi.shape[3]
        plan = self._shap_plan(hist, used, X.device)
        cand, m = plan[0], int(plan[1].numel())
        half = torch.zeros(n, m, U, C, dtype=torch.float64, device=X.device)
        half.index_add_(1, cand, Phi[:, :U, :U])
        del Phi
        V = torch.zeros(n, m, m, C, dtype=torch.float64, device=X.device)
        V.index_add_(2, cand, half)
        return V, plan

    def _pair_block(self, X: torch.Tensor, hist: List[dict]):
        """Top-K pair effects of one block of records: (columns [n, K, 2] (smaller first, -1 = no insight),
        pair effects [n, K, C])."""
        n, dev = X.shape[0], X.device
        V, (cand, plain_col, gcols) = self._folded(X, hist)
        m, C = V.shape[1], V.shape[3]
        ia, ib = torch.triu_indices(m, m, 1, device=dev)
        K = self._top_width(int(ia.numel()))
        if ia.numel() == 0 or n == 0:
            return (torch.full((n, K, 2), -1, dtype=torch.long, device=dev),
                    torch.zeros(n, K, C, dtype=torch.float64, device=dev))
        Vp = V[:, ia, ib] + V[:, ib, ia]
        del V
        Cc = self._reported_columns(X, plain_col, gcols)
        sel, okK = self._top_candidates(Vp, self._score_column(X, C))
        ca, cb = Cc.gather(1, ia[sel]), Cc.gather(1, ib[sel])
        pair = torch.stack([torch.minimum(ca, cb), torch.maximum(ca, cb)], 2)
        colsK = torch.where(okK[:, :, None], pair, torch.full_like(pair, -1))
        diffsK = Vp.gather(1, sel[:, :, None].expand(n, sel.shape[1], C))
        return colsK, diffsK

    def _block_rows(self, X: torch.Tensor) -> int:
        if X.shape[0] == 0:
            return 1
        phi = self._shap(X[:1])[0]
        return max(1, self.BLOCK_BYTES // (phi.shape[1] ** 2 * phi.shape[2] * 8))

    def main_effects(self, X: torch.Tensor) -> torch.Tensor:
        """The folded diagonal ``[n, m, C]``: every candidate's main effect (a group's includes the pairs
        among its members), candidates in the order of ``RecordInsightsSHAP``'s plan."""
        if self.histories is None:
            raise ValueError("RecordInsightsSHAPInteractions has not seen vector metadata yet")
        block = self._block_rows(X)
        return torch.cat([self._folded(X[a:a + block], self.histories)[0].diagonal(dim1=1, dim2=2).transpose(1, 2)
                          for a in range(0, max(X.shape[0], 1), block)])

    def _run(self, X: torch.Tensor, hist: List[dict]):
        block = self._block_rows(X)
        parts = [self._pair_block(X[a:a + block], hist) for a in range(0, X.shape[0], block)] or \
            [self._pair_block(X[:0], hist)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def transform_columns(self, *cols, ds=None):
        vec: VectorColumn = cols[0]
        if vec.metadata is not None:
            self.histories = vec.metadata.column_history()
        hist = self.histories
        if hist is None:
            raise ValueError("RecordInsightsSHAPInteractions needs the input vector metadata (column histories)")
        cidx, diffs = self._run(vec.values, hist)
        return PairInsightsColumn(cidx, diffs, [_history_json(h) for h in hist])

    def transform_row(self, *values):
        x = torch.as_tensor(np.asarray(values[0], np.float64))[None, :]
        if self.histories is None:
            raise ValueError("RecordInsightsSHAPInteractions has not seen vector metadata yet")
        cidx, diffs = self._pair_block(x, self.histories)
        return PairInsightsColumn(cidx, diffs, [_history_json(h) for h in self.histories]).row(0)


# ---------------------------------------------------------------------------------------------- Corr
def _pred_matrix(col) -> torch.Tensor:
    if isinstance(col, PredictionColumn):
        if col.probability.shape[1] > 0:
            return col.probability.to(torch.float64)
        return col.prediction.reshape(-1, 1).to(torch.float64)
    return col.values.to(torch.float64)


@register_stage
class RecordInsightsCorrModel(BinaryTransformer):
    operation_name = "recordInsightsCorr"
    output_type = T.TextMap
    allow_label_as_input = True

    def __init__(self, top_k=20, score_corr=None, norm=None, histories=None, uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.top_k = top_k
        self.score_corr = None if score_corr is None else np.asarray(score_corr, np.float64)
        self.norm = norm or {}
        self.histories = histories

    def _normalize(self, X: torch.Tensor) -> torch.Tensor:
        a = torch.as_tensor(self.norm["a"], dtype=torch.float64, device=X.device)
        b = torch.as_tensor(self.norm["b"], dtype=torch.float64, device=X.device)
        off = float(self.norm["offset"])
        Xd = X.to(torch.float64)
        return torch.where(b == 0, torch.zeros_like(Xd), (Xd - a) / torch.where(b == 0, torch.ones_like(b), b) - off)

    def _rows(self, X: torch.Tensor) -> List[Dict[str, str]]:
        d = X.shape[1]
        if self.histories is not None and len(self.histories) != d:
            raise ValueError("feature metadata size does not match feature size")
        Z = self._normalize(X)
        S = torch.as_tensor(np.nan_to_num(self.score_corr, nan=0.0), dtype=torch.float64, device=X.device)
        imp = Z[:, None, :] * S[None, :, :]                  # [n, P, d]
        k = min(int(self.top_k), d)
        _, idx = torch.topk(imp.abs(), k, dim=2)
        vals = imp.gather(2, idx)
        idx, vals = idx.cpu().numpy(), vals.cpu().numpy()
        out = []
        for i in range(X.shape[0]):
            acc: Dict[int, list] = {}
            for p in range(idx.shape[1]):
                for j, v in zip(idx[i, p], vals[i, p]):
                    acc.setdefault(int(j), []).append([p, float(v)])
            out.append({_history_json(self.histories[j]): json.dumps(v, separators=(",", ":"))
                        for j, v in acc.items()})
        return out

    def transform_columns(self, pred, vec, ds=None):
        return ObjectColumn(T.TextMap, self._rows(vec.values))

    def transform_row(self, *values):
        x = torch.as_tensor(np.asarray(values[1], np.float64))[None, :]
        return self._rows(x)[0]

    def ctor_args(self):
        return {"topK": self.top_k, "scoreCorr": None if self.score_corr is None else self.score_corr.tolist(),
                "norm": self.norm, "histories": self.histories}

    def load_ctor_args(self, a):
        self.top_k = a["topK"]
        self.score_corr = None if a["scoreCorr"] is None else np.asarray(a["scoreCorr"], np.float64)
        self.norm = a["norm"]
        self.histories = a["histories"]


@register_stage
class RecordInsightsCorr(BinaryEstimator):
    """(prediction, feature vector) -> TextMap of the top-K correlation-weighted features per record."""
    operation_name = "recordInsightsCorr"
    output_type = T.TextMap
    allow_label_as_input = True
    _defaults = {"norm_type": "minMax", "correlation_type": "pearson", "top_k": 20}

    def fit_columns(self, pred, vec, ds=None):
        from ...ops import stats as ST
        if vec.metadata is None:
            raise ValueError("second input feature must be a feature vector with OpVectorMetadata")
        P = _pred_matrix(pred)
        X = vec.values.to(torch.float64)
        psize, fsize = P.shape[1], X.shape[1]
        comb = torch.cat([X, P.to(X.device)], 1)
        C = ST.corr_matrix(comb, self.params["correlation_type"]).cpu().numpy()
        score_corr = C[fsize:fsize + psize, :fsize]
        cs = ST.col_stats(X)
        nt = self.params["norm_type"]
        mn, mx = cs["min"].cpu().numpy(), cs["max"].cpu().numpy()
        if nt == "minMax":
            norm = {"a": mn.tolist(), "b": (mx - mn).tolist(), "offset": 0.0, "name": nt}
        elif nt == "zNorm":
            norm = {"a": cs["mean"].cpu().numpy().tolist(), "b": np.sqrt(cs["variance"].cpu().numpy()).tolist(),
                    "offset": 0.0, "name": nt}
        elif nt == "minMaxCentered":
            norm = {"a": mn.tolist(), "b": ((mx - mn) / 2.0).tolist(), "offset": 1.0, "name": nt}
        else:
            raise ValueError(f"unknown norm type {nt}")
        return RecordInsightsCorrModel(self.params["top_k"], score_corr, norm, vec.metadata.column_history())

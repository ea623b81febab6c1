// CPU reference implementation of the histogram tree engine kernels.
//
// These are the host twins of the HIP kernels in ../hip/tree_*_kernels.hip and ../hip/forest_predict_kernels.hip and
// share their data layout exactly (see transmogrifai_amd/models/tree_engine.py for the orchestration):
//
//   Xb        uint8 [N][F] row-major binned feature matrix
//   rows      uint32 packed row entries: (row & 0xFFFFFF) | (weight << 24); with wide = 1 (training sets of
//             >= 2^24 rows) the 32-bit row id, weight 1
//   nodes     j = 0..n_nodes-1 : [node_begin[j], node_begin[j]+node_count[j]) slice of `rows`
//   features  node j histograms features feat_list[node_feat_off[j] + 0 .. node_nfeat[j]-1]
//   hist      int64 fixed point [node_hist_off[j] + (fl * B + bin) * S + s]; value = hist * qinv[model][s]
//             per-row contributions are rint(v * qscale[model][s]) exactly as in the HIP kernel, so the
//             integer sums (and therefore every split) are bit-identical between the two paths
//
// Stat modes (S = stats per bin):
//   0 CLS : S = n_classes, contribution w at class y[row]                  (gini / entropy trees)
//   1 VAR : S = 3, (w, w*t, w*t*t), t = t1[model*stride + row]              (variance trees, GBT)
//   2 GH  : S = 2, (w*g, w*h), g = t1[model*stride + row], h = t2[...]      (Newton / XGBoost-style)
//
// Reference hot loops being replaced: Spark MLlib DecisionTree/RandomForest/GBT per-level
// DTStatsAggregator (K23-K25 in SURVEY.md) and XGBoost4J hist building.
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#include <omp.h>

#include "common/tmog_abi.h"
#include "common/tree_rules.hpp"
#include "common/boost_eval.hpp"

using namespace tmog;  // the split / growth rules shared with the HIP twins

constexpr int kMaxS = 256;   // statistics per bin (classes); the HIP wide path has the same bound

extern "C" {

static inline float stat_target(const float* t, int64_t model, int64_t stride, int64_t row) {
  return t[model * stride + row];
}

int tmog_hist_build_cpu(const uint8_t* Xb, int64_t N, int F, const uint32_t* rows, int n_nodes,
                        const int64_t* node_begin, const int64_t* node_count, const int32_t* node_feat_off,
                        const int32_t* node_nfeat, const int32_t* feat_list, const int32_t* node_model,
                        const int64_t* node_hist_off, int64_t* hist, int B, int mode, int S, const float* y,
                        const float* t1, const float* t2, int64_t model_stride, const float* qscale, int wide) {
  (void)N;
#pragma omp parallel for schedule(dynamic, 1)
  for (int j = 0; j < n_nodes; ++j) {
    const int nf = node_nfeat[j];
    const int32_t* fl = feat_list + node_feat_off[j];
    int64_t* h = hist + node_hist_off[j];
    std::memset(h, 0, sizeof(int64_t) * (size_t)nf * B * S);
    const int64_t b0 = node_begin[j], cnt = node_count[j];
    const int64_t model = node_model ? node_model[j] : 0;
    const float* qs = qscale + model * S;
    for (int64_t i = 0; i < cnt; ++i) {
      const uint32_t e = rows[b0 + i];
      // packed row | weight << 24, or (wide: >= 2^24-row training sets) the row itself with weight 1
      const int64_t r = wide ? (int64_t)e : (int64_t)(e & 0xFFFFFFu);
      const int64_t wi = wide ? 1 : (int64_t)(e >> 24);
      const float w = (float)wi;
      int64_t st[kMaxS];
      if (mode == 0) {
        st[(int)y[r]] = wi;
      } else if (mode == 1) {
        const float t = stat_target(t1, model, model_stride, r);
        const float wt = w * t;
        st[0] = wi;
        st[1] = (int64_t)(int)rintf(wt * qs[1]);
        st[2] = (int64_t)(int)rintf((wt * t) * qs[2]);
      } else {
        st[0] = (int64_t)(int)rintf((w * stat_target(t1, model, model_stride, r)) * qs[0]);
        st[1] = (int64_t)(int)rintf((w * stat_target(t2, model, model_stride, r)) * qs[1]);
      }
      const uint8_t* xr = Xb + r * (int64_t)F;
      if (mode == 0) {           // one class slot per row
        const int cls = (int)y[r];
        for (int f = 0; f < nf; ++f) h[((int64_t)f * B + xr[fl[f]]) * S + cls] += st[cls];
        continue;
      }
      for (int f = 0; f < nf; ++f) {
        const int bin = xr[fl[f]];
        int64_t* hb = h + ((int64_t)f * B + bin) * S;
        for (int s = 0; s < S; ++s) hb[s] += st[s];
      }
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------- split finding
// (impurity kinds, gains and the node parameter slots: common/tree_rules.hpp)
int tmog_split_find_cpu(const int64_t* hist, int n_nodes, const int64_t* node_hist_off, const int32_t* node_nfeat,
                        const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* feat_nbins, int B,
                        int S, int kind, const float* node_params, int missing_bin, const int32_t* node_model,
                        const double* qinv, int32_t* out_feat, int32_t* out_bin, float* out_gain,
                        uint8_t* out_default_left, float* out_left, float* out_total, uint8_t* rec,
                        int64_t rec_bytes, int fp_mlo, int fp_nml, int fp_obase) {
#pragma omp parallel for schedule(dynamic, 4)
  for (int j = 0; j < n_nodes; ++j) {
    const int64_t* h = hist + node_hist_off[j];
    const int nf = node_nfeat[j];
    const int32_t* fl = feat_list + node_feat_off[j];
    const float* P = node_params + (int64_t)j * kPrmStride;
    const double* q = qinv + (int64_t)(node_model ? node_model[j] : 0) * S;
    const double min_inst = P[kPrmMinInst], min_gain = P[kPrmMinGain], mcw = P[kPrmMcw], lambda = P[kPrmLambda];
    const bool allow_missing = P[kPrmAllowMissing] > 0.5f && missing_bin >= 0;
    int64_t totq[kMaxS] = {0};
    double tot[kMaxS];
    // totals from feature 0 (every row is counted once per feature, including the missing bin)
    for (int b = 0; b < B; ++b)
      for (int s = 0; s < S; ++s) totq[s] += h[(int64_t)b * S + s];
    for (int s = 0; s < S; ++s) {
      tot[s] = (double)totq[s] * q[s];
      out_total[(int64_t)j * S + s] = (float)tot[s];
    }
    double tcount;
    const double pimp = impurity<0>([&](int s) { return tot[s]; }, S, kind, &tcount);
    const double parent_gain = kind == 3 ? newton_parent(tot[0], tot[1], lambda) : 0.0;
    double best = -INFINITY;
    int bf = -1, bb = -1, bdl = 0, bfi = -1;
    int64_t bleft[kMaxS] = {0};
    for (int f = 0; f < nf; ++f) {
      const int gf = fl[f];
      const int nb = feat_nbins[gf];
      const int64_t* hf = h + (int64_t)f * B * S;
      int64_t miss[kMaxS] = {0};
      if (allow_missing)
        for (int s = 0; s < S; ++s) miss[s] = hf[(int64_t)missing_bin * S + s];
      bool any_miss = false;
      for (int s = 0; s < S; ++s) any_miss |= miss[s] != 0;
      // an empty missing bin: the dl = 1 candidates repeat the dl = 0 ones and never win a tie
      for (int dl = 0; dl < (allow_missing ? (any_miss ? 2 : 1) : 1); ++dl) {
        int64_t lq[kMaxS];
        for (int s = 0; s < S; ++s) lq[s] = dl ? miss[s] : 0;
        // with a missing bin, dl = 0 also tries b = nb - 1: every present value left, missing right
        // (XGBoost's present-vs-missing split; the only candidate of a one-bin indicator column)
        const int b_end = nb - 1 + ((allow_missing && dl == 0) ? 1 : 0);
        for (int b = 0; b < b_end; ++b) {
          double left[kMaxS], right[kMaxS];
          for (int s = 0; s < S; ++s) {
            lq[s] += hf[(int64_t)b * S + s];
            left[s] = (double)lq[s] * q[s];
            right[s] = (double)(totq[s] - lq[s]) * q[s];
          }
          double gain;
          if (kind == 3) {
            if (newton_invalid(left[1], right[1], mcw)) continue;
            gain = newton_gain(left[0], left[1], right[0], right[1], lambda, parent_gain);
          } else {
            double lc, rc;
            const double li = impurity<0>([&](int s) { return left[s]; }, S, kind, &lc);
            const double ri = impurity<0>([&](int s) { return right[s]; }, S, kind, &rc);
            if (!impurity_split_gain(pimp, tcount, lc, li, rc, ri, min_inst, min_gain, &gain)) continue;
          }
          if (gain > best) {   // first wins: the (feature, dl, bin) scan order is better()'s tie-break
            best = gain; bf = gf; bb = b; bdl = dl; bfi = f;
            for (int s = 0; s < S; ++s) bleft[s] = lq[s];
          }
        }
      }
    }
    out_feat[j] = bf;
    out_bin[j] = bb;
    out_gain[j] = bf >= 0 ? (float)best : -INFINITY;
    out_default_left[j] = (uint8_t)bdl;
    for (int s = 0; s < S; ++s) out_left[(int64_t)j * S + s] = (float)((double)bleft[s] * q[s]);
    if (rec) {   // feature-parallel split record
      uint8_t* r = rec + (int64_t)j * rec_bytes;
      fp_rec_store(r, bf >= 0, SplitCand{best, bfi, bb, bdl}, fp_mlo, fp_nml, fp_obase, [&] { return bf; });
      std::memcpy(r + kFpLeft, out_left + (int64_t)j * S, 4 * (size_t)S);
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------- partition
// Stable partition of every splitting node's rows into [left | right] written at out_begin[j].
// out_left_count[j] receives the number of left rows. Nodes with split_feat < 0 are skipped.
int tmog_partition_cpu(const uint8_t* Xb, int F, const uint32_t* rows_in, uint32_t* rows_out, int n_nodes,
                       const int64_t* node_begin, const int64_t* node_count, const int32_t* split_feat,
                       const int32_t* split_bin, const uint8_t* default_left, int missing_bin,
                       const int64_t* out_begin, int64_t* out_left_count, int wide) {
#pragma omp parallel for schedule(dynamic, 1)
  for (int j = 0; j < n_nodes; ++j) {
    if (split_feat[j] < 0) { out_left_count[j] = 0; continue; }
    const int f = split_feat[j], sb = split_bin[j];
    const auto dl = [&] { return default_left[j] != 0; };
    const uint32_t* in = rows_in + node_begin[j];
    const int64_t cnt = node_count[j];
    int64_t nl = 0;
    for (int64_t i = 0; i < cnt; ++i) {
      const int bin = Xb[(int64_t)(wide ? in[i] : (in[i] & 0xFFFFFFu)) * F + f];
      nl += goes_left(bin, sb, dl, missing_bin);
    }
    uint32_t* out = rows_out + out_begin[j];
    int64_t li = 0, ri = nl;
    for (int64_t i = 0; i < cnt; ++i) {
      const int bin = Xb[(int64_t)(wide ? in[i] : (in[i] & 0xFFFFFFu)) * F + f];
      if (goes_left(bin, sb, dl, missing_bin)) out[li++] = in[i]; else out[ri++] = in[i];
    }
    out_left_count[j] = nl;
  }
  return 0;
}

// -------------------------------------------------------------------------------------- predict
// Flat forest: model m owns trees [model_tree_off[m], model_tree_off[m+1]) and rows
// row_list[model_row_off[m] .. model_row_off[m+1]) (row_list == nullptr => rows 0..n_m-1).
// Tree t starts at node tree_off[t]; nodes are int4 (feat, bin, left, right) with global child
// indices, left < 0 marks a leaf. out[i][K] = sum_t w_t * leaf_value[leaf(t, row_i)].
int tmog_forest_predict_cpu(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                            const int32_t* row_list, const int64_t* model_tree_off, const int64_t* tree_off,
                            const float* tree_weight, const int32_t* nodes, const uint8_t* default_left,
                            int missing_bin, const float* leaf_value, int K, float* out) {
  for (int m = 0; m < n_models; ++m) {
    const int64_t r0 = model_row_off[m], r1 = model_row_off[m + 1];
#pragma omp parallel for schedule(static)
    for (int64_t i = r0; i < r1; ++i) {
      const int64_t row = row_list ? row_list[i] : (i - r0);
      const uint8_t* xr = Xb + row * (int64_t)F;
      float* o = out + i * K;
      for (int c = 0; c < K; ++c) o[c] = 0.f;
      for (int64_t t = model_tree_off[m]; t < model_tree_off[m + 1]; ++t) {
        int64_t k = tree_off[t];
        while (nodes[4 * k + 2] >= 0) {
          const auto dl = [&] { return default_left[k] != 0; };
          const bool gl = goes_left(xr[nodes[4 * k]], nodes[4 * k + 1], dl, missing_bin);
          k = gl ? nodes[4 * k + 2] : nodes[4 * k + 3];
        }
        const float w = tree_weight[t];
        for (int c = 0; c < K; ++c) o[c] += w * leaf_value[k * K + c];
      }
    }
  }
  return 0;
}

// -------------------------------------------------------------------------------- staged evaluation
// Host twin of ../hip/staged_eval_kernels.hip (contract in common/tmog_abi.h): the trees of a stage are walked and
// added per row in tree order, then the stage's metric is taken over the rows in row order.
int tmog_forest_staged_eval_cpu(const uint8_t* Xb, int F, const int32_t* row_list, int64_t n, const float* y,
                                const int32_t* nodes, const uint8_t* default_left, const float* leaf_value,
                                const int64_t* tree_off, const float* tree_weight, int missing_bin,
                                const int64_t* stage_off, int S, const int32_t* tree_col, int K, int metric,
                                double scale, int bins, double* margins, double* values, int64_t* counts,
                                int32_t* tables) {
  if (!eval_metric_known(metric) || K < 1 || (!eval_metric_multi(metric) && K != 1)) return 1;
  if (n <= 0 || S <= 0) return 0;
  std::vector<double> term(eval_metric_counted(metric) || metric == TMOG_EVAL_AUPR ? 0 : n);
  std::vector<int32_t> mark(term.empty() ? n : 0);   // a row's error bit or table slot
  for (int s = 0; s < S; ++s) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = row_list ? row_list[i] : i;
      const uint8_t* xr = Xb + row * (int64_t)F;
      double* mr = margins + i * K;
      for (int64_t t = stage_off[s]; t < stage_off[s + 1]; ++t) {
        int64_t k = tree_off[t];
        while (nodes[4 * k + 2] >= 0) {
          const auto dl = [&] { return default_left[k] != 0; };
          const bool gl = goes_left(xr[nodes[4 * k]], nodes[4 * k + 1], dl, missing_bin);
          k = gl ? nodes[4 * k + 2] : nodes[4 * k + 3];
        }
        mr[tree_col ? tree_col[t] : 0] += (double)tree_weight[t] * (double)leaf_value[k];
      }
      const float yr = y[row];
      const auto mc = [&](int c) { return mr[c]; };
      switch (metric) {
        case TMOG_EVAL_LOGLOSS: term[i] = eval_logloss(mr[0], scale, (double)yr); break;
        case TMOG_EVAL_ERROR: mark[i] = eval_error(mr[0], scale, (double)yr); break;
        case TMOG_EVAL_AUPR: mark[i] = eval_aupr_slot(mr[0], scale, yr, bins); break;
        case TMOG_EVAL_SQERR: term[i] = eval_sqerr(mr[0], (double)yr); break;
        case TMOG_EVAL_ABSERR: term[i] = eval_abserr(mr[0], (double)yr); break;
        case TMOG_EVAL_MLOGLOSS: term[i] = eval_mlogloss(mc, K, eval_label(yr, K)); break;
        default: mark[i] = eval_merror(mc, K, (int)yr); break;
      }
    }
    if (metric == TMOG_EVAL_AUPR) {
      int32_t* tb = tables + (int64_t)s * 2 * bins;
      for (int64_t i = 0; i < n; ++i) ++tb[mark[i]];
    } else if (eval_metric_counted(metric)) {
      int64_t c = 0;
      for (int64_t i = 0; i < n; ++i) c += mark[i];
      counts[s] += c;
    } else {
      double acc = 0.0;
      for (int64_t i = 0; i < n; ++i) acc += term[i];
      values[s] = acc;
    }
  }
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------- split finding
// Spark MLlib RandomForest.findSplitsForContinuousFeature (2.4) on a row sample, per feature:
// distinct values + counts, then midpoints chosen by the greedy stride rule. sample is [S][F]
// row-major; out is [F][max_splits] padded with +inf; n_out[f] = number of thresholds.
extern "C" int tmog_find_splits_cpu(const double* sample, int64_t S, int F, int max_splits, double* out,
                                    int32_t* n_out) {
#pragma omp parallel for schedule(dynamic, 4)
  for (int f = 0; f < F; ++f) {
    std::vector<double> v;
    v.reserve(S);
    for (int64_t i = 0; i < S; ++i) {
      const double x = sample[i * F + f];
      if (!std::isnan(x)) v.push_back(x);
    }
    double* o = out + (int64_t)f * max_splits;
    for (int k = 0; k < max_splits; ++k) o[k] = INFINITY;
    n_out[f] = 0;
    if (v.empty()) continue;
    std::sort(v.begin(), v.end());
    std::vector<double> vals;
    std::vector<int64_t> cnts;
    for (size_t i = 0; i < v.size(); ++i) {
      if (vals.empty() || v[i] != vals.back()) { vals.push_back(v[i]); cnts.push_back(1); }
      else cnts.back()++;
    }
    const int64_t possible = (int64_t)vals.size() - 1;
    const int64_t num_samples = (int64_t)v.size();
    int n = 0;
    if (possible <= 0) {
      n = 0;
    } else if (possible <= max_splits) {
      for (int64_t i = 1; i <= possible; ++i) o[n++] = (vals[i - 1] + vals[i]) / 2.0;
    } else {
      const double stride = (double)num_samples / (max_splits + 1);
      int64_t cur = cnts[0];
      double target = stride;
      for (size_t i = 1; i < vals.size() && n < max_splits; ++i) {
        const int64_t prev = cur;
        cur += cnts[i];
        const double pg = std::fabs((double)prev - target), cg = std::fabs((double)cur - target);
        if (pg < cg) { o[n++] = (vals[i - 1] + vals[i]) / 2.0; target += stride; }
      }
    }
    n_out[f] = n;
  }
  return 0;
}

// Native twin of tree_engine._finalize_py (one job group's created nodes -> flat forest arrays):
// leaf values (class frequencies / mean / Newton step -G/(H+lambda)*eta), XGBoost gamma pruning
// (bottom-up: children are created after their parents, so a reverse sweep sees final children),
// reachability from the roots, per-tree stable regrouping, child renumbering and (boosting) the leaf
// value of every created node id (pruned descendants take their nearest kept ancestor's value).
// Same float64 arithmetic and float32 roundings as the numpy version, so the arrays are identical.
// Returns the kept node count; outputs are sized for n nodes.
extern "C" int64_t tmog_tree_finalize_cpu(int64_t n, int T, const int64_t* tree, const int64_t* feat_in,
                                          const int64_t* bin, const uint8_t* dl, const double* gain, const double* tot,
                                          int S, const int64_t* left_in, const int64_t* right_in, int mode, int kind,
                                          int K, const double* job_lam, const double* job_eta,
                                          const double* job_gamma, int with_gid, int64_t* tree_off, int32_t* nodes,
                                          uint8_t* dl_out, float* value_out, float* gain_out, float* cover_out,
                                          float* gid_value) {
  std::vector<double> value((size_t)n * K), cover(n);
  for (int64_t i = 0; i < n; ++i) {
    const double* t = tot + (size_t)i * S;
    if (mode == 0) {
      double s = 0;
      for (int c = 0; c < S; ++c) s += t[c];
      // a class frequency t[c] / s is leaf_value's guarded mean (mode 1) of (s, t[c]); lambda and eta are not read
      for (int c = 0; c < K; ++c) value[(size_t)i * K + c] = leaf_value(1, s, t[c], 0.0, 0.0);
      cover[i] = s;
    } else if (mode == 1) {
      value[i] = leaf_value(mode, t[0], t[1], 0.0, 0.0);
      cover[i] = t[0];
    } else {
      const int64_t j = tree[i];
      value[i] = leaf_value(mode, t[0], t[1], job_lam[j], job_eta[j]);
      cover[i] = t[1];
    }
  }
  std::vector<int64_t> left(left_in, left_in + n), right(right_in, right_in + n), feat(feat_in, feat_in + n);
  if (kind == 3) {   // KIND_NEWTON
    for (int64_t i = n - 1; i >= 0; --i) {
      if (left[i] < 0) continue;
      if (left[left[i]] < 0 && left[right[i]] < 0 && gain[i] < job_gamma[tree[i]]) {
        left[i] = right[i] = -1;
        feat[i] = -1;
      }
    }
  }
  std::vector<uint8_t> reach(n, 0);
  for (int t = 0; t < T && t < n; ++t) reach[t] = 1;
  for (int64_t i = 0; i < n; ++i)
    if (reach[i] && left[i] >= 0) reach[left[i]] = reach[right[i]] = 1;
  std::vector<int64_t> cnt(T + 1, 0);
  for (int64_t i = 0; i < n; ++i)
    if (reach[i]) cnt[tree[i] + 1]++;
  for (int t = 0; t < T; ++t) cnt[t + 1] += cnt[t];
  for (int t = 0; t <= T; ++t) tree_off[t] = cnt[t];
  std::vector<int64_t> new_id(n, -1), order(cnt[T]);
  {
    std::vector<int64_t> cur(cnt.begin(), cnt.end() - 1);
    for (int64_t i = 0; i < n; ++i)
      if (reach[i]) {
        const int64_t p = cur[tree[i]]++;
        order[p] = i;
        new_id[i] = p;
      }
  }
  const int64_t m = cnt[T];
  for (int64_t p = 0; p < m; ++p) {
    const int64_t i = order[p];
    const bool isint = left[i] >= 0;
    nodes[p * 4 + 0] = isint ? (int32_t)feat[i] : 0;
    nodes[p * 4 + 1] = isint ? (int32_t)bin[i] : 0;
    nodes[p * 4 + 2] = isint ? (int32_t)new_id[left[i]] : -1;
    nodes[p * 4 + 3] = isint ? (int32_t)new_id[right[i]] : -1;
    dl_out[p] = isint ? dl[i] : 0;
    for (int c = 0; c < K; ++c) value_out[p * K + c] = (float)value[(size_t)i * K + c];
    gain_out[p] = isint ? (float)gain[i] : 0.f;
    cover_out[p] = (float)cover[i];
  }
  if (with_gid) {
    std::vector<int64_t> parent(n, -1);
    for (int64_t i = 0; i < n; ++i)
      if (left_in[i] >= 0) {
        parent[left_in[i]] = i;
        parent[right_in[i]] = i;
      }
    for (int64_t i = 0; i < n; ++i) {
      if (reach[i] || parent[i] < 0) {
        for (int c = 0; c < K; ++c) gid_value[i * K + c] = (float)value[(size_t)i * K + c];
      } else {
        for (int c = 0; c < K; ++c) gid_value[i * K + c] = gid_value[parent[i] * K + c];
      }
    }
  }
  return m;
}

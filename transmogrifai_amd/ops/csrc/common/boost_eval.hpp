// The evaluation metrics of a boosted model, as a function of one row's margin(s), written once for the staged
// evaluation kernel (hip/staged_eval_kernels.hip) and its host twin (host/tree_cpu.cpp
// tmog_forest_staged_eval_cpu). Everything is fp64 from the fp64 margin; the metric codes are the TMOG_EVAL_*
// constants of common/tmog_abi.h. Stateless free functions of scalar arguments, as in tree_rules.hpp.
//
//   logloss   log1p(exp(-|s m|)) + max(s m, 0) - y s m     s: margin scale (1 XGBoost, 2 Spark GBT)
//   error     (s m > 0) != (y > 0.5)                       counted
//   aupr      the (label, score-bin) slot of boost_epilogue_kernel (hip/boost_kernels.hip)
//   sqerr     (m - y)^2
//   abserr    |m - y|
//   mlogloss  logsumexp(m[0..K)) - m[clamp(label, 0, K - 1)]
//   merror    first maximal class != label                 counted
#pragma once
#include <cmath>
#include <cstdint>

#include "common/tmog_abi.h"
#include "common/tree_rules.hpp"

namespace tmog {

TMOG_HD bool eval_metric_known(int metric) { return metric >= TMOG_EVAL_LOGLOSS && metric <= TMOG_EVAL_MERROR; }
// counted metrics accumulate an int64 per stage, aupr a count table, every other a floating sum
TMOG_HD bool eval_metric_counted(int metric) { return metric == TMOG_EVAL_ERROR || metric == TMOG_EVAL_MERROR; }
TMOG_HD bool eval_metric_multi(int metric) { return metric == TMOG_EVAL_MLOGLOSS || metric == TMOG_EVAL_MERROR; }

// max(s m, 0) - y s m is taken first: for a 0/1 label it is exactly 0, s m or -s m, so a well classified row's tiny
// log1p term is not added to and subtracted from a large margin.
TMOG_HD double eval_logloss(double m, double s, double y) {
  TMOG_FP_EXACT
  const double sm = s * m;
  return ::log1p(::exp(-::fabs(sm))) + (::fmax(sm, 0.0) - y * sm);
}

TMOG_HD int eval_error(double m, double s, double y) {
  TMOG_FP_EXACT
  return ((s * m > 0.0) != (y > 0.5)) ? 1 : 0;
}

// Index into a [2 (label)][bins] table, bins in descending score order (evaluators/metrics.py
// binned_aupr_from_counts): the same expression as boost_epilogue_kernel's slot.
TMOG_HD int eval_aupr_slot(double m, double s, float y, int bins) {
  TMOG_FP_EXACT
  const double pr = 1.0 / (1.0 + ::exp(-(s * m)));
  const float sc = ::fminf(::fmaxf((float)pr, 0.f), 1.f);
  const int b = (int)(sc * (float)(bins - 1));
  return (y > 0.5f ? 1 : 0) * bins + (bins - 1 - b);
}

TMOG_HD double eval_sqerr(double m, double y) {
  TMOG_FP_EXACT
  const double d = m - y;
  return d * d;
}

TMOG_HD double eval_abserr(double m, double y) {
  TMOG_FP_EXACT
  return ::fabs(m - y);
}

TMOG_HD int eval_label(float y, int K) {
  const int l = (int)y;
  return l < 0 ? 0 : (l > K - 1 ? K - 1 : l);
}

// The K-class terms read the margins through m(c), c in [0, K): no per-lane array of K values is held. With a the
// first maximal class, logsumexp(m) - m[l] = (m[a] - m[l]) + log1p(sum_{c != a} exp(m[c] - m[a])): two
// non-negative parts, so the term keeps its relative accuracy when the labelled class dominates.
template <class M> TMOG_HD int eval_argmax(M m, int K) {
  int a = 0;
  double mx = m(0);
  for (int c = 1; c < K; ++c) {
    const double v = m(c);
    if (v > mx) {
      mx = v;
      a = c;
    }
  }
  return a;
}

template <class M> TMOG_HD double eval_mlogloss(M m, int K, int label) {
  TMOG_FP_EXACT
  const int a = eval_argmax(m, K);
  const double mx = m(a);
  double se = 0.0;
  for (int c = 0; c < K; ++c)
    if (c != a) se += ::exp(m(c) - mx);
  return (mx - m(label)) + ::log1p(se);
}

template <class M> TMOG_HD int eval_merror(M m, int K, int label) { return eval_argmax(m, K) != label ? 1 : 0; }

}  // namespace tmog

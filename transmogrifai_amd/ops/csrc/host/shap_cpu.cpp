// Host twins of ../hip/shap_kernels.hip (same arguments minus the stream; path layout in models/tree_engine.py
// forest_paths): exact path-dependent TreeSHAP and SHAP interaction values over merged leaf paths in fp64.
//
// For one (row, path) with elements e < m of zero fraction z_e and one fraction o_e in {0, 1}: EXTEND builds the
// permutation weights w[0 .. m], UNWOUND gives each element's sum and phi_e = v * (o_e - z_e) * sum_e (Lundberg et
// al. 2018, Algorithm 2). The interaction of two elements i != j is 1/2 * (o_i - z_i) * phi_j(path without i), so
// both twins run the same two functions over "all elements except `skip`", skip = -1 for the plain values.
// Plain fp64 sums in path order (the kernels sum in fixed point and use reciprocal multiplies: the two agree to
// rounding, not bit for bit); rows are independent (OpenMP).
#include <algorithm>
#include <cstdint>
#include <vector>
#include <omp.h>

#include "common/tmog_abi.h"
#include "common/forest_walk.hpp"

namespace {

int64_t longest_path(int64_t P, const int64_t* p_off) {
  int64_t m = 0;
  for (int64_t p = 0; p < P; ++p) m = std::max(m, p_off[p + 1] - p_off[p]);
  return m;
}

// one[e] = the row satisfies element e of the path's m; false when the path's game is identically 0 for the row
// (an unsatisfied element of zero fraction 0)
inline bool one_fractions(const uint8_t* xr, const int32_t* used, const int32_t* feat, const int32_t* rng,
                          const double* z, int m, int missing_bin, uint8_t* one) {
  bool dead = false;
  for (int e = 0; e < m; ++e) {
    one[e] = tmog::element_satisfied(rng[e], xr[used[feat[e]]], missing_bin);
    dead = dead || (!one[e] && z[e] == 0.0);
  }
  return !dead;
}

// EXTEND over the m elements (zero fractions z, one fractions one) except element `skip`: w[0 .. len], len the
// number of elements taken.
inline void extend(double* w, const uint8_t* one, const double* z, int m, int skip) {
  w[0] = 1.0;
  int l = 0;
  for (int e = 0; e < m; ++e) {
    if (e == skip) continue;
    ++l;
    w[l] = 0.0;
    for (int k = l - 1; k >= 0; --k) {
      if (one[e]) w[k + 1] += w[k] * (double)(k + 1) / (double)(l + 1);
      w[k] = z[e] * w[k] * (double)(l - k) / (double)(l + 1);
    }
  }
}

// UNWOUND: the sum of the weights w[0 .. len] with an element of one fraction o and zero fraction z taken out.
inline double unwound_sum(const double* w, int len, bool o, double z) {
  double total = 0.0;
  if (o) {
    double next = w[len];
    for (int j = len - 1; j >= 0; --j) {
      const double tmp = next / (double)(j + 1);
      total += tmp;
      next = w[j] - tmp * z * (double)(len - j);
    }
  } else {
    for (int j = len - 1; j >= 0; --j) total += w[j] / z / (double)(len - j);
  }
  return total;
}

}  // namespace

extern "C" {

// out[i][U + 1][C]: phi_e += v * (o_e - z_e) * sum_e per path, the bias slot U gets the row-independent bias[C]
// (sum of v * prod z).
int tmog_forest_shap_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         int64_t P, const int64_t* p_off, const int32_t* p_out, const double* p_val, int KV,
                         const double* bias, const int32_t* e_feat, const int32_t* e_rng, const double* e_z,
                         const int64_t* bin_off, int missing_bin, int C, double scale, double* out) {
  (void)bin_off;
  (void)scale;
  const int64_t max_m = longest_path(P, p_off);
  const int64_t slots = (int64_t)(U + 1) * C;
#pragma omp parallel
  {
    std::vector<double> w(max_m + 1);
    std::vector<uint8_t> one(max_m + 1);
#pragma omp for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = row_list ? row_list[i] : i;
      const uint8_t* xr = Xb + row * (int64_t)F;
      double* o = out + i * slots;
      for (int64_t k = 0; k < slots; ++k) o[k] = 0.0;
      for (int c = 0; c < C; ++c) o[(int64_t)U * C + c] = bias[c];
      for (int64_t p = 0; p < P; ++p) {
        const int64_t eo = p_off[p];
        const int m = (int)(p_off[p + 1] - eo);
        if (!one_fractions(xr, used, e_feat + eo, e_rng + eo, e_z + eo, m, missing_bin, one.data()) || m == 0) continue;
        const double* val = p_val + p * KV;
        double* oc = o + p_out[p];
        extend(w.data(), one.data(), e_z + eo, m, -1);
        for (int e = 0; e < m; ++e) {
          const double z = e_z[eo + e];
          const double total = unwound_sum(w.data(), m, one[e], z);
          const double phi = total * (double)(m + 1) * ((one[e] ? 1.0 : 0.0) - z);
          double* of = oc + (int64_t)e_feat[eo + e] * C;
          for (int c = 0; c < KV; ++c) of[c] += phi * val[c];
        }
      }
    }
  }
  return 0;
}

// tri is [n][U][U][C], every cell written; the unordered pair of compact features u < v is counted once, in cell
// (u, v).
int tmog_forest_shap_interactions_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U,
                                      const int32_t* used, int64_t P, const int64_t* p_off, const int32_t* p_out,
                                      const double* p_val, int KV, const double* bias, const int32_t* e_feat,
                                      const int32_t* e_rng, const double* e_z, const int64_t* bin_off,
                                      int missing_bin, int C, double scale, double* tri) {
  (void)bias;
  (void)bin_off;
  (void)scale;
  const int64_t max_m = longest_path(P, p_off);
  const int64_t slots = (int64_t)U * U * C;
#pragma omp parallel
  {
    std::vector<double> w(max_m + 1);
    std::vector<uint8_t> one(max_m + 1);
#pragma omp for schedule(static)
    for (int64_t r = 0; r < n; ++r) {
      const int64_t row = row_list ? row_list[r] : r;
      const uint8_t* xr = Xb + row * (int64_t)F;
      double* o = tri + r * slots;
      for (int64_t k = 0; k < slots; ++k) o[k] = 0.0;
      for (int64_t p = 0; p < P; ++p) {
        const int64_t eo = p_off[p];
        const int m = (int)(p_off[p + 1] - eo);
        if (m < 2 || !one_fractions(xr, used, e_feat + eo, e_rng + eo, e_z + eo, m, missing_bin, one.data())) continue;
        const double* val = p_val + p * KV;
        const int ms = m - 1;    // the sub-path without the conditioning element
        for (int i = 0; i < m; ++i) {
          const int ui = e_feat[eo + i];
          const double fi = 0.5 * ((one[i] ? 1.0 : 0.0) - e_z[eo + i]);
          extend(w.data(), one.data(), e_z + eo, m, i);
          for (int e = 0; e < m; ++e) {
            const int ue = e_feat[eo + e];
            if (e == i || ue <= ui) continue;      // each pair once, from its smaller feature
            const double z = e_z[eo + e];
            const double total = unwound_sum(w.data(), ms, one[e], z);
            const double pair = fi * total * (double)(ms + 1) * ((one[e] ? 1.0 : 0.0) - z);
            double* oc = o + ((int64_t)ui * U + ue) * C + p_out[p];
            for (int c = 0; c < KV; ++c) oc[c] += pair * val[c];
          }
        }
      }
    }
  }
  return 0;
}

}  // extern "C"

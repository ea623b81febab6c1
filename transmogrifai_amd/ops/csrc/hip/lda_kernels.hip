// Latent Dirichlet allocation: the sparse variational E-step and the topic statistics (CDNA4, gfx950).
//
// A document holds a few dozen distinct terms out of thousands of columns, and its E-step is a fixed-point
// iteration over those terms' rows of the topic table, repeated up to 100 times with its own stopping point
// (stages/feature/nlp_stages.py lda_e_step is the dense [N, V] form of the same arithmetic). The work here is
// proportional to nnz * K; everything is fp64, as the dense path is.
//
//   lda_estep_kernel    one wave per document, kWaves documents in flight per workgroup, each wave with its own
//                       LDS slice. The wave gathers its document's rows of expEbT [V][K] and its counts into the
//                       slice once and iterates out of LDS; terms past the slice's capacity are re-read from
//                       expEbT (L2) in every iteration, with the same arithmetic in the same order, so a result
//                       does not depend on where that boundary falls. Documents come from a queue (iteration
//                       counts differ by 50x between documents): a persistent grid, each wave taking the next
//                       document index with an atomic add. A document's result does not depend on the wave that
//                       ran it, so the outputs are bitwise reproducible.
//   lane mapping        lane = slice * Kp + k, Kp the power of two >= K, S = 64 / Kp term slices. One round
//                       handles S terms: phinorm_t = sum_k expEt_k B[t][k] is a butterfly over the Kp lanes of
//                       a group (DPP moves below 16 lanes), the gamma update accumulates B[t][k] c_t / phinorm_t
//                       per lane over its strided terms and is summed across the slices once per iteration.
//                       No reduction goes through LDS memory. Rows are stored with pitch K: the active lanes of
//                       a round read S * K consecutive doubles, which no two lanes share a bank for, so the
//                       pitch is not padded (the gather writes with the same mapping). This rests on the
//                       address pattern alone; a padded pitch was not measured against it.
//   lda_sstats_kernel   partial[seg][k] = sum over a CSC segment's entries of expEt[doc][k] r[entry]: one wave
//                       per segment of <= 4096 non-zeros of one column, same lane mapping
//   lda_fold_kernel     sstats[k][v] = expEb[k][v] * (column v's segment partials, in segment order): no
//                       floating-point atomics anywhere, a column without documents gives exactly 0
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"

namespace {

// ---- launch sizes, written once
constexpr int kWaves = 4;                   // documents in flight per workgroup
constexpr int kBlock = 64 * kWaves;
constexpr int kMaxK = 64;

// doubles in one wave's LDS slice: 8 KiB up to 16 topics (32 KiB per workgroup), 16 KiB above (64 KiB)
__host__ __device__ constexpr int slice_doubles(int Kp) { return Kp <= 16 ? 1024 : 2048; }
// terms a slice holds: K doubles of the topic table and the count per term
__host__ __device__ constexpr int slice_terms(int K, int Kp) { return slice_doubles(Kp) / (K + 1); }
int pow2_at_least(int K) {
  int p = 1;
  while (p < K) p <<= 1;
  return p;
}

// ---- cross-lane sums. Every lane of the wave must be active at these.
template <int CTRL>
__device__ __forceinline__ double dpp(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kHalfMirror = 0x141, kRowMirror = 0x140;
constexpr int kRowRor1 = 0x121, kRowRor2 = 0x122, kRowRor4 = 0x124, kRowRor8 = 0x128;

// sum over the Kp lanes of a group (lanes that share a term slice); every lane of the group gets the same bits.
// After the quad steps a quad is uniform, so mirroring 8 and then 16 lanes pairs each quad with the others.
template <int Kp>
__device__ __forceinline__ double group_sum(double x) {
  if (Kp >= 2) x += dpp<kQuadXor1>(x);
  if (Kp >= 4) x += dpp<kQuadXor2>(x);
  if (Kp >= 8) x += dpp<kHalfMirror>(x);
  if (Kp >= 16) x += dpp<kRowMirror>(x);
  if (Kp >= 32) x += __shfl_xor(x, 16, 64);
  if (Kp >= 64) x += __shfl_xor(x, 32, 64);
  return x;
}

// sum over the 64 / Kp lanes that hold the same topic k (one per slice). Widest step first: after the steps of
// 32 and 16 the four rows agree, after a rotation by 8 the row has period 8, and so on down to Kp.
template <int Kp>
__device__ __forceinline__ double slice_sum(double x) {
  if (Kp <= 32) x += __shfl_xor(x, 32, 64);
  if (Kp <= 16) x += __shfl_xor(x, 16, 64);
  if (Kp <= 8) x += dpp<kRowRor8>(x);
  if (Kp <= 4) x += dpp<kRowRor4>(x);
  if (Kp <= 2) x += dpp<kRowRor2>(x);
  if (Kp <= 1) x += dpp<kRowRor1>(x);
  return x;
}

// writes of some lanes of a wave to its LDS slice are read by other lanes of the same wave
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// digamma for x > 0: psi(x) = psi(x + n) - sum 1 / (x + i) up to x + n >= 10, then the asymptotic series through
// x^-14 (the first dropped term is below 5e-17 there)
__device__ __forceinline__ double digamma_pos(double x) {
  double r = 0.0;
  while (x < 10.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double i = 1.0 / x, i2 = i * i;
  const double p = 1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 -
                   i2 * (691.0 / 32760 - i2 * (1.0 / 12))))));
  return r + log(x) - 0.5 * i - i2 * p;
}

// exp(digamma(g_k) - digamma(sum_k g_k)) in lane (slice, k), 0 in the lanes past K. With two or more slices the
// odd slices evaluate digamma of the sum and the even ones digamma of g_k, and neighbours exchange.
template <int Kp>
__device__ __forceinline__ double exp_elog_theta(double g, bool kv, int s) {
  const double gs = group_sum<Kp>(g);
  double elt;
  if (Kp <= 32) {
    const bool odd = s & 1;
    const double mine = digamma_pos(odd ? gs : (kv ? g : 1.0));
    const double other = __shfl_xor(mine, Kp, 64);
    elt = odd ? other - mine : mine - other;
  } else {
    elt = digamma_pos(kv ? g : 1.0) - digamma_pos(gs);
  }
  return kv ? exp(elt) : 0.0;
}

__global__ void lda_queue_reset_kernel(unsigned* queue) { *queue = 0u; }

template <int Kp>
__global__ void __launch_bounds__(kBlock) lda_estep_kernel(const int64_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ col,
                                                           const float* __restrict__ val, int64_t N,
                                                           const double* __restrict__ expEbT, int K,
                                                           const double* __restrict__ alpha, int iters, double tol,
                                                           unsigned* __restrict__ queue, double* __restrict__ gamma,
                                                           int32_t* __restrict__ n_iter, double* __restrict__ expEt,
                                                           double* __restrict__ r) {
  __shared__ double lds[kWaves * slice_doubles(Kp)];
  __shared__ unsigned next_doc[kWaves];
  constexpr int S = 64 / Kp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane & (Kp - 1), s = lane / Kp;
  const bool kv = k < K;
  const int cap = slice_terms(K, Kp);
  double* B = lds + wave * slice_doubles(Kp);      // [cap][K] rows of expEbT
  double* cnt = B + cap * K;                       // [cap] counts
  const double a_k = kv ? alpha[k] : 0.0;

  // The document queue. Lane 0 takes an index with an atomic add and hands it to the wave through LDS, once before
  // the loop and then at the end of every document, so that the loop's head is the same code for every lane. (With
  // the take at the head, behind the same lane test as the store of n_iter at the tail, the compiler joined the
  // two across the back edge and ran the other lanes ahead of lane 0, which then never took the next index.)
  if (lane == 0) next_doc[wave] = atomicAdd(queue, 1u);
  for (;;) {
    wave_lds_sync();
    const int64_t d = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)next_doc[wave]);
    if (d >= N) break;
    const int64_t a = row_ptr[d];
    const int n = (int)(row_ptr[d + 1] - a);

    wave_lds_sync();                               // the previous document's reads are done
    const int nl = min(n, cap);
#pragma unroll 4
    for (int t = s; t < nl; t += S)
      if (kv) B[t * K + k] = expEbT[(int64_t)col[a + t] * K + k];
    double csum = 0.0;
    for (int t = lane; t < n; t += 64) {
      const double c = (double)val[a + t];
      if (t < cap) cnt[t] = c;
      csum += c;
    }
    csum = group_sum<64>(csum);
    wave_lds_sync();

    // one term of this lane's slice: b = B[t][k], c = count_t (both 0 past the end), from LDS or from L2
    auto term = [&](int t, double& b, double& c) {
      b = 0.0;
      c = 0.0;
      if (t < n) {
        if (t < cap) {
          c = cnt[t];
          if (kv) b = B[t * K + k];
        } else {
          c = (double)val[a + t];
          if (kv) b = expEbT[(int64_t)col[a + t] * K + k];
        }
      }
    };

    double g = kv ? 1.0 + csum / (double)K : 0.0;
    double e;
    int it = 0;
    bool done = false;
    for (;;) {
      e = exp_elog_theta<Kp>(g, kv, s);
      if (it >= iters || done) break;
      double acc = 0.0;
      for (int t0 = 0; t0 < n; t0 += S) {
        double b, c;
        term(t0 + s, b, c);
        const double ph = group_sum<Kp>(e * b) + 1e-100;
        acc += b * (c / ph);
      }
      acc = slice_sum<Kp>(acc);
      const double nw = kv ? a_k + e * acc : 0.0;
      const double change = group_sum<Kp>(fabs(nw - g)) / (double)K;
      g = nw;
      ++it;
      done = change < tol;
    }

    for (int t0 = 0; t0 < n; t0 += S) {
      double b, c;
      term(t0 + s, b, c);
      const double ph = group_sum<Kp>(e * b) + 1e-100;
      if (k == 0 && t0 + s < n) r[a + t0 + s] = c / ph;
    }
    if (s == 0 && kv) {
      gamma[d * K + k] = g;
      expEt[d * K + k] = e;
    }
    if (lane == 0) {
      n_iter[d] = it;
      next_doc[wave] = atomicAdd(queue, 1u);
    }
  }
}

template <int Kp>
__global__ void __launch_bounds__(kBlock) lda_sstats_kernel(const int64_t* __restrict__ seg_begin,
                                                            const int32_t* __restrict__ csc_row,
                                                            const int64_t* __restrict__ csc_pos, int64_t n_seg,
                                                            const double* __restrict__ expEt,
                                                            const double* __restrict__ r, int K,
                                                            double* __restrict__ partial) {
  constexpr int S = 64 / Kp;
  const int lane = threadIdx.x & 63;
  const int k = lane & (Kp - 1), s = lane / Kp;
  const int64_t seg = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= n_seg) return;
  const int64_t a = seg_begin[seg], b = seg_begin[seg + 1];
  double acc = 0.0;
  if (k < K) {
#pragma unroll 4
    for (int64_t i = a + s; i < b; i += S) acc += expEt[(int64_t)csc_row[i] * K + k] * r[csc_pos[i]];
  }
  acc = slice_sum<Kp>(acc);
  if (s == 0 && k < K) partial[seg * K + k] = acc;
}

// one thread per (k, v): the column's segment partials in segment order, scaled by expEb[k][v]
__global__ void __launch_bounds__(256) lda_fold_kernel(const int64_t* __restrict__ col_seg, int64_t V, int K,
                                                       const double* __restrict__ partial,
                                                       const double* __restrict__ expEbT,
                                                       double* __restrict__ sstats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * K) return;
  const int64_t k = i / V, v = i - k * V;
  double acc = 0.0;
  for (int64_t sg = col_seg[v]; sg < col_seg[v + 1]; ++sg) acc += partial[sg * K + k];
  sstats[i] = expEbT[v * K + k] * acc;
}

// workgroups of lda_estep_kernel<Kp> that a device holds at once (registers and LDS): asked of the runtime once per
// device and instantiation (0: not asked yet, or the query failed). The occupancy query answers for the current
// device, which is dev. No lock: two threads asking at once store the same value.
constexpr int kMaxDevices = 64;
template <int Kp>
int resident_blocks(int dev) {
  static int cached[kMaxDevices];
  if (dev < 0 || dev >= kMaxDevices) return 0;
  if (cached[dev] == 0) {
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lda_estep_kernel<Kp>, kBlock, 0) == hipSuccess)
      cached[dev] = cus * per_cu;
  }
  return cached[dev];
}

// F(1) .. F(64) for the instantiation that serves K
#define TM_LDA_BY_KP(Kp, F)       \
  switch (Kp) {                   \
    case 1: F(1); break;          \
    case 2: F(2); break;          \
    case 4: F(4); break;          \
    case 8: F(8); break;          \
    case 16: F(16); break;        \
    case 32: F(32); break;        \
    default: F(64); break;        \
  }

}  // namespace

extern "C" {

int tmog_hip_lda_lds_terms(int K) {
  if (K < 1 || K > kMaxK) return 0;
  return slice_terms(K, pow2_at_least(K));
}

int tmog_hip_lda_estep(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N, const double* expEbT,
                       int K, const double* alpha, int iters, double tol, uint32_t* queue, double* gamma,
                       int32_t* n_iter, double* expEt, double* r, hipStream_t stream) {
  if (K < 1 || K > kMaxK || N > (int64_t)INT32_MAX) return -2;
  if (N == 0) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -3;
  const int Kp = pow2_at_least(K);
  hipLaunchKernelGGL(lda_queue_reset_kernel, dim3(1), dim3(1), 0, stream, queue);
  // a persistent grid: as many workgroups as the device holds at once, or one wave per document
#define TM_ESTEP(KP)                                                                                            \
  {                                                                                                             \
    const int resident = resident_blocks<KP>(dev);                                                              \
    if (resident < 1) return -3;                                                                                \
    hipLaunchKernelGGL(lda_estep_kernel<KP>, dim3((unsigned)min((N + kWaves - 1) / kWaves, (int64_t)resident)), \
                       dim3(kBlock), 0, stream, row_ptr, col, val, N, expEbT, K, alpha, iters, tol, queue, gamma, \
                       n_iter, expEt, r);                                                                       \
  }
  TM_LDA_BY_KP(Kp, TM_ESTEP)
#undef TM_ESTEP
  return (int)hipGetLastError();
}

int tmog_hip_lda_sstats(const int64_t* seg_begin, const int32_t* csc_row, const int64_t* csc_pos, int64_t n_seg,
                        const int64_t* col_seg, int64_t V, const double* expEt, const double* r, const double* expEbT,
                        int K, double* partial, double* sstats, hipStream_t stream) {
  if (K < 1 || K > kMaxK) return -2;
  const int Kp = pow2_at_least(K);
#define TM_SSTATS(KP)                                                                                          \
  hipLaunchKernelGGL(lda_sstats_kernel<KP>, dim3((unsigned)((n_seg + kWaves - 1) / kWaves)), dim3(kBlock), 0, \
                     stream, seg_begin, csc_row, csc_pos, n_seg, expEt, r, K, partial)
  if (n_seg > 0) { TM_LDA_BY_KP(Kp, TM_SSTATS) }
#undef TM_SSTATS
  if (V > 0)
    hipLaunchKernelGGL(lda_fold_kernel, dim3((unsigned)((V * K + 255) / 256)), dim3(256), 0, stream, col_seg, V, K,
                       partial, expEbT, sstats);
  return (int)hipGetLastError();
}

}  // extern "C"

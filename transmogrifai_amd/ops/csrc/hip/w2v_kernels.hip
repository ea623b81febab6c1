// Word2Vec: window-batched skip-gram with negative sampling, and the document mean (CDNA4, gfx950).
//
// A skip-gram window is a small dense problem (Ji et al., "Parallelizing Word2Vec in shared and distributed
// memory"): the vectors of the up to 2w <= 16 words around a position against the vectors of the centre word and
// S <= 15 negatives shared by the window. Its logits are one 16x16 tile and its two gradient products 16x16 by
// 16xDp tiles, the shapes of v_mfma_f32_16x16x4_f32. Nothing of the corpus but its token ids exists: the contexts
// of a position are found from the position inside the kernel. Roles are word2vec.c's: contexts read emb_in,
// the centre and the negatives read emb_out.
//
//   w2v_window_kernel   one wave per window. The wave stages the 16 In rows and the 16 Out rows into its own LDS
//                       tiles with 16-byte loads (consecutive lanes read consecutive 16 bytes of a row), computes
//                       L = In . Out^T by Dp / 4 MFMA steps, turns L into E = scale * (label - sigmoid(L)) in
//                       registers (masked to the valid slots and columns), passes E through a 16x17 LDS tile to
//                       the lanes that need it as the A operand of the next products, and forms Gin = E . Out and
//                       Gout = E^T . In in 16-column chunks of 4 MFMA steps each. A chunk's results overwrite the
//                       columns of the tiles they were computed from (In <- Gin, Out <- Gout; no later chunk
//                       reads them), so the tiles leave as they came: full rows, 16 bytes a lane, into the slabs
//                       gin / gout [B][16][Dp] next to the keys [B][16] (the table row a slab row belongs to, V
//                       for none). No atomics.
//   LDS layout          a tile row r holds its Dp floats rotated by rot(r) = 16 ((r + r/4) % 4) + 4 (r / 4) within
//                       a pitch of 64, 128 or 256 floats (the tier of Dp). The pitch is a multiple of the 64
//                       banks, so the bank of (r, k) is (k + rot(r)) % 64. The logits read rows c = 0..15 at
//                       k = 4s + q (16 rotations, all different multiples of 4: 64 banks), the gradient products
//                       rows 4t + q at k = n0 + c (the four rotations 16 apart: 64 banks). Only the write-back of
//                       a chunk (rows 4q + r) meets a 2-way conflict on 12 of the 64 banks. This rests on the
//                       address pattern; it was not measured against a padded pitch. The rotations are multiples
//                       of 4, so a 16-byte piece of a row stays one piece.
//   LDS budget          two tiles of 16 x pitch floats per wave, 8 / 16 / 32 KiB; waves per workgroup (4 / 2 / 1)
//                       keep a workgroup's static LDS under 64 KiB. What bounds the waves on a CU is the tile
//                       size, not the grouping.
//   w2v_apply_kernel    table[key] += the slab rows keyed to it, for keys sorted by a stable sort (order[] gives the
//   w2v_fold_kernel     slab row of every sorted position). The sorted positions are cut every kSegCap; a group of
//                       Dp / 4 lanes walks one such chunk, 16 bytes of the row per lane, and sums each run of
//                       equal keys in sorted order. A run that lies inside the chunk is added to its table row
//                       there. A run that crosses a cut leaves its pieces (each at most kSegCap rows) as partials,
//                       at most one leading and one trailing piece per chunk, and the fold kernel adds them up
//                       in position order, from the chunk in which the run starts, and updates the row: every
//                       row is read, updated and written once, by one lane per 16 bytes, in an order fixed by the
//                       sort alone. Sentinel keys are walked over without touching the slab.
//   w2v_doc_mean_kernel out[d] = mean of vectors[tok] over document d's tokens: one wave per document, fp64 sums,
//                       zeros for an empty document.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- limits and launch sizes, written once
constexpr int kMaxW = 8, kMaxS = 15, kMaxDp = 256;
constexpr int kSegCap = 32;                 // slab rows one lane group sums before a run is cut
constexpr int kApplyBlock = 256;
constexpr int kMeanWaves = 4;

// writes of some lanes of a wave to its LDS tiles are read by other lanes of the same wave
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int rot(int r) { return 16 * (((r & 3) + (r >> 2)) & 3) + 4 * (r >> 2); }

template <int PITCH, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) w2v_window_kernel(
    const float* __restrict__ emb_in, const float* __restrict__ emb_out, int V, int Dp,
    const int32_t* __restrict__ tok, int64_t T, const int64_t* __restrict__ doc_ptr,
    const int32_t* __restrict__ doc_id, const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int B, int w,
    int S, const int32_t* __restrict__ n_pos, float lr, float* __restrict__ gin, float* __restrict__ gout,
    int32_t* __restrict__ key_in, int32_t* __restrict__ key_out) {
  __shared__ __attribute__((aligned(16))) float tiles[WAVES][2][16 * PITCH];
  __shared__ float es_all[WAVES][16 * 17];
  __shared__ int32_t keys_all[WAVES][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * WAVES + wave;
  if (b >= B) return;                       // a whole wave; the kernel has no workgroup barrier
  float* In = tiles[wave][0];
  float* Out = tiles[wave][1];
  float* es = es_all[wave];
  int32_t* keys = keys_all[wave];

  // ---- keys: lanes 0..15 the context slots (offsets -w..-1, 1..w), lanes 16..31 the centre and the negatives
  if (lane < 32) {
    const int64_t t = pos[b];
    int key = V;
    if (t >= 0 && t < T) {
      if (lane < 16) {
        if (lane < 2 * w) {
          const int64_t p = t + (lane < w ? lane - w : lane - w + 1);
          const int64_t d = doc_id[t];
          if (p >= doc_ptr[d] && p < doc_ptr[d + 1]) key = tok[p];
        }
      } else if (lane == 16) {
        key = tok[t];
      } else if (lane - 16 <= S) {
        key = neg[b * S + (lane - 17)];
      }
    }
    if ((unsigned)key > (unsigned)V) key = V;     // an id outside the table updates nothing and is never read
    keys[lane] = key;
    (lane < 16 ? key_in : key_out)[b * 16 + (lane & 15)] = key;
  }
  wave_lds_sync();

  // ---- stage: 32 rows of Dp floats, 16 bytes per lane, consecutive lanes along a row
  const int c4 = Dp >> 2;
  for (int e = lane; e < 32 * c4; e += 64) {
    const int row = e / c4, kc = e - row * c4, r = row & 15;
    const int key = keys[row];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (key < V) v = *(const f32x4*)((row < 16 ? emb_in : emb_out) + (int64_t)key * Dp + 4 * kc);
    *(f32x4*)(tiles[wave][row >> 4] + r * PITCH + ((4 * kc + rot(r)) & (PITCH - 1))) = v;
  }
  wave_lds_sync();

  // ---- L[i][j] = sum_k In[i][k] Out[j][k]: this lane ends with L[4q + r][c], r = 0..3
  f32x4 l0 = {0.f, 0.f, 0.f, 0.f}, l1 = {0.f, 0.f, 0.f, 0.f};
  {
    const float* ia = In + c * PITCH;
    const float* ob = Out + c * PITCH;
    const int k0 = q + rot(c);
    for (int s = 0; s < c4; s += 2) {             // Dp / 4 is a multiple of 4
      const int ka = (4 * s + k0) & (PITCH - 1), kb = (4 * s + 4 + k0) & (PITCH - 1);
      l0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ia[ka], ob[ka], l0, 0, 0, 0);
      l1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ia[kb], ob[kb], l1, 0, 0, 0);
    }
    l0 += l1;
  }

  // ---- E[i][j] = scale_j (label_j - sigmoid(L[i][j])) on valid cells. 1 - sigmoid(x) = 1 / (1 + e^x) and
  // sigmoid(x) = 1 / (1 + e^-x): neither cancels, so a saturated cell keeps its relative accuracy.
  {
    const int np = *n_pos;
    const float a_pos = np > 0 ? lr / (float)np : 0.f;
    const float scale = c == 0 ? a_pos : -(a_pos / (float)S);
    const bool colv = c <= S && keys[16 + c] < V;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * q + r;
      const float g = 1.f / (1.f + expf(c == 0 ? l0[r] : -l0[r]));
      es[i * 17 + c] = (colv && keys[i] < V) ? scale * g : 0.f;
    }
  }
  wave_lds_sync();
  float ein[4], eout[4];                          // E[c][4t + q] and E[4t + q][c]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ein[t] = es[c * 17 + 4 * t + q];
    eout[t] = es[(4 * t + q) * 17 + c];
  }

  // ---- Gin = E . Out and Gout = E^T . In, 16 columns at a time, written back over the columns they came from
  for (int n0 = 0; n0 < Dp; n0 += 16) {
    f32x4 gi = {0.f, 0.f, 0.f, 0.f}, go = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = 4 * t + q;
      const int off = r * PITCH + ((n0 + c + rot(r)) & (PITCH - 1));
      gi = __builtin_amdgcn_mfma_f32_16x16x4f32(ein[t], Out[off], gi, 0, 0, 0);
      go = __builtin_amdgcn_mfma_f32_16x16x4f32(eout[t], In[off], go, 0, 0, 0);
    }
    wave_lds_sync();                              // every lane has read these columns
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      const int off = row * PITCH + ((n0 + c + rot(row)) & (PITCH - 1));
      In[off] = gi[r];
      Out[off] = go[r];
    }
  }
  wave_lds_sync();

  // ---- the tiles leave as they came
  for (int e = lane; e < 32 * c4; e += 64) {
    const int row = e / c4, kc = e - row * c4, r = row & 15;
    const f32x4 v = *(const f32x4*)(tiles[wave][row >> 4] + r * PITCH + ((4 * kc + rot(r)) & (PITCH - 1)));
    *(f32x4*)((row < 16 ? gin : gout) + (b * 16 + r) * (int64_t)Dp + 4 * kc) = v;
  }
}

// ---- the scatter-add. Thread -> (chunk of kSegCap sorted positions, 16 bytes of the row); a chunk's lanes are
// 1 << lpr_shift consecutive threads, of which the first Dp / 4 work.
__device__ __forceinline__ bool apply_item(int lpr_shift, int Dp, int64_t n_chunk, int64_t& chunk, int& col) {
  const int64_t gid = (int64_t)blockIdx.x * kApplyBlock + threadIdx.x;
  chunk = gid >> lpr_shift;
  col = 4 * (int)(gid & ((1 << lpr_shift) - 1));
  return chunk < n_chunk && col < Dp;
}

__global__ void __launch_bounds__(kApplyBlock) w2v_apply_kernel(float* __restrict__ emb, int V, int Dp,
                                                                const float* __restrict__ slab,
                                                                const int32_t* __restrict__ skey,
                                                                const int64_t* __restrict__ order, int64_t M,
                                                                int64_t n_chunk, int lpr_shift,
                                                                float* __restrict__ partial,
                                                                int32_t* __restrict__ tail) {
  int64_t chunk;
  int col;
  if (!apply_item(lpr_shift, Dp, n_chunk, chunk, col)) return;
  const int64_t a = chunk * kSegCap, e = min(a + (int64_t)kSegCap, M);
  bool starts_crossing = false;                   // the chunk's last run starts here and goes on in the next chunk
  for (int64_t i = a; i < e;) {
    const int k = skey[i];
    const bool live = (unsigned)k < (unsigned)V;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int64_t j = i;
    do {
      if (live) {
        const int64_t row = order[j];
        if (row >= 0 && row < M) acc += *(const f32x4*)(slab + row * Dp + col);
      }
      ++j;
    } while (j < e && skey[j] == k);
    if (live) {
      const bool starts = i > a || a == 0 || skey[a - 1] != k;
      const bool ends = j < e || e == M || skey[e] != k;
      if (starts && ends) {
        f32x4* p = (f32x4*)(emb + (int64_t)k * Dp + col);
        *p += acc;
      } else {
        *(f32x4*)(partial + (chunk * 2 + (starts ? 1 : 0)) * Dp + col) = acc;
        starts_crossing = starts;
      }
    }
    i = j;
  }
  if (col == 0) tail[chunk] = starts_crossing;
}

__global__ void __launch_bounds__(kApplyBlock) w2v_fold_kernel(float* __restrict__ emb, int Dp,
                                                               const int32_t* __restrict__ skey, int64_t M,
                                                               int64_t n_chunk, int lpr_shift,
                                                               const float* __restrict__ partial,
                                                               const int32_t* __restrict__ tail) {
  int64_t chunk;
  int col;
  if (!apply_item(lpr_shift, Dp, n_chunk, chunk, col)) return;
  if (!tail[chunk]) return;
  const int k = skey[min((chunk + 1) * kSegCap, M) - 1];
  f32x4 acc = *(const f32x4*)(partial + (chunk * 2 + 1) * Dp + col);
  for (int64_t c2 = chunk + 1; c2 < n_chunk && skey[c2 * kSegCap] == k; ++c2)
    acc += *(const f32x4*)(partial + (c2 * 2) * Dp + col);
  f32x4* p = (f32x4*)(emb + (int64_t)k * Dp + col);
  *p += acc;
}

// ---- document means. A wave's 64 lanes are 64 / L token slices of L = 1 << lsh columns; the slices are summed
// by a butterfly (every lane of the wave active), the same order whatever the schedule.
__global__ void __launch_bounds__(64 * kMeanWaves) w2v_doc_mean_kernel(const float* __restrict__ vec, int V, int D,
                                                                       const int32_t* __restrict__ tok,
                                                                       const int64_t* __restrict__ doc_ptr, int64_t N,
                                                                       int lsh, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * kMeanWaves + (threadIdx.x >> 6);
  if (d >= N) return;
  const int L = 1 << lsh, G = 64 >> lsh;
  const int col0 = lane & (L - 1), s = lane >> lsh;
  const int64_t a = doc_ptr[d], e = doc_ptr[d + 1];
  for (int cb = 0; cb < D; cb += L) {
    const int col = cb + col0;
    double acc = 0.0;
    if (col < D) {
      for (int64_t i = a + s; i < e; i += G) {
        const int tk = tok[i];
        if ((unsigned)tk < (unsigned)V) acc += (double)vec[(int64_t)tk * D + col];
      }
    }
    for (int m = 32; m >= L; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (s == 0 && col < D) out[d * D + col] = e > a ? (float)(acc / (double)(e - a)) : 0.f;
  }
}

int log2_at_least(int n) {
  int s = 0;
  while ((1 << s) < n) ++s;
  return s;
}

}  // namespace

extern "C" {

int tmog_hip_w2v_seg_cap() { return kSegCap; }

int tmog_hip_w2v_window(const float* emb_in, const float* emb_out, int V, int Dp, const int32_t* tok, int64_t T,
                        const int64_t* doc_ptr, const int32_t* doc_id, const int32_t* pos, const int32_t* neg, int B,
                        int w, int S, const int32_t* n_pos, float lr, float* gin, float* gout, int32_t* key_in,
                        int32_t* key_out, hipStream_t stream) {
  if (V < 1 || Dp < 16 || Dp > kMaxDp || (Dp & 15) || w < 1 || w > kMaxW || S < 1 || S > kMaxS || B < 0 ||
      T > (int64_t)INT32_MAX)
    return -2;
  if (B == 0) return 0;
#define TM_W2V_WINDOW(PITCH, WAVES)                                                                              \
  hipLaunchKernelGGL((w2v_window_kernel<PITCH, WAVES>), dim3((unsigned)((B + WAVES - 1) / WAVES)),                 \
                     dim3(64 * WAVES), 0, stream, emb_in, emb_out, V, Dp, tok, T, doc_ptr, doc_id, pos, neg, B, w, \
                     S, n_pos, lr, gin, gout, key_in, key_out)
  if (Dp <= 64) {
    TM_W2V_WINDOW(64, 4);
  } else if (Dp <= 128) {
    TM_W2V_WINDOW(128, 2);
  } else {
    TM_W2V_WINDOW(256, 1);
  }
#undef TM_W2V_WINDOW
  return (int)hipGetLastError();
}

int tmog_hip_w2v_apply(float* emb, int V, int Dp, const float* slab, const int32_t* skey, const int64_t* order,
                       int64_t M, float* partial, int32_t* tail, hipStream_t stream) {
  if (V < 1 || Dp < 16 || Dp > kMaxDp || (Dp & 15) || M < 0) return -2;
  if (M == 0) return 0;
  const int lpr_shift = log2_at_least(Dp / 4);
  const int64_t n_chunk = (M + kSegCap - 1) / kSegCap;
  const int64_t blocks = ((n_chunk << lpr_shift) + kApplyBlock - 1) / kApplyBlock;
  if (blocks > (int64_t)INT32_MAX) return -2;
  hipLaunchKernelGGL(w2v_apply_kernel, dim3((unsigned)blocks), dim3(kApplyBlock), 0, stream, emb, V, Dp, slab, skey,
                     order, M, n_chunk, lpr_shift, partial, tail);
  hipLaunchKernelGGL(w2v_fold_kernel, dim3((unsigned)blocks), dim3(kApplyBlock), 0, stream, emb, Dp, skey, M, n_chunk,
                     lpr_shift, partial, tail);
  return (int)hipGetLastError();
}

int tmog_hip_w2v_doc_mean(const float* vec, int V, int D, const int32_t* tok, const int64_t* doc_ptr, int64_t N,
                          float* out, hipStream_t stream) {
  if (V < 1 || D < 1 || N < 0) return -2;
  if (N == 0) return 0;
  const int lsh = log2_at_least(D < 64 ? D : 64);
  hipLaunchKernelGGL(w2v_doc_mean_kernel, dim3((unsigned)((N + kMeanWaves - 1) / kMeanWaves)), dim3(64 * kMeanWaves),
                     0, stream, vec, V, D, tok, doc_ptr, N, lsh, out);
  return (int)hipGetLastError();
}

}  // extern "C"

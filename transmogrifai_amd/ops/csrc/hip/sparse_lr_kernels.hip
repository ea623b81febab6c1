// Fused binary objective over the sparse design for the linear learners (CDNA4, gfx950).
//
// Binary logistic regression and LinearSVC on a wide, mostly-zero matrix (hashed text, pivots) keep the matrix as
// ops/linear.py SparseDesign: a CSR of the sparse columns and a small dense block Xd [N][nd]. One launch of
// sparse_lr_kernel evaluates P problems on it -- the contract of tmog_hip_lr_objective (linear_kernels.hip): with
// m = X v_p + b_p,  f_p = sum_i w_ip l(m),  r_p = sum_i w_ip l'(m)  and, with grad, R[i][p] = w_ip l'(m) in fp32 for
// SparseDesign.tmm. No [N][P] margin array exists: a value pass writes nothing per row.
//
//   lanes     A wave's 64 lanes are (row slot) x (problem column): PC = 16, 32 or 64 problem columns (chosen from P
//             at launch), so a wave works on RS = 64 / PC = 4, 2 or 1 rows at once. The usual batch of 8 grid points
//             x 3 folds = 24 problems fills 48 of 64 lanes with two rows a wave (csr_spmm_kernel: 24 lanes, one row).
//             P above 64 runs in chunks of 64 on blockIdx.y.
//   sparse    The PC lanes of a slot load PC (col, val) pairs of their row into a register batch; the pairs are
//             broadcast from it in groups of kU, every group's V row gathers issued before its FMAs (kU independent
//             loads in flight per wave, as sparse_kernels.hip describes). The loop bounds are the longest row of the
//             wave's slots; past its own end a row's pairs are (column 0, 0.f): the load is of a valid V row and its
//             value is replaced by 0.f before the FMA, so a V row that is not finite reaches only the rows that hold
//             a non-zero in its column, as in csr_spmm_kernel.
//   dense     Up to kNdMax dense columns the kernel holds V_d [nd][PC] in LDS and adds the dense block's part of
//             the margin itself: the slot's lanes read the Xd row with 16-byte loads (nd a multiple of 4; dword loads
//             otherwise) into a register batch and broadcast it against the LDS rows. kNdMax = 128: V_d is at most
//             128 x 64 x 4 = 32 KB of the CU's 160 KB, so four workgroups (16 waves) still share a CU, and the design
//             matrices this path is for have a handful of dense columns. Above the bound the caller computes the dense
//             margins with the library GEMM and passes them as the addend madd [N][ldm].
//   weights   Problem p reads column wmap[p] of W: the grid points of one fold share a weight column.
//   sums      f and r accumulate in fp64 per lane (the products w l and w l' are taken in fp64, exactly) over a
//             persistent row loop: wave g of the grid takes the row groups g, g + waves, ... Row slots are folded by
//             cross-lane moves, waves through LDS in wave order, and each workgroup writes one fp64 partial per
//             problem column, f_part / r_part [nblk][nchunk * PC]; fold_partials_kernel adds them in one fixed
//             order into f [P] and r [P]. No atomics: two runs on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hip/tmog_hip_abi.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;      // waves per workgroup
constexpr int kU = 8;          // V row gathers in flight per wave
constexpr int kNdMax = 128;    // dense columns whose V_d stays in LDS (32 KB at PC = 64)

// the formulas of linear_kernels.hip loss_and_grad
__device__ __forceinline__ void loss_and_grad(int loss, float m, float y, float ysc, float* l, float* g) {
  if (loss == 0) {              // logistic
    const float am = fabsf(m);
    const float e = __expf(-am);
    const float u = 1.f + e;
    const float lp = (u == 1.f) ? e : __logf(u) * __fdividef(e, u - 1.f);
    *l = fmaxf(m, 0.f) + lp - y * m;
    const float inv = __builtin_amdgcn_rcpf(u);
    const float sig = m >= 0.f ? inv : e * inv;
    *g = sig - y;
  } else if (loss == 1) {       // hinge
    const float ys = 2.f * y - 1.f;
    const float marg = ys * m;
    *l = fmaxf(1.f - marg, 0.f);
    *g = marg < 1.f ? -ys : 0.f;
  } else {                      // squared, label pre-scaled per problem
    const float r = m - y / ysc;
    *l = 0.5f * r * r;
    *g = r;
  }
}

// The dense block's part of one margin: acc += sum_k Xd[row][k] Vd[k][pc], k in order. VW values per lane and batch
// (4: one 16-byte load, rows are 16-byte aligned because nd % 4 == 0; 1: a dword load).
template <int PC, int VW>
__device__ __forceinline__ float dense_part(const float* __restrict__ xrow, bool row_ok, int nd,
                                            const float* __restrict__ Vd, int slot, int pc, float acc) {
  for (int base = 0; base < nd; base += VW * PC) {
    const int k0 = base + VW * pc;
    float xv[VW];
#pragma unroll
    for (int u = 0; u < VW; ++u) xv[u] = 0.f;
    if (row_ok && k0 < nd) {
      if (VW == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xrow + k0);
#pragma unroll
        for (int u = 0; u < VW; ++u) xv[u] = t[u];
      } else {
        xv[0] = xrow[k0];
      }
    }
    const int n = min(VW * PC, nd - base);          // wave-uniform; a multiple of VW
    const float* vk = Vd + base * PC + pc;
    for (int t = 0; t < n; t += VW) {
#pragma unroll
      for (int u = 0; u < VW; ++u) {
        const float x = __shfl(xv[u], slot * PC + t / VW, 64);
        acc = fmaf(x, vk[(t + u) * PC], acc);
      }
    }
  }
  return acc;
}

template <int PC, bool GRAD>
__global__ void __launch_bounds__(64 * kWaves) sparse_lr_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t N,
    const float* __restrict__ Vs, int ldv, const float* __restrict__ Xd, int nd, const float* __restrict__ Vdg,
    const float* __restrict__ madd, int ldm, const float* __restrict__ y, const float* __restrict__ W, int ldw,
    const int32_t* __restrict__ wmap, int P, const float* __restrict__ bias, int loss,
    const float* __restrict__ yscale, float* __restrict__ R, int ldr, double* __restrict__ f_part,
    double* __restrict__ r_part) {
  constexpr int RS = 64 / PC;                      // row slots per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double* sf = reinterpret_cast<double*>(lds_raw);                 // [2][kWaves][PC] wave partials
  float* Vd = reinterpret_cast<float*>(sf + 2 * kWaves * PC);      // [nd][PC]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int slot = lane / PC, pc = lane % PC;
  const int p = blockIdx.y * PC + pc;              // this lane's problem
  const bool p_ok = p < P;
  const int pl = p_ok ? p : P - 1;                 // a column that exists: loads need no guard, results are dropped
  const bool dense_in = Xd != nullptr && nd > 0;
  const bool dense_vec = (nd & 3) == 0 && (reinterpret_cast<uintptr_t>(Xd) & 15) == 0;    // 16-byte aligned rows

  if (dense_in) {
    for (int i = threadIdx.x; i < nd * PC; i += 64 * kWaves) {
      const int k = i / PC, j = blockIdx.y * PC + i % PC;
      Vd[i] = j < P ? Vdg[(int64_t)k * ldv + j] : 0.f;
    }
    __syncthreads();
  }
  const float bp = bias[pl];
  const float ysp = yscale ? yscale[pl] : 1.f;
  const int wc = wmap[pl];
  const float* vcol = Vs + pl;
  double f_acc = 0.0, r_acc = 0.0;

  const int64_t ngroups = (N + RS - 1) / RS;
  const int64_t gstride = (int64_t)gridDim.x * kWaves;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < ngroups; g += gstride) {
    const int64_t row = g * RS + slot;
    const bool row_ok = row < N;
    const int64_t a = row_ok ? row_ptr[row] : 0;
    const int nrow = row_ok ? (int)(row_ptr[row + 1] - a) : 0;
    int nmax = nrow;                               // the longest row of the wave's slots
    if (RS >= 2) nmax = max(nmax, __shfl_xor(nmax, 32, 64));
    if (RS >= 4) nmax = max(nmax, __shfl_xor(nmax, 16, 64));
    // the row's scalars ride ahead of the gathers
    const float yv = row_ok ? y[row] : 0.f;
    const float w = row_ok ? W[row * ldw + wc] : 0.f;
    const float ma = (madd != nullptr && row_ok) ? madd[row * ldm + pl] : 0.f;

    float acc = 0.f;
    for (int base = 0; base < nmax; base += PC) {
      const bool have = base + pc < nrow;
      const int my_i = have ? col[a + base + pc] : 0;
      const float my_v = have ? val[a + base + pc] : 0.f;
      const int n = min(PC, nmax - base);          // wave-uniform
      for (int t = 0; t < n; t += kU) {
        float xs[kU], vv[kU];
#pragma unroll
        for (int k = 0; k < kU; ++k) {
          const int src = slot * PC + t + k;       // t + k < PC: PC is a multiple of kU
          const int i = __shfl(my_i, src, 64);
          xs[k] = __shfl(my_v, src, 64);
          vv[k] = vcol[(int64_t)i * ldv];
        }
#pragma unroll
        for (int k = 0; k < kU; ++k) acc = fmaf(xs[k], base + t + k < nrow ? vv[k] : 0.f, acc);
      }
    }
    float dm = ma;                                 // the dense block's part: a sum of its own, or the caller's
    if (dense_in) {
      const float* xrow = Xd + (row_ok ? row : 0) * (int64_t)nd;
      dm = dense_vec ? dense_part<PC, 4>(xrow, row_ok, nd, Vd, slot, pc, 0.f)
                     : dense_part<PC, 1>(xrow, row_ok, nd, Vd, slot, pc, 0.f);
    }
    if (row_ok && p_ok) {
      float l, gd;
      loss_and_grad(loss, (acc + dm) + bp, yv, ysp, &l, &gd);
      f_acc = fma((double)l, (double)w, f_acc);
      r_acc = fma((double)gd, (double)w, r_acc);
      if (GRAD) R[row * ldr + p] = gd * w;
    }
  }

  // row slots by cross-lane moves, waves through LDS in wave order
  if (RS >= 2) {
    f_acc += __shfl_xor(f_acc, 32, 64);
    r_acc += __shfl_xor(r_acc, 32, 64);
  }
  if (RS >= 4) {
    f_acc += __shfl_xor(f_acc, 16, 64);
    r_acc += __shfl_xor(r_acc, 16, 64);
  }
  if (slot == 0) {
    sf[wave * PC + pc] = f_acc;
    sf[(kWaves + wave) * PC + pc] = r_acc;
  }
  __syncthreads();
  if (threadIdx.x < PC) {
    double fs = 0.0, rs = 0.0;
    for (int wv = 0; wv < kWaves; ++wv) {
      fs += sf[wv * PC + threadIdx.x];
      rs += sf[(kWaves + wv) * PC + threadIdx.x];
    }
    const int64_t o = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * PC + threadIdx.x;
    f_part[o] = fs;
    r_part[o] = rs;
  }
}

// f[p] = sum_b f_part[b][p], r[p] = sum_b r_part[b][p] in one fixed order: a wave per output, lane t adds the blocks
// t, t + 64, ... in order (independent loads; one thread walking all of them in turn cost more than the pass it
// follows), then the 64 lane sums are added in lane order
__global__ void __launch_bounds__(64) fold_partials_kernel(const double* __restrict__ f_part,
                                                           const double* __restrict__ r_part, int nblk, int width,
                                                           int P, double* __restrict__ f, double* __restrict__ r) {
  __shared__ double lane_sum[64];
  const int i = blockIdx.x;                        // 2 P outputs
  const int p = i < P ? i : i - P;
  const double* part = (i < P ? f_part : r_part) + p;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) acc += part[(int64_t)b * width];
  lane_sum[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int t = 0; t < 64; ++t) s += lane_sum[t];
    (i < P ? f : r)[p] = s;
  }
}

template <int PC>
int launch(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N, const float* Vs, int ldv,
           const float* Xd, int nd, const float* Vd, const float* madd, int ldm, const float* y, const float* W,
           int ldw, const int32_t* wmap, int P, const float* bias, int loss, const float* yscale, int grad, float* R,
           int ldr, double* f_part, double* r_part, int nblk, double* f, double* r, hipStream_t stream) {
  const dim3 grid((unsigned)nblk, (unsigned)((P + PC - 1) / PC));
  const size_t lds = 2 * kWaves * PC * sizeof(double) + (Xd ? (size_t)nd * PC * sizeof(float) : 0);
  if (grad)
    hipLaunchKernelGGL((sparse_lr_kernel<PC, true>), grid, dim3(64 * kWaves), lds, stream, row_ptr, col, val, N, Vs,
                       ldv, Xd, nd, Vd, madd, ldm, y, W, ldw, wmap, P, bias, loss, yscale, R, ldr, f_part, r_part);
  else
    hipLaunchKernelGGL((sparse_lr_kernel<PC, false>), grid, dim3(64 * kWaves), lds, stream, row_ptr, col, val, N, Vs,
                       ldv, Xd, nd, Vd, madd, ldm, y, W, ldw, wmap, P, bias, loss, yscale, R, ldr, f_part, r_part);
  hipLaunchKernelGGL(fold_partials_kernel, dim3((unsigned)(2 * P)), dim3(64), 0, stream, f_part, r_part,
                     nblk, (int)grid.y * PC, P, f, r);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int tmog_hip_sparse_lr_nd_max() { return kNdMax; }

int tmog_hip_sparse_lr_chunk(int P) { return P <= 16 ? 16 : P <= 32 ? 32 : 64; }

int tmog_hip_sparse_lr_objective(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                                 const float* Vs, int ldv, const float* Xd, int nd, const float* Vd,
                                 const float* madd, int ldm, const float* y, const float* W, int ldw,
                                 const int32_t* wmap, int P, const float* bias, int loss, const float* yscale,
                                 int grad, float* R, int ldr, double* f_part, double* r_part, int nblk, double* f,
                                 double* r, hipStream_t stream) {
  if (P <= 0 || nblk <= 0 || N < 0 || loss < 0 || loss > 2) return -2;
  if (Xd != nullptr && (nd < 0 || nd > kNdMax || Vd == nullptr)) return -2;
  if (grad && R == nullptr) return -2;
#define TM_SLR(PCV)                                                                                                  \
  return launch<PCV>(row_ptr, col, val, N, Vs, ldv, Xd, nd, Vd, madd, ldm, y, W, ldw, wmap, P, bias, loss, yscale,  \
                     grad, R, ldr, f_part, r_part, nblk, f, r, stream)
  const int pc = tmog_hip_sparse_lr_chunk(P);
  if (pc == 16) TM_SLR(16);
  if (pc == 32) TM_SLR(32);
  TM_SLR(64);
#undef TM_SLR
}

}  // extern "C"

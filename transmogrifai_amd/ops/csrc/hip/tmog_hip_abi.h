// The C ABI of libtmog_hip.so: every exported tmog_hip_* launcher, declared once.
//
// Every .hip translation unit includes this header, so hipcc checks each definition -- and each call from
// another translation unit -- against it, and ops/_native.py derives the ctypes signatures from it. Same
// restricted style as common/tmog_abi.h (one declaration per ';', named parameters, scalar types and pointers
// only). Kernel launchers return 0 on success (ops/_native.py check()).
#pragma once

#include <hip/hip_runtime.h>

#include "common/tmog_abi.h"

extern "C" {

// ---- hip/boost_kernels.hip
int tmog_hip_boost_epilogue(const uint32_t* entries, const int32_t* gid, int64_t n_entries, const float* gid_value,
                            const int64_t* gid_tree, const int64_t* tree_job, int64_t N, double* F, float* G,
                            float* H, const float* y, int objective, int32_t* auc_hist, int bins, int64_t n_gid,
                            int64_t n_trees, int64_t P, hipStream_t stream, uint32_t* amax, int wide_rows);
int tmog_hip_boost_prologue(const uint32_t* tam_prev, uint32_t* tam_next, const float* comp, float* amax, int P,
                            const int32_t* act, int T, const int64_t* job_off, const uint32_t* root, uint32_t* rows,
                            int64_t total, const float* G, const float* H, int64_t stride, int32_t* gh, float* qscale,
                            double* qinv, float qmax, int wide, hipStream_t stream);
int tmog_hip_poisson_pack(const int64_t* rows, int64_t n, const int64_t* offsets, int k, const double* cdf, int ncdf,
                          unsigned long long* counts, const int64_t* base, int32_t* out, hipStream_t stream);
int tmog_hip_row_uniform(const int64_t* row_ids, int64_t n, const int64_t* offsets, int k_seeds, double* out,
                         hipStream_t stream);
int tmog_hip_aupr_counts(const int32_t* counts, int K, int bins, double* out, hipStream_t stream);

// ---- hip/boost_multi_kernels.hip
int tmog_hip_boost_margin_add(const uint32_t* entries, const int32_t* gid, int64_t n_entries, const float* gid_value,
                              const int64_t* gid_tree, const int64_t* tree_job, int64_t N, double* F, int64_t n_gid,
                              int64_t n_trees, int64_t Q, int wide_rows, hipStream_t stream);
int tmog_hip_softmax_grad(const int64_t* rows, const int64_t* row_off, const int64_t* models, int M, int64_t max_rows,
                          int K, int64_t N, int64_t P, const double* F, const float* y, float* G, float* H,
                          uint32_t* amax, int32_t* err, hipStream_t stream);

// ---- hip/csv_kernels.hip
int tmog_hip_csv_fields(const uint8_t* buf, const int64_t* row_start, const int64_t* row_end, int64_t nrows,
                        int ncols, int sep, int64_t* fstart, int32_t* nfields, hipStream_t stream);
int tmog_hip_csv_parse_num(const uint8_t* buf, const int64_t* fstart, const int32_t* nfields, int64_t nrows,
                           int ncols, const int32_t* cols, const int32_t* kind, int nout, int64_t* out,
                           uint8_t* valid, uint8_t* slow, hipStream_t stream);
int tmog_hip_csv_hash_text(const uint8_t* buf, const int64_t* fstart, const int32_t* nfields, int64_t nrows,
                           int ncols, const int32_t* cols, int nout, uint64_t* hash, int64_t* span, uint64_t* check,
                           hipStream_t stream);

// ---- hip/dense_kernels.hip
int tmog_hip_rowgemm(const float* A, int64_t lda, int64_t a_pstride, const float* B, int64_t ldb, int64_t b_pstride,
                     int btrans, int bg, int64_t b_gstride, const float* bias, int64_t bias_pstride,
                     int64_t bias_gstride, float* C, int64_t ldc, int64_t c_pstride, int cg, int64_t c_gstride,
                     int64_t N, int K, int M, int P, int epi, hipStream_t stream);
int tmog_hip_xtd_chunks(int64_t N, int K, int M, int P, int target_blocks);
int tmog_hip_xtd(const float* A, int64_t lda, int64_t a_pstride, const float* D, int64_t ldd, int64_t d_pstride,
                 int dg, int64_t d_gstride, int64_t N, int K, int M, int P, int S, float* part, double* out,
                 hipStream_t stream);

// ---- hip/lda_kernels.hip: documents as CSR (int32 columns sorted per row, fp32 counts), expEbT [V][K] fp64.
// tmog_hip_lda_lds_terms is the number of terms of one document that iterate out of LDS (0 for an unsupported K);
// queue is one word of scratch for the document queue; partial holds n_seg x K doubles
int tmog_hip_lda_lds_terms(int K);
int tmog_hip_lda_estep(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N, const double* expEbT,
                       int K, const double* alpha, int iters, double tol, uint32_t* queue, double* gamma,
                       int32_t* n_iter, double* expEt, double* r, hipStream_t stream);
int tmog_hip_lda_sstats(const int64_t* seg_begin, const int32_t* csc_row, const int64_t* csc_pos, int64_t n_seg,
                        const int64_t* col_seg, int64_t V, const double* expEt, const double* r, const double* expEbT,
                        int K, double* partial, double* sstats, hipStream_t stream);

// ---- hip/w2v_kernels.hip: tables [V][Dp] fp32 (Dp a multiple of 16, at most 256), the corpus as token ids with
// doc_ptr [N + 1] / doc_id [T]; slabs gin, gout [B][16][Dp] with keys [B][16] (V: no row). n_pos is one word on the
// device (the valid context slots of the batch), lr the SGD rate: a_pos = lr / n_pos, a_neg = a_pos / S.
// tmog_hip_w2v_apply takes the keys sorted (stable) with order[i] the slab row of sorted position i;
// tmog_hip_w2v_seg_cap is the number of slab rows summed before a run of equal keys is cut; partial holds
// 2 * ceil(M / cap) * Dp floats and tail ceil(M / cap) words of scratch
int tmog_hip_w2v_seg_cap();
int tmog_hip_w2v_window(const float* emb_in, const float* emb_out, int V, int Dp, const int32_t* tok, int64_t T,
                        const int64_t* doc_ptr, const int32_t* doc_id, const int32_t* pos, const int32_t* neg, int B,
                        int w, int S, const int32_t* n_pos, float lr, float* gin, float* gout, int32_t* key_in,
                        int32_t* key_out, hipStream_t stream);
int tmog_hip_w2v_apply(float* emb, int V, int Dp, const float* slab, const int32_t* skey, const int64_t* order,
                       int64_t M, float* partial, int32_t* tail, hipStream_t stream);
int tmog_hip_w2v_doc_mean(const float* vec, int V, int D, const int32_t* tok, const int64_t* doc_ptr, int64_t N,
                          float* out, hipStream_t stream);

// ---- hip/linear_bf16_kernels.hip
int tmog_hip_lr_bf16_blocks_per_cu(int dpad, int grad);
int tmog_hip_lr_bf16(const void* Xr, int64_t ldr, int64_t N, int dpad, const float* y, const float* W, int ldw,
                     const int32_t* wcol, int pc, const float* V, const float* bias, int loss, const float* yscale,
                     int grad, double* fp, double* rp, float* gp, int nblk, hipStream_t stream);

// ---- hip/linear_kernels.hip
int tmog_hip_lr_epilogue_grad(const float* X, int64_t N, int d, const float* M, const float* y, const float* W,
                              int ldw, int wcol0, int P, const float* bias, int loss, const float* yscale, int grad,
                              double* f_part, double* r_part, float* G_part, int nblk, hipStream_t stream);
int tmog_hip_lr_blocks_per_cu(int grad);
int tmog_hip_lr_objective(const float* X, int64_t N, int d, const float* y, const float* W, int ldw, int wcol0, int P,
                          const float* V, const float* bias, int loss, const float* yscale, int grad, double* f_part,
                          double* r_part, float* G_part, int nblk, hipStream_t stream);
int tmog_hip_lr_objective_mixed(const void* Xm, int64_t N, int d, const int32_t* colmap, int cpr, int nce,
                                const float* y, const float* W, int ldw, int wcol0, int P, const float* V,
                                const float* bias, int loss, const float* yscale, int grad, double* f_part,
                                double* r_part, float* G_part, int nblk, hipStream_t stream);
int tmog_hip_owlqn_direction(const double* U, const double* g, const double* l1, const double* S, const double* Y,
                             const double* RHO, int d1, int P, int m, int hist_n, double* D, double* pg, double* xi,
                             double* dnorm, hipStream_t stream);
int tmog_hip_owlqn_candidate(const double* U, const double* D, const double* xi, const double* l1, const double* pg,
                             const double* alpha, int d1, int P, double* cand, double* l1t, double* dd,
                             hipStream_t stream);

// ---- hip/loco_kernels.hip
int tmog_hip_forest_loco(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         const int32_t* slot_meta, int G, int64_t T, const int64_t* tree_off, const int32_t* nodes,
                         int64_t n_nodes, const float* value, int KV, const float* tree_weight,
                         const int32_t* tree_out, int missing_bin, int C, double scale, double* out,
                         hipStream_t stream);

// ---- hip/loco_linear_kernels.hip
int tmog_hip_loco_linear(const void* X, int x_fp64, int64_t n, int d, int64_t ldx, const double* W, const double* b,
                         int Cm, int link, double link_param, const int32_t* cand_of_col, int n_plain, int G,
                         const double* gsize, int top_k, int abs_mode, int leave_out, int64_t* cols, double* diffs,
                         hipStream_t stream);

// ---- hip/metric_kernels.hip
int tmog_hip_binary_areas(const void* s, int is_f64, const int64_t* idx, int64_t n, int J, const uint8_t* lab,
                          double* out_pr, double* out_roc, hipStream_t stream);

// ---- hip/mlp_kernels.hip
int tmog_hip_mlp_bias_sigmoid(float* Z, int P, int64_t N, int B, const float* bias, hipStream_t stream);
int tmog_hip_mlp_sigmoid_backprop(float* D, const float* A, int P, int64_t N, int B, int nblk, double* part,
                                  hipStream_t stream);

// ---- hip/mnl_kernels.hip
int tmog_hip_mnl_epilogue(const float* M2, int64_t N, int P, int K, const float* bias, const float* y, const float* W,
                          int ldw, const int32_t* wmap, int grad, void* R2, double* f_part, double* r_part, int nblk,
                          hipStream_t stream);
int tmog_hip_mnl_bf16(const void* X, int64_t ldx, int64_t N, int dpad, const float* y, const float* W, int ldw,
                      const int32_t* wcol, int pc, int K, const void* Vt, const float* bias, int grad, void* R2,
                      double* f_part, double* r_part, int nblk, hipStream_t stream);

// ---- hip/quantize_kernels.hip
int tmog_hip_quantize(const float* X, int64_t N, int F, const float* thr, int MS, int missing_bin, int has_mv,
                      float missing_value, uint8_t* out, hipStream_t stream);

// ---- hip/pd_kernels.hip
int tmog_hip_forest_pd(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                       const int32_t* slot_of_used, int Q, int NB, int64_t T, const int64_t* tree_off,
                       const int32_t* nodes, int64_t n_nodes, const float* value, int KV, const float* tree_weight,
                       const int32_t* tree_out, int missing_bin, int C, double scale, int mode, void* out,
                       hipStream_t stream);

// ---- hip/pd_pair_kernels.hip
int tmog_hip_forest_pd_pairs(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                             const int32_t* pair_slots, int Pn, int NB, int64_t T, const int64_t* tree_off,
                             const int32_t* nodes, int64_t n_nodes, const float* value, int KV,
                             const float* tree_weight, const int32_t* tree_out, int missing_bin, int C, double scale,
                             int mode, void* out, hipStream_t stream);

// ---- hip/rff_kernels.hip
int tmog_hip_rff_summary(const void* const* vals, const uint8_t* const* valid, const int32_t* dtype, int64_t n, int F,
                         const void* label, int label_dt, double* out, hipStream_t stream);
int tmog_hip_rff_hist(const void* const* vals, const uint8_t* const* valid, const int32_t* dtype, int64_t n, int F,
                      const double* lo, const double* hi, int bins, unsigned int* hist, hipStream_t stream);

// ---- hip/shap_kernels.hip
int tmog_hip_forest_shap(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         int64_t P, const int64_t* p_off, const int32_t* p_out, const double* p_val, int KV,
                         const double* bias, const int32_t* e_feat, const int32_t* e_rng, const double* e_z,
                         const int64_t* bin_off, int missing_bin, int C, double scale, double* out,
                         hipStream_t stream);
int tmog_hip_forest_shap_interactions(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U,
                                      const int32_t* used, int64_t P, const int64_t* p_off, const int32_t* p_out,
                                      const double* p_val, int KV, const double* bias, const int32_t* e_feat,
                                      const int32_t* e_rng, const double* e_z, const int64_t* bin_off,
                                      int missing_bin, int C, double scale, double* tri, hipStream_t stream);

// ---- hip/sparse_kernels.hip
int tmog_hip_csr_spmm(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N, const float* V, int C,
                      float* M, int ldm, int accumulate, hipStream_t stream);
int tmog_hip_csc_spmm_t(const int64_t* seg_begin, const int32_t* row, const float* val, int64_t n_seg,
                        const int64_t* col_seg, int64_t ds, const float* R, int C, int ldr, float* partial, double* G,
                        hipStream_t stream);
int tmog_hip_softmax_epilogue(float* M, int64_t N, int P, int K, const float* bias, const float* y, const float* W,
                              int ldw, float* Lw, int grad, hipStream_t stream);
int tmog_hip_colsum(const float* R, int64_t N, int C, int nblk, double* part, hipStream_t stream);

// ---- hip/sparse_build_kernels.hip: the CSR and the CSC of the non-zeros of a dense device matrix X [N][d] (fp32, or
// fp64 with f64; row stride ldx elements, unit column stride; d <= TMOG_SPARSE_BUILD_DMAX, N < 2^31), in row tiles of
// TMOG_SPARSE_BUILD_TR rows, T = ceil(N / TR) of them. tmog_hip_sparse_build_count writes tile_cnt [T][d] (non-zeros
// of a column in a tile) and nz [d] (of a column). tmog_hip_sparse_build_fill takes smap [d] (a column's rank among the
// kept columns, ascending, or -1) and col_start [kept + 1] (the kept columns' first CSC positions, the scan of their
// nz) and writes row_ptr [N + 1], col / val [nnz] (CSR, row-major, columns ascending) and csc_row [nnz] (CSC,
// column-major, rows ascending), csc_val / csc_val_sq / csc_pos [nnz] (the value, its square, the CSR position; each
// skipped when null) and row_sum [N] (fp64, a row's values added in column order; skipped when null). Scratch:
// tile_off [T][d] int32, tile_nnz [T], tile_start [T + 1]. No atomics: two runs write the same bits
#define TMOG_SPARSE_BUILD_TR 64
#define TMOG_SPARSE_BUILD_DMAX 16384
int tmog_hip_sparse_build_count(const void* X, int f64, int64_t ldx, int64_t N, int d, uint8_t* tile_cnt, int64_t* nz,
                                hipStream_t stream);
int tmog_hip_sparse_build_fill(const void* X, int f64, int64_t ldx, int64_t N, int d, const int32_t* smap,
                               const int64_t* col_start, const uint8_t* tile_cnt, int32_t* tile_off,
                               int32_t* tile_nnz, int64_t* tile_start, int64_t* row_ptr, int32_t* col, float* val,
                               int32_t* csc_row, float* csc_val, float* csc_val_sq, int64_t* csc_pos,
                               double* row_sum, hipStream_t stream);

// ---- hip/sparse_lr_kernels.hip: the fused binary objective on a sparse design (CSR of the sparse columns with
// Vs [ds][ldv], dense block Xd [N][nd] with Vd [nd][ldv], nd <= tmog_hip_sparse_lr_nd_max(); Xd null: no dense block
// in the kernel, madd [N][ldm] -- or null -- is added to the margins instead). Problem p weighs row i by
// W[i][wmap[p]]. f_part / r_part hold nblk x ceil(P / chunk) x chunk doubles, chunk = tmog_hip_sparse_lr_chunk(P);
// f [P] and r [P] are their sums in a fixed order; R [N][ldr] is written only with grad
int tmog_hip_sparse_lr_nd_max();
int tmog_hip_sparse_lr_chunk(int P);
int tmog_hip_sparse_lr_objective(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                                 const float* Vs, int ldv, const float* Xd, int nd, const float* Vd,
                                 const float* madd, int ldm, const float* y, const float* W, int ldw,
                                 const int32_t* wmap, int P, const float* bias, int loss, const float* yscale,
                                 int grad, float* R, int ldr, double* f_part, double* r_part, int nblk, double* f,
                                 double* r, hipStream_t stream);

// ---- hip/sparse_mnl_kernels.hip: the fused multinomial objective on a sparse design, P problems of 2 <= K <= 16
// classes, columns p*K + k (Vs [ds][ldv], Xd / Vd / madd / W / wmap as for tmog_hip_sparse_lr_objective, nd <=
// tmog_hip_sparse_mnl_nd_max(); y holds class ids, one outside [0, K): loss 0, no one-hot term). A launch runs
// chunk = tmog_hip_sparse_mnl_chunk(P, K) problems side by side on rows = tmog_hip_sparse_mnl_rows(P, K) rows a wave
// (both 0 for an unsupported P or K); f_part / r_part hold nblk x ceil(P / chunk) x (64 / rows) doubles; out
// [P + P*K] is f [P] then rsum [P*K], their sums in a fixed order; R [N][ldr] is written only with grad
int tmog_hip_sparse_mnl_nd_max();
int tmog_hip_sparse_mnl_chunk(int P, int K);
int tmog_hip_sparse_mnl_rows(int P, int K);
int tmog_hip_sparse_mnl_objective(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                                  const float* Vs, int ldv, const float* Xd, int nd, const float* Vd,
                                  const float* madd, int ldm, const float* y, const float* W, int ldw,
                                  const int32_t* wmap, int P, int K, const float* bias, int grad, float* R, int ldr,
                                  double* f_part, double* r_part, int nblk, double* out, hipStream_t stream);

// ---- hip/sparse_mlp_kernels.hip: one objective pass of P multilayer perceptrons (one or two sigmoid hidden layers
// of width h1, h2 <= 64, h2 = 0 for one; softmax over 2 <= K <= 16 classes) on a sparse design, nd <=
// tmog_hip_sparse_mlp_nd_max(). Per problem: W1s [ds][h1], W1d [nd][h1], b1 [h1], Wm [h1][h2], bm [h2] (h2 > 0),
// WL [h2 or h1][K], bL [K]; row weights W[i][p], wsum [P] their sums in fp32. part holds P x nblk x 4 wave rows of
// tmog_hip_sparse_mlp_npart(h1, h2) doubles; out [P][npart] is their sum in a fixed order: the loss sum | db1 |
// dWm | dbm | dWL | dbL, each padded to tmog_hip_sparse_mlp_pad() of its widths (K to 16), gradients of the
// weighted mean. Without grad only out[p][0] is written and nothing per row; with grad dZ1[i][p * h1 + j] too
int tmog_hip_sparse_mlp_nd_max();
int tmog_hip_sparse_mlp_pad(int width);
int tmog_hip_sparse_mlp_npart(int h1, int h2);
int tmog_hip_sparse_mlp_pass(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                             const float* W1s, int ds, const float* Xd, int nd, const float* W1d, const float* b1,
                             const float* Wm, const float* bm, const float* WL, const float* bL, const float* y,
                             const float* W, int ldw, const float* wsum, int P, int h1, int h2, int K, int grad,
                             float* dZ1, int64_t ldz, double* part, int nblk, double* out, hipStream_t stream);

// ---- hip/sparse_gram_kernels.hip: fp64 weighted Grams and margins of a sparse design (ops/linear.py SparseDesign:
// CSR row_ptr / col / val and segmented CSC seg_begin / csc_row / csc_val / col_seg of the ds sparse columns, dense
// block Xd [N][dd]). tmog_hip_sparse_wgram writes, for k < K, every row and column of G [K][D][D] (D = ds + dd + 1,
// + 1 with Y) that belongs to a sparse column: G_k = A_k^T diag(W[:, k]) A_k, A_k = [X | 1 | Y_k] (Y [N][ldy], column
// k with per_weight, else column 0; null: no response column). pos [ds + dd + 1 (+ 1)] is the row / column of G of
// the sparse columns, then the dense columns, then the 1 and Y columns; the block of the latter three is the caller's.
// An item is `nslice` segments of one column: item_col / item_seg [n_items] (column, first segment; columns ascending)
// and col_item [ds + 1] (first item of a column). wp <= tmog_hip_sparse_wgram_width_max() positions are served in
// one pass (wider blocks in ranges of wp), dd <= tmog_hip_sparse_wgram_dd_max(), and the partial buffer
// n_items x tmog_hip_sparse_wgram_kw() x wp doubles stays within tmog_hip_sparse_wgram_part_bytes().
// tmog_hip_sparse_margin_f64 writes eta [N][lde] (columns < P) = Xs Bs + Xd Bd + b0 with Bs [ds][ldb], Bd [dd][ldb],
// b0 [P] or null, all fp64
int tmog_hip_sparse_wgram_kw();
int tmog_hip_sparse_wgram_width_max();
int tmog_hip_sparse_wgram_dd_max();
int64_t tmog_hip_sparse_wgram_part_bytes();
int tmog_hip_sparse_wgram(const int64_t* seg_begin, const int32_t* csc_row, const float* csc_val,
                          const int64_t* col_seg, const int32_t* item_col, const int64_t* item_seg,
                          const int64_t* col_item, int64_t n_items, int nslice, const int64_t* row_ptr,
                          const int32_t* col, const float* val, int64_t N, int ds, const float* Xd, int dd,
                          const double* W, int64_t ldw, int K, const double* Y, int64_t ldy, int per_weight,
                          const int32_t* pos, int wp, double* G, hipStream_t stream);
int tmog_hip_sparse_margin_f64(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t N,
                               const double* Bs, int ldb, const float* Xd, int dd, const double* Bd, const double* b0,
                               int P, double* eta, int64_t lde, hipStream_t stream);

// ---- hip/stats_kernels.hip
int tmog_hip_class_colsum(const float* X, int64_t n, int d, int64_t ld, const int32_t* codes, int P, int L,
                          double* out, hipStream_t stream);
int tmog_hip_col_stats(const float* X, const void* unused, int64_t n, int d, int64_t ld, double* out,
                       hipStream_t stream);
int tmog_hip_weighted_colsums(const float* X, int64_t n, int d, int64_t ldx, const float* W, int64_t ldw, int P,
                              double* out, hipStream_t stream);
int tmog_hip_wgram(const float* X, int64_t n, int d, int64_t ldx, const double* W, int64_t ldw, int K,
                   const double* Y, int64_t ldy, int per_weight, double* G, hipStream_t stream);
int tmog_hip_gram_aug(const float* X, int64_t n, int d, int64_t ld, const float* mu, const int32_t* y, int L,
                      double* G, hipStream_t stream);
int tmog_hip_col_bf16_exact(const float* X, int64_t n, int d, int64_t ld, unsigned* low_bits, hipStream_t stream);
int tmog_hip_bf16_pack(const float* X, int64_t n, int64_t ld, const int32_t* y, const int32_t* src,
                       const int32_t* mode, const float* mu, const float* sc, void* B, int64_t ldb,
                       hipStream_t stream);
int tmog_hip_gram_bf16(const void* A, int64_t n, int64_t lda, int D, double* G, hipStream_t stream);

// ---- hip/text_kernels.hip
int tmog_hip_hash_tokens(const uint8_t* data, const int64_t* tok_offs, int64_t T, const uint8_t* prefix, int32_t plen,
                         int32_t seed, int32_t num_features, int32_t base, int32_t* out, hipStream_t stream);
int tmog_hip_hash_tf_rows(const void* feats, int n_feats, int64_t n, int W, int binary, float* out, int64_t ld,
                          int64_t off, hipStream_t stream);
int tmog_hip_hash_feat_bytes();
int tmog_hip_code_count(const void* codes, const int32_t* nv, int max_v, int n_cols, int64_t n, void* counts,
                        hipStream_t stream);
int tmog_hip_bucketize(const double* x, const uint8_t* ok, int64_t n, const double* splits, int ns, int left_incl,
                       int track_invalid, int track_nulls, float* out, int64_t ld, int64_t off, int width,
                       unsigned long long* bad, hipStream_t stream);
int tmog_hip_date_unit_circle(const int64_t* ms, const uint8_t* ok, int64_t n, int period, int shift, int size,
                              float* out, int64_t ld, int64_t off, hipStream_t stream);

// ---- hip/tree_grow_hip.hip: the native grower on the GPU backend. The handle is a GrowResult
void* tmog_hip_grow_forest(const GrowArgs* args);
void tmog_hip_grow_timing(int64_t* out, int reset);
int tmog_hip_slot_stream(int slot, void* stream, int set);
void tmog_hip_set_oom_handler(void (*fn)());
void tmog_hip_fail_alloc(long n);
int tmog_hip_grow_status(void* h, char* msg, int cap);
int64_t tmog_hip_grow_nodes(void* h, int g);
int64_t tmog_hip_grow_leaf_count(void* h, int g);
void tmog_hip_grow_copy(void* h, int g, int64_t* tree, int64_t* feat, int64_t* bin, uint8_t* dl, double* gain,
                        double* tot, int64_t* left, int64_t* right);
void tmog_hip_grow_free(void* h);
int tmog_hip_rccl_unique_id(char* out, int cap);
void* tmog_hip_rccl_comm_init(const char* id_bytes, int world, int rank);
int tmog_hip_fp_allgather(const void* send, void* recv, int64_t bytes, void* comm, int world, hipStream_t stream);
int tmog_hip_rccl_comm_destroy(void* comm);

// ---- The tree level kernels, four translation units. `items` are HistItem / PartItem / LeafItem arrays on the device.
// The trailing `const int*` of a launcher (dcount, dm, dnp, dn) is null for host-planned levels; for device-planned
// levels (tree_resident.hip) it points at the item / node / pair / segment count on the device and the count passed by
// value is an upper bound that sizes the grid.

// ---- hip/tree_hist_kernels.hip: histograms; tmog_hip_tree_prime loads the code objects of all four units
int tmog_hip_debug_flags(int flags);
int tmog_hip_hist_build(const uint8_t* Xb, int F, const uint32_t* rows, const void* items, int n_items,
                        const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* node_model,
                        const int64_t* node_hist_off, int64_t* hist, int B, int mode, int S, const float* y,
                        const float* t1, const float* t2, int64_t stride, const float* qscale, int skip_bin,
                        const int64_t* csr_ptr, const uint16_t* csr_col, int Sc, int n_wide, int need_general,
                        hipStream_t stream, const int32_t* gh_words, const int* dcount, int wide_rows,
                        const uint8_t* Xh, int Fh);
int tmog_hip_hist_subtract(int64_t* hist, const int64_t* parent, const int64_t* parent_off, const int64_t* small_off,
                           const int64_t* out_off, const int64_t* size, int n, int64_t max_size, int64_t dense,
                           int per, int S, hipStream_t stream);
int tmog_hip_zero_segments(int64_t* hist, const int64_t* off, const int64_t* size, int n, int64_t max_size,
                           int64_t dense, int per, int S, hipStream_t stream, int n_dense, const int* dn);
int tmog_hip_tree_prime();
int tmog_hip_hist_stat_chunk(int B, int S);

// ---- hip/tree_split_kernels.hip: split finding
int tmog_hip_split_find(const int64_t* hist, int n_nodes, const int64_t* node_hist_off, const int32_t* node_nfeat,
                        const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* feat_nbins, int B,
                        int S, int kind, const float* node_params, int missing_bin, const int32_t* node_model,
                        const double* qinv, int max_nfeat, void* cand_ws, int32_t* out_feat, int32_t* out_bin,
                        float* out_gain, uint8_t* out_dl, float* out_left, float* out_total, int64_t* cursors,
                        int n_multi, void* rec, int64_t rec_bytes, int fp_mlo, int fp_nml, int fp_obase,
                        hipStream_t stream, unsigned* done, const int* dm);
int tmog_hip_pair_scan(int64_t* hist, const int64_t* parent, const int64_t* parent_off, const int32_t* small_j,
                       const int32_t* big_j, int n_pairs, const int64_t* node_hist_off, const int32_t* node_nfeat,
                       const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* feat_nbins, int B,
                       int S, int kind, const float* node_params, int missing_bin, const int32_t* node_model,
                       const double* qinv, int max_nfeat, void* cand_ws, int n_multi, hipStream_t stream,
                       const int* dnp);
int tmog_hip_fp_merge(const void* recv, int R, int m, int64_t rec_bytes, int S, int32_t* out_feat, int32_t* out_bin,
                      float* out_gain, uint8_t* out_dl, float* out_left, hipStream_t stream);
int tmog_hip_fp_merge_dev(const void* recv, int R, int m_stride, int64_t rec_bytes, int S, int32_t* out_feat,
                          int32_t* out_bin, float* out_gain, uint8_t* out_dl, float* out_left, const int* dm,
                          hipStream_t stream);
size_t tmog_hip_split_cand_bytes(int n_nodes, int max_nfeat, int B, int S);

// ---- hip/tree_partition_kernels.hip: row partition and leaf collection
int tmog_hip_partition_fused(const uint8_t* Xb, int F, const uint32_t* rows_in, uint32_t* rows_out, const void* items,
                             int n_items, const int64_t* node_begin, const int64_t* node_count,
                             const int32_t* split_feat, const int32_t* split_bin, const uint8_t* dl,
                             const float* node_params, const float* split_gain, int missing_bin, int64_t* cursors,
                             const uint8_t* XbT, int64_t N, hipStream_t stream, const int32_t* gh_in, int32_t* gh_out,
                             const int* dcount, int wide_rows);
int tmog_hip_leaf_collect(const uint32_t* rows, const void* items, int n_items, uint32_t* out_rows, int32_t* out_gid,
                          hipStream_t stream, const uint32_t* rows_alt, const int* dcount);

// ---- hip/forest_predict_kernels.hip: forest scoring over the growers' node arrays
int tmog_hip_forest_predict_multi(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                  const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                  const int64_t* tree_off, const float* tree_weight, const int32_t* nodes,
                                  const uint8_t* default_left, int missing_bin, const float* leaf_value, int K,
                                  const uint32_t* node_mask, const int32_t* var_off, const int32_t* var_depth,
                                  const int64_t* var_out_off, float* out, hipStream_t stream);
int tmog_hip_forest_predict(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                            const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                            const int64_t* tree_off, const float* tree_weight, const int32_t* nodes,
                            const uint8_t* default_left, int missing_bin, const float* leaf_value, int K, float* out,
                            hipStream_t stream);
// The same scoring over a packed node image (16 bytes per node: feat | bin << 16 | default_left << 24, variant stop
// mask, left, right) that tmog_hip_forest_image builds once per forest; tmog_hip_predict_v1 is TMOG_PREDICT_V1=1,
// which selects the direct node source (the two entries above) for every forest.
int tmog_hip_predict_v1();
int tmog_hip_forest_image(const int32_t* nodes, const uint8_t* default_left, const uint32_t* node_mask, int64_t n,
                          int32_t* image, hipStream_t stream);
int tmog_hip_forest_predict_multi_image(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                        const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                        const int64_t* tree_off, const float* tree_weight, const int32_t* image,
                                        int missing_bin, const float* leaf_value, int K, const int32_t* var_off,
                                        const int32_t* var_depth, const int64_t* var_out_off, int max_variants,
                                        float* out, hipStream_t stream);
int tmog_hip_forest_predict_image(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                                  const int32_t* row_list, int64_t max_rows, const int64_t* model_tree_off,
                                  const int64_t* tree_off, const float* tree_weight, const int32_t* image,
                                  int missing_bin, const float* leaf_value, int K, float* out, hipStream_t stream);

// ---- hip/staged_eval_kernels.hip: the contract of tmog_forest_staged_eval_cpu (common/tmog_abi.h); slab holds
// ceil(n / TMOG_EVAL_BLOCK) x S doubles, the per-workgroup partial sums that values[] is reduced from in a fixed order
int tmog_hip_forest_staged_eval(const uint8_t* Xb, int F, const int32_t* row_list, int64_t n, const float* y,
                                const int32_t* nodes, const uint8_t* default_left, const float* leaf_value,
                                const int64_t* tree_off, const float* tree_weight, int missing_bin,
                                const int64_t* stage_off, int S, const int32_t* tree_col, int K, int metric,
                                double scale, int bins, double* margins, double* values, int64_t* counts,
                                int32_t* tables, double* slab, hipStream_t stream);

// ---- hip/tree_resident.hip: device-planned growth of one job group on the caller's stream
int64_t tmog_hip_resident_cap_nodes(const GrowArgs* args);
int tmog_hip_plan_profile(uint64_t* out, int reset);
int tmog_hip_resident_error(char* msg, int cap);
int tmog_hip_grow_resident(const GrowArgs* args, const ResidentIO* io);

// ---- hip/vector_kernels.hip
int tmog_hip_masked_colsum(const void* vals, const void* valid, const int32_t* dtype, int n_cols, int64_t n,
                           int64_t rows_per_chunk, double* part, hipStream_t stream);
int tmog_hip_gather_rows_cols(const void* col_base, const int64_t* col_ld, const int64_t* rows, int64_t m, int k,
                              float* out, hipStream_t stream);
int tmog_hip_onehot_pivot(const void* codes, const void* luts, const int32_t* lut_n, const int64_t* off, int n_cols,
                          int64_t n, float* out, int64_t W, hipStream_t stream);
int tmog_hip_vectorize_numeric(const void* vals, const void* valid, const float* fills, int64_t n, int F,
                               const void* r1, const void* r2, const void* r3, float* out, int64_t W, int track,
                               hipStream_t stream);

}  // extern "C"

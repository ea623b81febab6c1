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

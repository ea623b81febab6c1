// The C ABI of libtmog_host.so, and the structs and constants both native libraries share with Python.
//
// This header is the ONLY declaration of these entry points. Every host translation unit includes it, so the
// compiler checks each definition against it (a conflicting extern "C" redeclaration is an error), and
// ops/_native.py reads it to derive the ctypes signatures, struct layouts and constants -- nothing is retyped.
//
// Restricted style, so that the small reader in ops/_native.py stays a reader and not a C parser: plain C, one
// declaration per ';', every parameter named, only fixed-width / builtin scalar types and pointers, no macros or
// default arguments inside parameter lists, constants as `#define NAME integer`. Comments are free.
// (The two CPython-API functions of host/utf8_pack.cpp take PyObject* and stay declared where they are loaded.)
#pragma once

#include <assert.h>
#include <stddef.h>
#include <stdint.h>

// ---- constants mirrored by Python (models/tree_engine.py reads them from here)
#define TMOG_N_SLOTS 32            // native per-group resource slots of the GPU grower (tree_grow_hip.hip slots())
#define TMOG_SLOT_LANE 8           // slots one concurrently running learner thread owns
#define TMOG_REC_FIXED 7           // resident record words before the S totals: tree feat bin dl gain left right
#define TMOG_CSR_ITEM_ROWS 1024    // rows per CSR histogram item (GPU)
#define TMOG_PART_ITEM_ROWS 1024   // rows per partition item (GPU)
#define TMOG_PM_VK 32              // forest_predict_multi_kernel: variants x classes accumulated per thread

// ---- metrics of the staged forest evaluation (common/boost_eval.hpp has the per-row terms)
#define TMOG_EVAL_LOGLOSS 0        // binary, K = 1: floating sum
#define TMOG_EVAL_ERROR 1          // binary: count
#define TMOG_EVAL_AUPR 2           // binary: [2][bins] count table per stage
#define TMOG_EVAL_SQERR 3          // regression: floating sum
#define TMOG_EVAL_ABSERR 4         // regression: floating sum
#define TMOG_EVAL_MLOGLOSS 5       // K classes: floating sum
#define TMOG_EVAL_MERROR 6         // K classes: count
#define TMOG_EVAL_BLOCK 256        // rows per workgroup of the kernel: its slab holds ceil(n / 256) x S partial sums

// ---- flags of a histogram item (HistItem.excl); REG, CSR and WIDE are also the flags of a feature group
#define TMOG_ITEM_SOLE 1           // this item alone covers the node's rows for its features (plain stores)
#define TMOG_ITEM_REG 2            // every feature of the group has one present bin (register accumulation)
#define TMOG_ITEM_CSR 4            // CSR item: walks the rows' lists of one-present-bin columns
#define TMOG_ITEM_LIVE0 8          // only the bin-0 words of each feature are written out
#define TMOG_ITEM_WIDE 16          // wide-load item: contiguous dword-aligned physical columns
#define TMOG_ITEM_SC_SHIFT 8       // bits 8..15: statistic chunk

// ---- work items of the tree level kernels (hip/tree_hist_kernels.hip, hip/tree_partition_kernels.hip), laid out by
// common/tree_plan.hpp for the host planner (common/tree_grow.hpp) and the device planner (hip/tree_resident.hip)
typedef struct FeatGroup {
  int32_t f0, nf;   // local features [f0, f0 + nf) of one histogram item (nf <= 64)
  int32_t flags;    // TMOG_ITEM_REG | TMOG_ITEM_CSR | TMOG_ITEM_WIDE
} FeatGroup;

typedef struct HistItem {
  int32_t node;     // node slot
  int32_t fg0;      // first local feature of this group
  int32_t nf;       // features in this group (<= 64)
  int32_t excl;     // TMOG_ITEM_* flags | statistic chunk << TMOG_ITEM_SC_SHIFT
  int64_t begin;    // first row entry
  int64_t count;    // row entries in this chunk
} HistItem;

typedef struct PartItem {
  int32_t node;
  int32_t pad;
  int64_t begin;      // absolute position of the chunk in rows_in
  int64_t count;
  int64_t out_left;   // absolute output position for this chunk's first left row
  int64_t out_right;  // absolute output position for this chunk's first right row
} PartItem;

typedef struct LeafItem {
  int64_t begin;    // first entry in rows
  int64_t count;
  int64_t out;      // output position
  int32_t gid;      // node id
  int32_t buf;      // row buffer: 0 = rows, 1 = rows_alt (device-planned levels collect from both)
} LeafItem;

static_assert(sizeof(HistItem) == 32 && sizeof(PartItem) == 40 && sizeof(LeafItem) == 32, "item layout");
static_assert(sizeof(FeatGroup) == 12, "group layout");

// A level's items. Nodes that need a histogram take node slots in node order. Each gets partition items of
// TMOG_PART_ITEM_ROWS rows (one item when it has fewer, an empty node included). A built node (needed, not derived
// from its parent and sibling) gets histogram items: per feature group, per statistic chunk, per row chunk, of
// TMOG_CSR_ITEM_ROWS rows for the CSR group and chunk_rows for every other; only groups without REG / CSR take one
// item per statistic chunk; SOLE marks the only row chunk, LIVE0 the REG / CSR groups when the one-present-bin
// columns' live words are bin 0 only (live_dense >= 0). The list holds the WIDE items of every node first, then the
// others. A node split over row chunks accumulates atomically and is zeroed first: the whole node when any chunk_rows
// group has several chunks (or no dense prefix is known), else the region past live_dense when only the CSR group
// has. Leaf items cut a node's rows into chunk_rows slices (none for an empty node), written one node after the other.

// ---- arguments of one grower call (tmog_grow_forest_cpu / tmog_hip_grow_forest / tmog_hip_grow_resident)
typedef struct GrowArgs {
  const uint8_t* Xb;
  int64_t N;
  int32_t F, mode, kind, S, B, missing_bin;
  int64_t chunk_rows;
  int32_t subtract, collect_leaves;
  const float* y;
  const float* t1;
  const float* t2;
  int64_t stride;
  const float* qscale;
  const double* qinv;
  const int32_t* n_bins;
  int32_t T;
  const int32_t* job_model;
  const int32_t* job_depth;
  const double* job_min_inst;
  const double* job_min_gain;
  const double* job_mcw;
  const double* job_lambda;
  const double* job_eps;
  const int32_t* job_fsub;
  const int64_t* job_count;   // root entries per job (job-major in rows)
  uint32_t* rows;             // packed root entries (device / host), overwritten
  uint32_t* rows_alt;         // scratch of the same size
  uint32_t* leaf_rows;        // collect_leaves: final leaf of every entry (same size as rows)
  int32_t* leaf_gid;
  int32_t n_groups;
  const int32_t* group_start;  // [n_groups + 1] job boundaries
  int64_t rng_seed;
  void* stream;               // GPU: caller's stream (groups wait on it; it waits on the groups)
  const int32_t* n_bins_host; // host copy of n_bins (feature grouping for the histogram kernel), may be null
  // GPU, sparse missing bin: CSR of the one-present-bin columns (row -> local ids, in n_bins order, of
  // the columns whose bin is the present bin 0); null when absent
  const int64_t* csr_ptr;     // [N + 1]
  const uint16_t* csr_col;
  int32_t csr_nf;             // number of one-present-bin columns the CSR indexes
  // Feature-parallel growth (fp_world > 0; jobs without per-node feature subsets). Every rank runs the
  // same jobs on the same replicated rows and binned matrix but builds histograms and scans splits for
  // its own slice of the growth-order feature list only: positions [fp_mlo, fp_mhi) of the multi-bin
  // list and [fp_olo, fp_ohi) of the one-present-bin list (all features count as multi-bin outside the
  // sparse missing-bin mode). Per level the ranks all-gather one split record per node (fp_rec_bytes)
  // and every rank merges them with the split scan's total order, so all ranks partition identically
  // and the forests equal the single-rank ones bit for bit.
  int32_t fp_rank, fp_world;
  int32_t fp_mlo, fp_mhi, fp_olo, fp_ohi;
  void* const* fp_comm;       // GPU: one RCCL communicator per job group
  int (*fp_exchange)(void* ctx, int group, const void* send, void* recv, int64_t bytes);   // CPU all-gather
  void* fp_ctx;
  // GPU: first per-group resource slot (stream, staging, histogram buffers) of this call -- concurrent
  // calls (e.g. the XGBoost learner's pipelined job halves, one host thread each) use disjoint slots
  int32_t slot_base;
  // GPU, optional: feature-major copy of Xb ([F][N], row index = packed entry & 0xFFFFFF). The partition
  // reads one split-column byte per row; from the feature-major copy the bytes of a node's rows share
  // cache lines (from Xb every byte pulls its own line)
  const uint8_t* XbT;
  // GPU, MODE 2, optional: the entries' quantised statistics (int32 pairs q(w g), q(w h)), one per entry of
  // rows / rows_alt (same positions); the partition moves them with their entries so the histogram items
  // read them coalesced instead of gathering t1 / t2 by row id. n_entries = size of rows (and of these).
  int32_t* gh;
  int32_t* gh_alt;
  int64_t n_entries;
  // training sets of >= 2^24 rows: entries are plain 32-bit row ids of weight 1 instead of row | weight << 24
  // (weighted roots are expanded into repeated entries by the caller, models/tree_engine.py)
  int32_t wide_rows;
  // GPU, optional: row-major matrix the wide-load histogram items read instead of Xb -- the multi-bin columns
  // only (their Xb column positions), row stride Fh bytes (a multiple of 64: every row segment starts a cache
  // line and the matrix is smaller than Xb, so more of it stays in the Infinity Cache). Groups whose columns
  // reach past Fh stay on Xb.
  const uint8_t* Xh;
  int32_t Fh;
} GrowArgs;

// ---- outputs of one device-planned tree (tmog_hip_grow_resident)
typedef struct ResidentIO {
  int64_t* rec;          // [1 + cap_nodes][7 + S] int64: header (nodes, leaf entries, error bits), then node records
  float* gid_value;      // [cap_nodes] leaf output per created node id (pruning applied)
  int64_t* gid_tree;     // [cap_nodes] job of each created node
  int64_t cap_nodes;
  const double* job_eta;    // [T]
  const double* job_gamma;  // [T]
} ResidentIO;

#ifdef __cplusplus
extern "C" {
#endif

// sizeof of the shared structs as the compiler laid them out: 0 GrowArgs, 1 ResidentIO, 2 HistItem, 3 PartItem,
// 4 LeafItem (-1 otherwise). ops/_native.py compares them with its derived ctypes mirrors when the library loads.
int64_t tmog_abi_sizeof(int which);

// ---- host/hashing_cpu.cpp
int tmog_murmur3_batch(const uint8_t* bytes, const int64_t* offsets, int64_t n, int32_t seed, int32_t* out);
int tmog_hash_index_batch(const uint8_t* bytes, const int64_t* offsets, int64_t n, int32_t seed, int32_t num_features,
                          int32_t* out);

// ---- host/loco_cpu.cpp
// Exact leave-one-column-out sums by tree-path perturbation, out[i][U + G + 1][C] (fp64) for rows row_list[0 .. n)
// (null: rows 0 .. n-1) of Xb [.][F]. nodes is the forest's node array with the split column replaced by its slot u
// in used[U] and the default direction folded in: (u, bin | default_left << 16, left, right), left < 0 a leaf;
// slot_meta[u] = zero bin of used[u] | (group + 1) << 8 (group -1: none, G groups). Tree t's KV leaf values, times
// tree_weight[t], go to columns tree_out[t] + c of C. Slot u: the sum with column used[u] at its zero bin minus the
// unperturbed sum; slot U + g: the same with every column of group g replaced; the last slot: the unperturbed sum.
// scale: the power of two of the int64 fixed-point accumulation (hip/loco_kernels.hip has the bound).
int tmog_forest_loco_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         const int32_t* slot_meta, int G, int64_t T, const int64_t* tree_off, const int32_t* nodes,
                         const float* value, int KV, const float* tree_weight, const int32_t* tree_out,
                         int missing_bin, int C, double scale, double* out);

// ---- host/pd_cpu.cpp
// Exact partial dependence / ICE curves over the complete bin grid: for rows row_list[0 .. n) (null: rows 0 .. n-1)
// of Xb [.][F] and the Q requested columns, ice[i][q][b][C] = the forest's weighted leaf-value sum of row i with
// the q-th requested column replaced by bin b, b in [0, NB). nodes, used, value, tree_weight, tree_out, C are those
// of tmog_forest_loco_cpu; slot_of_used[u] = q of column used[u], or -1 when it is not requested (a requested
// column no tree splits on has no entry: its curve is the unperturbed sum). A missing bin inside the grid must be
// its last point, NB - 1; it follows the nodes' default directions. mode 0: out is ice, fp64 [n][Q][NB][C];
// mode != 0: out is the sum over the rows, fp64 [Q][NB][C]. Every contribution is rounded to the int64 fixed
// point of the power of two `scale` and summed as integers (hip/pd_kernels.hip has the rule and the bound; the
// sum takes a scale smaller by 2^ceil(log2 n)). walks (may be null): [0] += base walks, [1] += the walks of the
// step functions below them. Returns -1 for a grid the rule above excludes.
int tmog_forest_pd_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                       const int32_t* slot_of_used, int Q, int NB, int64_t T, const int64_t* tree_off,
                       const int32_t* nodes, const float* value, int KV, const float* tree_weight,
                       const int32_t* tree_out, int missing_bin, int C, double scale, int mode, double* out,
                       int64_t* walks);

// ---- host/pd_pairs_cpu.cpp
// Exact two-way partial dependence surfaces over the complete bin grid: for rows row_list[0 .. n) (null: rows
// 0 .. n-1) of Xb [.][F] and the Pn requested column pairs, ice2[i][p][bi][bj][C] = the forest's weighted leaf-value
// sum of row i with the pair's first column replaced by bin bi and its second by bin bj, both in [0, NB). The
// arguments are those of tmog_forest_pd_cpu except pair_slots [Pn][2]: the slots in used[U] of the pair's two
// columns, -1 for a column no tree splits on; the two slots of a pair differ unless both are -1, pairs may repeat.
// mode 0: out is ice2, fp64 [n][Pn][NB][NB][C]; mode != 0: out is the sum over the rows, fp64 [Pn][NB][NB][C]. The
// same int64 fixed point as tmog_forest_pd_cpu (hip/pd_pair_kernels.hip has the rule and the bound). walks (may be
// null): [0] += base walks, [1] += anchor searches, [2] += the walks of the rectangles below the anchors. Returns
// -1 for a grid the rule of tmog_forest_pd_cpu excludes.
int tmog_forest_pd_pairs_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                             const int32_t* pair_slots, int Pn, int NB, int64_t T, const int64_t* tree_off,
                             const int32_t* nodes, const float* value, int KV, const float* tree_weight,
                             const int32_t* tree_out, int missing_bin, int C, double scale, int mode, double* out,
                             int64_t* walks);

// ---- host/shap_cpu.cpp: host twins of hip/shap_kernels.hip (same arguments minus the stream), plain fp64 sums
int tmog_forest_shap_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U, const int32_t* used,
                         int64_t P, const int64_t* p_off, const int32_t* p_out, const double* p_val, int KV,
                         const double* bias, const int32_t* e_feat, const int32_t* e_rng, const double* e_z,
                         const int64_t* bin_off, int missing_bin, int C, double scale, double* out);
int tmog_forest_shap_interactions_cpu(const uint8_t* Xb, int F, int64_t n, const int32_t* row_list, int U,
                                      const int32_t* used, int64_t P, const int64_t* p_off, const int32_t* p_out,
                                      const double* p_val, int KV, const double* bias, const int32_t* e_feat,
                                      const int32_t* e_rng, const double* e_z, const int64_t* bin_off,
                                      int missing_bin, int C, double scale, double* tri);

// ---- host/streaming_histogram.cpp
void* tmog_shist_new(int max_bins, int max_spool, int64_t round_to);
void tmog_shist_free(void* h);
void tmog_shist_update(void* h, const double* p, const int64_t* m, int64_t n);
void tmog_shist_flush(void* h);
void tmog_shist_merge(void* h, void* other);
int64_t tmog_shist_size(void* h);
void tmog_shist_bins(void* h, double* points, int64_t* counts);
double tmog_shist_sum(void* h, double b);

// ---- host/text_clean.cpp
void tmog_clean_ascii_lens(const uint8_t* buf, const int64_t* offs, int64_t n, uint8_t* out, int64_t* lens,
                           uint8_t* fallback);
int64_t tmog_first_ids(const uint8_t* buf, const int64_t* starts, const int64_t* ends, int64_t n, int64_t* ids);

// ---- host/tokenizer.cpp
void* tmog_tok_run(const uint8_t* bytes, const int64_t* offs, int64_t n, int32_t lowercase, int32_t min_len,
                   int32_t use_stop);
void tmog_tok_sizes(void* h, int64_t* n_tokens, int64_t* n_bytes);
void tmog_tok_copy(void* h, uint8_t* bytes, int64_t* tok_offs, int64_t* row_ptr, uint8_t* fallback);
void tmog_tok_free(void* h);

// ---- host/tree_cpu.cpp: host twins of the tree kernels (bit-identical results)
int tmog_hist_build_cpu(const uint8_t* Xb, int64_t N, int F, const uint32_t* rows, int n_nodes,
                        const int64_t* node_begin, const int64_t* node_count, const int32_t* node_feat_off,
                        const int32_t* node_nfeat, const int32_t* feat_list, const int32_t* node_model,
                        const int64_t* node_hist_off, int64_t* hist, int B, int mode, int S, const float* y,
                        const float* t1, const float* t2, int64_t model_stride, const float* qscale, int wide);
int tmog_split_find_cpu(const int64_t* hist, int n_nodes, const int64_t* node_hist_off, const int32_t* node_nfeat,
                        const int32_t* node_feat_off, const int32_t* feat_list, const int32_t* feat_nbins, int B,
                        int S, int kind, const float* node_params, int missing_bin, const int32_t* node_model,
                        const double* qinv, int32_t* out_feat, int32_t* out_bin, float* out_gain,
                        uint8_t* out_default_left, float* out_left, float* out_total, uint8_t* rec, int64_t rec_bytes,
                        int fp_mlo, int fp_nml, int fp_obase);
int tmog_partition_cpu(const uint8_t* Xb, int F, const uint32_t* rows_in, uint32_t* rows_out, int n_nodes,
                       const int64_t* node_begin, const int64_t* node_count, const int32_t* split_feat,
                       const int32_t* split_bin, const uint8_t* default_left, int missing_bin,
                       const int64_t* out_begin, int64_t* out_left_count, int wide);
int tmog_forest_predict_cpu(const uint8_t* Xb, int F, int n_models, const int64_t* model_row_off,
                            const int32_t* row_list, const int64_t* model_tree_off, const int64_t* tree_off,
                            const float* tree_weight, const int32_t* nodes, const uint8_t* default_left,
                            int missing_bin, const float* leaf_value, int K, float* out);
// Staged evaluation of a boosted forest on rows row_list[0..n) (null: rows 0..n-1): for s in [0, S) the trees
// stage_off[s]..stage_off[s + 1] are walked (tree t starts at node tree_off[t]; leaf_value is [n_nodes][1]), margins[i]
// [tree_col[t]] += (double)tree_weight[t] * (double)leaf_value (margins is [n][K] fp64, in/out), then the metric of the
// updated margins over the n rows is stored: values[s] (floating sums, added in row order), counts[s] += (error
// counts) or tables[s][2][bins] += (aupr); the buffers a metric does not use may be null. y is indexed by row id.
// Returns non-zero for an unknown metric or a binary / regression metric with K != 1.
int tmog_forest_staged_eval_cpu(const uint8_t* Xb, int F, const int32_t* row_list, int64_t n, const float* y,
                                const int32_t* nodes, const uint8_t* default_left, const float* leaf_value,
                                const int64_t* tree_off, const float* tree_weight, int missing_bin,
                                const int64_t* stage_off, int S, const int32_t* tree_col, int K, int metric,
                                double scale, int bins, double* margins, double* values, int64_t* counts,
                                int32_t* tables);
int tmog_find_splits_cpu(const double* sample, int64_t S, int F, int max_splits, double* out, int32_t* n_out);
int64_t tmog_tree_finalize_cpu(int64_t n, int T, const int64_t* tree, const int64_t* feat_in, const int64_t* bin,
                               const uint8_t* dl, const double* gain, const double* tot, int S,
                               const int64_t* left_in, const int64_t* right_in, int mode, int kind, int K,
                               const double* job_lam, const double* job_eta, const double* job_gamma, int with_gid,
                               int64_t* tree_off, int32_t* nodes, uint8_t* dl_out, float* value_out, float* gain_out,
                               float* cover_out, float* gid_value);

// ---- host/tree_grow_cpu.cpp: the native grower on the CPU backend. The handle is a GrowResult
void* tmog_grow_forest_cpu(const GrowArgs* args);
int tmog_grow_status_cpu(void* h, char* msg, int cap);
int64_t tmog_grow_nodes_cpu(void* h, int g);
int64_t tmog_grow_leaf_count_cpu(void* h, int g);
void tmog_grow_copy_cpu(void* h, int g, int64_t* tree, int64_t* feat, int64_t* bin, uint8_t* dl, double* gain,
                        double* tot, int64_t* left, int64_t* right);
void tmog_grow_free_cpu(void* h);
// The work items of one level as both planners lay them out (a loop over common/tree_plan.hpp, for tests). Node i has
// count[i] rows from begin[i] and the planners' flag bits flags[i] (1 can split, 2 needs a histogram, 4 left node of
// a pair, 8 the pair's derived node); every node without bit 2 is collected as a leaf (gid i, buffer 0, output from 0).
// Histogram nodes take slots in node order, slot j at word j * hsz. totals[7] receives the numbers of histogram,
// partition and leaf items, of zero segments, of whole-node zero segments (listed first), of wide-load items and
// whether any item takes the byte-gather path. Null output arrays: only the totals are written.
void tmog_level_items_cpu(int n, const int64_t* count, const int64_t* begin, const int32_t* flags,
                          const FeatGroup* groups, int n_groups, int64_t chunk_rows, int n_sc, int64_t live_dense,
                          int64_t hsz, HistItem* hitems, PartItem* citems, LeafItem* litems, int64_t* z_off,
                          int64_t* z_size, int64_t* totals);

#ifdef __cplusplus
}  // extern "C"
#endif

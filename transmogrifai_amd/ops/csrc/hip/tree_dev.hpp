// What two or more of the tree translation units share on the device side: tree_hist_kernels.hip (histograms),
// tree_split_kernels.hip (split finding), tree_partition_kernels.hip (partition, leaf collection),
// forest_predict_kernels.hip (scoring) and the boosting-round kernels (boost_kernels.hip, boost_multi_kernels.hip).
// Anything with a single user stays in that user's file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define TM_MAX_S 16          // narrow split scan / staged-record path: S <= 16 statistics
#define TM_WIDE_MAX_S 256    // wide path (many classes): statistic-chunked histograms, LDS split scan
#define TM_WIDE_MAX_BS 16384 // wide split scan keeps one feature's B x S int64 histogram in LDS

namespace tmog {

// Entry decoding. Packed (default): row | weight << 24 (rows < 2^24). Wide rows (training sets of >= 2^24
// rows, GrowArgs.wide_rows): the entry is the 32-bit row id and every entry weighs 1 -- weighted roots are
// expanded into repeated entries by the host (models/tree_engine.py), which adds the same integer
// statistics to every histogram.
__device__ __forceinline__ uint32_t ent_row(uint32_t e, int wide) { return wide ? e : (e & 0xFFFFFFu); }
__device__ __forceinline__ uint32_t ent_w(uint32_t e, int wide) { return wide ? 1u : (e >> 24); }

// One per tree translation unit: asks for the attributes of a kernel of that unit (prime_kernel), which loads the
// unit's code object on the current device (tmog_hip_tree_prime, tree_hist_kernels.hip). Returns the hipError_t.
int prime_tree_hist();
int prime_tree_split();
int prime_tree_partition();
int prime_forest_predict();
template <class K>
inline int prime_kernel(K* kernel) {
  hipFuncAttributes at;
  return (int)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(kernel));
}

}  // namespace tmog

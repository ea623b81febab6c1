// CPU backend of the native tree grower (common/tree_grow.hpp): host memory, the tmog_*_cpu twins of
// the HIP kernels (tree_cpu.cpp), groups grown one after the other with the same per-group seeds as
// the GPU backend, so both produce bit-identical forests.
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "common/tmog_abi.h"
#include "common/tree_grow.hpp"

namespace {

struct CpuBackend {
  static constexpr bool kGPU = false;
  int group = 0;
  std::vector<uint8_t> fp_recv;
  std::vector<int32_t> feats;
  std::vector<uint8_t> res;
  std::vector<int64_t> hist[2];

  const int32_t* all_features(int F) {
    feats.resize(F);
    for (int i = 0; i < F; ++i) feats[i] = i;
    return feats.data();
  }
  const uint8_t* ship(const tmog::Staging& st, int) { return st.buf.data(); }
  int stat_chunk(int, int S) const { return S; }
  std::vector<uint8_t> fp_send;
  uint8_t* fp_send_buffer(size_t bytes) {
    fp_send.assign(bytes ? bytes : 8, 0);
    return fp_send.data();
  }
  int64_t* hist_buffer(int k, size_t words) {
    if (hist[k].size() < words) hist[k].resize(words + words / 4 + 16);
    return hist[k].data();
  }
  uint8_t* result_buffer(size_t bytes) {
    res.assign(bytes, 0);
    return res.data();
  }
  const uint8_t* fetch(const uint8_t* p, size_t) { return p; }
  void zero_segments(int64_t*, const int64_t*, const int64_t*, int, int64_t, int64_t, int, int, int) {}   // CPU hist zeroes per node
  void hist_build(const tmog::GrowArgs& g, const uint32_t* rows, const void*, int, const int32_t*,
                  const int32_t* flist, const int32_t*, const int64_t*, int64_t* hist, int nbuild,
                  const int64_t* bnb, const int64_t* bnc, const int32_t* bnfo, const int32_t* bnnf,
                  const int32_t* bnmd, const int64_t* bnho, int, int, int) {
    if (nbuild)
      tmog_hist_build_cpu(g.Xb, g.N, g.F, rows, nbuild, bnb, bnc, bnfo, bnnf, flist, bnmd, bnho, hist, g.B, g.mode,
                          g.S, g.y, g.t1, g.t2, g.stride, g.qscale, g.wide_rows);
  }
  void hist_subtract(int64_t* hist, const int64_t* prev, const int64_t* poff, const int64_t* soff,
                     const int64_t* ooff, const int64_t* size, int n, int64_t, int64_t, int, int) {
    for (int j = 0; j < n; ++j) {
      const int64_t* p = prev + poff[j];
      const int64_t* s = hist + soff[j];
      int64_t* o = hist + ooff[j];
      for (int64_t k = 0; k < size[j]; ++k) o[k] = p[k] - s[k];
    }
  }
  void split_find(const tmog::GrowArgs& g, const int64_t* hist, int m, const int64_t* nho, const int32_t* nnf,
                  const int32_t* nfo, const int32_t* flist, const float* params, const int32_t* nmd, int,
                  int32_t* feat, int32_t* bin, float* gain, uint8_t* dl, float* left, float* tot, int64_t*, int,
                  const tmog::FpSlice& fps) {
    tmog_split_find_cpu(hist, m, nho, nnf, nfo, flist, g.n_bins, g.B, g.S, g.kind, params, g.missing_bin, nmd, g.qinv,
                        feat, bin, gain, dl, left, tot, fps.rec, fps.rec_bytes, fps.mlo, fps.nml, fps.obase);
  }
  // all-gather through the caller's exchange function (torch.distributed gloo in the CPU tests)
  void fp_exchange_merge(const tmog::GrowArgs& g, const uint8_t* rec, int m, size_t rb, int32_t* feat, int32_t* bin,
                         float* gain, uint8_t* dl, float* left) {
    const size_t bytes = rb * (size_t)m;
    fp_recv.assign(bytes * (size_t)g.fp_world, 0);
    if (g.fp_exchange == nullptr) throw std::runtime_error("feature-parallel growth needs an exchange function");
    if (g.fp_exchange(g.fp_ctx, group, rec, fp_recv.data(), (int64_t)bytes) != 0)
      throw std::runtime_error("feature-parallel exchange failed");
    tmog::fp_merge_host(fp_recv.data(), g.fp_world, m, rb, g.S, feat, bin, gain, dl, left);
  }
  void partition_fused(const tmog::GrowArgs&, const uint32_t*, uint32_t*, const void*, int, const int64_t*,
                       const int64_t*, const int32_t*, const int32_t*, const uint8_t*, const float*, const float*,
                       int64_t*) {
    throw std::logic_error("partition_fused is the GPU backend's path");
  }
  void partition_nodes(const tmog::GrowArgs& g, const uint32_t* rows, uint32_t* rows_alt, int ns, const int64_t* nb,
                       const int64_t* nc, const int32_t* f, const int32_t* b, const uint8_t* d, const int64_t* ob,
                       int64_t* nl) {
    tmog_partition_cpu(g.Xb, g.F, rows, rows_alt, ns, nb, nc, f, b, d, g.missing_bin, ob, nl, g.wide_rows);
  }
  void leaf_collect(const uint32_t* rows, const void* items, int n, uint32_t* out_rows, int32_t* out_gid) {
    const tmog::LeafItemH* it = (const tmog::LeafItemH*)items;
    for (int i = 0; i < n; ++i) {
      std::memcpy(out_rows + it[i].out, rows + it[i].begin, sizeof(uint32_t) * it[i].count);
      for (int64_t k = 0; k < it[i].count; ++k) out_gid[it[i].out + k] = it[i].gid;
    }
  }
  void finish() {}
};

}  // namespace

extern "C" {

void* tmog_grow_forest_cpu(const tmog::GrowArgs* args) {
  tmog::GrowResult* res = new tmog::GrowResult();
  res->groups.resize(args->n_groups);
  try {
    const int ng = args->n_groups;
    if (args->fp_world > 0 && ng > 1 && std::getenv("TMOG_CPU_GROUP_THREADS") != nullptr) {
      // one host thread per group, as the GPU backend runs them: exercises the exchange turn order
      // (tmog::FpTurns) across ranks on the CPU (gloo) path
      tmog::FpTurns turns(ng);
      std::vector<std::string> errs(ng);
      std::vector<std::thread> th;
      for (int g = 0; g < ng; ++g) {
        th.emplace_back([&, g]() {
          try {
            CpuBackend bk;
            bk.group = g;
            tmog::grow_group(bk, *args, g, res->groups[g], &turns);
          } catch (const std::exception& e) {
            errs[g] = e.what();
          }
          turns.finish(g);
        });
      }
      for (auto& t : th) t.join();
      for (int g = 0; g < ng; ++g)
        if (!errs[g].empty()) throw std::runtime_error("group " + std::to_string(g) + ": " + errs[g]);
    } else {
      for (int g = 0; g < ng; ++g) {
        CpuBackend bk;
        bk.group = g;
        tmog::grow_group(bk, *args, g, res->groups[g]);
      }
    }
  } catch (const std::exception& e) {
    res->status = -1;
    res->error = e.what();
  }
  return res;
}

int tmog_grow_status_cpu(void* h, char* msg, int cap) {
  tmog::GrowResult* r = (tmog::GrowResult*)h;
  if (msg && cap > 0) {
    std::strncpy(msg, r->error.c_str(), cap - 1);
    msg[cap - 1] = 0;
  }
  return r->status;
}
int64_t tmog_grow_nodes_cpu(void* h, int g) { return tmog::result_nodes((tmog::GrowResult*)h, g); }
int64_t tmog_grow_leaf_count_cpu(void* h, int g) { return ((tmog::GrowResult*)h)->groups[g].leaf_count; }
void tmog_grow_copy_cpu(void* h, int g, int64_t* tree, int64_t* feat, int64_t* bin, uint8_t* dl, double* gain,
                        double* tot, int64_t* left, int64_t* right) {
  tmog::result_copy((tmog::GrowResult*)h, g, tree, feat, bin, dl, gain, tot, left, right);
}
void tmog_grow_free_cpu(void* h) { delete (tmog::GrowResult*)h; }

void tmog_level_items_cpu(int n, const int64_t* count, const int64_t* begin, const int32_t* flags,
                          const FeatGroup* groups, int n_groups, int64_t chunk_rows, int n_sc, int64_t live_dense,
                          int64_t hsz, HistItem* hitems, PartItem* citems, LeafItem* litems, int64_t* z_off,
                          int64_t* z_size, int64_t* totals) {
  using namespace tmog;
  auto work = [&](int i) { return node_work(flags[i], count[i], chunk_rows, groups, n_groups, n_sc, live_dense, hsz); };
  int64_t nh = 0, nc = 0, nl = 0, zw = 0, zc = 0, n_wide = 0, n_general = 0, n_zw = 0, leaf_pos = 0;
  for (int i = 0; i < n; ++i) n_zw += work(i).zero == kZeroNode;
  for (const bool wide : {true, false}) {
    int32_t j = 0;                                   // node slot: histogram nodes in node order
    for (int i = 0; i < n; ++i) {
      if (!(flags[i] & kNodeNeed)) continue;
      const NodeWork w = work(i);
      for (int64_t k = 0; k < (wide ? w.n_wide : w.n_other); ++k, ++nh)
        if (hitems)
          hitems[nh] = hist_item_at(wide, j, k, begin[i], count[i], chunk_rows, groups, n_groups, n_sc, live_dense);
      if (wide) {                                    // once per node: partition items, zero segment, totals
        for (int64_t k = 0; k < w.n_part; ++k, ++nc)
          if (citems) citems[nc] = part_item_at(j, k, begin[i], count[i]);
        if (w.zero != kZeroNone) {
          const int64_t at = w.zero == kZeroNode ? zw++ : n_zw + zc++;   // whole-node segments first
          if (z_off) zero_segment(w.zero, (int64_t)j * hsz, hsz, live_dense, &z_off[at], &z_size[at]);
        }
        n_wide += w.n_wide;
        n_general += w.n_general;
      }
      ++j;
    }
  }
  for (int i = 0; i < n; ++i) {
    if (flags[i] & kNodeNeed) continue;
    for (int64_t k = 0; k < leaf_items(count[i], chunk_rows); ++k, ++nl)
      if (litems) litems[nl] = leaf_item_at(k, begin[i], count[i], chunk_rows, leaf_pos, i, 0);
    leaf_pos += count[i] > 0 ? count[i] : 0;
  }
  const int64_t t[7] = {nh, nc, nl, zw + zc, n_zw, n_wide, n_general > 0};
  std::memcpy(totals, t, sizeof(t));
}

int64_t tmog_abi_sizeof(int which) {
  const int64_t sizes[] = {sizeof(GrowArgs), sizeof(ResidentIO), sizeof(HistItem), sizeof(PartItem), sizeof(LeafItem)};
  return which >= 0 && which < 5 ? sizes[which] : -1;
}

}  // extern "C"

// The memory of the native tree growers (tree_grow_hip.hip, tree_resident.hip): grow-only buffers kept per slot
// for the life of the process, and the staged host -> device copy built from them.
//
// * A buffer that grows frees its old block first and is left EMPTY (nullptr, capacity 0) until the new
//   allocation has succeeded: a failed growth can then never leave a capacity that describes freed memory
//   (the round-4 "out of memory, then illegal address on the next learner" fault: the next call saw
//   need <= cap and launched on the freed pointer). Pointer and capacity are private to the buffer types, so
//   no call site can break the rule.
// * How far a buffer grows past the request is the call site's policy (the `new_cap` argument), not the buffer's.
// * On hipErrorOutOfMemory the process-wide handler runs once and the allocation is retried. The Python
//   side registers a handler that returns torch's cached-but-unused blocks to the device
//   (torch.cuda.empty_cache), so the native buffers and torch's caching allocator draw on one budget
//   instead of the native growth failing while torch holds free cache.
// * Test hook: tmog_hip_fail_alloc(n) makes the n-th native allocation from now fail with
//   hipErrorOutOfMemory (without the handler), to prove a failed growth leaves a usable slot. Only the
//   stream-ordered device allocations (DevBuf) count.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

namespace tmog {

inline void hchk(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
inline void kchk(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string("kernel ") + what + " failed with code " + std::to_string(rc));
}

inline std::atomic<void (*)()> g_oom_handler{nullptr};
inline std::atomic<long> g_fail_at{0};

inline hipError_t dev_malloc_async(void** p, size_t bytes, hipStream_t s) {
  *p = nullptr;
  if (g_fail_at.load(std::memory_order_relaxed) > 0 && g_fail_at.fetch_sub(1) == 1) return hipErrorOutOfMemory;
  hipError_t e = hipMallocAsync(p, bytes, s);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();                 // not sticky: clear it before the retry
    if (auto h = g_oom_handler.load()) {
      h();
      e = hipMallocAsync(p, bytes, s);
    }
  }
  if (e != hipSuccess) *p = nullptr;
  return e;
}

// Grow-only block of one kind of memory (Mem: how a block is acquired and released).
template <class Mem>
class GrowBuf {
  uint8_t* p_ = nullptr;
  size_t cap_ = 0;

 public:
  // At least `bytes`; a growth allocates `new_cap` >= bytes. True when the block is new (contents undefined).
  // `copied`: see PinMem.
  bool need(size_t bytes, size_t new_cap, hipStream_t s, hipEvent_t copied = nullptr) {
    if (bytes <= cap_ && p_ != nullptr) return false;
    if (uint8_t* old = p_) {
      p_ = nullptr;
      cap_ = 0;
      Mem::release(old, s, copied);
    }
    p_ = Mem::acquire(new_cap, s);
    cap_ = new_cap;
    return true;
  }
  template <class T = uint8_t>
  T* as() const { return reinterpret_cast<T*>(p_); }
  size_t capacity() const { return cap_; }
};

// Stream-ordered device memory; every use of the block is ordered on the stream it grows on.
struct DevMem {
  static void release(uint8_t* p, hipStream_t s, hipEvent_t) { hchk(hipFreeAsync(p, s), "hipFreeAsync"); }
  static uint8_t* acquire(size_t bytes, hipStream_t s) {
    void* q = nullptr;
    const hipError_t e = dev_malloc_async(&q, bytes, s);
    if (e != hipSuccess)
      throw std::runtime_error("hipMallocAsync(" + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    return static_cast<uint8_t*>(q);
  }
};
// Pinned host memory. Before a block is freed the copies that use it must be over: `copied`, the event behind
// the last of them, is waited for when given, else the stream is synchronised.
struct PinMem {
  static void release(uint8_t* p, hipStream_t s, hipEvent_t copied) {
    hchk(copied ? hipEventSynchronize(copied) : hipStreamSynchronize(s), "sync before pinned realloc");
    hchk(hipHostFree(p), "hipHostFree");
  }
  static uint8_t* acquire(size_t bytes, hipStream_t) {
    void* q = nullptr;
    hchk(hipHostMalloc(&q, bytes, hipHostMallocDefault), "hipHostMalloc");
    return static_cast<uint8_t*>(q);
  }
};
// Plain hipMalloc memory (never from the stream-ordered pool of DevMem) for RCCL send / receive buffers: the
// collective library inspects and may register the buffers it is given.
struct RawMem {
  static void release(uint8_t* p, hipStream_t s, hipEvent_t) {
    hchk(hipStreamSynchronize(s), "sync before rccl buffer realloc");
    hchk(hipFree(p), "hipFree");
  }
  static uint8_t* acquire(size_t bytes, hipStream_t) {
    void* q = nullptr;
    hchk(hipMalloc(&q, bytes), "hipMalloc");
    return static_cast<uint8_t*>(q);
  }
};
using DevBuf = GrowBuf<DevMem>;
using PinBuf = GrowBuf<PinMem>;
using RawBuf = GrowBuf<RawMem>;

// A host block to the device in one async copy through pinned memory. The pinned block is rewritten only after
// its previous copy has completed (the event; created on first use).
struct StagedCopy {
  PinBuf pin;
  DevBuf dev;
  hipEvent_t copied = nullptr;

  const uint8_t* ship(const void* src, size_t bytes, size_t pin_cap, size_t dev_cap, hipStream_t s) {
    if (copied) hchk(hipEventSynchronize(copied), "stage copy wait");
    else hchk(hipEventCreateWithFlags(&copied, hipEventDisableTiming), "event create");
    pin.need(bytes, pin_cap, s, copied);
    dev.need(bytes, dev_cap, s);
    if (bytes) {
      std::memcpy(pin.as(), src, bytes);
      hchk(hipMemcpyAsync(dev.as(), pin.as(), bytes, hipMemcpyHostToDevice, s), "stage copy");
      hchk(hipEventRecord(copied, s), "event record");
    }
    return dev.as();
  }
};

// Per-node ticket counters of the fused split reduction: zeroed when (re)allocated; the kernels leave them zeroed.
class Tickets {
  DevBuf buf_;
  bool zeroed_ = false;

 public:
  unsigned* need(size_t m, size_t new_cap_bytes, hipStream_t s) {
    if (buf_.need(m * sizeof(unsigned), new_cap_bytes, s)) zeroed_ = false;
    if (!zeroed_) {
      hchk(hipMemsetAsync(buf_.as(), 0, buf_.capacity(), s), "memset done");
      zeroed_ = true;
    }
    return buf_.as<unsigned>();
  }
};

}  // namespace tmog

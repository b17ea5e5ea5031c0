// runtime_internal.h -- what the units behind the C ABI share (runtime.cpp, string_dict.cpp): the context, the error macro and the
// device / pinned buffers with their accounting.  The globals are defined once, in runtime.cpp.
#ifndef SSGPU_RUNTIME_INTERNAL_H_
#define SSGPU_RUNTIME_INTERNAL_H_

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "engine.h"

using ssgpu::LowerOptions;
#define SSGPU_INTERNAL __attribute__((visibility("hidden")))   // crosses units, not the library's boundary

#define HIP_TRY(ctx, expr)                                                          \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      (ctx)->err = _e == hipErrorOutOfMemory ? std::string("Memory exceeded: ") + #expr : std::string(#expr) + ": " + hipGetErrorString(_e); \
      return _e == hipErrorOutOfMemory ? SSGPU_ERROR_MEMORY_EXCEEDED : SSGPU_ERROR_HIP; \
    }                                                                                \
  } while (0)

struct ssgpu_ctx {
  // plans and blocks hold a reference: the context outlives them whatever order a garbage-collected host
  // destroys the handles in (ssgpu_ctx_destroy only drops the owner's reference)
  std::atomic<int> refs{1};
  int device = -1;
  hipStream_t stream = nullptr, copy_stream = nullptr;
  // ssgpu_block_upload copies on the copy stream; a run that reads the block through raw column pointers (ssgpu_plan_run / ssgpu_expr_evaluate
  // with ssgpu_block_column's answers, instead of ssgpu_plan_run_block) used to race with those copies -- seen as a wrong Evaluate result
  // of the C++ facade on a loaded GPU.  Every upload raises the flag; the next run of ANY plan of the context orders its stream behind the copies.
  std::atomic<bool> copy_pending{false};
  hipEvent_t copy_ev = nullptr;
  bool own_stream = false;
  int cu_count = 0;
  std::string err;
  LowerOptions opt;
  int64_t grid_limit = 0;        // 0 = CUs * residency
  int64_t out_arena = 1;         // 1: a stage's large result is one allocation with skewed column bases (ensure_out_cols), 0: a buffer per column
  int64_t tile_map = 1;          // which tile a workgroup of a pipeline launch takes: 0 = its block index (neighbouring tiles on different XCDs), 1 = XCD-contiguous
                                 // chunks for launches that WRITE compacted / materialised rows (vm.h VM_FLAG_XCD_CHUNKS: lines two tiles share merge in one L2), 2 = for every launch
  int64_t wgs_per_cu = 3;        // resident 4-wave workgroups per CU (<= 4 at the kernel's 128-VGPR budget; 3 streams best)
  int64_t group_capacity = 1 << 18;
  int64_t group_local = 1;       // 0: never use the LDS pre-aggregation table
  int64_t group_partition = 1;   // 0: never switch to the partitioned GroupAggregate; 2: always use it
  int64_t part_n = 0;            // initial number of hash partitions (0 = 512)
  int64_t part_wgs_per_cu = 0;   // resident workgroups per CU of the scatter pass (0 = wgs_per_cu)
  int64_t part_lds_target = 0;   // LDS target of the scatter pass's tile (0 = lds_target_bytes)
  int64_t sort_records = 1;      // 0: always gather payload columns one by one
  int64_t sort_hybrid = 1;       // 0: never take the high-half-first shortcut for wide keys
  int64_t group_slab = 1;        // 0: never take the slab form of the partitioned GroupAggregate
  int64_t group_scout = 1;       // 0: no scout run ahead of the first large GroupAggregate run (see run_group_agg)
  int64_t group_scout_rows = 8 << 20;   // ... "large": inputs of at least this many rows (a smaller value helps first runs and costs steady ones: see run_group_agg)
  int64_t group_resident = 1;    // 0: plain stages take the slab form through scatter + aggregation like every other stage (tests, A/B)
  int64_t group_dense = 1;       // 0: never index group tables by the keys' value ranges (dense slots, see DenseState); SSGPU_GROUP_DENSE sets the process default
  int64_t dense_parts = 0;       // partitions of the dense partitioned shape (0 = 256, more -- the next power of two -- when the tables would outgrow 80 KiB)
  int64_t dense_min_rows = 1 << 16;   // inputs below this many rows never look for dense ranges (tests lower it to reach the dense kernels with small inputs)
  int64_t async_handoff = 1;     // 0: every stage hand-off reads the row count on the host (a stream synchronise), even where the next stage could take it from the device
  int64_t lazy_feedback = 0;     // 1: a GroupAggregate in its steady state leaves its overflow / feedback words on the stream instead of reading them back
                                 // at the end of every run, and a run may be REPEATED from the caller's input columns when its result is first touched
                                 // (an overflow seen late, a NaN in a floating MIN / MAX).  Off by default (round 5): ssgpu_plan_run returns with every
                                 // such decision made -- the input may be released or overwritten once the run has been synchronised.  Callers that
                                 // step a plan without touching the host opt in (distributed.py, sharded.h, bench.py) and keep their input alive.
  int64_t part_prefetch = 1;     // specialised partition aggregation, records of <= 6 words: the loads of trip k + 1 are issued before trip k's LDS atomics
  int64_t fuse_emit = 1;         // ScalarAggregate: the finish launch also emits the result row (0: a launch of its own, as until round 6)
  int64_t pscat_pipe = 1;        // specialised plain scatter: the software-pipelined form (tile k + 1 loaded, ranked and reserved while tile k is staged and flushed)
  int64_t pscat_threads = 0, pscat_rows = 0, pscat_wgs = 0;   // launch shape of the plain scatter (0: 1024 threads x 2 rows, one workgroup per CU; ssgpu_part_scatter_plain_geom)
  int64_t part_plain = 1;        // 0: never run the partition scatter as its own kernel (plain stages), always as the VM program
  int64_t sort_compact = 1;      // 0: never sort (high half << 32 | row id) words instead of (key, row id) pairs
  int64_t sort_hi_digits = 4;    // high digits the hybrid sort passes over before fixing ties: 2..4, 0 = by row count
  int64_t part_agg_lds = 0;      // LDS bytes of phase 2's workgroup (0 = 80 KiB: two workgroups per CU)
  int64_t profile = 1;           // record HIP events around kernels
  int64_t profile_total = 1;     // ... and around the whole run (kernel_ms); 0 keeps only the dominant kernel's pair
  int64_t debug_timing = 0;
  int64_t specialize = 3;        // plans created on this context run kernels specialised for them by runtime compilation (rtc.cpp):
                                 // 1 = yes, compiled when a kernel shape is first launched (the first run; a later run only if run
                                 // feedback moves a GroupAggregate to another execution shape) -- the run WAITS for the compiler;
                                 // 2 = where such a kernel EXISTS already -- loaded in this process or stored in the on-disk cache
                                 // by any earlier one -- and never compiled; 3 (the default) = like 2, and a kernel that is missing
                                 // when a run over >= specialize_min_rows rows wants it is compiled by the library's one worker
                                 // thread: no run ever waits for the compiler, the plan's later runs (and, through the disk cache,
                                 // later processes) pick the kernel up; 0 (and the legacy -1) = only plans that ask for it with
                                 // ssgpu_plan_specialize.
  int64_t specialize_min_rows = 1 << 22;   // option 3: runs over fewer input rows never start a compilation (their kernels take microseconds)
};

// Device memory a plan holds, against its soft quota (ssgpu_plan_set_memory_limit = MemoryLimit, memory.h:465): every
// DevBuf (re)allocated while a plan runs is charged to that plan; a request beyond the quota fails like an allocation the
// device cannot serve, which HIP_TRY turns into SSGPU_ERROR_MEMORY_EXCEEDED.
struct MemQuota { int64_t limit = -1; int64_t used = 0; };
extern SSGPU_INTERNAL thread_local MemQuota* g_quota;
struct QuotaScope { MemQuota* saved; explicit QuotaScope(MemQuota* q) : saved(g_quota) { g_quota = q; } ~QuotaScope() { g_quota = saved; } };

// process-wide accounting of what the library holds (ssgpu_memory_stats)
extern SSGPU_INTERNAL std::atomic<long long> g_dev_bytes, g_pinned_bytes;

// A small pool of device blocks between plans.  The reference's usage model is a cursor per query, drained once
// (test/guide/group_sort.cc:166,223): every query's first -- and only -- run would pay a hipMalloc per buffer (two dozen for a
// GroupAggregate, each 50 - 300 us: more than the kernels of a million-row input).  Blocks of a DESTROYED plan (its stream has been
// drained: nothing in flight can touch them) are parked here instead of freed, and the next plan's DevBuf::ensure takes one that
// fits (within 2x; small blocks by 4 KiB class) before it asks the driver.  Bounded: SSGPU_POOL_MB (default 4096, 0 = off) and
// 4096 blocks; what is parked still counts as held by the library (ssgpu_memory_stats.device_bytes).
struct DevPool {
  std::mutex m;
  std::multimap<size_t, std::pair<void*, int>> blocks;   // capacity -> (pointer, device)
  size_t bytes = 0;
  size_t limit() { static const size_t v = [] { const char* e = getenv("SSGPU_POOL_MB"); return (size_t)(e ? atoll(e) : 4096) << 20; }(); return v; }
  // The device of a parked block is the device of the POINTER (hipPointerGetAttributes), never the calling thread's current
  // device: ssgpu_plan_destroy may run while another context's device is current (round-5 advice).
  bool park(void* p, size_t cap) {
    if (limit() == 0) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int dev = attr.device;
    std::lock_guard<std::mutex> lock(m);
    if (bytes + cap > limit() || blocks.size() >= 4096) return false;
    blocks.emplace(cap, std::make_pair(p, dev)); bytes += cap;
    return true;
  }
  void* take(size_t want, size_t* cap) {
    int dev = 0;
    if (limit() == 0 || hipGetDevice(&dev) != hipSuccess) return nullptr;
    const size_t most = want <= 4096 ? 4096 : want * 2;
    std::lock_guard<std::mutex> lock(m);
    for (auto it = blocks.lower_bound(want); it != blocks.end() && it->first <= most; ++it)
      if (it->second.second == dev) { void* p = it->second.first; *cap = it->first; bytes -= it->first; blocks.erase(it); return p; }
    return nullptr;
  }
  // frees every parked block (dev < 0) or those of one device; returns the bytes given back to the driver
  size_t trim(int dev);
  size_t parked(int dev) {
    std::lock_guard<std::mutex> lock(m);
    size_t n = 0;
    for (auto& b : blocks) if (dev < 0 || b.second.second == dev) n += b.first;
    return n;
  }
};
extern SSGPU_INTERNAL DevPool g_pool;
extern SSGPU_INTERNAL thread_local bool tls_park_released;   // set while a plan whose stream has been drained is being destroyed

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool view = false;      // p points into somebody else's allocation (a block's arena): never freed, never regrown here
  MemQuota* q = nullptr;
  ~DevBuf() { release(); }
  void release() {
    if (p && !view) {
      if (q) q->used -= (int64_t)cap;
      if (!(tls_park_released && g_pool.park(p, cap))) { (void)hipFree(p); g_dev_bytes.fetch_sub((long long)cap); }
    }
    p = nullptr; cap = 0; q = nullptr; view = false;
  }
  void set_view(void* ptr, size_t bytes) { release(); p = ptr; cap = bytes; view = true; }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (view) return hipErrorInvalidValue;    // (a view has the size its owner gave it)
    size_t want = std::max<size_t>(bytes, 256);
    MemQuota* Q = g_quota;
    if (Q && Q->limit >= 0 && Q->used - (q == Q ? (int64_t)cap : 0) + (int64_t)want > Q->limit) return hipErrorOutOfMemory;
    static const bool trace = getenv("SSGPU_TRACE") != nullptr;   // development: (re)allocations of large buffers are slow and must not sit in a steady state
    if (trace && want >= (64u << 20)) fprintf(stderr, "[ssgpu trace] device buffer %zu -> %zu MiB\n", cap >> 20, want >> 20);
    release();
    size_t pooled_cap = 0;
    // (a plan under a quota allocates exactly what it asks for; a pooled block is still counted in g_dev_bytes)
    if (void* pooled = (Q && Q->limit >= 0) ? nullptr : g_pool.take(want, &pooled_cap)) { p = pooled; cap = pooled_cap; q = Q; if (q) q->used += (int64_t)cap; return hipSuccess; }
    hipError_t e = hipMalloc(&p, want);
    if (e == hipErrorOutOfMemory) {
      // the driver is out of memory while blocks of destroyed plans sit in the pool: give those back and ask once more
      (void)hipGetLastError();
      int dev = -1;
      if (hipGetDevice(&dev) == hipSuccess && g_pool.trim(dev) > 0) e = hipMalloc(&p, want);
    }
    if (e == hipSuccess) { cap = want; q = Q; g_dev_bytes.fetch_add((long long)want); if (q) q->used += (int64_t)want; } else p = nullptr;
    return e;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~PinnedBuf() { drop(); }
  void drop() { if (p) { (void)hipHostFree(p); g_pinned_bytes.fetch_sub((long long)cap); } p = nullptr; cap = 0; }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    drop();
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) { cap = want; g_pinned_bytes.fetch_add((long long)want); } else p = nullptr;
    return e;
  }
};

// A STRING dictionary packed for the device: `offs[n + 1]` into one byte heap (STRFN_HEAP_PAD zero bytes behind it)
struct DictDevice { DevBuf offs, heap; uint64_t n = 0; };

// ---- string_dict.cpp: the STRING dictionary's device work -----------------------------------------------------------------------
static const int64_t kMaxStringDomain = int64_t(1) << 30;   // the table's slot numbers stay 32-bit
// The device part, for any domain of n rows (`lens`: n + 1 words, `dnull`: n bytes): the distinct values sorted in StringPiece order
// -- on the device as out_off[D + 1] / out_heap (`heap_pad` bytes of slack behind the values, for readers of aligned words) and copied
// back once into off_h / heap_h -- and, for every target, codes[first + r] of its `rows` domain rows written to dst (0 for a NULL row).
// `scanned`: lens already holds the offsets (the caller needed the total to size the heap).  Returns with the stream idle.
struct DomainCodes { int32_t* dst; uint64_t first, rows; };
SSGPU_INTERNAL int encode_domain(ssgpu_ctx* c, hipStream_t s, const uint8_t* bytes, uint64_t* lens, bool scanned, const uint8_t* dnull, uint64_t n,
                                 const std::vector<DomainCodes>& targets, uint64_t heap_pad, std::vector<uint64_t>* off_h_out, std::vector<char>* heap_h_out,
                                 uint32_t* D_out, DevBuf& out_off, DevBuf& out_heap);

// The tables over one dictionary that a plan's programs gather from (Program::gathers of JOIN_GATHER_DICT_TABLE): the dictionary packed
// and uploaded once, one table per spec.  Dictionaries are immutable, so the tables are built lazily before the first run that needs
// them and again when the plan is handed another dictionary (`gen`: the stamp of the ssgpu_plan_set_dict call, so that a new dictionary
// at a freed one's address is not mistaken for it); freed with their owner.  The table of a string-producing node is not computed: the
// CLOSED dictionary brings it along (ssgpu_dict_close) and build() uploads it, after checking that the dictionary was closed under `steps`.
struct DictTables {
  bool built = false; uint64_t built_gen = 0; const ssgpu_dict* built_for = nullptr;
  DictDevice dev; DevBuf needle;
  std::map<ssgpu::DictTableSpec, DevBuf> tables;
  // a parse spec: `tables` holds the values, this the failure bytes; host_resolved: the FLOAT / DOUBLE entries the device left to the
  // host's strtof / strtod when the tables were last built
  std::map<ssgpu::DictTableSpec, DevBuf> failed;
  int64_t host_resolved = 0;
  bool current(const ssgpu_dict* d, uint64_t gen) const { return d && built && built_for == d && built_gen == gen; }
  // every table of `gathers` (one spec per gather, in program order) exists and belongs to `d`; `steps`: the owner's string-producing
  // nodes in evaluation order; *n_launches += the kernels launched
  SSGPU_INTERNAL int build(ssgpu_ctx* c, const ssgpu_dict* d, uint64_t gen, const std::vector<ssgpu::DictTableSpec>& gathers, const std::vector<ssgpu_string_step>& steps,
                           int32_t* n_launches);
  // what a gather of `spec` reads: the table and, for a parse spec, its failure bytes (NULL before build())
  SSGPU_INTERNAL void slot(const ssgpu::DictTableSpec& spec, const void** data, const uint8_t** is_null) const;
  // the describe() line of `spec`: function, needle (its length once the dictionary is known), case folding
  SSGPU_INTERNAL std::string describe(const ssgpu::DictTableSpec& spec, const ssgpu_dict* d) const;
};

#endif  // SSGPU_RUNTIME_INTERNAL_H_

// seams.cpp -- the host-side seams of the C ABI that own no device state: the BufferAllocator-shaped pinned allocator
// with its MemoryLimit quota (supersonic/base/memory/memory.h:100-233,465-520) and the order-preserving STRING
// dictionary (StringPiece order: supersonic/base/infrastructure/types_infrastructure.h:238-246; the Arena deep-copy rule:
// supersonic/base/memory/arena.h, cursor/core/filter.cc:205-230).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <iterator>
#include <limits>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ssgpu.h"

struct ssgpu_allocator {
  bool pinned = false;       // hipHostMalloc (a device is bound) or plain aligned host memory (bind-only context)
  int64_t quota = -1;        // soft quota in bytes, -1 = unlimited
  int64_t used = 0;
  std::unordered_map<void*, size_t> live;
};

extern "C" {

void* ssgpu_ctx_stream(ssgpu_ctx* ctx);
int ssgpu_ctx_has_device(const ssgpu_ctx* ctx);

int ssgpu_allocator_create(ssgpu_ctx* ctx, int64_t quota_bytes, ssgpu_allocator** out) {
  if (!ctx || !out) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_allocator* a = new ssgpu_allocator;
  a->pinned = ssgpu_ctx_has_device(ctx) != 0;
  a->quota = quota_bytes < 0 ? -1 : quota_bytes;
  *out = a;
  return SSGPU_OK;
}

static void raw_free(ssgpu_allocator* a, void* p) { if (a->pinned) (void)hipHostFree(p); else free(p); }
static void* raw_alloc(ssgpu_allocator* a, size_t bytes) {
  void* p = nullptr;
  const size_t n = std::max<size_t>(bytes, 1);           // zero-size requests return non-NULL data (memory.h:112-117)
  if (a->pinned) { if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } }
  else if (posix_memalign(&p, 256, (n + 255) & ~size_t(255)) != 0) return nullptr;
  return p;
}

void ssgpu_allocator_destroy(ssgpu_allocator* a) {
  if (!a) return;
  for (auto& kv : a->live) raw_free(a, kv.first);
  delete a;
}

int64_t ssgpu_allocator_available(const ssgpu_allocator* a) {
  if (!a) return 0;
  return a->quota < 0 ? std::numeric_limits<int64_t>::max() : std::max<int64_t>(a->quota - a->used, 0);
}
int64_t ssgpu_allocator_allocated(const ssgpu_allocator* a) { return a ? a->used : 0; }

int ssgpu_allocator_allocate(ssgpu_allocator* a, size_t requested, size_t minimal, void** out, size_t* granted) {
  if (!a || !out || minimal > requested) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  *out = nullptr; if (granted) *granted = 0;
  size_t grant = requested;
  if (a->quota >= 0) {
    const int64_t avail = std::max<int64_t>(a->quota - a->used, 0);
    if ((int64_t)grant > avail) grant = (size_t)avail;          // best effort: as much as the quota leaves ...
    if (grant < minimal) return SSGPU_ERROR_MEMORY_EXCEEDED;     // ... but never less than `minimal`
  }
  void* p = raw_alloc(a, grant);
  if (!p) return SSGPU_ERROR_MEMORY_EXCEEDED;
  a->live[p] = grant; a->used += (int64_t)grant;
  *out = p; if (granted) *granted = grant;
  return SSGPU_OK;
}

int ssgpu_allocator_reallocate(ssgpu_allocator* a, void* p, size_t requested, size_t minimal, void** out, size_t* granted) {
  if (!a || !out) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (!p) return ssgpu_allocator_allocate(a, requested, minimal, out, granted);
  auto it = a->live.find(p);
  if (it == a->live.end() || minimal > requested) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  const size_t old = it->second;
  size_t grant = requested;
  if (a->quota >= 0) {
    // conservative like the reference's mediator (memory.h, memory_test.cc:183-198: "realloc might degenerate to
    // create-copy-free"): the whole new size has to fit NEXT TO the old buffer
    const int64_t avail = std::max<int64_t>(a->quota - a->used, 0);
    if ((int64_t)grant > avail) grant = (size_t)avail;
    if (grant < minimal) { *out = nullptr; return SSGPU_ERROR_MEMORY_EXCEEDED; }       // the old buffer stays valid
  }
  void* q = raw_alloc(a, grant);
  if (!q) { *out = nullptr; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  memcpy(q, p, std::min(old, grant));
  raw_free(a, p);
  a->live.erase(it);
  a->live[q] = grant; a->used += (int64_t)grant - (int64_t)old;
  *out = q; if (granted) *granted = grant;
  return SSGPU_OK;
}

void ssgpu_allocator_free(ssgpu_allocator* a, void* p) {
  if (!a || !p) return;
  auto it = a->live.find(p);
  if (it == a->live.end()) return;
  a->used -= (int64_t)it->second;
  raw_free(a, p);
  a->live.erase(it);
}

}  // extern "C"

// ---- order-preserving dictionary ---------------------------------------------------------------------------------
struct ssgpu_dict {
  std::vector<std::string> values;                  // sorted: memcmp, then length == std::string's operator< on bytes
  // a CLOSED dictionary (ssgpu_dict_close): the step list it was closed under and, per step, T_k[code(v)] = code(f_k(v)) over its own codes
  std::vector<ssgpu_string_step> steps;
  std::vector<std::vector<int32_t>> step_tables;
  // value -> code, built on first use: a dictionary made on the device for a block is often only decoded, never looked up
  const std::unordered_map<std::string, int32_t>& codes() const {
    std::call_once(code_once, [this] { code.reserve(values.size()); for (size_t i = 0; i < values.size(); ++i) code[values[i]] = (int32_t)i; });
    return code;
  }
 private:
  mutable std::once_flag code_once;
  mutable std::unordered_map<std::string, int32_t> code;
};

extern "C" {

int ssgpu_dict_create(const char* const* strings, const int32_t* lengths, int64_t n, ssgpu_dict** out) {
  if (!out || n < 0 || (n > 0 && (!strings || !lengths))) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_dict* d = new ssgpu_dict;
  d->values.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) if (strings[i] && lengths[i] >= 0) d->values.emplace_back(strings[i], (size_t)lengths[i]);
  // std::string compares as unsigned bytes, shorter-is-less on a common prefix: the reference's StringPiece order
  std::sort(d->values.begin(), d->values.end());
  d->values.erase(std::unique(d->values.begin(), d->values.end()), d->values.end());
  if (d->values.size() > (size_t)std::numeric_limits<int32_t>::max()) { delete d; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  *out = d;
  return SSGPU_OK;
}
void ssgpu_dict_destroy(ssgpu_dict* d) { delete d; }
int32_t ssgpu_dict_size(const ssgpu_dict* d) { return d ? (int32_t)d->values.size() : 0; }

int ssgpu_dict_encode(const ssgpu_dict* d, const char* const* strings, const int32_t* lengths, const uint8_t* is_null, int64_t n, int32_t* codes) {
  if (!d || !codes || n < 0 || (n > 0 && (!strings || !lengths))) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  int rc = SSGPU_OK;
  const auto& code = d->codes();
  for (int64_t i = 0; i < n; ++i) {
    if (is_null && is_null[i]) { codes[i] = 0; continue; }
    auto it = code.find(std::string(strings[i] ? strings[i] : "", strings[i] ? (size_t)lengths[i] : 0));
    if (it == code.end()) { codes[i] = -1; rc = SSGPU_ERROR_INVALID_ARGUMENT_VALUE; } else codes[i] = it->second;
  }
  return rc;
}
int ssgpu_dict_decode(const ssgpu_dict* d, int32_t code, const char** bytes, int32_t* length) {
  if (!d || code < 0 || (size_t)code >= d->values.size() || !bytes || !length) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  *bytes = d->values[(size_t)code].data(); *length = (int32_t)d->values[(size_t)code].size();
  return SSGPU_OK;
}

// base U strings; remap[c] = the new code of base code c (both dictionaries are sorted, so one merge walk finds them)
int ssgpu_dict_extend(const ssgpu_dict* base, const char* const* strings, const int32_t* lengths, int64_t n, ssgpu_dict** out, int32_t* remap) {
  if (!base || !out || n < 0 || (n > 0 && (!strings || !lengths)) || (!remap && !base->values.empty())) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  std::vector<std::string> add;
  add.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) if (strings[i] && lengths[i] >= 0) add.emplace_back(strings[i], (size_t)lengths[i]);
  std::sort(add.begin(), add.end());
  add.erase(std::unique(add.begin(), add.end()), add.end());
  ssgpu_dict* d = new ssgpu_dict;
  d->values.reserve(base->values.size() + add.size());
  std::set_union(base->values.begin(), base->values.end(), add.begin(), add.end(), std::back_inserter(d->values));
  if (d->values.size() > (size_t)std::numeric_limits<int32_t>::max()) { delete d; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  size_t j = 0;
  for (size_t c = 0; c < base->values.size(); ++c) {
    while (d->values[j] != base->values[c]) ++j;
    remap[c] = (int32_t)j;
  }
  *out = d;
  return SSGPU_OK;
}

// internal (runtime.cpp, string_dict.cpp): a dictionary over values that are already sorted and unique -- the distinct strings of a device
// block in code order, `offsets[n + 1]` into `heap` -- taken as they are
int ssgpu_dict_create_sorted(const char* heap, const uint64_t* offsets, int64_t n, ssgpu_dict** out) {
  if (!out || n < 0 || n > (int64_t)std::numeric_limits<int32_t>::max()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_dict* d = new ssgpu_dict;
  d->values.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) d->values.emplace_back(heap + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
  *out = d;
  return SSGPU_OK;
}

// internal (string_dict.cpp: ssgpu_dict_close): makes `d` a closed dictionary -- `tables` holds n tables of ssgpu_dict_size(d) entries, one after the other
void ssgpu_dict_set_steps(ssgpu_dict* d, const ssgpu_string_step* steps, int32_t n, const int32_t* tables) {
  const size_t size = d->values.size();
  d->steps.assign(steps, steps + n);
  d->step_tables.resize((size_t)n);
  for (int32_t k = 0; k < n; ++k) d->step_tables[(size_t)k].assign(tables + (size_t)k * size, tables + ((size_t)k + 1) * size);
}
// ... and reads them back: the step count, steps[k] and T_k (ensure_dict_tables uploads it)
int32_t ssgpu_dict_step_count(const ssgpu_dict* d) { return d ? (int32_t)d->steps.size() : 0; }
const ssgpu_string_step* ssgpu_dict_step(const ssgpu_dict* d, int32_t k) { return d && k >= 0 && (size_t)k < d->steps.size() ? &d->steps[(size_t)k] : nullptr; }
const int32_t* ssgpu_dict_step_table_data(const ssgpu_dict* d, int32_t k) { return d && k >= 0 && (size_t)k < d->step_tables.size() ? d->step_tables[(size_t)k].data() : nullptr; }

int ssgpu_dict_step_table(const ssgpu_dict* d, int32_t k, int32_t* out_host) {
  if (!d || k < 0 || (size_t)k >= d->step_tables.size() || (!out_host && !d->values.empty())) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (!d->values.empty()) memcpy(out_host, d->step_tables[(size_t)k].data(), d->values.size() * sizeof(int32_t));
  return SSGPU_OK;
}

// internal (string_dict.cpp): the dictionary packed for the device -- `offsets[n + 1]` into one byte heap of ssgpu_dict_heap_bytes
uint64_t ssgpu_dict_heap_bytes(const ssgpu_dict* d) {
  uint64_t total = 0;
  if (d) for (const std::string& v : d->values) total += v.size();
  return total;
}
void ssgpu_dict_pack(const ssgpu_dict* d, uint64_t* offsets, char* heap) {
  uint64_t at = 0;
  const size_t n = d ? d->values.size() : 0;
  for (size_t i = 0; i < n; ++i) {
    offsets[i] = at;
    memcpy(heap + at, d->values[i].data(), d->values[i].size());
    at += d->values[i].size();
  }
  offsets[n] = at;
}

}  // extern "C"

// string_dict_kernels.hip -- one order-preserving STRING dictionary built on the device.
//
// A *string domain* is every STRING column of one block laid end to end: per-row lengths (scanned here into offsets), one
// byte heap, one NULL byte per row.  The kernels below turn it into the dictionary codes of ssgpu.h "STRING columns":
//   hash    -- every non-NULL row hashes its bytes: one lane per short string, a whole wave per long one;
//   insert  -- open addressing in HBM (capacity a power of two >= 2 x rows, so it never fills): a slot holds
//              (hash tag << 32 | row + 1), equal tags are confirmed by comparing the full bytes, and every row keeps its slot;
//   compact -- the occupied slots become the distinct list (wave-aggregated reservation);
//   sort    -- the distinct strings in StringPiece order (unsigned memcmp, then shorter first,
//              types_infrastructure.h:238-246): a bitonic network over (big-endian 8-byte prefix, distinct id) pairs whose
//              comparator falls back to the bytes after the prefix only on a tie, so any common prefix is handled;
//   rank / codes -- code[row] = rank[slot[row]], 0 for a NULL row;
//   gather  -- the distinct bytes in code order, for the one copy back to the host.
// The codes depend on the SET of strings alone: which row wins a slot, and the order in which slots are compacted, change
// nothing once the distinct strings are sorted (they are unique, so the sort has no ties to break).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch.h"

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;

#define STR_THREADS 256
#define STR_SCAN_ITEMS 4
#define STR_SCAN_TILE (STR_THREADS * STR_SCAN_ITEMS)   // 1024 elements per workgroup of the scan
#define STR_LONG 128                                   // longer strings are hashed / copied by a whole wave

// ---- exclusive scan of uint64 (in place; data[n] receives the total) -------------------------------------------------
__device__ __forceinline__ u64 block_exclusive_scan(u64 v, u64* lds, u64* total) {
  const u32 t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (u32 d = 1; d < STR_THREADS; d <<= 1) {
    const u64 add = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const u64 incl = lds[t];
  *total = lds[STR_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_scan_reduce_kernel(const u64* __restrict__ data, u64 n, u64* __restrict__ partials) {
  __shared__ u64 lds[STR_THREADS];
  const u64 base = (u64)blockIdx.x * STR_SCAN_TILE + (u64)threadIdx.x * STR_SCAN_ITEMS;
  u64 s = 0;
  for (int k = 0; k < STR_SCAN_ITEMS; ++k) if (base + k < n) s += data[base + k];
  u64 total;
  (void)block_exclusive_scan(s, lds, &total);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// one workgroup: the partial sums in place, exclusive; the grand total goes to data[n]
__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_scan_partials_kernel(u64* __restrict__ partials, u64 np, u64* __restrict__ data, u64 n) {
  __shared__ u64 lds[STR_THREADS];
  u64 carry = 0;
  for (u64 lo = 0; lo < np; lo += STR_THREADS) {
    const u64 i = lo + threadIdx.x;
    const u64 v = i < np ? partials[i] : 0;
    u64 total;
    const u64 ex = block_exclusive_scan(v, lds, &total);
    if (i < np) partials[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) data[n] = carry;
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_scan_apply_kernel(u64* __restrict__ data, u64 n, const u64* __restrict__ partials) {
  __shared__ u64 lds[STR_THREADS];
  const u64 base = (u64)blockIdx.x * STR_SCAN_TILE + (u64)threadIdx.x * STR_SCAN_ITEMS;
  u64 v[STR_SCAN_ITEMS], s = 0;
  for (int k = 0; k < STR_SCAN_ITEMS; ++k) { v[k] = base + k < n ? data[base + k] : 0; s += v[k]; }
  u64 total;
  u64 run = partials[blockIdx.x] + block_exclusive_scan(s, lds, &total);
  for (int k = 0; k < STR_SCAN_ITEMS; ++k) if (base + k < n) { data[base + k] = run; run += v[k]; }
}

// ---- hashing ------------------------------------------------------------------------------------------------------------
// H(s) = mix(len * K0 + SUM_i mix(w_i + (i + 1) * K1)), w_i the i-th little-endian 8-byte word zero-padded: the sum does not
// depend on the order the words are visited in, so a wave can split a long string across its lanes and reduce.
__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__device__ __forceinline__ u64 load_word_le(const u8* p, u64 len, u64 i) {
  const u64 lo = i * 8;
  const u64 m = len - lo < 8 ? len - lo : 8;
  u64 w = 0;
  for (u64 k = 0; k < m; ++k) w |= (u64)p[lo + k] << (8 * k);
  return w;
}
__device__ __forceinline__ u64 load_word_be(const u8* p, u64 len, u64 i) {
  const u64 lo = i * 8;
  u64 w = 0;
  for (u64 k = 0; k < 8; ++k) w = (w << 8) | (lo + k < len ? (u64)p[lo + k] : 0);
  return w;
}
__device__ __forceinline__ u64 word_term(u64 w, u64 i) { return mix64(w + (i + 1) * 0xd6e8feb86659fd93ull); }
__device__ __forceinline__ u64 hash_finish(u64 sum, u64 len) { return mix64(sum + len * 0x9e3779b97f4a7c15ull); }

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_hash_kernel(const u8* __restrict__ bytes, const u64* __restrict__ offs, const u8* __restrict__ nulls,
                                                                     u64 n, u64* __restrict__ hashes) {
  const u64 row = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n && !nulls[row];
  const u64 off = live ? offs[row] : 0, len = live ? offs[row + 1] - off : 0;
  if (live && len <= STR_LONG) {
    u64 s = 0;
    for (u64 i = 0; i * 8 < len; ++i) s += word_term(load_word_le(bytes + off, len, i), i);
    hashes[row] = hash_finish(s, len);
  }
  // long strings: the whole wave walks the words of one of them at a time (the loop is wave-uniform)
  u64 todo = __ballot(live && len > STR_LONG);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 o = __shfl(off, src, 64), l = __shfl(len, src, 64);
    u64 s = 0;
    for (u64 i = lane; i * 8 < l; i += 64) s += word_term(load_word_le(bytes + o, l, i), i);
    s = wave_sum(s);
    if ((int)lane == src) hashes[row] = hash_finish(s, l);
  }
}

// ---- insert -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool bytes_equal(const u8* a, const u8* b, u64 len) {
  for (u64 k = 0; k < len; ++k) if (a[k] != b[k]) return false;
  return true;
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_insert_kernel(const u8* __restrict__ bytes, const u64* __restrict__ offs, const u8* __restrict__ nulls,
                                                                       const u64* __restrict__ hashes, u64 n, u64* table, u64 mask,
                                                                       u32* __restrict__ row_slot, u32* __restrict__ error) {
  const u64 row = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  if (row >= n) return;
  if (nulls[row]) { row_slot[row] = 0xffffffffu; return; }
  const u64 h = hashes[row];
  const u64 tag = h >> 32;
  const u64 mine = (tag << 32) | (row + 1);
  const u64 off = offs[row], len = offs[row + 1] - off;
  u64 slot = h & mask;
  for (u64 probe = 0; probe <= mask; ++probe) {
    u64 cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      const u64 prev = atomicCAS(&table[slot], 0ull, mine);
      if (prev == 0) { row_slot[row] = (u32)slot; return; }
      cur = prev;
    }
    if ((cur >> 32) == tag) {
      const u64 other = (cur & 0xffffffffull) - 1;
      const u64 ooff = offs[other];
      if (offs[other + 1] - ooff == len && bytes_equal(bytes + off, bytes + ooff, len)) { row_slot[row] = (u32)slot; return; }
    }
    slot = (slot + 1) & mask;
  }
  atomicOr(error, 1u);     // (cannot happen: the table has at least twice as many slots as rows)
  row_slot[row] = 0xffffffffu;
}

// ---- compact: occupied slots -> distinct ids ----------------------------------------------------------------------------
__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_compact_kernel(const u64* __restrict__ table, u64 cap, const u8* __restrict__ bytes,
                                                                        const u64* __restrict__ offs, u32* count, u32* __restrict__ d_slot,
                                                                        u64* __restrict__ d_off, u64* __restrict__ d_len, u64* __restrict__ d_key,
                                                                        u32* __restrict__ d_idx) {
  const u64 slot = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const u64 e = slot < cap ? table[slot] : 0;
  const u64 occupied = __ballot(e != 0);
  if (!occupied) return;
  u32 base = 0;
  if (lane == 0) base = atomicAdd(count, (u32)__popcll(occupied));
  base = __shfl(base, 0, 64);
  if (e == 0) return;
  const u32 id = base + (u32)__popcll(occupied & ((1ull << lane) - 1));
  const u64 row = (e & 0xffffffffull) - 1;
  const u64 off = offs[row], len = offs[row + 1] - off;
  d_slot[id] = (u32)slot; d_off[id] = off; d_len[id] = len;
  d_key[id] = load_word_be(bytes + off, len, 0);
  d_idx[id] = id;
}

// ---- bitonic sort of (prefix key, distinct id) in StringPiece order -----------------------------------------------------
#define STR_PAD 0xffffffffu
__device__ __forceinline__ bool str_less(u64 ka, u32 a, u64 kb, u32 b, const u8* bytes, const u64* d_off, const u64* d_len) {
  if (b == STR_PAD) return a != STR_PAD;
  if (a == STR_PAD) return false;
  if (ka != kb) return ka < kb;
  // the zero-padded first 8 bytes tie: compare what follows them, then the lengths (a proper prefix is less)
  const u64 la = d_len[a], lb = d_len[b];
  const u8* pa = bytes + d_off[a];
  const u8* pb = bytes + d_off[b];
  const u64 m = la < lb ? la : lb;
  for (u64 k = 8; k < m; ++k) if (pa[k] != pb[k]) return pa[k] < pb[k];
  return la < lb;
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_pad_kernel(u64* __restrict__ key, u32* __restrict__ idx, u64 d, u64 p) {
  const u64 i = d + (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  if (i < p) { key[i] = ~0ull; idx[i] = STR_PAD; }
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_bitonic_kernel(u64* __restrict__ key, u32* __restrict__ idx, u32 lj, u64 k, u64 half,
                                                                        const u8* __restrict__ bytes, const u64* __restrict__ d_off,
                                                                        const u64* __restrict__ d_len) {
  const u64 t = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  if (t >= half) return;
  const u64 j = 1ull << lj;
  const u64 i = ((t >> lj) << (lj + 1)) | (t & (j - 1));   // the lower element of the pair; its partner is i + j
  const u64 l = i + j;
  const bool ascending = (i & k) == 0;
  const u64 ki = key[i], kl = key[l];
  const u32 ii = idx[i], il = idx[l];
  const bool swap = ascending ? str_less(kl, il, ki, ii, bytes, d_off, d_len) : str_less(ki, ii, kl, il, bytes, d_off, d_len);
  if (swap) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
}

// ---- rank, codes, gather ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_rank_kernel(const u32* __restrict__ idx, const u32* __restrict__ d_slot, const u64* __restrict__ d_len,
                                                                     u64 d, int* __restrict__ slot_rank, u64* __restrict__ out_len) {
  const u64 i = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  if (i >= d) return;
  const u32 id = idx[i];
  slot_rank[d_slot[id]] = (int)i;
  out_len[i] = d_len[id];
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_codes_kernel(const u32* __restrict__ row_slot, const u8* __restrict__ nulls,
                                                                      const int* __restrict__ slot_rank, u64 n, int* __restrict__ codes) {
  const u64 r = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  if (r >= n) return;
  const u32 s = row_slot[r];
  codes[r] = (nulls[r] || s == 0xffffffffu) ? 0 : slot_rank[s];
}

__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_gather_kernel(const u8* __restrict__ bytes, const u64* __restrict__ d_off, const u32* __restrict__ idx,
                                                                       const u64* __restrict__ out_off, u64 d, u8* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = i < d;
  const u64 src = live ? d_off[idx[i]] : 0, dst = live ? out_off[i] : 0, len = live ? out_off[i + 1] - dst : 0;
  if (live && len <= STR_LONG) for (u64 k = 0; k < len; ++k) out[dst + k] = bytes[src + k];
  u64 todo = __ballot(live && len > STR_LONG);
  while (todo) {
    const int who = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 s = __shfl(src, who, 64), o = __shfl(dst, who, 64), l = __shfl(len, who, 64);
    for (u64 k = lane; k < l; k += 64) out[o + k] = bytes[s + k];
  }
}

// codes of one dictionary -> codes of another through a remap table (code c -> remap[c]); NULL rows stay 0
__global__ __launch_bounds__(STR_THREADS) void ssgpu_str_recode_kernel(const int* __restrict__ src, const u8* __restrict__ nulls, const int* __restrict__ remap,
                                                                       int n_remap, u64 n, int* __restrict__ dst) {
  const u64 r = (u64)blockIdx.x * STR_THREADS + threadIdx.x;
  if (r >= n) return;
  const int c = src[r];
  dst[r] = (nulls && nulls[r]) || c < 0 || c >= n_remap ? 0 : remap[c];
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
static inline unsigned grid_for(u64 n, u64 per) { return (unsigned)((n + per - 1) / per); }

uint64_t ssgpu_str_scan_partials(uint64_t n) { return n ? (n + STR_SCAN_TILE - 1) / STR_SCAN_TILE : 1; }
hipError_t ssgpu_launch_str_scan(uint64_t* data, uint64_t n, uint64_t* partials, hipStream_t s) {
  const u64 np = ssgpu_str_scan_partials(n);
  if (n) hipLaunchKernelGGL(ssgpu_str_scan_reduce_kernel, dim3((unsigned)np), dim3(STR_THREADS), 0, s, (const u64*)data, (u64)n, (u64*)partials);
  hipLaunchKernelGGL(ssgpu_str_scan_partials_kernel, dim3(1), dim3(STR_THREADS), 0, s, (u64*)partials, n ? np : (u64)0, (u64*)data, (u64)n);
  if (n) hipLaunchKernelGGL(ssgpu_str_scan_apply_kernel, dim3((unsigned)np), dim3(STR_THREADS), 0, s, (u64*)data, (u64)n, (const u64*)partials);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_hash(const uint8_t* bytes, const uint64_t* offs, const uint8_t* nulls, uint64_t n, uint64_t* hashes, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_hash_kernel, dim3(grid_for(n, STR_THREADS)), dim3(STR_THREADS), 0, s, bytes, (const u64*)offs, nulls, (u64)n, (u64*)hashes);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_insert(const uint8_t* bytes, const uint64_t* offs, const uint8_t* nulls, const uint64_t* hashes, uint64_t n,
                                   uint64_t* table, uint64_t cap, uint32_t* row_slot, uint32_t* error, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_insert_kernel, dim3(grid_for(n, STR_THREADS)), dim3(STR_THREADS), 0, s, bytes, (const u64*)offs, nulls,
                            (const u64*)hashes, (u64)n, (u64*)table, (u64)(cap - 1), row_slot, error);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_compact(const uint64_t* table, uint64_t cap, const uint8_t* bytes, const uint64_t* offs, uint32_t* count,
                                    uint32_t* d_slot, uint64_t* d_off, uint64_t* d_len, uint64_t* d_key, uint32_t* d_idx, hipStream_t s) {
  if (cap) hipLaunchKernelGGL(ssgpu_str_compact_kernel, dim3(grid_for(cap, STR_THREADS)), dim3(STR_THREADS), 0, s, (const u64*)table, (u64)cap, bytes,
                              (const u64*)offs, count, d_slot, (u64*)d_off, (u64*)d_len, (u64*)d_key, d_idx);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_sort(uint64_t* d_key, uint32_t* d_idx, uint64_t d, uint64_t p, const uint8_t* bytes, const uint64_t* d_off,
                                 const uint64_t* d_len, hipStream_t s) {
  if (p > d) hipLaunchKernelGGL(ssgpu_str_pad_kernel, dim3(grid_for(p - d, STR_THREADS)), dim3(STR_THREADS), 0, s, (u64*)d_key, d_idx, (u64)d, (u64)p);
  const u64 half = p / 2;
  for (u64 k = 2; k <= p; k <<= 1)
    for (u64 j = k >> 1; j > 0; j >>= 1)
      hipLaunchKernelGGL(ssgpu_str_bitonic_kernel, dim3(grid_for(half, STR_THREADS)), dim3(STR_THREADS), 0, s, (u64*)d_key, d_idx, (u32)__builtin_ctzll(j), k, half, bytes,
                         (const u64*)d_off, (const u64*)d_len);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_rank(const uint32_t* d_idx, const uint32_t* d_slot, const uint64_t* d_len, uint64_t d, int32_t* slot_rank,
                                 uint64_t* out_len, hipStream_t s) {
  if (d) hipLaunchKernelGGL(ssgpu_str_rank_kernel, dim3(grid_for(d, STR_THREADS)), dim3(STR_THREADS), 0, s, d_idx, d_slot, (const u64*)d_len, (u64)d,
                            (int*)slot_rank, (u64*)out_len);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_codes(const uint32_t* row_slot, const uint8_t* nulls, const int32_t* slot_rank, uint64_t n, int32_t* codes, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_codes_kernel, dim3(grid_for(n, STR_THREADS)), dim3(STR_THREADS), 0, s, row_slot, nulls, (const int*)slot_rank,
                            (u64)n, (int*)codes);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_gather(const uint8_t* bytes, const uint64_t* d_off, const uint32_t* d_idx, const uint64_t* out_off, uint64_t d,
                                   uint8_t* out, hipStream_t s) {
  if (d) hipLaunchKernelGGL(ssgpu_str_gather_kernel, dim3(grid_for(d, STR_THREADS)), dim3(STR_THREADS), 0, s, bytes, (const u64*)d_off, d_idx,
                            (const u64*)out_off, (u64)d, out);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_recode(const int32_t* src, const uint8_t* nulls, const int32_t* remap, int32_t n_remap, uint64_t n, int32_t* dst,
                                   hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_recode_kernel, dim3(grid_for(n, STR_THREADS)), dim3(STR_THREADS), 0, s, (const int*)src, nulls, (const int*)remap,
                            (int)n_remap, (u64)n, (int*)dst);
  return hipGetLastError();
}

// string_fn_kernels.hip -- functions of a STRING value evaluated once per DISTINCT value.
//
// A STRING value in a plan is the INT32 code of the plan's order-preserving dictionary, so f(s) = T[code(s)] with
// T[c] = f(dictionary[c]).  The kernel below builds T on the device from the packed dictionary (`offsets[n + 1]` into one
// byte heap); the pipeline reads it per row with GATHER_32 (vm_body.inc).  Functions (reference OperatorIds):
//   OP_LENGTH            T[c] = byte length                                  (string_evaluators.h Length)
//   OP_STRING_OFFSET     T[c] = 1-based byte position of the FIRST occurrence of the needle, 0 when absent; an empty
//                        needle is found at 1 (string_evaluators.h:69-73: haystack.find(needle) + 1)
// `fold` compares through ascii_tolower on both sides (the TO_LOWER(haystack), TO_LOWER(needle) form StringContainsCI
// binds, string_bound_expressions.cc:193-205): only A-Z fold, bytes >= 0x80 are left alone.
//
// Work split, like the encoder's hash kernel (string_dict_kernels.hip): one lane per string of up to STRFN_LONG = 128
// bytes -- the same threshold, a string that short is at most two cache lines and a wave's 64 of them keep every lane
// busy -- and a whole wave per longer string.  Both forms walk the candidate start positions in ascending order over
// ALIGNED words of the heap (8 bytes per lane-form step, 16 bytes per lane per wave-form step: the heap is read once,
// whatever the strings' own alignment; it is allocated with STRFN_HEAP_PAD bytes of slack so the last aligned word is
// inside it), test the first needle byte in registers and compare the rest of the needle byte by byte straight from
// the heap -- so a match that runs on into the bytes another lane scans is found like any other.  In the wave form a
// step covers 64 x 16 consecutive bytes; the lanes' first matches are reduced with a MINIMUM and the loop stops at the
// first step that has one, which is the string's first occurrence.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch.h"
#include "opids.h"

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

#define STRFN_THREADS 256
#define STRFN_LONG 128
#define STRFN_NONE 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ u32 strfn_byte(u32 c, bool fold) { return (fold && c - 65u < 26u) ? (c | 0x20u) : c; }

// needle[1 .. nlen) against the bytes behind a position whose first byte already matched
__device__ __forceinline__ bool strfn_rest(const u8* __restrict__ h, const u8* __restrict__ needle, u32 nlen, bool fold) {
  for (u32 k = 1; k < nlen; ++k)
    if (strfn_byte(h[k], fold) != strfn_byte(needle[k], fold)) return false;
  return true;
}

__device__ __forceinline__ u64 strfn_wave_min(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
  return v;
}

__global__ __launch_bounds__(STRFN_THREADS) void ssgpu_str_fn_kernel(const u8* __restrict__ heap, const u64* __restrict__ offs, u64 n, int fn,
                                                                     const u8* __restrict__ needle, u32 nlen, int fold_i, u32* __restrict__ T) {
  const u64 row = (u64)blockIdx.x * STRFN_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n;
  const u64 off = live ? offs[row] : 0, len = live ? offs[row + 1] - off : 0;
  if (fn == OP_LENGTH) { if (live) T[row] = (u32)len; return; }
  const bool fold = fold_i != 0;
  if (nlen == 0) { if (live) T[row] = 1u; return; }               // "".find("") == 0
  const u32 n0 = strfn_byte(needle[0], fold);
  const bool fits = live && len >= (u64)nlen;                      // a needle longer than the string is nowhere in it
  if (live && (len <= STRFN_LONG || !fits)) {
    u64 first = STRFN_NONE;
    if (fits) {
      const u64 last = off + len - nlen;                           // last candidate start (absolute heap position)
      for (u64 a = off & ~7ull; a <= last && first == STRFN_NONE; a += 8) {
        const u64 w = *reinterpret_cast<const u64*>(heap + a);
        for (u32 b = 0; b < 8; ++b) {
          const u64 s = a + b;
          if (s < off || s > last) continue;
          if (strfn_byte((u32)(w >> (8 * b)) & 0xFFu, fold) != n0) continue;
          if (strfn_rest(heap + s, needle, nlen, fold)) { first = s - off; break; }
        }
      }
    }
    T[row] = first == STRFN_NONE ? 0u : (u32)(first + 1);
  }
  // long strings: the whole wave scans one of them at a time (every loop below is wave-uniform)
  u64 todo = __ballot(fits && len > STRFN_LONG);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 o = __shfl(off, src, 64), l = __shfl(len, src, 64);
    const u64 last = o + l - nlen;
    u64 found = STRFN_NONE;
    for (u64 base = o & ~15ull; base <= last; base += 64 * 16) {
      const u64 a = base + (u64)lane * 16;
      u64 first = STRFN_NONE;
      if (a <= last) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(heap + a);
#pragma unroll
        for (u32 b = 0; b < 16; ++b) {
          const u64 s = a + b;
          if (s < o || s > last) continue;
          if (strfn_byte((v[b >> 2] >> (8 * (b & 3))) & 0xFFu, fold) != n0) continue;
          if (strfn_rest(heap + s, needle, nlen, fold)) { first = s - o; break; }
        }
      }
      found = strfn_wave_min(first);
      if (found != STRFN_NONE) break;
    }
    if ((int)lane == src) T[row] = found == STRFN_NONE ? 0u : (u32)(found + 1);
  }
}

hipError_t ssgpu_launch_str_fn(const uint8_t* heap, const uint64_t* offs, uint64_t n, int fn, const uint8_t* needle, uint32_t needle_len,
                               int fold, uint32_t* table, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t grid = (n + STRFN_THREADS - 1) / STRFN_THREADS;
  hipLaunchKernelGGL(ssgpu_str_fn_kernel, dim3((unsigned)grid), dim3(STRFN_THREADS), 0, s, heap, (const u64*)offs, (u64)n, fn, needle, needle_len, fold, table);
  return hipGetLastError();
}

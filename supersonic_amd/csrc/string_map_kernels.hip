// string_map_kernels.hip -- string-PRODUCING functions evaluated once per DISTINCT value: the images of a dictionary.
//
// A STRING value in a plan is a code of the plan's one dictionary, so a function whose result is a STRING is a table
// T[code(s)] = code(f(s)) too -- once the dictionary holds every image (the CLOSED dictionary, ssgpu.h).  One closing step takes
// the packed dictionary D (`offsets[n + 1]` into one byte heap, the form string_dict.cpp: dict_upload makes) and builds the string
// domain "D's values followed by their images" -- 2n rows -- which then goes through the encoder of string_dict_kernels.hip:
//   length pass -- ssgpu_str_map_len_kernel: lens[i] = |v_i|, lens[n + i] = |f(v_i)|, src[i] = where the image's bytes start in
//                  D's heap.  Every function here maps a value to a SLICE of it, byte-transformed or not:
//                    OP_LTRIM / OP_RTRIM / OP_TRIM      strip byte 0x20 only (string_evaluators.h:96-120)
//                    OP_TOUPPER (OP_TOLOWER)            the whole value, folded on the way out (:122-146)
//                    OP_SUBSTRING                       substr(pos', len) with the evaluator's position rule (:41-67)
//                  so the length pass of SUBSTRING and the folds reads no byte at all, and the trims read the two ends only;
//   scan        -- string_dict_kernels.hip (the caller);
//   write pass  -- ssgpu_str_map_write_kernel: the image's bytes into the domain's heap behind D's own bytes, folded
//                  a-z -> A-Z (dir 1) or A-Z -> a-z (dir 2; ascii_toupper / ascii_tolower: bytes >= 0x80 and 0x00 untouched).
// Work split as in string_fn_kernels.hip: one lane per value of up to STRMAP_LONG = 128 bytes, a whole wave per longer one;
// the heap is read in ALIGNED 8-byte (lane form) / 16-byte (wave form) words -- its allocation extends STRFN_HEAP_PAD bytes
// past the last value and starts 16-byte aligned.  A long value's first and last non-space byte are found by the wave, 1 KiB
// per step from either end, with a minimum / maximum over the lanes; the loop stops at the first step that has one.
// OP_STRING_REPLACE is NOT a slice -- it searches the whole value, its image may be longer than the value and its bytes come from two
// places -- and has a length and a write pass of its own, ssgpu_str_replace_len_kernel / _write_kernel, further down.
//
// ssgpu_str_map_compose_kernel: after the last step, a step's (remap, table) pair -- codes of ITS dictionary D_k -- carried
// through the later steps' remaps into codes of the final dictionary (string_dict.cpp: ssgpu_dict_close).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch.h"
#include "opids.h"

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;
typedef unsigned char u8;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

#define STRMAP_THREADS 256
#define STRMAP_LONG 128
#define STRMAP_NONE 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ u32 strmap_fold(u32 c, int dir) {
  if (dir == 1) return c - 97u < 26u ? c & ~0x20u : c;
  if (dir == 2) return c - 65u < 26u ? c | 0x20u : c;
  return c;
}
__device__ __forceinline__ u64 strmap_wave_min(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ u64 strmap_wave_max(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
  return v;
}

// lane form: the first byte of [lo, hi) that is not a space (hi when there is none), over aligned 8-byte words
__device__ __forceinline__ u64 strmap_first_nonspace(const u8* __restrict__ heap, u64 lo, u64 hi) {
  for (u64 a = lo & ~7ull; a < hi; a += 8) {
    const u64 w = *reinterpret_cast<const u64*>(heap + a);
    for (u32 b = 0; b < 8; ++b) {
      const u64 s = a + b;
      if (s < lo) continue;
      if (s >= hi) return hi;
      if (((w >> (8 * b)) & 0xFFu) != 0x20u) return s;
    }
  }
  return hi;
}
// lane form: one past the last byte of [lo, hi) that is not a space (lo when there is none)
__device__ __forceinline__ u64 strmap_last_nonspace(const u8* __restrict__ heap, u64 lo, u64 hi) {
  if (hi <= lo) return lo;
  for (u64 a = (hi - 1) & ~7ull;; a -= 8) {
    const u64 w = *reinterpret_cast<const u64*>(heap + a);
    for (int b = 7; b >= 0; --b) {
      const u64 s = a + (u64)b;
      if (s >= hi) continue;
      if (s < lo) return lo;
      if (((w >> (8 * b)) & 0xFFu) != 0x20u) return s + 1;
    }
    if (a <= lo) return lo;   // (a is a multiple of 8 above lo >= 0 otherwise: a - 8 does not wrap)
  }
}

// wave form (every loop is wave-uniform): the same two searches for one long value, 64 x 16 bytes per step
__device__ __forceinline__ u64 strmap_wave_first_nonspace(const u8* __restrict__ heap, u64 lo, u64 hi, u32 lane) {
  for (u64 base = lo & ~15ull; base < hi; base += 64 * 16) {
    const u64 a = base + (u64)lane * 16;
    u64 first = STRMAP_NONE;
    if (a < hi) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(heap + a);
#pragma unroll
      for (u32 b = 0; b < 16; ++b) {
        const u64 s = a + b;
        if (s < lo || s >= hi || first != STRMAP_NONE) continue;
        if (((v[b >> 2] >> (8 * (b & 3))) & 0xFFu) != 0x20u) first = s;
      }
    }
    const u64 found = strmap_wave_min(first);
    if (found != STRMAP_NONE) return found;
  }
  return hi;
}
__device__ __forceinline__ u64 strmap_wave_last_nonspace(const u8* __restrict__ heap, u64 lo, u64 hi, u32 lane) {
  if (hi <= lo) return lo;
  // lane l of a step reads the 16-byte word l words below the step's top one; positions are signed so that a step may reach below 0
  for (i64 top = (i64)((hi - 1) & ~15ull); top + 16 > (i64)lo; top -= 64 * 16) {
    const i64 a = top - (i64)lane * 16;
    u64 last = 0;                                    // one past the lane's last non-space byte, 0 = none
    if (a >= 0 && a + 16 > (i64)lo) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(heap + a);
#pragma unroll
      for (u32 b = 0; b < 16; ++b) {
        const u64 s = (u64)a + b;
        if (s < lo || s >= hi) continue;
        if (((v[b >> 2] >> (8 * (b & 3))) & 0xFFu) != 0x20u) last = s + 1;
      }
    }
    const u64 found = strmap_wave_max(last);
    if (found) return found;
  }
  return lo;
}

// lens: 2n + 1 words (the last one is the scan's); src: n words
__global__ __launch_bounds__(STRMAP_THREADS) void ssgpu_str_map_len_kernel(const u8* __restrict__ heap, const u64* __restrict__ offs, u64 n, int fn, int has_len,
                                                                           i64 pos, i64 sublen, u64* __restrict__ lens, u64* __restrict__ src) {
  const u64 row = (u64)blockIdx.x * STRMAP_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n;
  const u64 off = live ? offs[row] : 0, len = live ? offs[row + 1] - off : 0;
  const bool trims = fn == OP_LTRIM || fn == OP_RTRIM || fn == OP_TRIM;
  u64 lo = off, hi = off + len;                      // the image is heap[lo, hi)
  if (fn == OP_SUBSTRING) {
    // SubstringTernary / SubstringBinary: a position > 0 counts from 1, one <= 0 from the end and is clamped at 0; StringPiece::substr clamps both
    i64 p = pos;
    if (p > 0) p -= 1; else { p += (i64)len; if (p < 0) p = 0; }
    const u64 start = (u64)p < len ? (u64)p : len;
    const u64 room = len - start;
    const u64 want = has_len ? (sublen > 0 ? (u64)sublen : 0) : room;
    lo = off + start; hi = lo + (want < room ? want : room);
  } else if (trims && live && len <= STRMAP_LONG) {
    if (fn != OP_RTRIM) lo = strmap_first_nonspace(heap, off, off + len);
    if (fn != OP_LTRIM) hi = strmap_last_nonspace(heap, lo, off + len);
  }
  if (trims) {
    u64 todo = __ballot(live && len > STRMAP_LONG);
    while (todo) {
      const int who = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const u64 o = __shfl(off, who, 64), l = __shfl(len, who, 64);
      u64 a = o, b = o + l;
      if (fn != OP_RTRIM) a = strmap_wave_first_nonspace(heap, o, o + l, lane);
      if (fn != OP_LTRIM) b = strmap_wave_last_nonspace(heap, a, o + l, lane);
      if ((int)lane == who) { lo = a; hi = b; }
    }
  }
  if (live) { lens[row] = len; lens[n + row] = hi - lo; src[row] = lo; }
}

// image i = heap[src[i], src[i] + its length) -> out[dst_offs[i], dst_offs[i + 1]), folded by `dir`
__global__ __launch_bounds__(STRMAP_THREADS) void ssgpu_str_map_write_kernel(const u8* __restrict__ heap, const u64* __restrict__ src, const u64* __restrict__ dst_offs,
                                                                             u64 n, int dir, u8* __restrict__ out) {
  const u64 row = (u64)blockIdx.x * STRMAP_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n;
  const u64 from = live ? src[row] : 0, to = live ? dst_offs[row] : 0, len = live ? dst_offs[row + 1] - to : 0;
  if (live && len <= STRMAP_LONG) {
    const u64 end = from + len;
    for (u64 a = from & ~7ull; a < end; a += 8) {
      const u64 w = *reinterpret_cast<const u64*>(heap + a);
      for (u32 b = 0; b < 8; ++b) {
        const u64 s = a + b;
        if (s >= from && s < end) out[to + (s - from)] = (u8)strmap_fold((u32)(w >> (8 * b)) & 0xFFu, dir);
      }
    }
  }
  u64 todo = __ballot(live && len > STRMAP_LONG);
  while (todo) {
    const int who = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 f = __shfl(from, who, 64), t = __shfl(to, who, 64), l = __shfl(len, who, 64);
    const u64 end = f + l;
    for (u64 a = (f & ~15ull) + (u64)lane * 16; a < end; a += 64 * 16) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(heap + a);
#pragma unroll
      for (u32 b = 0; b < 16; ++b) {
        const u64 s = a + b;
        if (s >= f && s < end) out[t + (s - f)] = (u8)strmap_fold((v[b >> 2] >> (8 * (b & 3))) & 0xFFu, dir);
      }
    }
  }
}

// ---- OP_STRING_REPLACE (string_evaluators.h:76-90 -> utils/strings/util.cc:201-222, replace_all): the first producer whose image is
// no slice of its value.  Matches are leftmost and non-overlapping, found left to right (pos = find(needle, start); start = pos +
// |needle|), the substitute is never searched again, bytes are bytes, and an empty needle leaves the value as it is.  Both passes make
// the same SELECTION of matches and differ in what they do with it:
//   length pass  lens[n + i] = |v_i| + matches_i * (|sub| - |needle|);
//   write pass   source byte s outside every selected match goes to s - start + k(s) * (|sub| - |needle|), k(s) = the number of selected
//                matches that start before s, and every selected match writes the substitute at the place its first byte would get.
// A candidate start s is tested only while s + |needle| <= the value's end, so no match runs on into the next value's bytes (values are
// packed end to end), and an empty needle or one longer than the value reads nothing.
// Lane form: ascending candidate starts over aligned 8-byte words; after a match the walk goes on at s + |needle|.
// Wave form: a step is 64 lanes x one aligned 16-byte word = 1 KiB; a lane tests its 16 starts (first byte in registers, the rest of the
// needle from the heap) into a 16-bit mask, and the step is resolved in 16 SUB-STEPS of 64 consecutive starts: the lanes' mask bits are
// brought into position order with one shuffle and a ballot, and the wave resolves the greedy selection on that wave-uniform 64-bit mask --
// lowest set bit p, clear everything below p + |needle| -- carrying two things from sub-step to sub-step and from step to step: the
// running match count and the position up to which bytes are covered by the last selected match (a needle may span many sub-steps).
// The four lanes that own a sub-step's bytes keep its (selected, covered, count before) triple and write their own 16 bytes from
// registers afterwards; no byte moves between lanes.
struct StrRepArgs { const u8* heap; const u8* needle; const u8* sub; u8* out; u32 nlen, slen; };

__device__ __forceinline__ bool strrep_rest(const u8* __restrict__ h, const u8* __restrict__ needle, u32 nlen) {
  for (u32 k = 1; k < nlen; ++k)
    if (h[k] != needle[k]) return false;
  return true;
}
__device__ __forceinline__ void strrep_put_sub(const StrRepArgs& A, u64 at) {
  for (u32 k = 0; k < A.slen; ++k) A.out[at + k] = A.sub[k];
}

// one value heap[off, off + len) by one lane -> its match count; WRITE: its image to out[to ...)
template <bool WRITE>
__device__ __forceinline__ u64 strrep_lane(const StrRepArgs& A, u64 off, u64 len, u64 to) {
  const bool fits = A.nlen != 0 && len >= (u64)A.nlen;
  if (!WRITE && !fits) return 0;
  const u64 end = off + len, last = fits ? end - A.nlen : 0;       // last candidate start
  const u64 stop = WRITE ? end : last + 1;
  const u32 n0 = fits ? A.needle[0] : 0u;
  const i64 delta = (i64)A.slen - (i64)A.nlen;
  u64 count = 0, next = off;                                       // bytes below `next` are covered by the last match
  for (u64 a = off & ~7ull; a < stop; a += 8) {
    const u64 w = *reinterpret_cast<const u64*>(A.heap + a);
    for (u32 b = 0; b < 8; ++b) {
      const u64 s = a + b;
      if (s < off || s >= stop || s < next) continue;
      const u32 c = (u32)(w >> (8 * b)) & 0xFFu;
      if (fits && s <= last && c == n0 && strrep_rest(A.heap + s, A.needle, A.nlen)) {
        if (WRITE) strrep_put_sub(A, (u64)((i64)(to + (s - off)) + (i64)count * delta));
        ++count; next = s + A.nlen;
        continue;
      }
      if (WRITE) A.out[(u64)((i64)(to + (s - off)) + (i64)count * delta)] = (u8)c;
    }
  }
  return count;
}

// one value heap[o, o + l) by the whole wave (every loop is wave-uniform) -> its match count; WRITE: its image to out[t ...)
template <bool WRITE>
__device__ __forceinline__ u64 strrep_wave(const StrRepArgs& A, u64 o, u64 l, u64 t, u32 lane) {
  const bool fits = A.nlen != 0 && l >= (u64)A.nlen;
  if (!WRITE && !fits) return 0;
  const u64 end = o + l, last = fits ? end - A.nlen : 0;
  const u64 stop = WRITE ? end : last + 1;
  const u32 n0 = fits ? A.needle[0] : 0u;
  const i64 delta = (i64)A.slen - (i64)A.nlen;
  u64 count = 0, covered = o;                                      // wave-uniform: matches so far; bytes below `covered` are inside one
  for (u64 base = o & ~15ull; base < stop; base += 64 * 16) {
    const u64 a = base + (u64)lane * 16;
    u32x4 v = {0u, 0u, 0u, 0u};
    u32 mine = 0;                                                  // bit b: the needle is at a + b
    if (a < stop) {
      v = *reinterpret_cast<const u32x4*>(A.heap + a);
      if (fits) {
#pragma unroll
        for (u32 b = 0; b < 16; ++b) {
          const u64 s = a + b;
          if (s < o || s > last) continue;
          if (((v[b >> 2] >> (8 * (b & 3))) & 0xFFu) != n0) continue;
          if (strrep_rest(A.heap + s, A.needle, A.nlen)) mine |= 1u << b;
        }
      }
    }
    u64 my_sel = 0, my_cov = 0, my_cnt = 0;                        // of the sub-step that holds this lane's 16 bytes
#pragma unroll 1
    for (u32 j = 0; j < 16; ++j) {
      const u64 sb = base + 64ull * j;                             // the sub-step's starts are sb + 0 .. 63, start sb + i on bit i
      if (sb >= stop) break;
      const u32 from = (u32)__shfl((int)mine, (int)(4 * j + (lane >> 4)), 64);
      u64 m = __ballot((from >> (lane & 15)) & 1u);
      const u64 cnt_in = count;
      u64 sel = 0, cov = 0;
      if (covered > sb) { const u64 k = covered - sb; cov = k >= 64 ? ~0ull : (1ull << k) - 1; }
      m &= ~cov;
      while (m) {
        const u32 p = (u32)__ffsll((long long)m) - 1;
        const u64 e = (u64)p + A.nlen;                             // the match covers bits [p, e)
        sel |= 1ull << p; ++count; covered = sb + e;
        const u64 below_p = (1ull << p) - 1;
        if (e >= 64) { cov |= ~below_p; m = 0; }
        else { const u64 below_e = (1ull << e) - 1; cov |= below_e & ~below_p; m &= ~below_e; }
      }
      if ((lane >> 2) == j) { my_sel = sel; my_cov = cov; my_cnt = cnt_in; }
    }
    if (WRITE && a < end) {
#pragma unroll 1                                                   // (unrolled, the 16 substitute loops cost 256 VGPRs instead of 128)
      for (u32 b = 0; b < 16; ++b) {
        const u64 s = a + b;
        if (s < o || s >= end) continue;
        const u32 bit = (lane & 3) * 16 + b;
        const u64 k = my_cnt + (u64)__popcll(my_sel & ((1ull << bit) - 1));
        const u64 at = (u64)((i64)(t + (s - o)) + (i64)k * delta);
        if ((my_sel >> bit) & 1) strrep_put_sub(A, at);
        else if (!((my_cov >> bit) & 1)) A.out[at] = (u8)((v[b >> 2] >> (8 * (b & 3))) & 0xFFu);
      }
    }
  }
  return count;
}

// lens: 2n + 1 words (the last one is the scan's): lens[i] = |v_i|, lens[n + i] = |replace(v_i)|
__global__ __launch_bounds__(STRMAP_THREADS) void ssgpu_str_replace_len_kernel(const u8* __restrict__ heap, const u64* __restrict__ offs, u64 n,
                                                                               const u8* __restrict__ needle, u32 nlen, u32 slen, u64* __restrict__ lens) {
  const u64 row = (u64)blockIdx.x * STRMAP_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n;
  const u64 off = live ? offs[row] : 0, len = live ? offs[row + 1] - off : 0;
  const StrRepArgs A = {heap, needle, nullptr, nullptr, nlen, slen};
  const bool searched = live && nlen != 0 && len >= (u64)nlen;     // anything else has no match and reads nothing
  u64 count = 0;
  if (searched && len <= STRMAP_LONG) count = strrep_lane<false>(A, off, len, 0);
  u64 todo = __ballot(searched && len > STRMAP_LONG);
  while (todo) {
    const int who = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 c = strrep_wave<false>(A, __shfl(off, who, 64), __shfl(len, who, 64), 0, lane);
    if ((int)lane == who) count = c;
  }
  if (live) { lens[row] = len; lens[n + row] = (u64)((i64)len + (i64)count * ((i64)slen - (i64)nlen)); }
}

// image i -> out[dst_offs[i], dst_offs[i + 1]); a lane's job when the value AND its image are at most STRMAP_LONG bytes, the wave's otherwise
// (a short value with a long image is a lane's worth of reading and a wave's worth of writing)
__global__ __launch_bounds__(STRMAP_THREADS) void ssgpu_str_replace_write_kernel(const u8* __restrict__ heap, const u64* __restrict__ offs, const u64* __restrict__ dst_offs,
                                                                                 u64 n, const u8* __restrict__ needle, u32 nlen, const u8* __restrict__ sub, u32 slen,
                                                                                 u8* __restrict__ out) {
  const u64 row = (u64)blockIdx.x * STRMAP_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n;
  const u64 off = live ? offs[row] : 0, len = live ? offs[row + 1] - off : 0;
  const u64 to = live ? dst_offs[row] : 0, image = live ? dst_offs[row + 1] - to : 0;
  const StrRepArgs A = {heap, needle, sub, out, nlen, slen};
  const bool lng = len > STRMAP_LONG || image > STRMAP_LONG;
  if (live && !lng) (void)strrep_lane<true>(A, off, len, to);
  u64 todo = __ballot(live && lng);
  while (todo) {
    const int who = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    (void)strrep_wave<true>(A, __shfl(off, who, 64), __shfl(len, who, 64), __shfl(to, who, 64), lane);
  }
}

// One step's codes (n remap entries, then n table entries, codes of the step's own dictionary) through `later` -- that dictionary's
// codes -> the final dictionary's, NULL = the step is the last one: to_final[i] = the final code of the step's input value i, and
// table[to_final[i]] = the final code of its image.  `table` was zeroed: entries of values that joined after the step stay 0.
__global__ __launch_bounds__(STRMAP_THREADS) void ssgpu_str_map_compose_kernel(const int* __restrict__ codes, u64 n, const int* __restrict__ later, u64 n_later,
                                                                               u64 n_final, int* __restrict__ to_final, int* __restrict__ table) {
  const u64 i = (u64)blockIdx.x * STRMAP_THREADS + threadIdx.x;
  if (i >= n) return;
  u64 a = (u64)(u32)codes[i], b = (u64)(u32)codes[n + i];
  if (later) { a = a < n_later ? (u64)(u32)later[a] : 0; b = b < n_later ? (u64)(u32)later[b] : 0; }
  if (a >= n_final) a = 0;                             // (cannot happen: codes are ranks in the step's dictionary)
  if (b >= n_final) b = 0;
  to_final[i] = (int)a;
  table[a] = (int)b;
}

static inline unsigned strmap_grid(u64 n) { return (unsigned)((n + STRMAP_THREADS - 1) / STRMAP_THREADS); }

hipError_t ssgpu_launch_str_map_len(const uint8_t* heap, const uint64_t* offs, uint64_t n, int fn, int has_len, int64_t pos, int64_t len,
                                    uint64_t* lens, uint64_t* src, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_map_len_kernel, dim3(strmap_grid(n)), dim3(STRMAP_THREADS), 0, s, heap, (const u64*)offs, (u64)n, fn, has_len, (i64)pos,
                            (i64)len, (u64*)lens, (u64*)src);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_map_write(const uint8_t* heap, const uint64_t* src, const uint64_t* dst_offs, uint64_t n, int dir, uint8_t* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_map_write_kernel, dim3(strmap_grid(n)), dim3(STRMAP_THREADS), 0, s, heap, (const u64*)src, (const u64*)dst_offs, (u64)n, dir, out);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_replace_len(const uint8_t* heap, const uint64_t* offs, uint64_t n, const uint8_t* needle, uint32_t needle_len, uint32_t sub_len,
                                        uint64_t* lens, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_replace_len_kernel, dim3(strmap_grid(n)), dim3(STRMAP_THREADS), 0, s, heap, (const u64*)offs, (u64)n, needle, needle_len, sub_len,
                            (u64*)lens);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_replace_write(const uint8_t* heap, const uint64_t* offs, const uint64_t* dst_offs, uint64_t n, const uint8_t* needle, uint32_t needle_len,
                                          const uint8_t* sub, uint32_t sub_len, uint8_t* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_replace_write_kernel, dim3(strmap_grid(n)), dim3(STRMAP_THREADS), 0, s, heap, (const u64*)offs, (const u64*)dst_offs, (u64)n, needle,
                            needle_len, sub, sub_len, out);
  return hipGetLastError();
}
hipError_t ssgpu_launch_str_map_compose(const int32_t* codes, uint64_t n, const int32_t* later, uint64_t n_later, uint64_t n_final, int32_t* to_final,
                                        int32_t* table, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ssgpu_str_map_compose_kernel, dim3(strmap_grid(n)), dim3(STRMAP_THREADS), 0, s, (const int*)codes, (u64)n, (const int*)later, (u64)n_later,
                            (u64)n_final, (int*)to_final, (int*)table);
  return hipGetLastError();
}

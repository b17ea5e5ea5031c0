// string_parse_kernels.hip -- PARSE_STRING (OP_PARSE_STRING_QUIET / OP_PARSE_STRING_NULLING): a STRING value turned into a number,
// once per DISTINCT value.
//
// Like string_fn_kernels.hip: a STRING value in a plan is the code of the plan's dictionary, so parse(s) = V[code(s)] and
// "the parse failed" = F[code(s)].  The kernel below builds both tables from the packed dictionary (`offsets[n + 1]` into one
// byte heap); the pipeline reads V with GATHER_8 / _32 / _64 and F with GATHER_NULL on the same slot (vm_body.inc).
//
// What is parsed is the value CUT AT ITS FIRST 0x00 BYTE (the reference hands input.as_string().c_str() to its parsers,
// expression_evaluators.h:73-78).  isspace = the six bytes ' ' \t \n \v \f \r (ascii_isspace; bytes >= 0x80 are not space).
//   INT32 / UINT32 / INT64 / UINT64   safe_strto*, base 10 (numbers.cc:565-751): strip isspace from both ends (nothing left: failure,
//       0); one optional '-' / '+' (nothing behind it: failure, 0; '-' on an unsigned target: failure, 0); then digits only -- the
//       first other byte is a failure whose value is the conversion of the digits before it; overflow is a failure with value max,
//       underflow one with value min; the limits themselves parse.  The loop is the reference's: multiply, then add (subtract),
//       each behind its vmax / 10 (vmin / 10) pre-check -- here on the magnitude in 64-bit unsigned, which gives the same answers.
//   BOOL   types_infrastructure.cc:178-205: strip ' ' \t \r (only these; \n stays), then true / yes / false / no whatever the
//       case (A-Z only).  Anything else -- anything longer than 5 bytes after the trim -- fails; a failure's value is false.
//   DOUBLE / FLOAT   safe_strtod / safe_strtof are glibc's strtod / strtof.  The device takes the EXACT FAST PATH only:
//           isspace* [+-]? digits* ('.' digits*)? ([eE] [+-]? digit{1,4})? isspace*
//       with a mantissa digit, at most 19 significant digits (leading zeros dropped, before and behind the point) -- the mantissa w
//       is exact in 64 bits --, at most STRPARSE_WINDOW bytes from the first byte behind the sign that is not '0' to the end of
//       the trimmed value (what one lane walks), and for DOUBLE w <= 2^53, e = exponent - fraction digits in [-22, 22]; for FLOAT
//       w <= 2^24, |e| <= 10.  There w and 10^|e| are exact, so ONE correctly rounded multiply or divide is the correctly rounded
//       result (Clinger); the sign goes on last ("-0" is -0.0); a FLOAT never goes through a double.  Every other value but the
//       empty one (a failure with value 0: no parser is asked) is marked STRPARSE_HARD in F and left to the host, which calls
//       strtod / strtof on the value's own bytes and patches both tables (string_dict.cpp).  The device never decides that a floating
//       parse FAILED.
//
// Work split as in string_fn_kernels.hip: one lane per value of up to STRPARSE_LONG = 128 bytes, a whole wave per longer value
// -- a long value is still a legal number (200 spaces, then "7"; 300 zeros, then "12").  Both forms first find the same five
// positions -- the first 0x00, the first and the last byte in front of it that is no space, behind the sign the first byte that
// is not '0' and the first that is no digit -- the lane form with loops of its own over the value (aligned 8-byte words of the
// heap), the wave form by MIN / MAX reductions over steps of 64 x 16 aligned bytes (every loop wave-uniform, none longer than the
// value).  From there ONE lane converts, with the same code in both forms: at most 21 significant digits of an integer (a 21st
// is an overflow in every target), at most STRPARSE_WINDOW bytes of a floating value, at most 5 bytes of a BOOL.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch.h"
#include "../../include/ssgpu.h"

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

#define STRPARSE_THREADS 256
#define STRPARSE_LONG 128
#define STRPARSE_NONE 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ bool strparse_space(u32 c, bool bool_set) {
  return bool_set ? (c == 32u || c == 9u || c == 13u) : (c == 32u || c - 9u < 5u);
}
__device__ __forceinline__ bool strparse_digit(u32 c) { return c - 48u < 10u; }

__device__ __forceinline__ u64 strparse_wave_min(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ u64 strparse_wave_max(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
  return v;
}

// positions relative to the value's first byte.  nul: the first 0x00 (len: none); [b, e): what is left of [0, nul) without the
// spaces at both ends (b == e: nothing); p: behind the sign; z / nd: the first byte of [p, e) that is not '0' / no digit (e: none)
struct StrParseSpan { u64 nul, b, e, p, z, nd; bool neg; };

// ---- the conversions: one lane, the value's bytes straight from the heap ------------------------------------------------
// integers: v = the value's first byte.  Returns the failure byte; *out = the value's bits in 64 bits (the low half for 32)
__device__ u8 strparse_int(const u8* __restrict__ v, const StrParseSpan& S, int to_type, u64* out) {
  *out = 0;
  if (S.b >= S.e || S.p >= S.e) return 1;                             // nothing, or a sign alone
  const bool is_unsigned = to_type == SSGPU_UINT32 || to_type == SSGPU_UINT64;
  if (is_unsigned && S.neg) return 1;
  // the largest magnitude: vmax, or -vmin of a negative number
  const u64 lim = to_type == SSGPU_INT32 ? (S.neg ? 0x80000000ull : 0x7FFFFFFFull) : to_type == SSGPU_UINT32 ? 0xFFFFFFFFull
                  : to_type == SSGPU_INT64 ? (S.neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull) : 0xFFFFFFFFFFFFFFFFull;
  const u64 lim_over_10 = lim / 10;
  const u64 stop = S.nd < S.e ? S.nd : S.e;
  u64 m = 0;
  bool over = false;
  for (u64 i = S.z; i < stop && i < S.z + 21; ++i) {                  // v[z] is 1-9: the 21st digit overflows every target
    const u64 d = (u64)v[i] - 48u;
    if (m > lim_over_10) { over = true; break; }
    m *= 10;
    if (m > lim - d) { over = true; break; }
    m += d;
  }
  if (over) m = lim;
  *out = S.neg ? 0ull - m : m;
  return (over || S.nd < S.e) ? 1 : 0;
}

// BOOL: at most 5 bytes matter
__device__ u8 strparse_bool(const u8* __restrict__ v, const StrParseSpan& S, u64* out) {
  *out = 0;
  const u64 n = S.e - S.b;
  if (S.b >= S.e || n > 5) return 1;
  u64 w = 0;                                                          // the bytes, A-Z folded, first byte lowest
  for (u64 i = 0; i < n; ++i) { u32 c = v[S.b + i]; if (c - 65u < 26u) c |= 0x20u; w |= (u64)c << (8 * i); }
  const u64 t_true = 0x65757274ull, t_yes = 0x736579ull, t_false = 0x65736C6166ull, t_no = 0x6F6Eull;
  if ((n == 4 && w == t_true) || (n == 3 && w == t_yes)) { *out = 1; return 0; }
  if ((n == 5 && w == t_false) || (n == 2 && w == t_no)) return 0;
  return 1;
}

__device__ const double strparse_p10_f64[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
__device__ const float strparse_p10_f32[11] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f};

// DOUBLE / FLOAT: 0 with the value's bits in *out, or STRPARSE_HARD
__device__ u8 strparse_float(const u8* __restrict__ v, const StrParseSpan& S, bool is_f32, u64* out) {
  *out = 0;
  if (S.nul == 0) return 1;                                           // the empty value: *str == '\0', no parser is asked
  if (S.b >= S.e || S.p >= S.e) return STRPARSE_HARD;
  if (S.e - S.z > STRPARSE_WINDOW) return STRPARSE_HARD;
  u64 i = S.z, w = 0;
  int nsig = 0, frac = 0;
  bool digits = S.z > S.p;                                            // the zeros in front are mantissa digits
  for (; i < S.e && strparse_digit(v[i]); ++i) { if (++nsig > 19) return STRPARSE_HARD; w = w * 10 + ((u64)v[i] - 48u); digits = true; }
  if (i < S.e && v[i] == 46u) {
    for (++i; i < S.e && strparse_digit(v[i]); ++i) {
      const u64 d = (u64)v[i] - 48u;
      if (nsig > 0 || d != 0) { if (++nsig > 19) return STRPARSE_HARD; w = w * 10 + d; }
      ++frac; digits = true;
    }
  }
  if (!digits) return STRPARSE_HARD;
  int ex = 0;
  if (i < S.e && (v[i] | 0x20u) == 101u) {
    ++i;
    bool eneg = false;
    if (i < S.e && (v[i] == 45u || v[i] == 43u)) { eneg = v[i] == 45u; ++i; }
    int nd = 0;
    for (; i < S.e && strparse_digit(v[i]); ++i) { if (++nd > 4) return STRPARSE_HARD; ex = ex * 10 + (int)(v[i] - 48u); }
    if (nd == 0) return STRPARSE_HARD;
    if (eneg) ex = -ex;
  }
  if (i != S.e) return STRPARSE_HARD;
  const int e10 = ex - frac;
  if (is_f32) {
    if (w > (1ull << 24) || e10 < -10 || e10 > 10) return STRPARSE_HARD;
    const float x = (float)(u32)w;                                    // exact: w <= 2^24
    float r = e10 < 0 ? __fdiv_rn(x, strparse_p10_f32[-e10]) : __fmul_rn(x, strparse_p10_f32[e10]);
    if (S.neg) r = -r;
    *out = (u64)__float_as_uint(r);
  } else {
    if (w > (1ull << 53) || e10 < -22 || e10 > 22) return STRPARSE_HARD;
    const double x = (double)w;                                       // exact: w <= 2^53
    double r = e10 < 0 ? __ddiv_rn(x, strparse_p10_f64[-e10]) : __dmul_rn(x, strparse_p10_f64[e10]);
    if (S.neg) r = -r;
    *out = (u64)__double_as_longlong(r);
  }
  return 0;
}

__device__ void strparse_convert(const u8* __restrict__ v, const StrParseSpan& S, int to_type, u64 row, void* __restrict__ values, u8* __restrict__ failed) {
  u64 bits = 0;
  u8 f;
  if (to_type == SSGPU_BOOL) f = strparse_bool(v, S, &bits);
  else if (to_type == SSGPU_DOUBLE || to_type == SSGPU_FLOAT) f = strparse_float(v, S, to_type == SSGPU_FLOAT, &bits);
  else f = strparse_int(v, S, to_type, &bits);
  if (to_type == SSGPU_BOOL) static_cast<u8*>(values)[row] = (u8)bits;
  else if (to_type == SSGPU_INT32 || to_type == SSGPU_UINT32 || to_type == SSGPU_FLOAT) static_cast<u32*>(values)[row] = (u32)bits;
  else static_cast<u64*>(values)[row] = bits;
  failed[row] = f;
}

// the sign at b (BOOL has none)
__device__ __forceinline__ void strparse_sign(const u8* __restrict__ v, StrParseSpan* S, bool has_sign) {
  S->neg = false; S->p = S->b;
  if (has_sign && S->b < S->e) { const u32 c = v[S->b]; S->neg = c == 45u; if (c == 45u || c == 43u) S->p = S->b + 1; }
  S->z = S->e; S->nd = S->e;
}

__global__ __launch_bounds__(STRPARSE_THREADS) void ssgpu_str_parse_kernel(const u8* __restrict__ heap, const u64* __restrict__ offs, u64 n, int to_type,
                                                                           void* __restrict__ values, u8* __restrict__ failed) {
  const u64 row = (u64)blockIdx.x * STRPARSE_THREADS + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = row < n;
  const u64 off = live ? offs[row] : 0, len = live ? offs[row + 1] - off : 0;
  const bool bool_set = to_type == SSGPU_BOOL;
  if (live && len <= STRPARSE_LONG) {
    StrParseSpan S;
    u64 first = STRPARSE_NONE, last = 0;
    S.nul = len;
    for (u64 a = off & ~7ull; a < off + len && S.nul == len; a += 8) {
      const u64 w = *reinterpret_cast<const u64*>(heap + a);
      for (u32 k = 0; k < 8; ++k) {
        const u64 s = a + k;
        if (s < off || s >= off + len) continue;
        const u32 c = (u32)(w >> (8 * k)) & 0xFFu;
        if (c == 0) { S.nul = s - off; break; }
        if (!strparse_space(c, bool_set)) { if (first == STRPARSE_NONE) first = s - off; last = s - off + 1; }
      }
    }
    S.b = first == STRPARSE_NONE ? 0 : first; S.e = first == STRPARSE_NONE ? 0 : last;
    strparse_sign(heap + off, &S, !bool_set);
    if (!bool_set) {
      for (u64 a = (off + S.p) & ~7ull; a < off + S.e && S.nd == S.e; a += 8) {
        const u64 w = *reinterpret_cast<const u64*>(heap + a);
        for (u32 k = 0; k < 8; ++k) {
          const u64 s = a + k;
          if (s < off + S.p || s >= off + S.e) continue;
          const u32 c = (u32)(w >> (8 * k)) & 0xFFu;
          if (c != 48u && S.z == S.e) S.z = s - off;
          if (!strparse_digit(c)) { S.nd = s - off; break; }
        }
      }
    }
    strparse_convert(heap + off, S, to_type, row, values, failed);
  }
  // long values: the whole wave scans one of them at a time (every loop below is wave-uniform)
  u64 todo = __ballot(live && len > STRPARSE_LONG);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const u64 o = __shfl(off, src, 64), l = __shfl(len, src, 64);
    StrParseSpan S;
    u64 first = STRPARSE_NONE, last = 0;
    S.nul = l;
    for (u64 base = o & ~15ull; base < o + l && S.nul == l; base += 64 * 16) {
      const u64 a = base + (u64)lane * 16;
      u64 lnul = STRPARSE_NONE, lfirst = STRPARSE_NONE, llast = 0;
      if (a < o + l) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(heap + a);
#pragma unroll
        for (u32 k = 0; k < 16; ++k) {
          const u64 s = a + k;
          if (s < o || s >= o + l || lnul != STRPARSE_NONE) continue;
          const u32 c = (v[k >> 2] >> (8 * (k & 3))) & 0xFFu;
          if (c == 0) { lnul = s - o; continue; }
          if (!strparse_space(c, bool_set)) { if (lfirst == STRPARSE_NONE) lfirst = s - o; llast = s - o + 1; }
        }
      }
      const u64 wnul = strparse_wave_min(lnul);
      // what lies behind the step's first 0x00 does not count (a lane in front of it has seen no 0x00 of its own)
      if (lfirst != STRPARSE_NONE && lfirst > wnul) lfirst = STRPARSE_NONE;
      if (llast > wnul) llast = 0;
      const u64 wfirst = strparse_wave_min(lfirst), wlast = strparse_wave_max(llast);
      if (first == STRPARSE_NONE) first = wfirst;
      if (wlast > last) last = wlast;
      if (wnul != STRPARSE_NONE) S.nul = wnul;
    }
    S.b = first == STRPARSE_NONE ? 0 : first; S.e = first == STRPARSE_NONE ? 0 : last;
    strparse_sign(heap + o, &S, !bool_set);                           // (every lane reads the same byte)
    if (!bool_set) {
      const u64 lo = o + S.p, hi = o + S.e;
      for (u64 base = lo & ~15ull; base < hi && S.nd == S.e; base += 64 * 16) {
        const u64 a = base + (u64)lane * 16;
        u64 lz = STRPARSE_NONE, lnd = STRPARSE_NONE;
        if (a < hi) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(heap + a);
#pragma unroll
          for (u32 k = 0; k < 16; ++k) {
            const u64 s = a + k;
            if (s < lo || s >= hi) continue;
            const u32 c = (v[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            if (c != 48u && lz == STRPARSE_NONE) lz = s - o;
            if (!strparse_digit(c) && lnd == STRPARSE_NONE) lnd = s - o;
          }
        }
        const u64 wz = strparse_wave_min(lz), wnd = strparse_wave_min(lnd);
        if (S.z == S.e && wz != STRPARSE_NONE) S.z = wz;
        if (wnd != STRPARSE_NONE) S.nd = wnd;
      }
    }
    if ((int)lane == src) strparse_convert(heap + o, S, to_type, row, values, failed);
  }
}

hipError_t ssgpu_launch_str_parse(const uint8_t* heap, const uint64_t* offs, uint64_t n, int to_type, void* values, uint8_t* failed, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t grid = (n + STRPARSE_THREADS - 1) / STRPARSE_THREADS;
  hipLaunchKernelGGL(ssgpu_str_parse_kernel, dim3((unsigned)grid), dim3(STRPARSE_THREADS), 0, s, heap, (const u64*)offs, (u64)n, to_type, values, failed);
  return hipGetLastError();
}

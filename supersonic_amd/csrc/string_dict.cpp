// string_dict.cpp -- the STRING dictionary's device work: the encoder chain that turns a domain of byte strings into sorted distinct
// values and codes (string_dict_kernels.hip), the tables over a dictionary that a plan's programs gather from (string_fn_kernels.hip,
// string_parse_kernels.hip; a closed dictionary's own tables are only uploaded) and the ABI entry points that work on a dictionary
// without a plan: ssgpu_dict_eval, ssgpu_dict_parse, ssgpu_dict_close (string_map_kernels.hip).  Nothing here knows a plan: the
// runtime hands in a context, a dictionary, the specs of the tables and the plan's step list.
#include <chrono>
#include <deque>
#include <locale.h>
#include <set>
#include <string.h>

#include "runtime_internal.h"

using namespace ssgpu;

// ---- the encoder chain (runtime_internal.h: encode_domain) ------------------------------------------------------------------
int encode_domain(ssgpu_ctx* c, hipStream_t s, const uint8_t* bytes, uint64_t* lens, bool scanned, const uint8_t* dnull, uint64_t n,
                  const std::vector<DomainCodes>& targets, uint64_t heap_pad, std::vector<uint64_t>* off_h_out, std::vector<char>* heap_h_out,
                  uint32_t* D_out, DevBuf& out_off, DevBuf& out_heap) {
  std::vector<uint64_t>& off_h = *off_h_out;
  std::vector<char>& heap_h = *heap_h_out;
  off_h.assign(1, 0);
  heap_h.clear();
  uint32_t D = 0;
  if (n) {
    uint64_t cap = 64, np2 = 1;
    while (cap < 2 * n) cap <<= 1;
    while (np2 < n) np2 <<= 1;
    DevBuf partials, hashes, table, row_slot, flags, d_slot, d_off, d_len, d_key, d_idx, slot_rank;
    const bool alloc_ok =
        partials.ensure(ssgpu_str_scan_partials(n) * 8) == hipSuccess && hashes.ensure(n * 8) == hipSuccess && table.ensure(cap * 8) == hipSuccess &&
        row_slot.ensure(n * 4) == hipSuccess && flags.ensure(8) == hipSuccess && d_slot.ensure(n * 4) == hipSuccess && d_off.ensure(n * 8) == hipSuccess &&
        d_len.ensure(n * 8) == hipSuccess && d_key.ensure(np2 * 8) == hipSuccess && d_idx.ensure(np2 * 4) == hipSuccess &&
        slot_rank.ensure(cap * 4) == hipSuccess && out_off.ensure((n + 1) * 8) == hipSuccess;
    if (!alloc_ok) { c->err = "Memory exceeded: the STRING dictionary's device tables"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
    const uint64_t* offs = lens;
    if (!scanned) HIP_TRY(c, ssgpu_launch_str_scan(lens, n, partials.as<uint64_t>(), s));
    HIP_TRY(c, ssgpu_launch_str_hash(bytes, offs, dnull, n, hashes.as<uint64_t>(), s));
    HIP_TRY(c, hipMemsetAsync(table.p, 0, cap * 8, s));
    HIP_TRY(c, hipMemsetAsync(flags.p, 0, 8, s));
    HIP_TRY(c, ssgpu_launch_str_insert(bytes, offs, dnull, hashes.as<uint64_t>(), n, table.as<uint64_t>(), cap, row_slot.as<uint32_t>(),
                                       flags.as<uint32_t>() + 1, s));
    HIP_TRY(c, ssgpu_launch_str_compact(table.as<uint64_t>(), cap, bytes, offs, flags.as<uint32_t>(), d_slot.as<uint32_t>(), d_off.as<uint64_t>(),
                                        d_len.as<uint64_t>(), d_key.as<uint64_t>(), d_idx.as<uint32_t>(), s));
    uint32_t fl[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(fl, flags.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (fl[1]) { c->err = "STRING dictionary: hash table overflow"; return SSGPU_ERROR_UNKNOWN; }
    D = fl[0];
    uint64_t p2 = 1;
    while (p2 < D) p2 <<= 1;
    HIP_TRY(c, ssgpu_launch_str_sort(d_key.as<uint64_t>(), d_idx.as<uint32_t>(), D, D ? p2 : 0, bytes, d_off.as<uint64_t>(), d_len.as<uint64_t>(), s));
    HIP_TRY(c, ssgpu_launch_str_rank(d_idx.as<uint32_t>(), d_slot.as<uint32_t>(), d_len.as<uint64_t>(), D, slot_rank.as<int32_t>(), out_off.as<uint64_t>(), s));
    HIP_TRY(c, ssgpu_launch_str_scan(out_off.as<uint64_t>(), D, partials.as<uint64_t>(), s));
    for (const DomainCodes& t : targets)
      HIP_TRY(c, ssgpu_launch_str_codes(row_slot.as<uint32_t>() + t.first, dnull + t.first, slot_rank.as<int32_t>(), t.rows, t.dst, s));
    off_h.resize((size_t)D + 1);
    HIP_TRY(c, hipMemcpyAsync(off_h.data(), out_off.p, ((size_t)D + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (out_heap.ensure(std::max<uint64_t>(off_h[D], 1) + heap_pad) != hipSuccess) { c->err = "Memory exceeded: the STRING dictionary's values"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
    if (heap_pad) HIP_TRY(c, hipMemsetAsync(static_cast<char*>(out_heap.p) + off_h[D], 0, heap_pad, s));
    HIP_TRY(c, ssgpu_launch_str_gather(bytes, d_off.as<uint64_t>(), d_idx.as<uint32_t>(), out_off.as<uint64_t>(), D, out_heap.as<uint8_t>(), s));
    heap_h.resize((size_t)off_h[D]);
    if (off_h[D]) HIP_TRY(c, hipMemcpyAsync(heap_h.data(), out_heap.p, (size_t)off_h[D], hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  *D_out = D;
  return SSGPU_OK;
}

// ---- tables over the STRING dictionary (string_fn_kernels.hip) ------------------------------------------------------
namespace {
int dict_upload(ssgpu_ctx* c, const ssgpu_dict* d, DictDevice* out) {
  const uint64_t n = (uint64_t)ssgpu_dict_size(d), hb = ssgpu_dict_heap_bytes(d);
  std::vector<uint64_t> offs(n + 1);
  std::vector<char> heap(hb + 1);
  ssgpu_dict_pack(d, offs.data(), heap.data());
  HIP_TRY(c, out->offs.ensure((n + 1) * 8));
  HIP_TRY(c, out->heap.ensure(hb + STRFN_HEAP_PAD));
  HIP_TRY(c, hipMemcpyAsync(out->offs.p, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (hb) HIP_TRY(c, hipMemcpyAsync(out->heap.p, heap.data(), hb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(static_cast<char*>(out->heap.p) + hb, 0, STRFN_HEAP_PAD, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host copies above go out of scope)
  out->n = n;
  return SSGPU_OK;
}
// table[c] = fn(value c); an empty dictionary gets ONE entry: NULL rows carry code 0 and the gather still reads table[0]
int dict_table_build(ssgpu_ctx* c, const DictDevice& D, int fn, const char* needle, uint32_t nlen, bool fold, DevBuf* needle_dev, DevBuf* table) {
  HIP_TRY(c, table->ensure((size_t)std::max<uint64_t>(D.n, 1) * 4));
  if (D.n == 0) { HIP_TRY(c, hipMemsetAsync(table->p, 0, 4, c->stream)); return SSGPU_OK; }
  HIP_TRY(c, needle_dev->ensure(std::max<uint32_t>(nlen, 1)));
  if (fn == OP_STRING_OFFSET && nlen) HIP_TRY(c, hipMemcpyAsync(needle_dev->p, needle, nlen, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, ssgpu_launch_str_fn(D.heap.as<const uint8_t>(), D.offs.as<const uint64_t>(), D.n, fn, needle_dev->as<const uint8_t>(), fn == OP_STRING_OFFSET ? nlen : 0u,
                                 fold ? 1 : 0, table->as<uint32_t>(), c->stream));
  return SSGPU_OK;
}
// PARSE_STRING: values[c] = value c parsed as `to_type`, failed[c] = 1 where that parse fails (string_parse_kernels.hip).  The device decides
// the integer and BOOL targets alone.  Of a FLOAT / DOUBLE table it fills what lies on its exact fast path and marks the rest
// STRPARSE_HARD; those entries are finished here with the reference's own parser -- glibc strtof / strtod in the C locale on the value's
// bytes cut at the first 0x00, the value kept whatever the outcome (safe_strtof / safe_strtod, numbers.cc:802-829) -- and both tables
// patched before anything reads them.  *host_resolved += the number of such entries.  An empty dictionary gets one entry, 0 / not failed.
static locale_t parse_c_locale() { static locale_t loc = newlocale(LC_ALL_MASK, "C", (locale_t)0); return loc; }
int dict_parse_build(ssgpu_ctx* c, const DictDevice& D, const ssgpu_dict* d, int to_type, DevBuf* values, DevBuf* failed, int64_t* host_resolved,
                     hipEvent_t after_kernel = nullptr /* recorded behind the kernel, in front of the host's share */) {
  const size_t w = (size_t)dtype_width(to_type), n = (size_t)D.n;
  HIP_TRY(c, values->ensure(std::max<size_t>(n, 1) * w));
  HIP_TRY(c, failed->ensure(std::max<size_t>(n, 1)));
  if (n == 0) {
    HIP_TRY(c, hipMemsetAsync(values->p, 0, w, c->stream)); HIP_TRY(c, hipMemsetAsync(failed->p, 0, 1, c->stream));
    if (after_kernel) HIP_TRY(c, hipEventRecord(after_kernel, c->stream));
    return SSGPU_OK;
  }
  HIP_TRY(c, ssgpu_launch_str_parse(D.heap.as<const uint8_t>(), D.offs.as<const uint64_t>(), D.n, to_type, values->p, failed->as<uint8_t>(), c->stream));
  if (after_kernel) HIP_TRY(c, hipEventRecord(after_kernel, c->stream));
  if (!dtype_is_float(to_type)) return SSGPU_OK;
  std::vector<uint8_t> f(n);
  HIP_TRY(c, hipMemcpyAsync(f.data(), failed->p, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<size_t> hard;
  for (size_t i = 0; i < n; ++i) if (f[i] == STRPARSE_HARD) hard.push_back(i);
  if (hard.empty()) return SSGPU_OK;
  std::vector<char> v(n * w);
  HIP_TRY(c, hipMemcpyAsync(v.data(), values->p, n * w, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::string text;
  for (size_t i : hard) {
    const char* bytes = nullptr; int32_t len = 0;
    if (ssgpu_dict_decode(d, (int32_t)i, &bytes, &len) != SSGPU_OK) { c->err = "PARSE_STRING: the dictionary lost a value"; return SSGPU_ERROR_UNKNOWN; }
    text.assign(bytes, (size_t)len);
    const char* str = text.c_str();   // (cut at the first 0x00 by whoever reads it as a C string)
    char* end = nullptr;
    if (to_type == SSGPU_FLOAT) { const float x = strtof_l(str, &end, parse_c_locale()); memcpy(v.data() + i * w, &x, w); }
    else { const double x = strtod_l(str, &end, parse_c_locale()); memcpy(v.data() + i * w, &x, w); }
    if (end != str) while (*end == ' ' || (unsigned)(*end - 9) < 5u) ++end;   // ascii_isspace
    f[i] = (*str != '\0' && *end == '\0') ? 0 : 1;
  }
  HIP_TRY(c, hipMemcpyAsync(values->p, v.data(), n * w, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(failed->p, f.data(), n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host copies go out of scope)
  *host_resolved += (int64_t)hard.size();
  return SSGPU_OK;
}
}  // namespace

// ---- the table set of one owner (a plan) ------------------------------------------------------------------------------------------
int DictTables::build(ssgpu_ctx* c, const ssgpu_dict* d, uint64_t gen, const std::vector<DictTableSpec>& gathers, const std::vector<ssgpu_string_step>& steps,
                      int32_t* n_launches) {
  if (!d) {
    bool parses = false, others = false;
    for (const DictTableSpec& g : gathers) (g.kind() == DictTableSpec::PARSE ? parses : others) = true;
    if (parses && !others && steps.empty()) { c->err = "PARSE_STRING of a STRING value needs the plan's dictionary (ssgpu_plan_set_dict)"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    c->err = steps.empty() ? "LENGTH / STRING_OFFSET / PARSE_STRING of a STRING value need the plan's dictionary (ssgpu_plan_set_dict)"
                           : "LTRIM / RTRIM / TRIM / TO_UPPER / SUBSTRING / STRING_REPLACE need the plan's dictionary, closed under the plan's steps (ssgpu_plan_string_steps, "
                             "ssgpu_dict_close, ssgpu_plan_set_dict)";
    return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  }
  if (current(d, gen)) return SSGPU_OK;
  built = false;
  // String-producing nodes gather from the tables the CLOSED dictionary brings along (ssgpu_dict_close): the run computes nothing, but it
  // reads no table that is not its own -- the plan's step list must be a subsequence of the list the dictionary was closed under (a later
  // step's domain contains every earlier one's; the derived plans of chunked execution, the NaN-exact repeat and the skip form hold subsets)
  const int32_t dict_steps = ssgpu_dict_step_count(d);
  { int32_t k = 0;
    for (const ssgpu_string_step& s : steps) {
      while (k < dict_steps && !same_step(*ssgpu_dict_step(d, k), s)) ++k;
      if (k == dict_steps) {
        c->err = std::string("LTRIM / RTRIM / TRIM / TO_UPPER / SUBSTRING / STRING_REPLACE make STRING values: the plan's dictionary must be closed under the plan's ") +
                 std::to_string(steps.size()) + " step(s) (ssgpu_plan_string_steps, ssgpu_dict_close, ssgpu_plan_set_dict); this one " +
                 (dict_steps ? "was closed under another list of " + std::to_string(dict_steps) + " step(s)" : std::string("is not closed"));
        return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
      }
      ++k;
    } }
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (an earlier run may still read the tables that are replaced now)
  host_resolved = 0;
  bool computed = false;   // some table is COMPUTED from the packed dictionary (LENGTH / STRING_OFFSET / PARSE_STRING)
  for (const DictTableSpec& g : gathers) computed = computed || g.kind() != DictTableSpec::PRODUCER;
  int rc = computed ? dict_upload(c, d, &dev) : SSGPU_OK;
  if (rc != SSGPU_OK) return rc;
  const int32_t n = ssgpu_dict_size(d);
  std::set<DictTableSpec> parse_built;
  for (const DictTableSpec& g : gathers) {
    if (g.kind() == DictTableSpec::PRODUCER) {
      // the table of the LAST step with this spec: its domain is the largest.  An empty dictionary still gets one entry, 0.
      DevBuf& table = tables[g];
      int32_t k = dict_steps - 1;
      while (k >= 0 && !same_step(*ssgpu_dict_step(d, k), g)) --k;
      if (k < 0) { c->err = "internal: a producer table without its step"; return SSGPU_ERROR_UNKNOWN; }
      HIP_TRY(c, table.ensure((size_t)std::max<int32_t>(n, 1) * 4));
      if (n) HIP_TRY(c, hipMemcpyAsync(table.p, ssgpu_dict_step_table_data(d, k), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
      else HIP_TRY(c, hipMemsetAsync(table.p, 0, 4, c->stream));
      continue;
    }
    if (g.kind() == DictTableSpec::PARSE) {   // the same (target type) slot in several programs: built once
      if (!parse_built.insert(g).second) continue;
      rc = dict_parse_build(c, dev, d, g.to_type, &tables[g], &failed[g], &host_resolved);
      if (rc != SSGPU_OK) return rc;
      *n_launches += 1;
      continue;
    }
    const char* needle_bytes = ""; int32_t nlen = 0;
    if (g.fn == OP_STRING_OFFSET && ssgpu_dict_decode(d, g.needle_code, &needle_bytes, &nlen) != SSGPU_OK) {
      c->err = "STRING_OFFSET: the needle's code " + std::to_string(g.needle_code) + " is outside the plan's dictionary of " + std::to_string(n) + " values (ssgpu_plan_set_dict)";
      return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
    }
    rc = dict_table_build(c, dev, g.fn, needle_bytes, (uint32_t)nlen, g.fold, &needle, &tables[g]);
    if (rc != SSGPU_OK) return rc;
    *n_launches += 1;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  built = true; built_for = d; built_gen = gen;
  return SSGPU_OK;
}

void DictTables::slot(const DictTableSpec& spec, const void** data, const uint8_t** is_null) const {
  auto it = tables.find(spec);
  *data = it != tables.end() ? it->second.p : nullptr; *is_null = nullptr;
  if (spec.kind() != DictTableSpec::PARSE) return;
  auto f = failed.find(spec);   // PARSE_STRING: the slot's NULL mask is the failure table (GATHER_NULL of ParseStringNulling)
  if (f != failed.end()) *is_null = f->second.as<const uint8_t>();
}

std::string DictTables::describe(const DictTableSpec& g, const ssgpu_dict* d) const {
  std::string line = std::string("dictionary table: ") + string_fn_name(g.fn);
  switch (g.kind()) {
    case DictTableSpec::PRODUCER:
      if (g.fn == OP_STRING_REPLACE) line += " needle code " + std::to_string(g.pos) + " substitute code " + std::to_string(g.len);
      if (g.fn == OP_SUBSTRING) line += " position " + std::to_string(g.pos) + (g.has_len ? " length " + std::to_string(g.len) : std::string(" to the end"));
      return line + " (codes of the closed dictionary)\n";
    case DictTableSpec::PARSE:
      line += std::string(" to ") + dtype_name(g.to_type) + " (values and failure bytes)";
      if (built && dtype_is_float(g.to_type)) line += " host-resolved entries of the plan's floating tables: " + std::to_string(host_resolved);
      return line + "\n";
    case DictTableSpec::COMPUTED: break;
  }
  if (g.fn != OP_STRING_OFFSET) return line + "\n";
  const char* bytes = nullptr; int32_t len = 0;
  return line + " needle code " + std::to_string(g.needle_code) +
         (d && ssgpu_dict_decode(d, g.needle_code, &bytes, &len) == SSGPU_OK ? " length " + std::to_string(len) : std::string(" length unknown (no dictionary yet)")) +
         " fold " + (g.fold ? "1" : "0") + "\n";
}

// ---- a dictionary's tables without a plan ---------------------------------------------------------------------------------------------
namespace {
// What ssgpu_dict_eval and ssgpu_dict_parse share once their own arguments are checked: the device and result-buffer checks, the
// dictionary's upload and -- debug_timing, development -- the events around the call's parts, read back on stderr by the tools/ benches.
struct DictCall {
  ssgpu_ctx* c; const bool timed;
  DictDevice D;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  explicit DictCall(ssgpu_ctx* ctx) : c(ctx), timed(ctx->debug_timing != 0) {}
  ~DictCall() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
  // ev[0], the upload, ev[1]; `n_events`: how many of ev the caller records
  int begin(const ssgpu_dict* d, bool has_result_buffer, const char* who, int n_events) {
    if (c->device < 0) { c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
    if (ssgpu_dict_size(d) > 0 && !has_result_buffer) { c->err = std::string(who) + ": no result buffer"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (timed) { for (int i = 0; i < n_events; ++i) HIP_TRY(c, hipEventCreate(&ev[i])); HIP_TRY(c, hipEventRecord(ev[0], c->stream)); }
    const int rc = dict_upload(c, d, &D);
    return rc != SSGPU_OK ? rc : mark(1);
  }
  int mark(int i) { if (timed) HIP_TRY(c, hipEventRecord(ev[i], c->stream)); return SSGPU_OK; }
  float ms(int from, int to) const { float t = 0; (void)hipEventElapsedTime(&t, ev[from], ev[to]); return t; }
};
}  // namespace

extern "C" {

// T[c] = fn(value c) for every value of `d`, on the device (string_fn_kernels.hip) -- the tables a plan gathers LENGTH / STRING_OFFSET
// from, without a plan.  fn: OP_LENGTH (needle ignored) or OP_STRING_OFFSET.  out_host: ssgpu_dict_size(d) entries.
int ssgpu_dict_eval(ssgpu_ctx* c, const ssgpu_dict* d, int32_t fn, const char* needle, int32_t needle_len, int32_t fold_case, int32_t* out_host) {
  if (!c) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (!d || (fn != OP_LENGTH && fn != OP_STRING_OFFSET) || needle_len < 0 || (needle_len > 0 && !needle)) {
    c->err = "ssgpu_dict_eval: a dictionary, fn " + std::to_string(OP_LENGTH) + " (LENGTH) or " + std::to_string(OP_STRING_OFFSET) + " (STRING_OFFSET) and the needle's bytes";
    return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  }
  DictCall call(c);   // (tools/string_fn_bench.py reads its times)
  int rc = call.begin(d, out_host != nullptr, "ssgpu_dict_eval", 3);
  if (rc != SSGPU_OK) return rc;
  const int32_t n = ssgpu_dict_size(d);
  DevBuf needle_dev, table;
  rc = dict_table_build(c, call.D, fn, needle, (uint32_t)needle_len, fold_case != 0, &needle_dev, &table);
  if (rc == SSGPU_OK) rc = call.mark(2);
  if (rc != SSGPU_OK) return rc;
  if (n > 0) HIP_TRY(c, hipMemcpyAsync(out_host, table.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (call.timed) fprintf(stderr, "[ssgpu dict_eval] values %d upload_ms %.4f kernel_ms %.4f\n", n, call.ms(0, 1), call.ms(1, 2));
  return SSGPU_OK;
}
// The PARSE_STRING tables of `d` without a plan (string_parse_kernels.hip + the host's strtof / strtod for what the device leaves):
// out_values_host: ssgpu_dict_size(d) entries of to_type's width, out_failed_host: one byte per value, *out_host_resolved: how many
// entries the host finished.
int ssgpu_dict_parse(ssgpu_ctx* c, const ssgpu_dict* d, int32_t to_type, void* out_values_host, uint8_t* out_failed_host, int64_t* out_host_resolved) {
  if (!c) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (!d || !(dtype_is_numeric(to_type) || to_type == SSGPU_BOOL)) {
    c->err = "ssgpu_dict_parse: a dictionary and a target type of INT32, UINT32, INT64, UINT64, FLOAT, DOUBLE or BOOL";
    return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  }
  DictCall call(c);   // (tools/string_parse_bench.py reads its times)
  int rc = call.begin(d, out_values_host && out_failed_host, "ssgpu_dict_parse", 4);
  if (rc != SSGPU_OK) return rc;
  const int32_t n = ssgpu_dict_size(d);
  DevBuf values, failed;
  int64_t resolved = 0;
  rc = dict_parse_build(c, call.D, d, to_type, &values, &failed, &resolved, call.timed ? call.ev[3] : nullptr);
  if (rc == SSGPU_OK) rc = call.mark(2);
  if (rc != SSGPU_OK) return rc;
  if (n > 0) {
    HIP_TRY(c, hipMemcpyAsync(out_values_host, values.p, (size_t)n * (size_t)dtype_width(to_type), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out_failed_host, failed.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out_host_resolved) *out_host_resolved = resolved;
  // host_ms: a floating target's read-back of the failure bytes, the host's strtof / strtod and the patched tables' way back
  if (call.timed)
    fprintf(stderr, "[ssgpu dict_parse] values %d upload_ms %.4f kernel_ms %.4f host_ms %.4f host_resolved %lld\n", n, call.ms(0, 1), call.ms(1, 3), call.ms(3, 2), (long long)resolved);
  return SSGPU_OK;
}

}  // extern "C"

namespace {
// What one step of ssgpu_dict_close builds its domain in and from; it lives until the encoder has read the domain.
struct StepDomain {
  DevBuf lens, src, dheap, dnull, partials, needle_dev, sub_dev;
  int reserve(ssgpu_ctx* c, uint64_t n) {   // for a step over n values (the heap and the constants follow in build_step_domain)
    HIP_TRY(c, lens.ensure((2 * n + 1) * 8));
    HIP_TRY(c, src.ensure(std::max<uint64_t>(n, 1) * 8));
    HIP_TRY(c, dnull.ensure(std::max<uint64_t>(2 * n, 1)));
    HIP_TRY(c, partials.ensure(ssgpu_str_scan_partials(2 * n) * 8));
    return SSGPU_OK;
  }
};
// Step k's domain: the n values of D_(k-1) followed by their images under `step` -- the length pass (string_map_kernels.hip), the scan,
// D_(k-1)'s bytes copied to the front of the domain's heap and the write pass behind them.  Leaves the 2n + 1 scanned offsets in
// dom->lens, the bytes in dom->dheap and 2n zero NULL bytes in dom->dnull (`dom` reserved for n values).  `needle` / `sub`: a STRING_REPLACE step's constants as bytes.
int build_step_domain(ssgpu_ctx* c, hipStream_t s, const DictDevice& in, const ssgpu_string_step& step, const std::string& needle, const std::string& sub, StepDomain* dom) {
  const uint64_t n = in.n;
  const int fn = step.fn;
  DevBuf &lens = dom->lens, &src = dom->src, &dheap = dom->dheap, &dnull = dom->dnull, &partials = dom->partials, &needle_dev = dom->needle_dev, &sub_dev = dom->sub_dev;
  if (fn == OP_STRING_REPLACE) {
    HIP_TRY(c, needle_dev.ensure(std::max<size_t>(needle.size(), 1))); HIP_TRY(c, sub_dev.ensure(std::max<size_t>(sub.size(), 1)));
    if (!needle.empty()) HIP_TRY(c, hipMemcpyAsync(needle_dev.p, needle.data(), needle.size(), hipMemcpyHostToDevice, s));
    if (!sub.empty()) HIP_TRY(c, hipMemcpyAsync(sub_dev.p, sub.data(), sub.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(c, ssgpu_launch_str_replace_len(in.heap.as<const uint8_t>(), in.offs.as<const uint64_t>(), n, needle_dev.as<const uint8_t>(), (uint32_t)needle.size(),
                                            (uint32_t)sub.size(), lens.as<uint64_t>(), s));
  } else {
    HIP_TRY(c, ssgpu_launch_str_map_len(in.heap.as<const uint8_t>(), in.offs.as<const uint64_t>(), n, fn, step.has_len ? 1 : 0, step.pos, step.len,
                                        lens.as<uint64_t>(), src.as<uint64_t>(), s));
  }
  HIP_TRY(c, ssgpu_launch_str_scan(lens.as<uint64_t>(), 2 * n, partials.as<uint64_t>(), s));
  uint64_t ends[2] = {0, 0};             // the domain's heap: D_(k-1)'s bytes end at ends[0], the images at ends[1]
  HIP_TRY(c, hipMemcpyAsync(&ends[0], lens.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(&ends[1], lens.as<uint64_t>() + 2 * n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, dheap.ensure(ends[1] + 8));
  if (ends[0]) HIP_TRY(c, hipMemcpyAsync(dheap.p, in.heap.p, ends[0], hipMemcpyDeviceToDevice, s));
  if (fn == OP_STRING_REPLACE)
    HIP_TRY(c, ssgpu_launch_str_replace_write(in.heap.as<const uint8_t>(), in.offs.as<const uint64_t>(), lens.as<const uint64_t>() + n, n, needle_dev.as<const uint8_t>(),
                                              (uint32_t)needle.size(), sub_dev.as<const uint8_t>(), (uint32_t)sub.size(), dheap.as<uint8_t>(), s));
  else
    HIP_TRY(c, ssgpu_launch_str_map_write(in.heap.as<const uint8_t>(), src.as<const uint64_t>(), lens.as<const uint64_t>() + n, n, fn == OP_TOUPPER ? 1 : fn == OP_TOLOWER ? 2 : 0,
                                          dheap.as<uint8_t>(), s));
  HIP_TRY(c, hipMemsetAsync(dnull.p, 0, std::max<uint64_t>(2 * n, 1), s));
  return SSGPU_OK;
}
}  // namespace

extern "C" {

// The closed dictionary (ssgpu.h): D_k = D_(k-1) U f_k(D_(k-1)), one step after the other on the device.  A step's domain is D_(k-1)'s
// values followed by their images -- one (lengths, heap) pair of 2n rows: the length pass (string_map_kernels.hip), the scan, D_(k-1)'s
// bytes copied to the front of the domain's heap and the write pass behind them -- and goes through the block encoder's chain
// (encode_domain): the sorted distinct values are D_k, packed on the device as the next step's input, the first n codes are the
// step's remap (D_(k-1) code -> D_k code) and the second n its table in D_k codes.  After the last step the compose kernel carries
// every (remap, table) pair through the later remaps into D_final's codes, last step first; what it leaves for step 1 is base's remap.
int ssgpu_dict_close(ssgpu_ctx* c, const ssgpu_dict* base, const ssgpu_string_step* steps, int32_t n_steps, ssgpu_dict** out, int32_t* remap) {
  if (!c) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (c->device < 0) { c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  const uint64_t n0 = base ? (uint64_t)ssgpu_dict_size(base) : 0;
  if (!base || !out || n_steps < 0 || (n_steps > 0 && !steps) || (n0 > 0 && !remap)) { c->err = "ssgpu_dict_close: a dictionary, its steps, and room for the dictionary and the remap"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  for (int32_t k = 0; k < n_steps; ++k) {
    const int fn = steps[k].fn;
    if (!is_string_producer(fn) && fn != OP_TOLOWER) {
      std::string ids;
      for (int id : {OP_LTRIM, OP_RTRIM, OP_TRIM, OP_TOUPPER, OP_TOLOWER, OP_SUBSTRING, OP_STRING_REPLACE}) ids += (ids.empty() ? "" : " / ") + std::to_string(id);
      c->err = "ssgpu_dict_close: step " + std::to_string(k) + " is no string-producing function (" + ids + ")";
      return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
    }
  }
  // STRING_REPLACE: a step's pos / len are the codes of its needle / substitute in `base` -- constants of the plan, so values of D_0 -- and
  // are resolved to bytes once, here; the closed dictionary remembers the step with the two codes in ITS codes (below)
  std::vector<std::pair<std::string, std::string>> replace_bytes((size_t)n_steps);
  for (int32_t k = 0; k < n_steps; ++k) {
    if (steps[k].fn != OP_STRING_REPLACE) continue;
    const char* nb = nullptr; const char* sb = nullptr; int32_t nl = 0, sl = 0;
    if (steps[k].pos < 0 || steps[k].pos >= (int64_t)n0 || steps[k].len < 0 || steps[k].len >= (int64_t)n0 ||
        ssgpu_dict_decode(base, (int32_t)steps[k].pos, &nb, &nl) != SSGPU_OK || ssgpu_dict_decode(base, (int32_t)steps[k].len, &sb, &sl) != SSGPU_OK) {
      c->err = "ssgpu_dict_close: step " + std::to_string(k) + " (STRING_REPLACE): needle code " + std::to_string(steps[k].pos) + " / substitute code " +
               std::to_string(steps[k].len) + " outside the base dictionary of " + std::to_string(n0) + " values";
      return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
    }
    replace_bytes[(size_t)k] = {std::string(nb, (size_t)nl), std::string(sb, (size_t)sl)};
  }
  if (n_steps == 0) return ssgpu_dict_extend(base, nullptr, nullptr, 0, out, remap);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const bool timed = c->debug_timing != 0;   // development: where a step's time goes, on stderr (tools/string_map_bench.py)
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  DictDevice cur[2];
  int rc = dict_upload(c, base, &cur[0]);
  if (rc != SSGPU_OK) return rc;
  std::deque<DevBuf> codes;              // per step: 2 x n_(k-1) codes of D_k
  std::vector<uint64_t> n_in(1, n0);     // n_in[k] = |D_k|
  std::vector<uint64_t> off_h;
  std::vector<char> heap_h;
  for (int32_t k = 0; k < n_steps; ++k) {
    const DictDevice& in = cur[k & 1];
    DictDevice& next = cur[(k + 1) & 1];
    const uint64_t n = in.n;
    if (2 * n > (uint64_t)kMaxStringDomain) { c->err = "ssgpu_dict_close: more than 2^29 values in a step's dictionary"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    codes.emplace_back();
    DevBuf& kc = codes.back();
    HIP_TRY(c, kc.ensure(std::max<uint64_t>(2 * n, 1) * 4));
    StepDomain dom;
    rc = dom.reserve(c, n);
    if (rc != SSGPU_OK) return rc;
    const auto t0 = now();
    const int fn = steps[k].fn;
    rc = build_step_domain(c, s, in, steps[k], replace_bytes[(size_t)k].first, replace_bytes[(size_t)k].second, &dom);
    if (rc != SSGPU_OK) return rc;
    if (timed) HIP_TRY(c, hipStreamSynchronize(s));
    const auto t1 = now();
    uint32_t D = 0;
    rc = encode_domain(c, s, dom.dheap.as<uint8_t>(), dom.lens.as<uint64_t>(), true, dom.dnull.as<uint8_t>(), 2 * n, {{kc.as<int32_t>(), 0, 2 * n}}, STRFN_HEAP_PAD, &off_h, &heap_h, &D,
                       next.offs, next.heap);
    if (rc != SSGPU_OK) return rc;
    if (n == 0) {   // an empty dictionary stays empty: give the next step the packed form of nothing
      HIP_TRY(c, next.offs.ensure(8)); HIP_TRY(c, next.heap.ensure(STRFN_HEAP_PAD));
      HIP_TRY(c, hipMemsetAsync(next.offs.p, 0, 8, s)); HIP_TRY(c, hipMemsetAsync(next.heap.p, 0, STRFN_HEAP_PAD, s));
      HIP_TRY(c, hipStreamSynchronize(s));
    }
    next.n = D;
    n_in.push_back(D);
    if (timed) fprintf(stderr, "[ssgpu dict_close] step %d fn %d values %llu -> %u map_ms %.4f encode_ms %.4f\n", k, fn, (unsigned long long)n, D, ms(t0, t1), ms(t1, now()));
  }
  // compose, last step first: `later` maps D_k's codes to D_final's (nothing for the last step); the step leaves D_(k-1)'s in `to_final`
  const uint64_t n_final = n_in[(size_t)n_steps];
  DevBuf tables, to_final[2];
  HIP_TRY(c, tables.ensure(std::max<uint64_t>(n_final * (uint64_t)n_steps, 1) * 4));
  HIP_TRY(c, hipMemsetAsync(tables.p, 0, std::max<uint64_t>(n_final * (uint64_t)n_steps, 1) * 4, s));
  const auto t2 = now();
  for (int32_t k = n_steps - 1; k >= 0; --k) {
    const uint64_t n = n_in[(size_t)k];
    DevBuf& mine = to_final[k & 1];
    HIP_TRY(c, mine.ensure(std::max<uint64_t>(n, 1) * 4));
    const int32_t* later = k == n_steps - 1 ? nullptr : to_final[(k + 1) & 1].as<int32_t>();
    HIP_TRY(c, ssgpu_launch_str_map_compose(codes[(size_t)k].as<int32_t>(), n, later, n_in[(size_t)k + 1], n_final, mine.as<int32_t>(),
                                            tables.as<int32_t>() + (uint64_t)k * n_final, s));
  }
  std::vector<int32_t> tables_h((size_t)(n_final * (uint64_t)n_steps));
  if (!tables_h.empty()) HIP_TRY(c, hipMemcpyAsync(tables_h.data(), tables.p, tables_h.size() * 4, hipMemcpyDeviceToHost, s));
  if (n0) HIP_TRY(c, hipMemcpyAsync(remap, to_final[0].p, n0 * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (timed) fprintf(stderr, "[ssgpu dict_close] compose_ms %.4f\n", ms(t2, now()));
  // (off_h / heap_h: the last step's distinct values, as the encoder copied them back)
  ssgpu_dict* d = nullptr;
  rc = ssgpu_dict_create_sorted(heap_h.data(), off_h.data(), (int64_t)n_final, &d);
  if (rc != SSGPU_OK) { c->err = "ssgpu_dict_close: too many distinct values"; return rc; }
  // a STRING_REPLACE step is remembered with its two constants as codes of THIS dictionary: the plan created anew over it bakes them so
  std::vector<ssgpu_string_step> kept(steps, steps + n_steps);
  for (ssgpu_string_step& st : kept)
    if (st.fn == OP_STRING_REPLACE) { st.has_len = 0; st.pos = remap[st.pos]; st.len = remap[st.len]; }
  ssgpu_dict_set_steps(d, kept.data(), n_steps, tables_h.data());
  *out = d;
  return SSGPU_OK;
}

}  // extern "C"

// runtime.cpp -- the C ABI (include/ssgpu.h): contexts, blocks, plans, execution.
//
// Execution is push-style and whole-shard: one ssgpu_plan_run drains the whole
// input through the fused pipeline kernel(s) of each stage, where the reference
// would pull 1024-row views through Cursor::Next (cursor/base/cursor.h:131-148).
// There is no CPU data path in this file: without a device every run fails.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <map>
#include <set>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <unistd.h>
#include <thread>
#include <unordered_set>
#include <vector>
#include <deque>
#include <functional>

#include "runtime_internal.h"

using namespace ssgpu;

static bool trace_on() { static const bool on = getenv("SSGPU_TRACE") != nullptr; return on; }   // development: shape decisions and fallbacks on stderr

thread_local MemQuota* g_quota = nullptr;

// process-wide accounting of what the library holds (ssgpu_memory_stats): the per-process measure behind the
// "repeated runs do not grow memory" contract (expression_test_helper.cc:213-245 watches its allocator the same way)
static std::atomic<uint64_t> g_dict_gen{0};   // stamps of ssgpu_plan_set_dict calls (ssgpu_plan::dict_gen)
std::atomic<long long> g_dev_bytes{0}, g_pinned_bytes{0};
static std::atomic<long long> g_live_plans{0}, g_live_blocks{0}, g_events{0};

DevPool g_pool;
size_t DevPool::trim(int dev) {
  std::vector<std::pair<void*, size_t>> out;
  {
    std::lock_guard<std::mutex> lock(m);
    for (auto it = blocks.begin(); it != blocks.end();)
      if (dev < 0 || it->second.second == dev) { out.emplace_back(it->second.first, it->first); bytes -= it->first; it = blocks.erase(it); } else ++it;
  }
  size_t freed = 0;
  for (auto& b : out) { (void)hipFree(b.first); g_dev_bytes.fetch_sub((long long)b.second); freed += b.second; }
  return freed;
}
static std::atomic<int> g_device_contexts{0};          // contexts with a device alive in this process: the last one to go empties the pool
thread_local bool tls_park_released = false;

struct OutCol { DevBuf data, nulls; bool nullable = false; uint32_t width = 8; };   // (views into StageExec::out_arena for large results)

struct StageExec {
  // device copies of the programs, finalised for tile_rows
  DevBuf prog_main, prog_count;
  // A kernel specialised by runtime compilation (rtc.cpp): a reference to a cached module function.  `static_lds` is the
  // LDS size it was compiled for when that exceeds what a module-loaded kernel may ask for dynamically (0 = dynamic).
  struct RtcSlot {
    void* h = nullptr; bool tried = false; uint32_t static_lds = 0, tag = 0;   // tag: what else the kernel was compiled for (partition count, rows per thread)
    // the request mode (rtc.cpp: 0 compile now, 1 caches only, 2 leave it to the worker) the slot came back empty-handed under: a
    // small first run of a specialize = 3 plan asks in mode 1 and misses -- a later LARGE run (mode 2) must ask again, or the plan
    // would stay on the interpreter for its lifetime (round-5 advice)
    int missed_mode = -1;
    bool stronger_mode_now() const { if (h || missed_mode < 0) return false; const int m = ssgpu_rtc_current_mode(); return missed_mode == 1 && m != 1; }
    // the kernel was being compiled when the slot asked (rtc.cpp: background compilation, or another plan's): the slot asks again --
    // not at every launch, the request rebuilds the kernel's key -- until it has it
    bool pending = false; std::chrono::steady_clock::time_point next_poll{};
    void drop() { if (h) ssgpu_rtc_release(h); h = nullptr; tried = false; static_lds = 0; tag = 0; pending = false; missed_mode = -1; }
    bool ask_again() {
      if (!pending) return false;
      const auto now = std::chrono::steady_clock::now();
      if (now < next_poll) return false;
      next_poll = now + std::chrono::milliseconds(20);
      return true;
    }
    void asked() { pending = !h && ssgpu_rtc_pending(); missed_mode = h ? -1 : ssgpu_rtc_current_mode(); if (pending) next_poll = std::chrono::steady_clock::now() + std::chrono::milliseconds(20); }
  };
  RtcSlot rtc_main;             // the main program's specialised kernel, h == NULL: interpreter
  std::vector<VmInstr> host_prog_main;   // the finalised main program (what rtc.cpp compiles)
  std::string rtc_why;          // why not, when specialisation was asked for and did not happen
  ProgramLayout lay{};
  ProgramLayout lay_count{};
  int n_instr_main = 0, n_instr_count = 0;
  int grid = 0;
  // scalar aggregates
  DevBuf wg_partials, slot_recs, slot_kind, emit_descs, state;
  // filter compaction
  DevBuf tile_counts, tile_offsets, total;
  DevBuf xstatus; uint64_t x_epoch = 0;   // group extraction (one launch, decoupled look-back): one status word per 512-slot tile, stamped with the run's epoch
  // group table
  DevBuf gkeys, gacc, gcnt, goverflow, gpattern, gmergeop;
  int group_wgs = 3;            // resident workgroups per CU of the group stage (adapted from run feedback)
  bool group_local = true;      // workgroup-private LDS pre-aggregation table in use
  int group_sub = 1;            // sub-tables of the LDS table (spreads same-group rows of a wave)
  // partitioned execution (many groups)
  bool group_partitioned = false;
  uint32_t part_n = 256;        // hash partitions (doubled when a partition overflows its LDS table)
  bool part_n_chosen = false;
  bool part_slab_failed = false;
  bool scouted = false;         // the scout run of run_group_agg has happened
  int64_t scout_full_rows = 0;
  bool part_slab = false;       // partitioned path without hash partitions: every aggregation workgroup holds all groups (few groups)
  double part_groups_est = 0;   // group count estimated by the direct path's run feedback
  uint32_t part_seg_growth = 1; // x4 whenever a (partition, workgroup) segment ran full
  bool part_failed = false;     // the partitioned shape could not hold this input: stay on the direct path
  DevBuf prog_pscatter, part_hist, part_recs;
  ProgramLayout lay_pscatter{};
  int n_instr_pscatter = 0;
  RtcSlot rtc_pscatter; std::vector<VmInstr> host_prog_pscatter;   // its specialised kernel (rtc.cpp)
  RtcSlot rtc_plain;            // ssgpu_part_scatter_plain_kernel specialised for this stage's record and a partition count (static_lds = its LDS size)
  RtcSlot rtc_part;             // ssgpu_part_agg_kernel specialised for this stage's aggregates and an LDS size (static_lds)
  RtcSlot rtc_resident;         // ssgpu_group_resident_kernel specialised for this stage's row source and aggregates
  RtcSlot rtc_hot;              // the same kernel for the heavy hitters' small table (hot_only)
  uint32_t hot_n = 0; uint64_t hot_keys[SSGPU_HOT_MAX] = {0};   // heavy-hitter keys found when a partition segment overflowed (kept for the plan's later runs)
  int64_t hot_sampled_run = -1; // the run (ssgpu_plan::n_runs) whose overflow last made the host look at a sample: once per run, so that a plan that meets
                                // other data later (other hot keys) finds them again
  DevBuf hot_out;
  // Dense slots (launch.h: DenseKeyMap): a plain stage whose key columns span small value ranges indexes its tables by the keys'
  // mixed-radix number instead of hashing them.  The ranges come from one pass over the key columns (the stage's first large
  // run, or ssgpu_plan_key_ranges) and are kept: a later row outside them raises the domain-miss flag, the ranges are widened
  // to the union and the run is repeated.  `fixed`: the caller set them (a sharded job's ranks must all use the same ones).
  struct DenseState {
    bool on = false, failed = false, checked = false, fixed = false, resident = false;
    uint32_t n_keys = 0, n_chunks = 1;
    uint64_t lo[8] = {0}, hi[8] = {0};   // order-preserving unsigned domain (signed columns: sign bit flipped); lo > hi: no value seen
    uint32_t span[8] = {0}, stride[8] = {0};
    uint64_t slots = 0;                  // product of the spans
    uint32_t np = 0, cap = 0;            // partitions (a multiple of n_chunks), table entries per partition: np * cap >= slots
    uint64_t chunk_bytes = 0;            // header + keys + acc + cnt of (np / n_chunks) * cap + 1 slots, rounded to 64
    int64_t widened = 0;                 // times a run met a key outside the ranges
  } dense;
  DevBuf dense_dom, dense_flags;
  void* dense_table = nullptr;           // ssgpu_plan_run_dense: the caller's table buffer (n_chunks * chunk_bytes) for THIS run
  std::vector<DevBuf> rowid_tmp;   // FIRST / LAST in GroupAggregate: extracted row ids per aggregate
  // hash joins fused into this stage: index (keys, rows, [special, flags]) per join
  std::vector<DevBuf> jkeys, jkeys_hi, jrows, jmisc;
  std::vector<DevBuf> jcounts, jstarts, jslot_of_row, jrows_sorted;   // NOT_UNIQUE joins: key -> run of rhs rows
  DevBuf jx_offsets, jx_lhs_idx, jx_rhs_row;                           // JOIN_EXPAND scratch
  std::vector<VmJoin> vm_joins;
  uint32_t capacity = 0;
  DevBuf error_flag;
  DevBuf debug, debug_pc, total2;
  // sort / clusters
  DevBuf skeys_a, skeys_b, skeys_c, sidx_a, sidx_b, shist, soffs, seg_id, sstatus, sticket, srecs, dflag;
  DevBuf rank_first, rank_of_seg, rank_row, rank_own;   // Stage::has_rank (rank_columns)
  DevBuf seg_counts, seg_offsets, seg_total;   // segment_ids() of a MATERIALIZE stage (its own: the stage's filter passes use tile_counts / total)
  DevBuf route_scratch;         // key-range exchange: per-destination counters + (destination, position) of every result row
  uint64_t sort_epoch = 0;      // one-sweep status words of earlier passes carry an older epoch
  bool emit_ready = false;
  bool emitted_with_finish = false;  // this run's finish launch also emitted the result row
  bool pattern_ready = false;
  // outputs
  DevBuf out_arena;          // large results: ONE allocation, `out` holds views into it (ensure_out_cols)
  std::vector<OutCol> out;
  int64_t out_rows = -1;     // -1: read lazily from `total`
  const void* out_rows_dev = nullptr;   // ... or, when set, from this device word of an EARLIER stage (a filter-less stage fed through a device-side row count)
  int64_t out_capacity = 0;
  // what the last run did (ssgpu_plan_stage_info)
  int last_group_shape = 0;     // 0 direct, 1 hash partitions, 2 slab
  int last_reruns = 0;          // attempts beyond the first (regrown table / segments / partitions)
  int last_sort_passes = 0, last_sort_mode = 0;
  bool last_plain_scatter = false;
  // Run feedback read lazily (steady state of a GroupAggregate that is the plan's last stage): the overflow / feedback
  // words of the run are copied to pinned memory on the stream and looked at when the result is first touched or the
  // plan runs again -- a run that did overflow after all is then repeated, synchronously, from the saved input columns.
  PinnedBuf fb_host;
  int fb_pending = 0;           // 0 none, 1 direct shape, 2 partitioned shape
  hipEvent_t fb_event = nullptr;   // recorded behind the copy of the feedback words (record_feedback)
  int steady = 0;               // consecutive synchronous runs that neither overflowed nor changed the stage's shape
  uint32_t steady_bypass = 0;   // direct shape: rows that bypassed the LDS table in the last synchronous run
};

struct ssgpu_result {
  ssgpu_plan* plan = nullptr;
  std::vector<PinnedBuf> host_data, host_nulls;
  std::vector<bool> fetched;
  std::vector<ssgpu_dict*> concat_dicts;   // per column: the strings of a CONCAT result (codes of that column index it), else NULL
  ~ssgpu_result() { for (ssgpu_dict* d : concat_dicts) if (d) ssgpu_dict_destroy(d); }
};

struct ssgpu_plan {
  ssgpu_ctx* ctx = nullptr;
  MemQuota quota;               // declared before `exec`: outlives the buffers charged to it
  int64_t expr_row_capacity = INT64_MAX;   // BoundExpressionTree::row_capacity() of a bound expression
  PlanDesc desc;
  std::vector<Stage> stages;
  std::vector<StageExec> exec;
  Schema result_schema;
  std::vector<std::string> attr_names;  // stable c_str for ssgpu_plan_attr
  std::vector<ssgpu_column> aux_cols;   // auxiliary input (rhs table of a HASH_JOIN), device pointers
  int64_t aux_rows = -1;
  std::string describe, describe_full;
  std::atomic<int> interrupted{0};
  int64_t n_runs = 0;           // runs started
  bool specialize = false;      // this plan's kernels are specialised by runtime compilation (ctx option at creation, or ssgpu_plan_specialize)
  bool cached_only = false;     // ... but only where the kernel exists already (option specialize = 2 / 3): no run of this plan waits for the compiler
  // BestEffortGroupAggregate (a stage with Stage::fold_cut): the row the last run's table had no room for (-1: every key fitted), the
  // capacity in force (a failed allocation lowers it below the operation's), the input window the next view starts with
  bool best_effort = false; int64_t be_cut = -1, be_capacity = 0, be_window = 0, be_base = 0, be_window_fail = 0;
  uint32_t group_capacity_hint = 0;   // first capacity of a direct-shape group table when the plan knows better than the context's default (best effort under a memory limit)
  bool lazy_feedback = false;   // the context's option at the time the plan was made, or ssgpu_plan_set_option: THIS plan's steady-state runs leave their feedback on the stream
  bool background = false;      // ... and what is missing is left to the worker thread (option 3) when a run of >= background_min_rows rows wants it
  int64_t background_min_rows = 0;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_dom0 = nullptr, ev_dom1 = nullptr;
  // the (dom0, dom1) pairs of the most recent profiled runs: ev_dom0 / ev_dom1 alias the current pair, so
  // a caller can time many asynchronous runs and read every kernel duration afterwards, without a sync in between
  static const int kEventRing = 256;
  hipEvent_t ring0[kEventRing] = {nullptr}, ring1[kEventRing] = {nullptr};
  uint64_t profiled_runs = 0;
  bool events_valid = false;
  ssgpu_counters counters{};
  std::vector<VmInstr> host_prog_scratch;
  bool partial_pending = false;
  int64_t last_rows = 0;
  bool deferred = false;        // some stage's run feedback has not been looked at yet (settle_plan)
  bool nan_seen = false;        // the last run met a NaN in a floating MIN / MAX (check_error_flags)
  const ssgpu_dict* dict = nullptr;   // the plan's STRING dictionary (ssgpu_plan_set_dict): CONCAT prints STRING inputs through it
  // the tables over that dictionary that the plan's programs gather from (string_dict.cpp), rebuilt when dict_gen moves: the stamp of
  // the ssgpu_plan_set_dict call
  uint64_t dict_gen = 0;
  DictTables dict_tables;
  std::vector<ssgpu_column> last_cols; int64_t last_base = 0; bool last_partial = false;   // the last run's input (a deferred overflow repeats it)
  // ssgpu_plan_run_host: two alternating sets of device columns the host rows are staged through, and the chunks' partial states
  std::vector<DevBuf> host_stage_data[2], host_stage_nulls[2];
  DevBuf host_states;
  // ssgpu_plan_stream_*: the same staging sets fed from a pinned pair the pushed rows are copied into (the caller's Views are only valid
  // until its child's next Next)
  struct HostStream {
    bool open = false; int rc = SSGPU_OK;
    int64_t chunk_rows = 0, fill = 0, pushed = 0, chunks = 0; int cur = 0;
    int kind = 1;                 // ssgpu_plan::StreamJob::kind of the open stream (1: ScalarAggregate states)
    std::vector<PinnedBuf> pin_data[2], pin_nulls[2];
    hipEvent_t uploaded[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    bool in_flight[2] = {false, false};
    void drop_events() {
      for (int b = 0; b < 2; ++b) {
        if (uploaded[b]) (void)hipEventDestroy(uploaded[b]);
        if (consumed[b]) (void)hipEventDestroy(consumed[b]);
        uploaded[b] = consumed[b] = nullptr; in_flight[b] = false;
      }
    }
  } host_stream;
  // Chunked execution of plans that are not one ScalarAggregate stage (ssgpu_plan_run_host / ssgpu_plan_stream_*; stream_job_* below):
  // kind 2 = every stage is row-local (Filter / Compute / Project / HashJoin): each chunk runs the plan itself and its result rows are
  // appended; kind 3 = the first blocking operation on the input's path is a GroupAggregate of mergeable aggregates: `head` (the plan up to
  // and including it, DOUBLE sums with their residuals) runs over every chunk, the partial tables are appended, and `tail` -- a
  // GroupAggregate of the merge functions over them, the single-run schema restored, then the operations above -- runs once at the end.
  struct StreamJob {
    int kind = 0;
    ssgpu_plan* head = nullptr; ssgpu_plan* tail = nullptr;     // kind 3: owned; kind 2: head == the plan itself
    std::vector<DevBuf> acc_data, acc_nulls;                    // the appended rows, one buffer per result column of `head`
    int64_t acc_rows = 0, acc_cap = 0;
    int64_t rows_hint = 0;      // ssgpu_plan_run_host, kind 2: the input's row count -- what a row-local plan returns at most; the first allocation
                                // of the accumulation takes it (when a quarter of the free device memory holds it) instead of growing by doubling
  };
  StreamJob* stream_job = nullptr;
  ssgpu_plan* skip_plan = nullptr;   // a bound expression's node-level form (ssgpu_expr_evaluate_skip): the same tree under IF($skip_i, NULL, e_i), made on first use
  int64_t run_row_end = 0;         // row_id_base + rows of the run in progress: one past the largest row id a stage can meet
  bool keep_error_flags = false;   // ... whose runs after the first leave the error words alone: an evaluation error of ANY chunk fails the run
  ssgpu_result result;
};

struct ssgpu_block {
  ssgpu_ctx* ctx = nullptr;
  Schema schema;
  int64_t capacity = 0, rows = 0;
  // Large blocks are ONE allocation: column i's data starts i x (its 2 MiB-rounded size + kBlockColumnSkew) into it, the NULL masks
  // follow.  A pipeline reads the same rows of all its columns at the same time; columns allocated one by one start at bases that are
  // congruent modulo every power of two the allocator aligns to, which puts those reads on the same HBM channels.  Measured on the
  // headline query (8 columns x 800 MB), same box, alternating: one allocation per column 0.786 of 8 TB/s, this layout 0.816 - 0.820
  // (profiles/r06_layout_ab.txt; the single-process skew sweep r06_stagger_sweep.txt is within process-to-process noise).  `data` /
  // `nulls` are views into it.
  DevBuf arena;
  std::vector<DevBuf> data, nulls;
  ssgpu_dict* dict = nullptr;   // the dictionary the STRING columns are codes of, when the block built it (ssgpu_block_dict)
};
static const size_t kBlockColumnSkew = 512, kBlockArenaMin = 32u << 20;

static int fail(ssgpu_ctx* ctx, const Status& s) { if (ctx) ctx->err = s.msg; return s.code; }
// the CONCAT description of result column `col` (Stage::ConcatCol), or NULL
static const Stage::ConcatCol* concat_of(const ssgpu_plan* p, int32_t col) {
  if (p->stages.empty()) return nullptr;
  for (auto& cc : p->stages.back().concat) if (cc.out_col == col) return &cc;
  return nullptr;
}

// every program of a stage, in the order the runtime looks at them
static std::array<const Program*, 3> stage_programs(const Stage& st) { return {&st.main, &st.count_pass, &st.part_scatter}; }
// f(spec) for the tables over the STRING dictionary that the plan's programs gather from (JOIN_GATHER_DICT_TABLE), in program order: once
// per gather, or -- `distinct` -- once per spec
template <typename F> static void for_each_dict_table(const ssgpu_plan* p, bool distinct, F f) {
  std::set<DictTableSpec> seen;
  for (auto& st : p->stages)
    for (const Program* pr : stage_programs(st))
      for (auto& g : pr->gathers)
        if (g.join_id == JOIN_GATHER_DICT_TABLE && (!distinct || seen.insert(g.table).second)) f(g.table);
}

extern "C" {

int ssgpu_abi_version(void) { return SSGPU_ABI_VERSION; }

int ssgpu_ctx_create(int device_id, ssgpu_ctx** out) {
  if (!out) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = new ssgpu_ctx;
  c->device = device_id;
  if (device_id >= 0) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device_id >= n) { delete c; return SSGPU_ERROR_NO_DEVICE; }
    if (hipSetDevice(device_id) != hipSuccess) { delete c; return SSGPU_ERROR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) { delete c; return SSGPU_ERROR_NO_DEVICE; }
    c->cu_count = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return SSGPU_ERROR_HIP; }
    c->own_stream = true;
    g_device_contexts.fetch_add(1);
    (void)ssgpu_pipeline_set_max_lds(160 * 1024);
    (void)ssgpu_part_agg_set_max_lds(160 * 1024);
  }
  // SSGPU_SPECIALIZE (development / test sweeps): the default of the `specialize` option for contexts of this process
  if (const char* e = getenv("SSGPU_SPECIALIZE")) c->specialize = atoi(e);
  if (const char* e = getenv("SSGPU_GROUP_DENSE")) c->group_dense = atoi(e);
  *out = c;
  return SSGPU_OK;
}

static void ctx_release(ssgpu_ctx* c) {
  if (c->refs.fetch_sub(1) != 1) return;
  if (c->device >= 0) {
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->copy_ev) { (void)hipEventDestroy(c->copy_ev); c->copy_ev = nullptr; }
    if (g_device_contexts.fetch_sub(1) == 1) (void)g_pool.trim(-1);   // nobody is left to take a parked block
  }
  delete c;
}
// Gives the device blocks the library keeps between plans (DevPool) back to the driver; device < 0 = every device.
int64_t ssgpu_pool_trim(int32_t device) { return (int64_t)g_pool.trim(device); }
void ssgpu_ctx_destroy(ssgpu_ctx* c) { if (c) ctx_release(c); }

int ssgpu_ctx_has_device(const ssgpu_ctx* c) { return c && c->device >= 0 ? 1 : 0; }
const char* ssgpu_last_error(const ssgpu_ctx* c) { return c ? c->err.c_str() : "null context"; }
void* ssgpu_ctx_stream(ssgpu_ctx* c) { return c ? (void*)c->stream : nullptr; }
void* ssgpu_ctx_copy_stream(ssgpu_ctx* c) { return c ? (void*)c->copy_stream : nullptr; }

int ssgpu_ctx_set_stream(ssgpu_ctx* c, void* s) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  c->stream = (hipStream_t)s; c->own_stream = false;
  return SSGPU_OK;
}

int ssgpu_ctx_synchronize(ssgpu_ctx* c) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
  return SSGPU_OK;
}

int ssgpu_ctx_set_option(ssgpu_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  std::string k(key);
  if (k == "tile_rows") {
    if (value != 0 && (value % VM_TILE_UNIT != 0 || value > 4 * VM_TILE_UNIT)) { c->err = "tile_rows must be 0 or 1, 2, 4 times the workgroup's row-pair count"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    c->opt.tile_rows = (int)value;
  } else if (k == "lds_target_bytes") c->opt.lds_target_bytes = (int)value;
  else if (k == "grid_limit") c->grid_limit = value;
  else if (k == "wgs_per_cu") c->wgs_per_cu = value > 0 ? value : 3;
  else if (k == "tile_map") c->tile_map = value;
  else if (k == "out_arena") c->out_arena = value;
  else if (k == "group_local") c->group_local = value;
  else if (k == "group_partition") c->group_partition = value;
  else if (k == "part_n") c->part_n = value;
  else if (k == "part_wgs_per_cu") c->part_wgs_per_cu = value;
  else if (k == "part_lds_target") c->part_lds_target = value;
  else if (k == "part_agg_lds") c->part_agg_lds = value;
  else if (k == "group_slab") c->group_slab = value;
  else if (k == "group_resident") c->group_resident = value;
  else if (k == "group_dense") c->group_dense = value;
  else if (k == "dense_parts") c->dense_parts = value;
  else if (k == "dense_min_rows") c->dense_min_rows = value;
  else if (k == "group_scout") c->group_scout = value;
  else if (k == "group_scout_rows") c->group_scout_rows = value;
  else if (k == "part_plain") c->part_plain = value;
  else if (k == "pscat_threads") c->pscat_threads = value;
  else if (k == "pscat_rows") c->pscat_rows = value;
  else if (k == "pscat_wgs") c->pscat_wgs = value;
  else if (k == "pscat_pipe") c->pscat_pipe = value;
  else if (k == "fuse_emit") c->fuse_emit = value;
  else if (k == "part_prefetch") c->part_prefetch = value;
  else if (k == "lazy_feedback") c->lazy_feedback = value;
  else if (k == "async_handoff") c->async_handoff = value;
  else if (k == "sort_records") c->sort_records = value;
  else if (k == "sort_hybrid") c->sort_hybrid = value;
  else if (k == "sort_hi_digits") c->sort_hi_digits = value;
  else if (k == "sort_compact") c->sort_compact = value;
  else if (k == "group_capacity") {
    int64_t cap = 1; while (cap < value) cap <<= 1;
    c->group_capacity = cap;
  } else if (k == "profile") c->profile = value;
  else if (k == "profile_total") c->profile_total = value;
  else if (k == "debug_timing") c->debug_timing = value;
  else if (k == "specialize") c->specialize = value;
  else if (k == "specialize_min_rows") c->specialize_min_rows = value < 0 ? 0 : value;
  else { c->err = "unknown option " + k; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  return SSGPU_OK;
}

int ssgpu_host_alloc(ssgpu_ctx* c, size_t bytes, void** out) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  HIP_TRY(c, hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault));
  return SSGPU_OK;
}
void ssgpu_host_free(ssgpu_ctx* c, void* p) { (void)c; if (p) (void)hipHostFree(p); }

// ---- blocks ---------------------------------------------------------------------
int ssgpu_block_create(ssgpu_ctx* c, const ssgpu_attr* schema, int32_t n, int64_t cap, ssgpu_block** out) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  ssgpu_block* b = new ssgpu_block;
  b->ctx = c; b->capacity = cap; b->rows = 0;
  b->data.resize(n); b->nulls.resize(n);
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    Attr a; a.name = schema[i].name ? schema[i].name : ""; a.dtype = schema[i].dtype; a.nullable = schema[i].nullable != 0;
    int w = dtype_width(a.dtype);
    if (w == 0) { delete b; c->err = "variable-length columns are outside the device hot path"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    b->schema.push_back(a);
    total += (size_t)cap * w + (a.nullable ? (size_t)cap : 0);
  }
  // rows << log2(size) bytes per column + rows bytes of null mask (block.cc:20-36)
  if (total >= kBlockArenaMin) {
    auto pitch = [](size_t bytes) { return ((bytes + (2u << 20) - 1) / (2u << 20)) * (2u << 20) + kBlockColumnSkew; };
    size_t need = 0;
    for (int i = 0; i < n; ++i) need += pitch((size_t)cap * dtype_width(b->schema[i].dtype)) + (b->schema[i].nullable ? pitch((size_t)cap) : 0);
    if (b->arena.ensure(need) != hipSuccess) { delete b; c->err = "device allocation failed"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
    size_t off = 0;
    for (int i = 0; i < n; ++i) { const size_t bytes = (size_t)cap * dtype_width(b->schema[i].dtype); b->data[i].set_view(b->arena.as<char>() + off, bytes); off += pitch(bytes); }
    for (int i = 0; i < n; ++i) if (b->schema[i].nullable) { b->nulls[i].set_view(b->arena.as<char>() + off, (size_t)cap); off += pitch((size_t)cap); }
  } else {
    for (int i = 0; i < n; ++i) {
      if (b->data[i].ensure((size_t)cap * dtype_width(b->schema[i].dtype)) != hipSuccess) { delete b; c->err = "device allocation failed"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
      if (b->schema[i].nullable && b->nulls[i].ensure((size_t)cap) != hipSuccess) { delete b; c->err = "device allocation failed"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
    }
  }
  c->refs.fetch_add(1);
  g_live_blocks.fetch_add(1);
  *out = b;
  return SSGPU_OK;
}
void ssgpu_block_destroy(ssgpu_block* b) { if (!b) return; ssgpu_ctx* c = b->ctx; ssgpu_dict_destroy(b->dict); delete b; g_live_blocks.fetch_sub(1); if (c) ctx_release(c); }

// ---- View file format: cursor/infrastructure/file_io.cc ---------------------------------------
static const int64_t kFileChunkRows = 8192;   // kMaxChunkRowCount, file_io.cc:70

// `bytes` at the FILE's current position into `dst`, advancing the position.  One thread copies out of the
// page cache at ~5 GB/s; four positional readers on quarter slabs keep the PCIe copy stream busier.
static bool read_slab(FILE* f, char* dst, size_t bytes) {
  const long pos = ftell(f);
  const int fd = fileno(f);
  const int kReaders = bytes >= (8u << 20) ? 4 : 1;
  const size_t part = (bytes + kReaders - 1) / kReaders;
  std::atomic<bool> ok{true};
  auto read_part = [&](int i) {
    size_t lo = (size_t)i * part, hi = std::min(bytes, lo + part);
    while (lo < hi) {
      const ssize_t got = pread(fd, dst + lo, hi - lo, (off_t)(pos + (long)lo));
      if (got <= 0) { ok = false; return; }
      lo += (size_t)got;
    }
  };
  std::vector<std::thread> readers;
  for (int i = 1; i < kReaders; ++i) readers.emplace_back(read_part, i);
  read_part(0);
  for (auto& t : readers) t.join();
  return ok && fseek(f, pos + (long)bytes, SEEK_SET) == 0;
}

// ---- STRING columns: one dictionary over every STRING column of a block (string_dict_kernels.hip) ------------------------
// The domain is the block's STRING columns end to end (column k's row r is domain row k x rows + r).  `lens` holds domain + 1
// words: the byte lengths, scanned here into offsets into `heap`; `dnull` one NULL byte per domain row.  Runs on the copy
// stream, writes the codes into the block's STRING columns and gives the block its dictionary.
static int encode_string_domain(ssgpu_ctx* c, ssgpu_block* b, const std::vector<int>& scols, DevBuf& heap, DevBuf& lens, DevBuf& dnull) {
  const uint64_t rows = (uint64_t)b->rows, n = rows * scols.size();
  std::vector<uint64_t> off_h;
  std::vector<char> heap_h;
  uint32_t D = 0;
  std::vector<DomainCodes> targets;
  for (size_t k = 0; k < scols.size(); ++k) targets.push_back({b->data[scols[k]].as<int32_t>(), k * rows, rows});
  DevBuf out_off, out_heap;
  const int erc = encode_domain(c, c->copy_stream, heap.as<uint8_t>(), lens.as<uint64_t>(), false, dnull.as<uint8_t>(), n, targets, 0, &off_h, &heap_h, &D, out_off, out_heap);
  if (erc != SSGPU_OK) return erc;
  ssgpu_dict* d = nullptr;
  const int rc = ssgpu_dict_create_sorted(heap_h.data(), off_h.data(), (int64_t)D, &d);
  if (rc != SSGPU_OK) { c->err = "STRING dictionary: too many distinct values"; return rc; }
  ssgpu_dict_destroy(b->dict);
  b->dict = d;
  return SSGPU_OK;
}

int ssgpu_block_create_from_file(ssgpu_ctx* c, const ssgpu_attr* schema, int32_t n, const char* path, ssgpu_block** out) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  FILE* f = path ? fopen(path, "rb") : nullptr;
  if (!f) { c->err = std::string("cannot open ") + (path ? path : "(null)"); return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  std::vector<int> width(n); std::vector<bool> nullable(n), is_str(n);
  std::vector<int> scols;            // STRING columns, in schema order: the dictionary's domain
  for (int i = 0; i < n; ++i) {
    width[i] = dtype_width(schema[i].dtype); nullable[i] = schema[i].nullable != 0; is_str[i] = schema[i].dtype == SSGPU_STRING;
    if (width[i] == 0) { fclose(f); c->err = "variable-length columns of the file format are outside the device hot path"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    if (is_str[i]) scols.push_back(i);
  }
  const size_t ns = scols.size();
  fseek(f, 0, SEEK_END);
  const int64_t fsize = (int64_t)ftell(f);
  rewind(f);
  // pass 1: chunk headers (the payload size follows from the row count and the schema) and, for STRING columns, their lengths
  int64_t total = 0, pos = 0; uint64_t rc = 0;
  std::vector<uint64_t> chunk_rows, chunk_bytes, chunk_sbytes;   // chunk_sbytes: ns words per chunk, the bytes of each STRING column's values
  std::vector<uint64_t> col_bytes(ns, 0), lens;
  bool header_ok = true, body_ok = true; const char* header_why = "";
  while (fread(&rc, 8, 1, f) == 1) {
    // a chunk never holds more than kMaxChunkRowCount rows (file_io.cc:70): anything else is a corrupt header, and
    // trusting it would seek by a garbage (possibly negative) distance
    if (rc == 0 || rc > (uint64_t)kFileChunkRows) { header_ok = false; header_why = rc == 0 ? " Chunk of size 0." : " Input chunk too large."; break; }   // file_io.cc:398-409
    const int64_t start_pos = pos;
    pos += 8;
    for (int i = 0, k = 0; i < n && body_ok; ++i) {
      if (nullable[i]) pos += (int64_t)rc;
      if (!is_str[i]) { pos += (int64_t)rc * width[i]; continue; }
      // ReadVariableLengthData (file_io.cc:442-474): rc uint64 lengths, then their sum of bytes -- which must lie inside the file
      lens.resize(rc);
      body_ok = pos + (int64_t)rc * 8 <= fsize && fseek(f, (long)pos, SEEK_SET) == 0 && fread(lens.data(), 8, rc, f) == rc;
      pos += (int64_t)rc * 8;
      uint64_t sum = 0;
      for (uint64_t j = 0; j < rc && body_ok; ++j) { body_ok = lens[j] <= (uint64_t)(fsize - pos) - sum; sum += lens[j]; }
      pos += (int64_t)sum;
      chunk_sbytes.push_back(sum); col_bytes[k++] += sum;
    }
    if (!body_ok || pos > fsize || fseek(f, (long)pos, SEEK_SET) != 0) { body_ok = false; break; }
    total += (int64_t)rc; chunk_rows.push_back(rc); chunk_bytes.push_back((uint64_t)(pos - start_pos));
  }
  if (!header_ok) { fclose(f); c->err = std::string("Reading cursor's data from the input file failed.") + header_why; return SSGPU_ERROR_GENERAL_IO_ERROR; }
  if (!body_ok) { fclose(f); c->err = "Reading cursor's data from the input file failed."; return SSGPU_ERROR_GENERAL_IO_ERROR; }
  if (total * (int64_t)ns > kMaxStringDomain) { fclose(f); c->err = "more than 2^30 STRING cells in one block"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  rewind(f);
  ssgpu_block* b = nullptr;
  int rcode = ssgpu_block_create(c, schema, n, std::max<int64_t>(total, 1), &b);
  if (rcode != SSGPU_OK) { fclose(f); return rcode; }
  // the STRING domain: lengths (column after column), one heap of bytes, one NULL byte per cell
  DevBuf dlens, dheap, dnull;
  std::vector<uint64_t> col_base(ns, 0), col_fill(ns, 0);
  uint64_t heap_bytes = 0;
  for (size_t k = 0; k < ns; ++k) { col_base[k] = heap_bytes; heap_bytes += col_bytes[k]; }
  bool ok = true;
  if (ns) ok = dlens.ensure(((size_t)total * ns + 1) * 8) == hipSuccess && dheap.ensure(heap_bytes + 8) == hipSuccess &&
               dnull.ensure(std::max<size_t>((size_t)total * ns, 1)) == hipSuccess;
  if (!ok) { fclose(f); ssgpu_block_destroy(b); c->err = "Memory exceeded: the STRING columns' lengths and bytes"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  // pass 2: two pinned slabs of whole chunks (headers included, >= 32 MiB or one chunk).  A slab crosses PCIe
  // as ONE copy into a device slab and a kernel scatters its column pieces (the format interleaves a few KiB
  // per column per chunk: tens of thousands of small copies per GB otherwise); slab k+1 is read from the file
  // while slab k is copied and unpacked on the copy stream.
  size_t slab_bytes = 32u << 20, max_pieces = 1;
  for (uint64_t cb : chunk_bytes) slab_bytes = std::max(slab_bytes, (size_t)cb);
  PinnedBuf stage[2], table[2]; DevBuf dslab[2], dtable[2]; hipEvent_t done[2] = {nullptr, nullptr};
  int64_t off = 0; int k = 0;
  { size_t run = 0, cnt = 0;   // most chunks that can share a slab
    for (uint64_t cb : chunk_bytes) { if (run + cb > slab_bytes) { max_pieces = std::max(max_pieces, cnt); run = 0; cnt = 0; } run += cb; ++cnt; }
    max_pieces = std::max(max_pieces, cnt) * (size_t)(3 * n); }
  for (int i = 0; i < 2 && ok; ++i)
    ok = stage[i].ensure(slab_bytes) == hipSuccess && table[i].ensure(max_pieces * sizeof(UnpackPiece)) == hipSuccess &&
         dslab[i].ensure(slab_bytes) == hipSuccess && dtable[i].ensure(max_pieces * sizeof(UnpackPiece)) == hipSuccess &&
         hipEventCreateWithFlags(&done[i], hipEventDisableTiming) == hipSuccess;
  for (size_t ci = 0; ok && ci < chunk_rows.size();) {
    size_t take = 0, bytes = 0;
    while (ci + take < chunk_rows.size() && bytes + chunk_bytes[ci + take] <= slab_bytes) { bytes += chunk_bytes[ci + take]; ++take; }
    if (hipEventSynchronize(done[k]) != hipSuccess) { ok = false; break; }   // slab k (host and device) free again
    char* base = reinterpret_cast<char*>(stage[k].p);
    if (!read_slab(f, base, bytes)) { ok = false; break; }
    UnpackPiece* pieces = reinterpret_cast<UnpackPiece*>(table[k].p);
    unsigned int np = 0;
    const char* p = base;
    for (size_t j = 0; j < take && ok; ++j) {
      uint64_t rows_here; memcpy(&rows_here, p, 8); p += 8;
      if (rows_here != chunk_rows[ci + j]) { ok = false; break; }
      for (int i = 0, sk = 0; i < n && ok; ++i) {
        if (nullable[i]) { pieces[np++] = {(unsigned long long)(p - base), (char*)b->nulls[i].p + off, rows_here}; p += rows_here; }
        if (!is_str[i]) {
          pieces[np++] = {(unsigned long long)(p - base), (char*)b->data[i].p + off * width[i], rows_here * (uint64_t)width[i]};
          p += (size_t)rows_here * width[i];
          continue;
        }
        // (the file is read twice: the lengths must still add up to what pass 1 sized the heap for)
        const uint64_t sbytes = chunk_sbytes[(ci + j) * ns + sk];
        uint64_t sum = 0, len;
        for (uint64_t r = 0; r < rows_here; ++r) { memcpy(&len, p + r * 8, 8); sum += len; }
        if (sum != sbytes) { ok = false; break; }
        pieces[np++] = {(unsigned long long)(p - base), (char*)dlens.p + ((uint64_t)sk * total + off) * 8, rows_here * 8};
        p += (size_t)rows_here * 8;
        pieces[np++] = {(unsigned long long)(p - base), (char*)dheap.p + col_base[sk] + col_fill[sk], sbytes};
        p += sbytes; col_fill[sk] += sbytes; ++sk;
      }
      off += (int64_t)rows_here;
    }
    if (ok) ok = hipMemcpyAsync(dslab[k].p, base, bytes, hipMemcpyHostToDevice, c->copy_stream) == hipSuccess &&
                 hipMemcpyAsync(dtable[k].p, pieces, np * sizeof(UnpackPiece), hipMemcpyHostToDevice, c->copy_stream) == hipSuccess &&
                 ssgpu_launch_unpack(dslab[k].as<char>(), dtable[k].as<UnpackPiece>(), np, c->copy_stream) == hipSuccess &&
                 hipEventRecord(done[k], c->copy_stream) == hipSuccess;
    ci += take; k ^= 1;
  }
  fclose(f);
  // every STRING cell's NULL byte, in domain order (a NOT_NULLABLE column has none)
  for (size_t sk = 0; ok && sk < ns; ++sk) {
    char* dst = (char*)dnull.p + sk * (size_t)total;
    ok = (nullable[scols[sk]] ? hipMemcpyAsync(dst, b->nulls[scols[sk]].p, (size_t)total, hipMemcpyDeviceToDevice, c->copy_stream)
                              : hipMemsetAsync(dst, 0, (size_t)total, c->copy_stream)) == hipSuccess;
  }
  if (ok) ok = hipStreamSynchronize(c->copy_stream) == hipSuccess;
  for (int i = 0; i < 2; ++i) if (done[i]) (void)hipEventDestroy(done[i]);
  if (!ok || off != total) { ssgpu_block_destroy(b); c->err = "Reading cursor's data from the input file failed."; return SSGPU_ERROR_GENERAL_IO_ERROR; }
  b->rows = total;
  if (ns) {
    const int erc = encode_string_domain(c, b, scols, dheap, dlens, dnull);
    if (erc != SSGPU_OK) { ssgpu_block_destroy(b); return erc; }
  }
  *out = b;
  return SSGPU_OK;
}

int ssgpu_block_create_from_host(ssgpu_ctx* c, const ssgpu_attr* schema, int32_t n, const ssgpu_host_column* cols, int64_t rows, ssgpu_block** out) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  if (!schema || !out || n < 0 || rows < 0 || (n > 0 && !cols)) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  std::vector<int> scols;
  for (int i = 0; i < n; ++i) {
    if (dtype_width(schema[i].dtype) == 0) { c->err = "variable-length columns other than STRING are outside the device hot path"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    if (schema[i].dtype != SSGPU_STRING) {
      if (rows && !cols[i].data) { c->err = "column without data"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
      continue;
    }
    const int64_t* o = cols[i].offsets;
    if (!o) { c->err = "a STRING column needs offsets[rows + 1]"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    if (o[0] < 0) { c->err = "STRING offsets must not be negative"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    for (int64_t r = 0; r < rows; ++r) if (o[r + 1] < o[r]) { c->err = "STRING offsets must not decrease"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    if (o[rows] > o[0] && !cols[i].data) { c->err = "column without data"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    scols.push_back(i);
  }
  const size_t ns = scols.size();
  if (rows * (int64_t)ns > kMaxStringDomain) { c->err = "more than 2^30 STRING cells in one block"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  ssgpu_block* b = nullptr;
  int rcode = ssgpu_block_create(c, schema, n, std::max<int64_t>(rows, 1), &b);
  if (rcode != SSGPU_OK) return rcode;
  hipStream_t s = c->copy_stream;
  uint64_t heap_bytes = 0;
  for (int i : scols) heap_bytes += (uint64_t)(cols[i].offsets[rows] - cols[i].offsets[0]);
  DevBuf dlens, dheap, dnull;
  std::vector<uint64_t> lens(ns ? (size_t)rows * ns + 1 : 0, 0);
  bool ok = !ns || (dlens.ensure(lens.size() * 8) == hipSuccess && dheap.ensure(heap_bytes + 8) == hipSuccess &&
                    dnull.ensure(std::max<size_t>((size_t)rows * ns, 1)) == hipSuccess);
  if (!ok) { ssgpu_block_destroy(b); c->err = "Memory exceeded: the STRING columns' lengths and bytes"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  uint64_t heap_off = 0;
  for (int i = 0, sk = 0; i < n && ok && rows; ++i) {
    if (schema[i].nullable) ok = (cols[i].is_null ? hipMemcpyAsync(b->nulls[i].p, cols[i].is_null, (size_t)rows, hipMemcpyHostToDevice, s)
                                                  : hipMemsetAsync(b->nulls[i].p, 0, (size_t)rows, s)) == hipSuccess;
    if (!ok) break;
    if (schema[i].dtype != SSGPU_STRING) {
      ok = hipMemcpyAsync(b->data[i].p, cols[i].data, (size_t)rows * dtype_width(schema[i].dtype), hipMemcpyHostToDevice, s) == hipSuccess;
      continue;
    }
    const int64_t* o = cols[i].offsets;
    for (int64_t r = 0; r < rows; ++r) lens[(size_t)sk * rows + r] = (uint64_t)(o[r + 1] - o[r]);
    const uint64_t nb = (uint64_t)(o[rows] - o[0]);
    char* nd = (char*)dnull.p + (size_t)sk * rows;
    if (nb) ok = hipMemcpyAsync((char*)dheap.p + heap_off, (const char*)cols[i].data + o[0], nb, hipMemcpyHostToDevice, s) == hipSuccess;
    // (a NOT_NULLABLE column's is_null, if given, is ignored, as the block keeps no mask for it)
    if (ok) ok = (schema[i].nullable && cols[i].is_null ? hipMemcpyAsync(nd, cols[i].is_null, (size_t)rows, hipMemcpyHostToDevice, s)
                                                        : hipMemsetAsync(nd, 0, (size_t)rows, s)) == hipSuccess;
    heap_off += nb; ++sk;
  }
  if (ok && ns && rows) ok = hipMemcpyAsync(dlens.p, lens.data(), lens.size() * 8, hipMemcpyHostToDevice, s) == hipSuccess;
  if (ok) ok = hipStreamSynchronize(s) == hipSuccess;
  if (!ok) { ssgpu_block_destroy(b); c->err = "copying the host columns to the device failed"; return SSGPU_ERROR_HIP; }
  b->rows = rows;
  if (ns) {
    const int erc = encode_string_domain(c, b, scols, dheap, dlens, dnull);
    if (erc != SSGPU_OK) { ssgpu_block_destroy(b); return erc; }
  }
  *out = b;
  return SSGPU_OK;
}

const ssgpu_dict* ssgpu_block_dict(const ssgpu_block* b) { return b ? b->dict : nullptr; }

int ssgpu_codes_recode(ssgpu_ctx* c, const int32_t* src, const uint8_t* is_null, int64_t rows, const int32_t* remap, int32_t n_remap, int32_t* dst) {
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  if (rows < 0 || n_remap < 0 || (rows > 0 && (!src || !dst)) || (n_remap > 0 && !remap)) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (!rows) return SSGPU_OK;
  DevBuf dremap;
  HIP_TRY(c, dremap.ensure(std::max<size_t>((size_t)n_remap * 4, 4)));
  if (c->copy_pending.load(std::memory_order_acquire)) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));   // (block uploads before it)
  if (n_remap) HIP_TRY(c, hipMemcpyAsync(dremap.p, remap, (size_t)n_remap * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, ssgpu_launch_str_recode(src, is_null, dremap.as<int32_t>(), n_remap, (uint64_t)rows, dst, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the remap table goes when this returns)
  return SSGPU_OK;
}
// `dict` (a block's, ssgpu_block_dict): its STRING columns leave in the variable-length layout instead of as codes
static int write_view_file(ssgpu_ctx* c, const char* path, int n, int64_t rows, const std::vector<const void*>& dev_data,
                           const std::vector<const uint8_t*>& dev_nulls, const std::vector<int>& width, const std::vector<bool>& nullable,
                           const ssgpu_dict* dict = nullptr, const std::vector<bool>& is_str = std::vector<bool>()) {
  FILE* f = path ? fopen(path, "wb") : nullptr;
  if (!f) { c->err = "Writing view to the output file failed."; return SSGPU_ERROR_GENERAL_IO_ERROR; }
  std::vector<char> host;
  std::vector<int32_t> codes; std::vector<uint64_t> lens; std::string run;
  bool ok = true;
  for (int64_t off = 0; off < rows && ok; off += kFileChunkRows) {
    const uint64_t rc = (uint64_t)std::min<int64_t>(kFileChunkRows, rows - off);
    ok = fwrite(&rc, 8, 1, f) == 1;
    for (int i = 0; i < n && ok; ++i) {
      if (nullable[i]) {
        host.assign((size_t)rc, 0);
        if (dev_nulls[i]) ok = hipMemcpy(host.data(), dev_nulls[i] + off, (size_t)rc, hipMemcpyDeviceToHost) == hipSuccess;
        ok = ok && fwrite(host.data(), 1, (size_t)rc, f) == (size_t)rc;
      }
      if (dict && is_str[i]) {
        // WriteVariableLengthData (file_io.cc:122-147): a uint64 length per row, 0 for NULL and empty, then the bytes in one run
        codes.resize((size_t)rc);
        ok = ok && hipMemcpy(codes.data(), reinterpret_cast<const char*>(dev_data[i]) + off * 4, (size_t)rc * 4, hipMemcpyDeviceToHost) == hipSuccess;
        lens.assign((size_t)rc, 0); run.clear();
        for (uint64_t r = 0; r < rc && ok; ++r) {
          if (nullable[i] && host[r]) continue;
          const char* v; int32_t len;
          ok = ssgpu_dict_decode(dict, codes[r], &v, &len) == SSGPU_OK;
          if (ok) { lens[r] = (uint64_t)len; run.append(v, (size_t)len); }
        }
        ok = ok && fwrite(lens.data(), 8, (size_t)rc, f) == (size_t)rc && fwrite(run.data(), 1, run.size(), f) == run.size();
        continue;
      }
      host.resize((size_t)rc * width[i]);
      ok = ok && hipMemcpy(host.data(), reinterpret_cast<const char*>(dev_data[i]) + off * width[i], host.size(), hipMemcpyDeviceToHost) == hipSuccess;
      ok = ok && fwrite(host.data(), 1, host.size(), f) == host.size();
    }
  }
  ok = fclose(f) == 0 && ok;
  if (!ok) { c->err = "Writing view to the output file failed."; return SSGPU_ERROR_GENERAL_IO_ERROR; }
  return SSGPU_OK;
}

int ssgpu_block_write_file(ssgpu_block* b, const char* path) {
  if (!b) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = b->ctx;
  HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
  const int n = (int)b->schema.size();
  std::vector<const void*> d(n); std::vector<const uint8_t*> z(n); std::vector<int> w(n); std::vector<bool> nl(n);
  std::vector<bool> st(n);
  for (int i = 0; i < n; ++i) { d[i] = b->data[i].p; z[i] = b->schema[i].nullable ? b->nulls[i].as<uint8_t>() : nullptr; w[i] = dtype_width(b->schema[i].dtype); nl[i] = b->schema[i].nullable; st[i] = b->schema[i].dtype == SSGPU_STRING; }
  return write_view_file(c, path, n, b->rows, d, z, w, nl, b->dict, st);
}

int ssgpu_block_upload(ssgpu_block* b, int32_t col, const void* hd, const uint8_t* hn, int64_t off, int64_t rows) {
  if (!b) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = b->ctx;
  if (col < 0 || col >= (int)b->schema.size() || off < 0 || off + rows > b->capacity) { c->err = "upload out of range"; return SSGPU_ERROR_TOO_MANY_ROWS; }
  const int w = dtype_width(b->schema[col].dtype);
  HIP_TRY(c, hipMemcpyAsync((char*)b->data[col].p + off * w, hd, (size_t)rows * w, hipMemcpyHostToDevice, c->copy_stream));
  if (b->schema[col].nullable) {
    if (hn) HIP_TRY(c, hipMemcpyAsync((char*)b->nulls[col].p + off, hn, (size_t)rows, hipMemcpyHostToDevice, c->copy_stream));
    else HIP_TRY(c, hipMemsetAsync((char*)b->nulls[col].p + off, 0, (size_t)rows, c->copy_stream));
  }
  if (off + rows > b->rows) b->rows = off + rows;
  c->copy_pending.store(true, std::memory_order_release);
  return SSGPU_OK;
}
int ssgpu_block_set_row_count(ssgpu_block* b, int64_t rows) {
  if (!b || rows < 0 || rows > b->capacity) return SSGPU_ERROR_TOO_MANY_ROWS;
  b->rows = rows; return SSGPU_OK;
}
int64_t ssgpu_block_row_count(const ssgpu_block* b) { return b ? b->rows : 0; }
int ssgpu_block_column(const ssgpu_block* b, int32_t col, ssgpu_column* out) {
  if (!b || col < 0 || col >= (int)b->schema.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  out->data = b->data[col].p;
  out->is_null = b->schema[col].nullable ? (const uint8_t*)b->nulls[col].p : nullptr;
  return SSGPU_OK;
}

// ---- plans ------------------------------------------------------------------------
// finishes a plan whose description is already in p->desc (ssgpu_plan_create; the head / tail plans of chunked execution)
static int plan_finish_create(ssgpu_ctx* c, ssgpu_plan* p, Status s, ssgpu_plan** out);
int ssgpu_plan_create(ssgpu_ctx* c, const ssgpu_plan_desc* d, ssgpu_plan** out) {
  if (!c || !d || !out) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_plan* p = new ssgpu_plan;
  p->ctx = c;
  return plan_finish_create(c, p, copy_plan_desc(d, &p->desc), out);
}
static int plan_finish_create(ssgpu_ctx* c, ssgpu_plan* p, Status s, ssgpu_plan** out) {
  p->ctx = c;
  if (s.ok()) s = lower_plan(p->desc, &p->stages, &p->result_schema, &p->describe);
  if (!s.ok()) { delete p; return fail(c, s); }
  for (auto& st : p->stages) {
    // every program must fit the CU's LDS at the smallest tile
    LowerOptions o = c->opt; o.tile_rows = VM_TILE_UNIT;
    if (!st.main.empty() && layout_program(st.main, o).lds_bytes > 160u * 1024u) {
      delete p; c->err = "expression needs more than 160 KiB of LDS per tile"; return SSGPU_ERROR_NOT_IMPLEMENTED;
    }
    // ... and the columns (and NULL masks) a program stages must fit the kernel's argument block.  (Until round 6 nothing looked: a Compute
    // over 26 NULLABLE columns -- 52 staged arrays against 48 slots -- wrote past VmParams::staged and returned wrong first / last columns.)
    for (const Program* pr : {&st.main, &st.count_pass, &st.part_scatter})
      if (pr->staged.size() > (size_t)VM_MAX_STAGED) {
        delete p; c->err = "a pipeline reads more than " + std::to_string(VM_MAX_STAGED) + " input arrays (columns + NULL masks)"; return SSGPU_ERROR_NOT_IMPLEMENTED;
      }
  }
  p->exec.resize(p->stages.size());
  for (auto& st : p->stages) if (st.kind == STAGE_FOLD_TAIL && st.fold_cut) { p->best_effort = true; p->be_capacity = st.fold_limit > 0 ? st.fold_limit : INT64_MAX; }
  for (auto& a : p->result_schema) p->attr_names.push_back(a.name);
  p->result.plan = p;
  p->specialize = c->specialize > 0;
  p->lazy_feedback = c->lazy_feedback != 0;
  p->cached_only = c->specialize == 2 || c->specialize == 3;
  p->background = c->specialize == 3; p->background_min_rows = c->specialize_min_rows;
  if (c->device >= 0) {
    (void)hipEventCreate(&p->ev_begin); (void)hipEventCreate(&p->ev_end); g_events.fetch_add(2);
  }
  c->refs.fetch_add(1);
  g_live_plans.fetch_add(1);
  *out = p;
  return SSGPU_OK;
}

// Options of ONE plan (ABI 9).  "lazy_feedback": what the context option of that name gives every plan created under it, for this
// plan only -- the sharded drivers opt their own plans in without changing the contract of other plans on a shared context.
int ssgpu_plan_set_option(ssgpu_plan* p, const char* key, int64_t value) {
  if (!p || !key) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  const std::string k = key;
  if (k == "lazy_feedback") { p->lazy_feedback = value != 0; return SSGPU_OK; }
  if (p->ctx) p->ctx->err = "unknown plan option '" + k + "'";
  return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
}

void ssgpu_plan_destroy(ssgpu_plan* p) {
  if (!p) return;
  if (p->skip_plan) { ssgpu_plan* q = p->skip_plan; p->skip_plan = nullptr; ssgpu_plan_destroy(q); }
  if (p->stream_job) {
    ssgpu_plan::StreamJob* j = p->stream_job; p->stream_job = nullptr;
    if (p->ctx && p->ctx->device >= 0) (void)hipStreamSynchronize(p->ctx->stream);
    if (j->tail) ssgpu_plan_destroy(j->tail);
    if (j->head && j->head != p) ssgpu_plan_destroy(j->head);
    delete j;
  }
  if (p->ctx && p->ctx->device >= 0) {
    (void)hipStreamSynchronize(p->ctx->stream);
    if (p->host_stream.open) { (void)hipStreamSynchronize(p->ctx->copy_stream); p->host_stream.drop_events(); p->host_stream.open = false; }   // (a stream nobody finished)
    if (p->ev_begin) { (void)hipEventDestroy(p->ev_begin); g_events.fetch_sub(1); }
    if (p->ev_end) { (void)hipEventDestroy(p->ev_end); g_events.fetch_sub(1); }
    for (int i = 0; i < ssgpu_plan::kEventRing; ++i) {
      if (p->ring0[i]) { (void)hipEventDestroy(p->ring0[i]); g_events.fetch_sub(1); }
      if (p->ring1[i]) { (void)hipEventDestroy(p->ring1[i]); g_events.fetch_sub(1); }
    }
  }
  // the stream is drained: no launch of this plan's specialised kernels is in flight -- drop the references (the
  // module of a kernel no other plan uses is unloaded, rtc.cpp)
  for (auto& ex : p->exec) { ex.rtc_main.drop(); ex.rtc_pscatter.drop(); ex.rtc_plain.drop(); ex.rtc_part.drop(); ex.rtc_resident.drop(); ex.rtc_hot.drop(); }
  for (auto& ex : p->exec) if (ex.fb_event) { (void)hipEventDestroy(ex.fb_event); ex.fb_event = nullptr; g_events.fetch_sub(1); }
  ssgpu_ctx* c = p->ctx;
  g_live_plans.fetch_sub(1);
  if (c && c->device >= 0) (void)hipSetDevice(c->device);   // frees and parks below belong to the plan's device, whatever is current
  tls_park_released = c && c->device >= 0;   // the stream was drained above: the plan's device blocks may go to the pool (DevPool)
  delete p;
  tls_park_released = false;
  if (c) ctx_release(c);
}

int32_t ssgpu_plan_attr_count(const ssgpu_plan* p) { return p ? (int32_t)p->result_schema.size() : 0; }
int ssgpu_plan_attr(const ssgpu_plan* p, int32_t i, ssgpu_attr* out) {
  if (!p || i < 0 || i >= (int)p->result_schema.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  out->name = p->attr_names[i].c_str();
  out->dtype = p->result_schema[i].dtype;
  out->nullable = p->result_schema[i].nullable ? 1 : 0;
  return SSGPU_OK;
}
const char* ssgpu_plan_describe(ssgpu_plan* p) {
  if (!p) return "";
  // one line per table over the STRING dictionary
  std::string lines;
  for_each_dict_table(p, true, [&](const DictTableSpec& spec) { lines += p->dict_tables.describe(spec, p->dict); });
  if (lines.empty()) return p->describe.c_str();
  p->describe_full = p->describe + lines;
  return p->describe_full.c_str();
}

int ssgpu_plan_program(const ssgpu_plan* cp, int32_t stage, const void** instrs, int32_t* n, int32_t* bytes) {
  ssgpu_plan* p = const_cast<ssgpu_plan*>(cp);
  if (!p || stage < 0 || stage >= (int)p->stages.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ProgramLayout L = layout_program(p->stages[stage].main, p->ctx->opt);
  finalize_program(p->stages[stage].main, L, &p->host_prog_scratch);
  *instrs = p->host_prog_scratch.data(); *n = (int32_t)p->host_prog_scratch.size(); *bytes = (int32_t)sizeof(VmInstr);
  return SSGPU_OK;
}

void ssgpu_interrupt(ssgpu_plan* p) { if (p) p->interrupted.store(1, std::memory_order_relaxed); }

}  // extern "C"

// ---- execution helpers -------------------------------------------------------------
namespace {

struct InCols { std::vector<ssgpu_column> cols; int64_t rows = 0;
                const unsigned long long* rows_dev = nullptr; };   // rows_dev: the row count lives on the device (a stage hand-off without a host round trip); `rows` is then an upper bound

int upload_program(ssgpu_ctx* c, const Program& prog, const ProgramLayout& L, DevBuf* dev, int* n_instr, std::vector<VmInstr>* scratch) {
  finalize_program(prog, L, scratch);
  *n_instr = (int)prog.code.size();  // without the trailing prefetch pad
  HIP_TRY(c, dev->ensure(std::max<size_t>(1, scratch->size()) * sizeof(VmInstr)));
  if (!scratch->empty())
    HIP_TRY(c, hipMemcpyAsync(dev->p, scratch->data(), scratch->size() * sizeof(VmInstr), hipMemcpyHostToDevice, c->stream));
  // the scratch vector is reused by the next upload: wait for this copy (pageable source is staged
  // synchronously by the runtime, so this is a formality and only happens on (re)layout)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SSGPU_OK;
}

// the staged columns of a program under a layout, as rtc.cpp bakes them into a specialised kernel (= what fill_params passes at run time)
static void staged_table(const Program& prog, const ProgramLayout& L, std::vector<uint32_t>* width, std::vector<uint32_t>* off) {
  width->clear(); off->clear();
  for (auto& sgd : prog.staged) { width->push_back(prog.regs[sgd.reg].width); off->push_back(prog.regs[sgd.reg].row_off * (uint32_t)(VM_TILE_UNIT * L.K)); }
}
// The kernel specialised for `prog` (rtc.cpp) that a launch needing `lds_bytes` of LDS can use, compiled on first need when
// the plan asked for specialisation; NULL = the interpreting kernel.  A launch beyond the 64 KiB of dynamic LDS a
// module-loaded kernel may have gets a build whose LDS is a static array of exactly that size (one build per size: the
// size fixes the occupancy, as it does for the interpreter).
void* rtc_for(ssgpu_plan* p, StageExec& ex, StageExec::RtcSlot& slot, const Program& prog, const ProgramLayout& L, const std::vector<VmInstr>& host_prog,
              int n_instr, uint32_t lds_bytes, const char* what) {
  if (!p->specialize) return nullptr;
  ssgpu_ctx* c = p->ctx;
  const uint32_t need_static = lds_bytes > 64u * 1024u ? ((lds_bytes + 15u) & ~15u) : 0u;
  if (slot.tried && slot.static_lds == need_static && !slot.ask_again() && !slot.stronger_mode_now()) return slot.h;
  if (slot.h) { (void)hipStreamSynchronize(c->stream); slot.drop(); }   // launches of the kernel being replaced may still be in flight
  const bool was_pending = slot.pending;
  slot.tried = true; slot.static_lds = need_static;
  std::vector<uint32_t> sw, so; staged_table(prog, L, &sw, &so);
  std::string why;
  slot.h = ssgpu_rtc_specialize(c->device, host_prog.data(), n_instr, L.K, prog.uses_math, sw.data(), so.data(), (int)sw.size(), need_static, &why);
  slot.asked();
  if (!slot.h && ex.rtc_why.empty()) ex.rtc_why = std::string(what) + why;
  if (slot.h && was_pending) ex.rtc_why.clear();
  return slot.h;
}

int prepare_stage(ssgpu_plan* p, size_t si) {
  ssgpu_ctx* c = p->ctx;
  Stage& st = p->stages[si];
  StageExec& ex = p->exec[si];
  if (st.main.empty()) return SSGPU_OK;
  ProgramLayout L = layout_program(st.main, c->opt);
  if (ex.prog_main.p && L.K == ex.lay.K) return SSGPU_OK;  // already prepared
  ex.lay = L;
  int rc = upload_program(c, st.main, L, &ex.prog_main, &ex.n_instr_main, &p->host_prog_scratch);
  if (rc != SSGPU_OK) return rc;
  ex.host_prog_main = p->host_prog_scratch;
  if (ex.rtc_main.h) (void)hipStreamSynchronize(c->stream);
  ex.rtc_main.drop(); ex.rtc_why.clear();   // another tile size is another program
  if (!st.count_pass.empty()) {
    // the count pass stages only the predicate's inputs: it takes the largest tile (fewer, longer tiles; its counts
    // are still per tile of the store pass)
    LowerOptions o = c->opt; o.tile_rows = VM_TILE_UNIT * 4;
    ex.lay_count = layout_program(st.count_pass, o);
    if (ex.lay_count.K < L.K) { o.tile_rows = VM_TILE_UNIT * L.K; ex.lay_count = layout_program(st.count_pass, o); }
    rc = upload_program(c, st.count_pass, ex.lay_count, &ex.prog_count, &ex.n_instr_count, &p->host_prog_scratch);
    if (rc != SSGPU_OK) return rc;
  }
  HIP_TRY(c, ex.error_flag.ensure(sizeof(uint32_t)));
  // slot kinds / emit descriptors are uploaded per run (they hold output pointers)
  return SSGPU_OK;
}

// ---- hash joins fused into a stage -------------------------------------------------------------
// The index over the rhs table is rebuilt at the start of every run of the stage (dimension
// tables are small next to the probing side; the build is one launch of ssgpu_join_build_kernel).
// Stable LSD radix sort of the row ids 0..n-1 by a device array of 32-bit keys (the sort stage's
// kernels and scratch buffers); *sorted points into the stage's index buffers.
int sort_rows_by_u32(ssgpu_plan* p, StageExec& ex, const uint32_t* keys32, uint64_t n, uint32_t** sorted) {
  ssgpu_ctx* c = p->ctx;
  const uint32_t nt = ssgpu_sort_tiles(n);
  HIP_TRY(c, ex.skeys_a.ensure(std::max<uint64_t>(n, 1) * 8)); HIP_TRY(c, ex.skeys_b.ensure(std::max<uint64_t>(n, 1) * 8));
  HIP_TRY(c, ex.sidx_a.ensure(std::max<uint64_t>(n, 1) * 4)); HIP_TRY(c, ex.sidx_b.ensure(std::max<uint64_t>(n, 1) * 4));
  HIP_TRY(c, ex.shist.ensure((size_t)std::max<uint32_t>(nt, 1) * 256 * 4)); HIP_TRY(c, ex.soffs.ensure((size_t)std::max<uint32_t>(nt, 1) * 256 * 4));
  HIP_TRY(c, ex.total.ensure(8)); HIP_TRY(c, ex.total2.ensure(16));
  uint64_t* ka = ex.skeys_a.as<uint64_t>(); uint64_t* kb = ex.skeys_b.as<uint64_t>();
  uint32_t* ia = ex.sidx_a.as<uint32_t>(); uint32_t* ib = ex.sidx_b.as<uint32_t>();
  HIP_TRY(c, ssgpu_launch_sort_iota(ia, n, c->stream));
  if (n > 0) {
    const unsigned long long init[2] = {0ull, ~0ull};
    HIP_TRY(c, hipMemcpyAsync(ex.total2.p, init, 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, ssgpu_launch_sort_load_keys(ka, ia, keys32, nullptr, 4, 0, 0, 0, n, ex.total2.as<unsigned long long>(), c->stream));
    unsigned long long bits[2];
    HIP_TRY(c, hipMemcpyAsync(bits, ex.total2.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t varying = bits[0] ^ bits[1];
    for (uint32_t pass = 0; pass < 4; ++pass) {
      if (!((varying >> (pass * 8)) & 0xFFull)) continue;
      HIP_TRY(c, ssgpu_launch_sort_hist(ka, pass * 8, n, ex.shist.as<uint32_t>(), c->stream));
      HIP_TRY(c, ssgpu_launch_scan_counts(ex.shist.as<uint32_t>(), ex.soffs.as<uint32_t>(), (int)(nt * 256), ex.total.as<uint64_t>(), c->stream));
      HIP_TRY(c, ssgpu_launch_sort_scatter(ka, ia, kb, ib, pass * 8, n, ex.soffs.as<uint32_t>(), c->stream));
      std::swap(ka, kb); std::swap(ia, ib);
      p->counters.n_launches += 3;
    }
  }
  *sorted = ia;
  return SSGPU_OK;
}

int build_joins(ssgpu_plan* p, Stage& st, StageExec& ex) {
  ssgpu_ctx* c = p->ctx;
  if (st.joins.empty()) return SSGPU_OK;
  if (p->aux_rows < 0) { c->err = "this plan joins against an auxiliary input: call ssgpu_plan_set_aux_input first"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  const size_t nj = st.joins.size();
  ex.jkeys.resize(nj); ex.jkeys_hi.resize(nj); ex.jrows.resize(nj); ex.jmisc.resize(nj); ex.vm_joins.resize(nj);
  for (size_t j = 0; j < nj; ++j) {
    const JoinSpec& js = st.joins[j];
    if (js.form != JoinSpec::HASH) {
      // ForeignFilter / RowidMergeJoin: no index and no allocation beyond the flag word.  The slot carries the auxiliary table's row
      // count and, for the search, its key column as it lies -- whose order is verified here, where a HashJoin builds its index: one
      // adjacent-compare launch per run, since the table bound now need not be the one an earlier run saw.
      VmJoin& J = ex.vm_joins[j];
      memset(&J, 0, sizeof(J));
      J.capacity_mask = (uint32_t)p->aux_rows;      // (< VM_NONE: ssgpu_plan_set_aux_input)
      if (js.form == JoinSpec::SEARCH) {
        const long long* keys = static_cast<const long long*>(p->aux_cols[js.rhs_key_cols[0]].data);
        if (p->aux_rows > 0 && !keys) { c->err = "ForeignFilter: the filter's key column has no data"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
        J.keys = reinterpret_cast<const unsigned long long*>(keys);
        if (p->aux_rows > 1) {
          HIP_TRY(c, ex.jmisc[j].ensure(16));
          HIP_TRY(c, hipMemsetAsync(ex.jmisc[j].p, 0, 16, c->stream));
          HIP_TRY(c, ssgpu_launch_keys_ascending(keys, (unsigned long long)p->aux_rows, ex.jmisc[j].as<unsigned int>(), c->stream));
          uint32_t unordered = 0;
          HIP_TRY(c, hipMemcpyAsync(&unordered, ex.jmisc[j].p, 4, hipMemcpyDeviceToHost, c->stream));
          HIP_TRY(c, hipStreamSynchronize(c->stream));
          p->counters.n_launches += 1;
          if (unordered) { c->err = "ForeignFilter: the filter keys must be unique and ascending (a key is not greater than the one before it)"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
        }
      }
      continue;
    }
    uint64_t cap = 16; while (cap < (uint64_t)std::max<int64_t>(p->aux_rows, 1) * 2) cap <<= 1;
    if (cap > (1ull << 31)) { c->err = "hash join rhs table too large"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
    HIP_TRY(c, ex.jmisc[j].ensure(16));
    if (js.wide) {   // two-word keys: keys / keys_hi / rows arrays; a slot is free while rows[slot] == VM_NONE
      HIP_TRY(c, ex.jkeys[j].ensure(cap * 8)); HIP_TRY(c, ex.jkeys_hi[j].ensure(cap * 8)); HIP_TRY(c, ex.jrows[j].ensure(cap * 4));
      HIP_TRY(c, ssgpu_launch_fill_u32(ex.jrows[j].as<unsigned int>(), VM_NONE, cap, c->stream));
    } else {         // one-word keys: {key, answer} pairs, free while key == VM_KEY_EMPTY
      HIP_TRY(c, ex.jkeys[j].ensure(cap * 16));
      HIP_TRY(c, ssgpu_launch_fill_u64(ex.jkeys[j].as<uint64_t>(), VM_KEY_EMPTY, cap * 2, c->stream));
    }
    const uint32_t misc_init[4] = {VM_NONE, 0u, 0u, 0u};   // [0] special row, [1] flags
    HIP_TRY(c, hipMemcpyAsync(ex.jmisc[j].p, misc_init, 16, hipMemcpyHostToDevice, c->stream));
    JoinBuildParams B; memset(&B, 0, sizeof(B));
    B.n_keys = (unsigned)js.rhs_key_cols.size();
    for (size_t k = 0; k < js.rhs_key_cols.size(); ++k) {
      const ssgpu_column& col = p->aux_cols[js.rhs_key_cols[k]];
      B.key_data[k] = col.data; B.key_nulls[k] = p->desc.aux_schema[js.rhs_key_cols[k]].nullable ? col.is_null : nullptr;
      B.width[k] = js.fields[k].width; B.shift[k] = js.fields[k].shift; B.bits[k] = js.fields[k].bits; B.word[k] = js.fields[k].word;
    }
    B.capacity_mask = (uint32_t)(cap - 1); B.n_rows = (unsigned long long)p->aux_rows;
    B.keys = ex.jkeys[j].as<unsigned long long>(); B.rows = ex.jrows[j].as<unsigned int>();
    B.special = ex.jmisc[j].as<unsigned int>(); B.flags = ex.jmisc[j].as<unsigned int>() + 1;
    B.keys_hi = js.wide ? ex.jkeys_hi[j].as<unsigned long long>() : nullptr;
    if (js.multi) {
      const uint64_t nr = (uint64_t)std::max<int64_t>(p->aux_rows, 1);
      ex.jcounts.resize(nj); ex.jstarts.resize(nj); ex.jslot_of_row.resize(nj); ex.jrows_sorted.resize(nj);
      HIP_TRY(c, ex.jcounts[j].ensure((cap + 1) * 4)); HIP_TRY(c, ex.jstarts[j].ensure((cap + 1) * 4));
      HIP_TRY(c, ex.jslot_of_row[j].ensure(nr * 4)); HIP_TRY(c, ex.jrows_sorted[j].ensure(nr * 4));
      HIP_TRY(c, hipMemsetAsync(ex.jcounts[j].p, 0, (cap + 1) * 4, c->stream));
      B.counts = ex.jcounts[j].as<unsigned int>(); B.slot_of_row = ex.jslot_of_row[j].as<unsigned int>();
    }
    HIP_TRY(c, ssgpu_launch_join_build(B, c->stream));
    if (js.multi) {
      // run starts = exclusive scan of the per-key counts in slot order; the rhs row ids, stably sorted by
      // their slot, list every key's rows contiguously in that same order and in ascending row order
      HIP_TRY(c, ex.total.ensure(8));
      HIP_TRY(c, ssgpu_launch_scan_counts(ex.jcounts[j].as<uint32_t>(), ex.jstarts[j].as<uint32_t>(), (int)(cap + 1), ex.total.as<uint64_t>(), c->stream));
      uint32_t* sorted = nullptr;
      int rc = sort_rows_by_u32(p, ex, ex.jslot_of_row[j].as<uint32_t>(), (uint64_t)p->aux_rows, &sorted);
      if (rc != SSGPU_OK) return rc;
      if (p->aux_rows > 0) HIP_TRY(c, hipMemcpyAsync(ex.jrows_sorted[j].p, sorted, (size_t)p->aux_rows * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    uint32_t misc[4];
    HIP_TRY(c, hipMemcpyAsync(misc, ex.jmisc[j].p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (misc[1] == 2) { c->err = "hash join: index table overflow"; return SSGPU_ERROR_UNKNOWN; }
    if (misc[1]) { c->err = "hash join: the rhs keys were declared UNIQUE but a key occurs more than once"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
    VmJoin& J = ex.vm_joins[j];
    J.keys = ex.jkeys[j].as<unsigned long long>(); J.rows = ex.jrows[j].as<unsigned int>();
    J.special = ex.jmisc[j].as<unsigned int>(); J.capacity_mask = (uint32_t)(cap - 1);
    J.answer_slot = js.multi ? 1u : 0u; J.keys_hi = js.wide ? ex.jkeys_hi[j].as<unsigned long long>() : nullptr;
    p->counters.n_launches += 2;
  }
  return SSGPU_OK;
}
// the plan's step list (ssgpu_plan_string_steps): the string-producing nodes of every program of every stage, in the order they are evaluated
static void plan_string_steps(const ssgpu_plan* p, std::vector<ssgpu_string_step>* out) {
  for (auto& st : p->stages)
    for (const Program* pr : stage_programs(st))
      out->insert(out->end(), pr->string_steps.begin(), pr->string_steps.end());
}
static bool plan_has_dict_tables(const ssgpu_plan* p) {
  bool any = false;
  for_each_dict_table(p, false, [&](const DictTableSpec&) { any = true; });
  return any;
}
// before a run: every table the plan's programs gather from exists and belongs to the plan's current dictionary (string_dict.cpp)
int ensure_dict_tables(ssgpu_plan* p) {
  if (!plan_has_dict_tables(p) || p->dict_tables.current(p->dict, p->dict_gen)) return SSGPU_OK;
  std::vector<DictTableSpec> gathers;
  for_each_dict_table(p, false, [&](const DictTableSpec& spec) { gathers.push_back(spec); });
  std::vector<ssgpu_string_step> steps;
  plan_string_steps(p, &steps);
  return p->dict_tables.build(p->ctx, p->dict, p->dict_gen, gathers, steps, &p->counters.n_launches);
}

void apply_joins(const ssgpu_plan* p, const StageExec& ex, const Program& prog, VmParams* P) {
  for (size_t j = 0; j < ex.vm_joins.size() && j < VM_MAX_JOINS; ++j) P->join[j] = ex.vm_joins[j];
  for (size_t g = 0; g < prog.gathers.size() && g < VM_MAX_JOIN_COLS; ++g) {
    const JoinGather& jg = prog.gathers[g];
    if (jg.join_id == JOIN_GATHER_DICT_TABLE) {   // a table over the STRING dictionary, indexed by a code (ensure_dict_tables)
      p->dict_tables.slot(jg.table, &P->join_cols[g].data, &P->join_cols[g].is_null);
      continue;
    }
    if (jg.rhs_col < 0) {   // the per-key run arrays of a NOT_UNIQUE join, indexed by the probed slot
      const DevBuf& b = jg.rhs_col == JOIN_GATHER_RUN_START ? ex.jstarts[jg.join_id] : ex.jcounts[jg.join_id];
      P->join_cols[g].data = b.p; P->join_cols[g].is_null = nullptr;
      continue;
    }
    const ssgpu_column& col = p->aux_cols[prog.gathers[g].rhs_col];
    P->join_cols[g].data = col.data;
    P->join_cols[g].is_null = p->desc.aux_schema[prog.gathers[g].rhs_col].nullable ? col.is_null : nullptr;
  }
}

// debug_timing >= 2: per-instruction cycle profile of a stage program (development aid)
int attach_pc_profile(ssgpu_ctx* c, StageExec& ex, VmParams* P) {
  if (c->debug_timing < 2) return SSGPU_OK;
  HIP_TRY(c, ex.debug_pc.ensure((size_t)(P->n_instr + 1) * 8));
  HIP_TRY(c, hipMemsetAsync(ex.debug_pc.p, 0, (size_t)(P->n_instr + 1) * 8, c->stream));
  P->debug_pc = ex.debug_pc.as<unsigned long long>();
  P->debug_pc_lds_off = (P->lds_bytes + 7u) & ~7u;
  P->lds_bytes = P->debug_pc_lds_off + (uint32_t)(P->n_instr + 1) * 8u;
  return SSGPU_OK;
}
int print_pc_profile(ssgpu_ctx* c, StageExec& ex, const Program& prog, int n_instr) {
  if (c->debug_timing < 2) return SSGPU_OK;
  std::vector<unsigned long long> cyc((size_t)n_instr + 1);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(cyc.data(), ex.debug_pc.p, cyc.size() * 8, hipMemcpyDeviceToHost));
  double tot = 0; for (auto v : cyc) tot += (double)v;
  fprintf(stderr, "[ssgpu pc-profile] staging+wait %5.1f%%\n", 100.0 * (double)cyc[n_instr] / tot);
  for (int pc = 0; pc < n_instr && pc < (int)prog.code.size(); ++pc)
    fprintf(stderr, "[ssgpu pc-profile] %3d %-22s %5.1f%%\n", pc, vm_op_name(prog.code[pc].op), 100.0 * (double)cyc[pc] / tot);
  return SSGPU_OK;
}

int grid_for(ssgpu_ctx* c, const ProgramLayout& L, int n_tiles) {
  int per_cu = (int)std::min<uint32_t>((uint32_t)c->wgs_per_cu, (160u * 1024u) / std::max<uint32_t>(L.lds_bytes, 1));
  if (per_cu < 1) per_cu = 1;
  int64_t g = (int64_t)c->cu_count * per_cu;
  if (c->grid_limit > 0) g = std::min<int64_t>(g, c->grid_limit);
  g = std::min<int64_t>(g, std::max(1, n_tiles));
  return (int)std::max<int64_t>(g, 1);
}

// the stage's main program: its specialised kernel when the plan runs specialised kernels, else the interpreter
static hipError_t launch_main(ssgpu_plan* p, const Stage& st, StageExec& ex, const VmParams& P, int K, int grid) {
  ssgpu_ctx* c = p->ctx;
  if (p->specialize && !P.debug_pc) {
    void* h = rtc_for(p, ex, ex.rtc_main, st.main, ex.lay, ex.host_prog_main, ex.n_instr_main, P.lds_bytes, "");
    if (h) return ssgpu_launch_pipeline_rtc(h, P, grid, ex.rtc_main.static_lds != 0, c->stream);
  }
  return ssgpu_launch_pipeline(P, K, grid, c->stream);
}

void fill_params(VmParams* P, const Program& prog, const ProgramLayout& L, const DevBuf& dev_prog, int n_instr,
                 const InCols& in, int64_t row_id_base) {
  memset(P, 0, sizeof(*P));
  P->prog = dev_prog.as<const VmInstr>();
  P->n_instr = n_instr;
  P->n_staged = (int)prog.staged.size();
  P->n_outputs = prog.n_outputs;
  P->uses_math = prog.uses_math ? 1u : 0u;
  P->n_slots = prog.n_slots;
  P->n_rows = in.rows;
  P->n_rows_dev = in.rows_dev;
  P->row_id_base = row_id_base;
  P->tile_rows = VM_TILE_UNIT * L.K;
  P->n_tiles = (int)((in.rows + P->tile_rows - 1) / P->tile_rows);
  P->acc_lds_off = L.acc_off;
  P->scratch_lds_off = L.scratch_off;
  P->imm_pool_lds_off = L.imm_pool_off;
  P->const_lds_off = L.imm_pool_off + 16u * (uint32_t)prog.code.size();  // behind the constant pool
  P->lds_bytes = L.lds_bytes;
  for (size_t i = 0; i < prog.staged.size(); ++i) {
    const StagedInput& s = prog.staged[i];
    P->staged[i].src = s.is_null_mask ? (const void*)in.cols[s.col].is_null : in.cols[s.col].data;
    P->staged[i].lds_off = prog.regs[s.reg].row_off * (uint32_t)P->tile_rows;
    P->staged[i].width = prog.regs[s.reg].width;
  }
}

int ensure_out_cols(ssgpu_ctx* c, const Stage& st, StageExec& ex, int64_t rows) {
  ex.out.resize(st.out_schema.size());
  size_t total = 0;
  for (size_t i = 0; i < st.out_schema.size(); ++i) {
    OutCol& oc = ex.out[i];
    oc.width = (uint32_t)dtype_width(st.out_schema[i].dtype);
    oc.nullable = st.out_schema[i].nullable;
    total += (size_t)std::max<int64_t>(rows, 1) * (oc.width + (oc.nullable ? 1u : 0u));
  }
  if (c->out_arena && total >= kBlockArenaMin && st.out_schema.size() > 1) {
    // a large materialised result is laid out like a device block (ssgpu_block: one allocation, column bases skewed): its columns
    // are written in lockstep by the store pass / the sort's gather, and read in lockstep by the stage that follows
    auto pitch = [](size_t bytes) { return ((bytes + (2u << 20) - 1) / (2u << 20)) * (2u << 20) + kBlockColumnSkew; };
    bool fits = ex.out_arena.p != nullptr;
    for (size_t i = 0; i < ex.out.size() && fits; ++i)
      fits = ex.out[i].data.view && ex.out[i].data.cap >= (size_t)std::max<int64_t>(rows, 1) * ex.out[i].width + 16 &&
             (!ex.out[i].nullable || (ex.out[i].nulls.view && ex.out[i].nulls.cap >= (size_t)std::max<int64_t>(rows, 1) + 16));
    if (!fits) {
      size_t need = 0;
      for (auto& oc : ex.out) need += pitch((size_t)rows * oc.width + 16) + (oc.nullable ? pitch((size_t)rows + 16) : 0);
      for (auto& oc : ex.out) { oc.data.release(); oc.nulls.release(); }
      ex.out_arena.release();
      HIP_TRY(c, ex.out_arena.ensure(need));
      size_t off = 0;
      for (auto& oc : ex.out) { const size_t bytes = (size_t)rows * oc.width + 16; oc.data.set_view(ex.out_arena.as<char>() + off, bytes); off += pitch(bytes); }
      for (auto& oc : ex.out) if (oc.nullable) { oc.nulls.set_view(ex.out_arena.as<char>() + off, (size_t)rows + 16); off += pitch((size_t)rows + 16); }
    }
    ex.out_capacity = rows;
    return SSGPU_OK;
  }
  for (size_t i = 0; i < st.out_schema.size(); ++i) {
    OutCol& oc = ex.out[i];
    if (oc.data.view) oc.data.release();      // (a result that shrank below the arena's threshold: back to buffers of its own)
    if (oc.nulls.view) oc.nulls.release();
    HIP_TRY(c, oc.data.ensure((size_t)std::max<int64_t>(rows, 1) * oc.width + 16));
    if (oc.nullable) HIP_TRY(c, oc.nulls.ensure((size_t)std::max<int64_t>(rows, 1) + 16));
  }
  ex.out_capacity = rows;
  return SSGPU_OK;
}

// per-lane identities of the register-resident (fast) aggregate slots
void fill_fast_slots(VmParams* P, const Stage& st) {
  for (size_t i = 0; i < st.aggs.size() && i < VM_FAST_SLOTS; ++i) {
    const int kind = st.aggs[i].slot == (int)i ? st.aggs[i].slot_kind : SLOT_COUNT;
    uint64_t i0 = 0, i1 = 0;
    const double pinf = __builtin_inf(), ninf = -__builtin_inf(), nzero = -0.0;
    switch (kind) {
      case SLOT_SUM_DD: memcpy(&i0, &nzero, 8); break;            // -0.0 is the identity of IEEE +
      case SLOT_MIN_U64: i0 = ~0ull; break;
      case SLOT_MIN_F64: memcpy(&i0, &pinf, 8); break;
      case SLOT_MAX_F64: memcpy(&i0, &ninf, 8); break;
      case SLOT_FIRST: i1 = ~0ull; break;
      default: break;
    }
    P->slot_init0[i] = i0; P->slot_init1[i] = i1; P->slot_kind[i] = kind;
  }
}

// DISTINCT aggregates: the BOOL column "first row of its (keys, value) run" over the sorted stage input
int distinct_flags(ssgpu_ctx* c, const Stage& st, StageExec& ex, const InCols& in, ssgpu_column* out) {
  const uint32_t nk = (uint32_t)st.distinct_cols.size();
  if (nk > 16) { c->err = "DISTINCT aggregate under more than 15 group keys"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  const void* kdata[16] = {nullptr}; const uint8_t* knulls[16] = {nullptr}; uint32_t kwidth[16] = {0};
  for (uint32_t k = 0; k < nk; ++k) {
    const int col = st.distinct_cols[k];
    kdata[k] = in.cols[col].data; knulls[k] = in.cols[col].is_null; kwidth[k] = (uint32_t)dtype_width(st.in_schema[col].dtype);
  }
  HIP_TRY(c, ex.dflag.ensure((size_t)std::max<int64_t>(in.rows, 1)));
  HIP_TRY(c, ssgpu_launch_cluster_flags(kdata, knulls, kwidth, nk, (uint64_t)in.rows, ex.dflag.as<uint8_t>(), c->stream));
  out->data = ex.dflag.p; out->is_null = nullptr;
  return SSGPU_OK;
}

int prepare_scalar_emit(ssgpu_plan* p, size_t si, int* n_out);
int run_scalar_agg(ssgpu_plan* p, size_t si, const InCols& in0, int64_t row_id_base, bool stop_at_partial) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  InCols in = in0;
  if (!st.distinct_cols.empty()) {
    ssgpu_column f; const int rc = distinct_flags(c, st, ex, in0, &f); if (rc != SSGPU_OK) return rc;
    in.cols.push_back(f);
  }
  VmParams P;
  fill_params(&P, st.main, ex.lay, ex.prog_main, ex.n_instr_main, in, row_id_base);
  apply_joins(p, ex, st.main, &P);
  if (c->tile_map >= 2) P.flags |= VM_FLAG_XCD_CHUNKS;
  fill_fast_slots(&P, st);
  const int grid = grid_for(c, ex.lay, P.n_tiles);
  ex.grid = grid;
  const int ns = st.main.n_slots;
  HIP_TRY(c, ex.wg_partials.ensure((size_t)grid * ns * VM_WAVES * sizeof(VmAccRec)));
  HIP_TRY(c, ex.slot_recs.ensure((size_t)ns * sizeof(VmAccRec)));
  HIP_TRY(c, ex.state.ensure((size_t)ns * SSGPU_STATE_ARRAYS * sizeof(uint64_t)));
  if (!ex.slot_kind.p) {
    std::vector<int> kinds((size_t)ns, SLOT_COUNT);   // per SLOT (an aliased COUNT owns no slot)
    for (size_t i = 0; i < st.aggs.size(); ++i)
      if (st.aggs[i].slot == (int)i) kinds[i] = st.aggs[i].slot_kind;
    HIP_TRY(c, ex.slot_kind.ensure(kinds.size() * sizeof(int)));
    HIP_TRY(c, hipMemcpy(ex.slot_kind.p, kinds.data(), kinds.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  P.wg_partials = ex.wg_partials.as<VmAccRec>();
  P.error_flag = ex.error_flag.as<unsigned int>();
  if (c->debug_timing) {
    HIP_TRY(c, ex.debug.ensure((size_t)grid * 4 * 8));
    P.debug = ex.debug.as<unsigned long long>();
  }
  // (the stage's error word was cleared by run_plan)
  { int rc = attach_pc_profile(c, ex, &P); if (rc != SSGPU_OK) return rc; }
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
  HIP_TRY(c, launch_main(p, st, ex, P, ex.lay.K, grid));
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
  { int rc = print_pc_profile(c, ex, st.main, P.n_instr); if (rc != SSGPU_OK) return rc; }
  // a partial run (multi-GPU) leaves the reducible state next to the slot records, in the same launch; a whole run emits its result
  // row in it (emit_scalar_agg then has nothing left to launch)
  int n_emit = 0;
  ex.emitted_with_finish = false;
  if (!stop_at_partial && c->fuse_emit) { const int rc = prepare_scalar_emit(p, si, &n_emit); if (rc != SSGPU_OK) return rc; ex.emitted_with_finish = true; }
  HIP_TRY(c, ssgpu_launch_finish_slots(ex.wg_partials.as<VmAccRec>(), ns, grid * VM_WAVES, ex.slot_kind.as<int>(),
                                       ex.slot_recs.as<VmAccRec>(), stop_at_partial ? ex.state.as<uint64_t>() : nullptr, c->stream,
                                       ex.emitted_with_finish ? ex.emit_descs.as<EmitDesc>() : nullptr, n_emit));
  p->counters.n_launches += 2;
  p->counters.tile_rows = P.tile_rows; p->counters.grid = grid; p->counters.lds_bytes = (int32_t)ex.lay.lds_bytes;
  if (c->debug_timing) {
    std::vector<unsigned long long> dbg((size_t)grid * 4);
    HIP_TRY(c, hipMemcpy(dbg.data(), ex.debug.p, dbg.size() * 8, hipMemcpyDeviceToHost));
    double tot = 0, wait = 0, tiles = 0;
    for (int g = 0; g < grid; ++g) { tot += (double)dbg[g * 4]; wait += (double)dbg[g * 4 + 1]; tiles += (double)dbg[g * 4 + 2]; }
    fprintf(stderr, "[ssgpu debug] grid=%d tiles/wg=%.1f cycles/wg=%.0f wait=%.1f%% cycles/tile=%.0f (wait %.0f)\n", grid, tiles / grid,
            tot / grid, 100.0 * wait / tot, tot / tiles, wait / tiles);
  }
  return SSGPU_OK;
}

// Stage::seq_sums: SUM of a floating column into an integer result, folded row after row over the stage's input (its segments
// for a clustered stage, all rows for a scalar one); overwrites the COUNT the stage's program left in the result column
static const int64_t kSeqSumPiece = 1 << 21;   // rows one launch of the one-segment sequential fold takes (20 - 40 ms)
static int run_seq_sums(ssgpu_plan* p, Stage& st, StageExec& ex, const InCols& in, const uint32_t* seg_id) {
  ssgpu_ctx* c = p->ctx;
  auto kind_of = [](int dtype) {
    switch (dtype) {
      case SSGPU_INT32: return 0; case SSGPU_UINT32: return 1; case SSGPU_INT64: return 2; case SSGPU_UINT64: return 3;
      case SSGPU_FLOAT: return 4; default: return 5;
    }
  };
  for (auto& q : st.seq_sums) {
    const void* src = in.cols[q.in_col].data;
    const uint8_t* src_nulls = st.in_schema[q.in_col].nullable ? in.cols[q.in_col].is_null : nullptr;
    uint8_t* dst_nulls = ex.out[q.out_col].nullable ? ex.out[q.out_col].nulls.as<uint8_t>() : nullptr;
    const int sk = kind_of(st.in_schema[q.in_col].dtype), dk = kind_of(st.out_schema[q.out_col].dtype);
    if (seg_id || in.rows <= kSeqSumPiece) {
      HIP_TRY(c, ssgpu_launch_seq_sum(src, src_nulls, sk, seg_id, (uint64_t)in.rows, ex.out[q.out_col].data.p, dst_nulls, dk, c->stream));
      p->counters.n_launches += 1;
      continue;
    }
    // ONE segment of many rows (a ScalarAggregate): a single wavefront folds it, 10 - 20 ns per row -- seconds at 1e8 rows.  The fold
    // runs in pieces of kSeqSumPiece rows whose state stays on the device, and the host looks at the plan's interrupt flag
    // between them (Cursor::Interrupt, cursor.h:150-186: best effort, but not "after the next minute")
    HIP_TRY(c, ex.total2.ensure(16));
    for (int64_t first = 0; first < in.rows; first += kSeqSumPiece) {
      const int64_t end = std::min<int64_t>(in.rows, first + kSeqSumPiece);
      HIP_TRY(c, ssgpu_launch_seq_sum(src, src_nulls, sk, nullptr, (uint64_t)end, ex.out[q.out_col].data.p, dst_nulls, dk, c->stream,
                                      (uint64_t)first, ex.total2.as<uint64_t>(), first > 0 ? 1 : 0));
      p->counters.n_launches += 1;
      if (end < in.rows) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (p->interrupted.exchange(0)) { c->err = "interrupted"; return SSGPU_INTERRUPTED; }
      }
    }
  }
  return SSGPU_OK;
}

// the one-row result's output buffers and their emit descriptors (uploaded once: the buffers never move)
int prepare_scalar_emit(ssgpu_plan* p, size_t si, int* n_out) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  int rc = ensure_out_cols(c, st, ex, 1);
  if (rc != SSGPU_OK) return rc;
  *n_out = (int)st.aggs.size();
  if (!ex.emit_ready) {
    std::vector<EmitDesc> descs;
    for (size_t i = 0; i < st.aggs.size(); ++i) {
      EmitDesc d; d.data = ex.out[i].data.p; d.is_null = ex.out[i].nullable ? ex.out[i].nulls.as<uint8_t>() : nullptr;
      d.slot = st.aggs[i].slot; d.out_kind = st.aggs[i].emit_kind;
      descs.push_back(d);
    }
    HIP_TRY(c, ex.emit_descs.ensure(std::max<size_t>(descs.size(), 1) * sizeof(EmitDesc)));
    HIP_TRY(c, hipMemcpy(ex.emit_descs.p, descs.data(), descs.size() * sizeof(EmitDesc), hipMemcpyHostToDevice));
    ex.emit_ready = true;
  }
  return SSGPU_OK;
}

int emit_scalar_agg(ssgpu_plan* p, size_t si) {
  ssgpu_ctx* c = p->ctx; StageExec& ex = p->exec[si];
  int n_out = 0;
  const int rc = prepare_scalar_emit(p, si, &n_out);
  if (rc != SSGPU_OK) return rc;
  if (ex.emitted_with_finish) { ex.emitted_with_finish = false; ex.out_rows = 1; return SSGPU_OK; }   // (the finish launch of this run wrote the row)
  HIP_TRY(c, ssgpu_launch_emit_scalar(ex.slot_recs.as<VmAccRec>(), ex.emit_descs.as<EmitDesc>(), n_out, c->stream));
  p->counters.n_launches += 1;
  ex.out_rows = 1;
  return SSGPU_OK;
}

// Stage::segment_cols: the cluster number of every input row (the boundary count + scan + assign passes of run_clusters,
// without the key write-out) as one more input column
int segment_ids(ssgpu_ctx* c, const Stage& st, StageExec& ex, const InCols& in, ssgpu_column* out) {
  const uint32_t nk = (uint32_t)st.segment_cols.size();
  if (nk > 16) { c->err = "AggregateClusters with more than 16 keys"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  const void* kdata[16] = {nullptr}; const uint8_t* knulls[16] = {nullptr}; uint32_t kwidth[16] = {0};
  void* okdata[16] = {nullptr}; uint8_t* oknulls[16] = {nullptr};
  for (uint32_t k = 0; k < nk; ++k) {
    const int col = st.segment_cols[k];
    kdata[k] = in.cols[col].data; knulls[k] = st.in_schema[col].nullable ? in.cols[col].is_null : nullptr; kwidth[k] = (uint32_t)dtype_width(st.in_schema[col].dtype);
  }
  const uint64_t n = (uint64_t)in.rows;
  const int ntile = (int)((n + 511) / 512);
  HIP_TRY(c, ex.seg_counts.ensure((size_t)std::max(ntile, 1) * 4)); HIP_TRY(c, ex.seg_offsets.ensure((size_t)std::max(ntile, 1) * 4));
  HIP_TRY(c, ex.seg_total.ensure(8)); HIP_TRY(c, ex.seg_id.ensure(std::max<uint64_t>(n, 1) * 4));
  HIP_TRY(c, hipMemsetAsync(ex.seg_total.p, 0, 8, c->stream));
  HIP_TRY(c, ssgpu_launch_cluster_count(kdata, knulls, kwidth, nk, n, ex.seg_counts.as<uint32_t>(), c->stream));
  HIP_TRY(c, ssgpu_launch_scan_counts(ex.seg_counts.as<uint32_t>(), ex.seg_offsets.as<uint32_t>(), ntile, ex.seg_total.as<uint64_t>(), c->stream));
  HIP_TRY(c, ssgpu_launch_cluster_assign(kdata, knulls, kwidth, nk, okdata, oknulls, n, ex.seg_offsets.as<uint32_t>(), ex.seg_id.as<uint32_t>(), c->stream));
  out->data = ex.seg_id.p; out->is_null = nullptr;
  return SSGPU_OK;
}

// Stage::has_rank: the RESULT ROW of every input row under GroupAggregateOptions::max_unique_keys_in_result, and whether the row's own
// key keeps a result row.  The rows are sorted by the keys: cluster numbers (segment_ids) -> every cluster's first input row id
// -> the clusters ordered by it (their first-seen rank: the order RowHashSet::Insert numbers new keys in, row_hash_set.cc:458-517) -> per
// row min(rank, limit).  One host round trip (the cluster count); launches and an LSD sort over the CLUSTERS, not the rows.
int rank_columns(ssgpu_plan* p, const Stage& st, StageExec& ex, const InCols& in, ssgpu_column* rank_out, ssgpu_column* own_out) {
  ssgpu_ctx* c = p->ctx;
  // (the clusters are ordered by the 32-bit image of their first row id: every row id of this run has to fit)
  if (p->run_row_end >= (1ll << 32) - 1) { c->err = "DISTINCT / CONCAT aggregates under max_unique_keys_in_result: row ids beyond 2^32"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  ssgpu_column seg;
  int rc = segment_ids(c, st, ex, in, &seg);
  if (rc != SSGPU_OK) return rc;
  const uint64_t n = (uint64_t)in.rows;
  uint64_t n_seg = 0;
  HIP_TRY(c, hipMemcpyAsync(&n_seg, ex.seg_total.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, ex.rank_first.ensure(std::max<uint64_t>(n_seg, 1) * 4)); HIP_TRY(c, ex.rank_of_seg.ensure(std::max<uint64_t>(n_seg, 1) * 4));
  HIP_TRY(c, ex.rank_row.ensure(std::max<uint64_t>(n, 1) * 4)); HIP_TRY(c, ex.rank_own.ensure(std::max<uint64_t>(n, 1)));
  HIP_TRY(c, ssgpu_launch_seg_first(ex.seg_id.as<uint32_t>(), (const uint64_t*)in.cols[st.rank_rowid_col].data, n, ex.rank_first.as<uint32_t>(), c->stream));
  uint32_t* sorted = nullptr;
  rc = sort_rows_by_u32(p, ex, ex.rank_first.as<uint32_t>(), n_seg, &sorted);
  if (rc != SSGPU_OK) return rc;
  HIP_TRY(c, ssgpu_launch_rank_scatter(sorted, n_seg, ex.rank_of_seg.as<uint32_t>(), c->stream));
  HIP_TRY(c, ssgpu_launch_rank_rows(ex.seg_id.as<uint32_t>(), ex.rank_of_seg.as<uint32_t>(), n, (uint32_t)std::min<int64_t>(st.rank_limit, 0xFFFFFFFFll), ex.rank_row.as<uint32_t>(),
                                    ex.rank_own.as<uint8_t>(), c->stream));
  p->counters.n_launches += 3;
  rank_out->data = ex.rank_row.p; rank_out->is_null = nullptr;
  own_out->data = ex.rank_own.p; own_out->is_null = nullptr;
  return SSGPU_OK;
}

int run_materialize(ssgpu_plan* p, size_t si, const InCols& in0, int64_t row_id_base) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  int rc = ensure_out_cols(c, st, ex, in0.rows);
  if (rc != SSGPU_OK) return rc;
  ex.out_rows_dev = nullptr;
  InCols in = in0;
  if (!st.distinct_cols.empty()) {   // a further DISTINCT column's first-of-run flags, stored with the rows (lower.cpp)
    ssgpu_column f; rc = distinct_flags(c, st, ex, in0, &f); if (rc != SSGPU_OK) return rc;
    in.cols.push_back(f);
  }
  if (st.has_segment) {    // DISTINCT aggregates of clusters: the rows are stored with their cluster's number
    ssgpu_column f; rc = segment_ids(c, st, ex, in0, &f); if (rc != SSGPU_OK) return rc;
    in.cols.push_back(f);
  }
  if (st.has_rank) {       // DISTINCT aggregates under a key limit: the rows are stored with their result row
    ssgpu_column r, o; rc = rank_columns(p, st, ex, in0, &r, &o); if (rc != SSGPU_OK) return rc;
    in.cols.push_back(r); in.cols.push_back(o);
  }
  VmParams P;
  fill_params(&P, st.main, ex.lay, ex.prog_main, ex.n_instr_main, in, row_id_base);
  apply_joins(p, ex, st.main, &P);
  P.error_flag = ex.error_flag.as<unsigned int>();   // (cleared by run_plan)
  if (c->tile_map >= 1) P.flags |= VM_FLAG_XCD_CHUNKS;   // this launch writes rows: neighbouring tiles' shared output lines meet in one L2
  // output table: data column then (if nullable) its null mask, in out_schema order
  int oi = 0;
  for (size_t i = 0; i < ex.out.size(); ++i) {
    P.outputs[oi].dst = ex.out[i].data.p; P.outputs[oi].width = ex.out[i].width; ++oi;
    if (ex.out[i].nullable) { P.outputs[oi].dst = ex.out[i].nulls.p; P.outputs[oi].width = 1; ++oi; }
  }
  rc = attach_pc_profile(c, ex, &P);
  if (rc != SSGPU_OK) return rc;
  const int grid = grid_for(c, ex.lay, P.n_tiles);
  ex.grid = grid;
  p->counters.tile_rows = P.tile_rows; p->counters.grid = grid; p->counters.lds_bytes = (int32_t)ex.lay.lds_bytes;
  bool dom0_recorded = false;
  if (st.has_filter) {
    const int nt = std::max(P.n_tiles, 1);
    HIP_TRY(c, ex.tile_counts.ensure((size_t)nt * sizeof(uint32_t)));
    HIP_TRY(c, ex.tile_offsets.ensure((size_t)nt * sizeof(uint32_t)));
    HIP_TRY(c, ex.total.ensure(16));
    if (c->profile) { HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream)); dom0_recorded = true; }   // the stage's kernels: count pass, scan, store pass
    VmParams C;
    fill_params(&C, st.count_pass, ex.lay_count, ex.prog_count, ex.n_instr_count, in, row_id_base);
    apply_joins(p, ex, st.count_pass, &C);
    C.tile_counts = ex.tile_counts.as<unsigned int>();
    C.count_sub_k = ex.lay.K;
    if (c->tile_map >= 2) C.flags |= VM_FLAG_XCD_CHUNKS;
    C.error_flag = P.error_flag;
    const int cgrid = grid_for(c, ex.lay_count, C.n_tiles);
    HIP_TRY(c, ssgpu_launch_pipeline(C, ex.lay_count.K, cgrid, c->stream));
    HIP_TRY(c, ssgpu_launch_scan_counts(ex.tile_counts.as<uint32_t>(), ex.tile_offsets.as<uint32_t>(), P.n_tiles,
                                        ex.total.as<uint64_t>(), c->stream));
    P.tile_offsets = ex.tile_offsets.as<unsigned int>();
    p->counters.n_launches += 2;
    ex.out_rows = -1;
  } else if (in.rows_dev) {
    ex.out_rows = -1; ex.out_rows_dev = in.rows_dev;   // as many rows as came in: the same device word
  } else {
    ex.out_rows = in.rows;
  }
  if (c->profile && !dom0_recorded) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
  HIP_TRY(c, launch_main(p, st, ex, P, ex.lay.K, grid));
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
  p->counters.n_launches += 1;
  return print_pc_profile(c, ex, st.main, ex.n_instr_main);
}

// occupied slots of the global group table -> dense result rows in slot order
// FIRST / LAST inside Group/Clusters aggregates: the extracted column holds row ids (written to
// ex.rowid_tmp[j]); fetch the input column's values at those rows into the real output column.
static int gather_first_last(ssgpu_plan* p, Stage& st, StageExec& ex, size_t nk, const InCols& in, int64_t row_id_base,
                             const uint64_t* n_rows_dev, uint64_t n_rows_max) {
  ssgpu_ctx* c = p->ctx;
  for (size_t j = 0; j < st.aggs.size(); ++j) {
    const int col = st.aggs[j].gather_col;
    if (col < 0) continue;
    auto kind_of = [](int dtype) {   // 0 i32, 1 u32, 2 i64, 3 u64, 4 f32, 5 f64, 6 one byte (the gather converts between them)
      switch (dtype) {
        case SSGPU_INT32: case SSGPU_DATE: case SSGPU_STRING: return 0; case SSGPU_UINT32: return 1;
        case SSGPU_INT64: case SSGPU_DATETIME: return 2; case SSGPU_UINT64: return 3;
        case SSGPU_FLOAT: return 4; case SSGPU_DOUBLE: return 5; default: return 6;
      }
    };
    HIP_TRY(c, ssgpu_launch_gather_rowid(ex.out[nk + j].data.p, ex.out[nk + j].nullable ? ex.out[nk + j].nulls.as<uint8_t>() : nullptr,
                                         in.cols[col].data, ex.out[nk + j].width, kind_of(st.in_schema[col].dtype), kind_of(st.out_schema[nk + j].dtype),
                                         ex.rowid_tmp[j].as<uint64_t>(), st.aggs[j].gather_low32 ? 0xFFFFFFFFull : ~0ull, row_id_base,
                                         n_rows_dev, n_rows_max, c->stream));
    p->counters.n_launches += 1;
  }
  return SSGPU_OK;
}
static int ensure_rowid_tmp(ssgpu_ctx* c, Stage& st, StageExec& ex, uint64_t rows) {
  ex.rowid_tmp.resize(st.aggs.size());
  for (size_t j = 0; j < st.aggs.size(); ++j)
    if (st.aggs[j].gather_col >= 0) HIP_TRY(c, ex.rowid_tmp[j].ensure(std::max<uint64_t>(rows, 1) * 8));
  return SSGPU_OK;
}

int extract_groups(ssgpu_plan* p, Stage& st, StageExec& ex, uint32_t capacity, uint32_t ng, const InCols& in, int64_t row_id_base, uint32_t extra_slots = 0) {
  ssgpu_ctx* c = p->ctx;
  const size_t slots = (size_t)capacity + 1 + extra_slots;
  const int ntile = (int)((slots + 511) / 512);
  int rc = ensure_out_cols(c, st, ex, (int64_t)slots);
  if (rc != SSGPU_OK) return rc;
  HIP_TRY(c, ex.total.ensure(16));   // [rows u64][ticket u32][gave-up u32]: cleared by the run's ssgpu_group_init launch
  {
    const size_t had = ex.xstatus.cap;
    HIP_TRY(c, ex.xstatus.ensure((size_t)ntile * 8));
    ex.x_epoch = (ex.x_epoch + 1) & 0x3FFFFFFFull;
    if (ex.xstatus.cap != had || ex.x_epoch == 0) {   // words of earlier runs read as "not yet": cleared only when (re)allocated or the epoch wraps
      HIP_TRY(c, hipMemsetAsync(ex.xstatus.p, 0, ex.xstatus.cap, c->stream));
      if (ex.x_epoch == 0) ex.x_epoch = 1;
    }
  }
  GroupExtractParams G;
  memset(&G, 0, sizeof(G));
  G.keys = ex.gkeys.as<unsigned long long>();
  G.acc = ex.gacc.as<unsigned long long>(); G.cnt = ex.gcnt.as<unsigned int>();
  G.capacity = capacity; G.n_gaggs = ng; G.n_keys = (uint32_t)st.group_keys.size(); G.n_aggs_out = (uint32_t)st.aggs.size(); G.extra_slots = extra_slots;
  for (size_t k = 0; k < st.group_keys.size(); ++k) {
    const GroupKeyField& f = st.group_keys[k];
    G.keys_out[k].data = ex.out[k].data.p;
    G.keys_out[k].is_null = ex.out[k].nullable ? ex.out[k].nulls.as<uint8_t>() : nullptr;
    G.keys_out[k].shift = f.shift; G.keys_out[k].bits = f.bits; G.keys_out[k].nullbit = f.nullbit; G.keys_out[k].width = f.width;
  }
  const size_t nk = st.group_keys.size();
  rc = ensure_rowid_tmp(c, st, ex, slots);
  if (rc != SSGPU_OK) return rc;
  for (size_t j = 0; j < st.aggs.size(); ++j) {
    G.aggs_out[j].data = st.aggs[j].gather_col >= 0 ? ex.rowid_tmp[j].p : ex.out[nk + j].data.p;
    G.aggs_out[j].is_null = ex.out[nk + j].nullable ? ex.out[nk + j].nulls.as<uint8_t>() : nullptr;
    G.aggs_out[j].s = st.aggs[j].slot; G.aggs_out[j].out_kind = st.aggs[j].emit_kind; G.aggs_out[j].has_cnt = st.aggs[j].has_cnt ? 1 : 0;
  }
  // count + scan + extract as ONE launch (ticket-ordered tiles, decoupled look-back): same rows, same (slot) order
  HIP_TRY(c, ssgpu_launch_group_extract_lb(G, ex.xstatus.as<unsigned long long>(), ex.x_epoch, ex.total.as<unsigned int>(), ex.error_flag.as<unsigned int>(), c->stream));
  p->counters.n_launches += 1;
  rc = gather_first_last(p, st, ex, nk, in, row_id_base, ex.total.as<uint64_t>(), slots);
  if (rc != SSGPU_OK) return rc;
  ex.out_rows = -1;
  return SSGPU_OK;
}

// GroupAggregate with many groups (run feedback: the workgroup-private LDS table of the direct
// path is bypassed by most rows, i.e. the 24 G/s global atomic rate would bound the stage):
//   1. scatter pass     ONE pipeline launch: every selected row becomes a record (packed key + the distinct
//                       aggregate inputs) in the segment of its (hash partition, workgroup) -- segments are
//                       over-allocated and private to a workgroup, so there is no count pass and no scan
//   2. ssgpu_part_agg   one workgroup per partition aggregates its segments in LDS, no global atomics
//   3. the usual extraction over the dumped tables
// A segment that runs full (skewed keys) reruns with 4x larger segments; a partition with more groups than its
// LDS table holds reruns with twice the partitions.  *fallback is set when neither can be satisfied.
// Lazy run feedback (StageExec::fb_pending) needs nobody between this stage and the end of the run to wait for the host:
// the stage is the plan's last one, or every later stage is a filter-less materialising stage that takes its row count from
// the device (run_plan's hand-off) -- e.g. the merge plan of a sharded job: GroupAggregate -> Compute.
static bool tail_runs_without_host(const ssgpu_plan* p, size_t si) {
  if (!p->ctx->async_handoff && si + 1 < p->stages.size()) return false;
  for (size_t k = si + 1; k < p->stages.size(); ++k) {
    const Stage& nx = p->stages[k];
    if (!(nx.kind == STAGE_MATERIALIZE && !nx.has_filter && nx.distinct_cols.empty() && !nx.has_segment && !nx.has_rank && nx.joins.empty())) return false;
  }
  return true;
}
// the feedback words are copied to pinned memory on the stream; this event says when THAT copy is done (looking at them then
// does not have to wait for everything queued behind it: the next run of a stepping job starts while the step before is
// still in flight)
static int record_feedback(ssgpu_ctx* c, StageExec& ex) {
  if (!ex.fb_event) { HIP_TRY(c, hipEventCreateWithFlags(&ex.fb_event, hipEventDisableTiming)); g_events.fetch_add(1); }
  HIP_TRY(c, hipEventRecord(ex.fb_event, c->stream));
  return SSGPU_OK;
}

// ---- dense slots (launch.h: DenseKeyMap; StageExec::DenseState) -----------------------------------------------------------
static bool dense_signed(int dtype) { return dtype == SSGPU_INT32 || dtype == SSGPU_INT64 || dtype == SSGPU_DATE || dtype == SSGPU_DATETIME || dtype == SSGPU_STRING; }
static bool dense_eligible(const ssgpu_ctx* c, const Stage& st) {
  if (!c->group_dense || !c->group_partition || !st.plain.ok || c->part_plain == 0 || st.part_scatter.empty() || st.plain.keys.empty()) return false;
  for (auto& k : st.plain.keys)
    switch (k.dtype) {
      case SSGPU_INT32: case SSGPU_UINT32: case SSGPU_INT64: case SSGPU_UINT64: case SSGPU_BOOL: case SSGPU_DATE: case SSGPU_DATETIME: case SSGPU_STRING: break;
      default: return false;   // floating keys: bit patterns, not ranges
    }
  return true;
}
static void dense_entry_bytes(const Stage& st, uint32_t* entry, uint32_t* fixed, uint32_t* slot_bytes) {
  const uint32_t ng = (uint32_t)std::max(st.n_gaggs, 1);
  bool any_cnt = false;
  for (auto& a : st.aggs) any_cnt = any_cnt || a.has_cnt;
  const uint32_t stw = ng | 1u;
  *entry = 8u + stw * 8u + (any_cnt ? stw * 4u : 0u);
  *fixed = *entry + (1024u + 1u) * 4u + 64u + 64u;
  *slot_bytes = 8u + ng * 8u + (any_cnt ? ng * 4u : 0u);
}
// One pass over the key columns: value ranges (order-preserving unsigned domain) united into the stage's DenseState.
static int dense_find_ranges(ssgpu_plan* p, const Stage& st, StageExec& ex, const InCols& in) {
  ssgpu_ctx* c = p->ctx;
  const uint32_t nk = (uint32_t)st.plain.keys.size();
  auto& D = ex.dense;
  if (D.n_keys != nk) { D.n_keys = nk; for (uint32_t k = 0; k < 8; ++k) { D.lo[k] = ~0ull; D.hi[k] = 0ull; } }
  if (in.rows <= 0) return SSGPU_OK;
  PlainScatterParams S; memset(&S, 0, sizeof(S));
  S.n_rows = (unsigned long long)in.rows; S.n_keys = nk;
  unsigned int is_signed[8] = {0};
  for (uint32_t k = 0; k < nk; ++k) {
    const auto& K = st.plain.keys[k];
    S.keys[k].data = in.cols[K.col].data; S.keys[k].nulls = K.nullable ? in.cols[K.col].is_null : nullptr;
    S.keys[k].width = K.width; S.keys[k].shift = K.shift; S.keys[k].bits = K.bits; S.keys[k].nullbit = K.nullbit;
    is_signed[k] = dense_signed(K.dtype) ? 1u : 0u;
  }
  HIP_TRY(c, ex.dense_dom.ensure(3 * 8 * 8));
  const int grid = (int)std::min<int64_t>((int64_t)std::max(c->cu_count, 1) * 2, std::max<int64_t>(1, (in.rows + 4095) / 4096));
  HIP_TRY(c, ssgpu_launch_key_domain(S, is_signed, ex.dense_dom.as<unsigned long long>(), grid, c->stream));
  uint64_t out[24];
  HIP_TRY(c, hipMemcpyAsync(out, ex.dense_dom.p, (size_t)nk * 24, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  p->counters.n_launches += 1;
  for (uint32_t k = 0; k < nk; ++k) {
    if (!out[2 * nk + k]) continue;   // no value of this key here
    D.lo[k] = std::min(D.lo[k], out[k]); D.hi[k] = std::max(D.hi[k], out[nk + k]);
  }
  return SSGPU_OK;
}
// Spans, strides, slot count and table geometry from the ranges.  false: no usable table (ranges too wide for the row count or
// for SSGPU_DENSE_MAX_SLOTS).  tabled: the table goes to a caller's chunked buffer (sharded job): always the partitioned shape.
static bool dense_configure(const ssgpu_ctx* c, const Stage& st, StageExec& ex, uint32_t n_chunks, bool tabled, int64_t rows_hint) {
  auto& D = ex.dense;
  const uint32_t nk = (uint32_t)st.plain.keys.size();
  if (nk == 0 || nk > 8 || n_chunks == 0) return false;
  uint64_t slots = 1;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint64_t values = D.hi[k] >= D.lo[k] ? D.hi[k] - D.lo[k] : ~0ull;   // (minus one)
    if (D.hi[k] >= D.lo[k] && values >= (uint64_t)SSGPU_DENSE_MAX_SLOTS) return false;
    uint64_t span = (D.hi[k] >= D.lo[k] ? values + 1 : 0) + (st.plain.keys[k].nullable ? 1 : 0);
    if (span == 0) span = 1;
    D.span[k] = (uint32_t)span;
    slots *= span;
    if (slots > (uint64_t)SSGPU_DENSE_MAX_SLOTS) return false;
  }
  // the table's work (clearing, dumping, extracting D slots) must stay small next to the scan
  if (rows_hint > 0 && slots > (uint64_t)std::max<int64_t>(rows_hint / 4, 4096)) return false;
  uint32_t stride = 1;
  for (int k = (int)nk - 1; k >= 0; --k) { D.stride[k] = stride; stride *= D.span[k]; }
  D.slots = slots; D.n_chunks = n_chunks;
  uint32_t entry, fixed, slot_bytes;
  dense_entry_bytes(st, &entry, &fixed, &slot_bytes);
  const uint32_t budget80 = c->part_agg_lds > 0 ? (uint32_t)c->part_agg_lds : 80u * 1024u;
  if (fixed + 64u * entry > budget80) return false;
  const uint32_t cmax = (budget80 - fixed) / entry, cfull = (159u * 1024u - fixed) / entry;
  D.resident = !tabled && n_chunks == 1 && slots <= cfull && c->group_slab != 0 && c->group_resident != 0;
  if (D.resident) { D.np = 1; D.cap = (uint32_t)slots; }
  else {
    // partitions: 256 (one aggregation workgroup per CU) unless the tables would not fit 80 KiB of LDS, then the next power of
    // two -- measured on config #3's 100 172 slots, 100 M rows: 192 partitions 2.85 ms, 256 2.57, 384 2.95, 512 2.68, 1024 2.96
    // (profiles/r05_dense_parts.json; fewer partitions = fewer open output lines in the scatter, powers of two beat the others)
    const uint64_t np_min = (slots + cmax - 1) / cmax;
    uint64_t np;
    if (c->dense_parts > 0) np = std::max<uint64_t>((uint64_t)c->dense_parts, np_min);
    else { np = 256; while (np < np_min) np *= 2; }
    np = std::min(np, std::max<uint64_t>(np_min, std::max<uint64_t>(slots / 64, 1)));   // (at least 64 entries per partition where the slots allow)
    np = std::max<uint64_t>(np, 2);
    np = (np + n_chunks - 1) / n_chunks * n_chunks;
    if (np > 4096) return false;
    D.np = (uint32_t)np; D.cap = (uint32_t)((slots + np - 1) / np);
  }
  const uint64_t chunk_slots = (uint64_t)(D.np / n_chunks) * D.cap;
  D.chunk_bytes = (SSGPU_DENSE_HEADER + (chunk_slots + 1) * slot_bytes + 63ull) & ~63ull;
  return true;
}
static DenseKeyMap dense_map(const Stage& st, const StageExec& ex, bool tabled) {
  DenseKeyMap M; memset(&M, 0, sizeof(M));
  const auto& D = ex.dense;
  M.on = 1u; M.n_keys = (unsigned int)st.plain.keys.size();
  M.n_parts = D.np; M.parts_inv = (unsigned int)(0x100000000ull / D.np + 1ull);
  M.chunk_parts = tabled ? D.np / D.n_chunks : D.np;   // (a run into the plan's own table: one chunk, whatever a sharded job configured)
  M.part_cap = D.cap; M.chunk_slots = M.chunk_parts * D.cap;
  M.chunk_stride = tabled ? D.chunk_bytes : 0ull;
  for (size_t k = 0; k < st.plain.keys.size(); ++k) {
    const auto& K = st.plain.keys[k];
    const uint64_t lo_ord = D.hi[k] >= D.lo[k] ? D.lo[k] : (dense_signed(K.dtype) ? 0x8000000000000000ull : 0ull);
    M.keys[k].lo = dense_signed(K.dtype) ? lo_ord ^ 0x8000000000000000ull : lo_ord;   // back to the column's own bit pattern
    M.keys[k].span = D.span[k]; M.keys[k].stride = D.stride[k]; M.keys[k].shift = K.shift; M.keys[k].bits = K.bits; M.keys[k].nullbit = K.nullbit;
  }
  return M;
}

int run_group_agg_partitioned(ssgpu_plan* p, size_t si, const InCols& in, int64_t row_id_base, bool* fallback) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  const uint32_t ng = (uint32_t)std::max(st.n_gaggs, 1);
  *fallback = false;
  if (!ex.prog_pscatter.p) {
    LowerOptions o = c->opt;
    if (c->part_lds_target > 0) o.lds_target_bytes = (int)c->part_lds_target;
    ex.lay_pscatter = layout_program(st.part_scatter, o);
    int rc = upload_program(c, st.part_scatter, ex.lay_pscatter, &ex.prog_pscatter, &ex.n_instr_pscatter, &p->host_prog_scratch);
    if (rc != SSGPU_OK) return rc;
    ex.host_prog_pscatter = p->host_prog_scratch;
  }
  bool any_cnt = false;
  for (auto& a : st.aggs) any_cnt = any_cnt || a.has_cnt;
  const uint32_t W = st.part_rec_bytes / 8u;
  // phase 2's LDS (two 1024-thread workgroups per CU): per table entry the key, the accumulator words and the
  // contribution counts (C entries + the reserved one of the EMPTY-valued key), plus the segment offsets
  const uint32_t stw = ng | 1u;   // accumulator words of an LDS entry are an odd number of words apart (bank conflicts, see the kernel)
  const uint32_t entry = 8u + stw * 8u + (any_cnt ? stw * 4u : 0u);
  const uint32_t fixed = entry + (1024u + 1u) * 4u + 64u + 64u;
  // slab mode (few enough groups that ONE LDS table holds them all): no hash partitioning -- the scatter writes every
  // workgroup's records sequentially, each aggregation workgroup (1024 threads, the whole LDS) takes a slab of them into a
  // table of all groups and merges it into the global table.  Decided by run_group_agg from its group-count estimate.
  if (c->group_slab == 2 && !ex.part_slab_failed) ex.part_slab = true;   // forced (tests)
  // dense slots: the geometry was fixed with the key ranges (dense_configure) -- one table of all slots fed from the input columns
  // (resident), or np partitions of cap entries each
  const bool dense = ex.dense.on;
  const bool tabled = dense && ex.dense_table != nullptr;   // the table goes to the caller's chunked buffer (ssgpu_plan_run_dense)
  if (dense) { ex.part_slab = ex.dense.resident; ex.part_n = ex.dense.np; ex.part_n_chosen = true; }
  const uint32_t budget = ex.part_slab ? 159u * 1024u : (c->part_agg_lds > 0 ? (uint32_t)c->part_agg_lds : 80u * 1024u);
  if (fixed + 64u * entry > budget) { *fallback = true; return SSGPU_OK; }
  uint32_t C = (budget - fixed) / entry;
  if (dense) { if (ex.dense.cap > C) { if (trace_on()) fprintf(stderr, "[ssgpu trace] dense: cap %u > C %u\n", ex.dense.cap, C); *fallback = true; return SSGPU_OK; } C = std::max(ex.dense.cap, 1u); }
  HIP_TRY(c, ex.gpattern.ensure(ng * 8));
  if (!ex.pattern_ready) {
    std::vector<uint64_t> pattern(ng, 0);
    for (size_t i = 0; i < st.group_acc_init.size(); ++i) pattern[i] = st.group_acc_init[i];
    HIP_TRY(c, hipMemcpy(ex.gpattern.p, pattern.data(), ng * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, ex.gmergeop.ensure(ng * 4));
    std::vector<uint32_t> mop(ng, VM_MERGE_ADD_U64);
    for (size_t i = 0; i < st.group_merge_op.size(); ++i) mop[i] = st.group_merge_op[i];
    HIP_TRY(c, hipMemcpy(ex.gmergeop.p, mop.data(), ng * 4, hipMemcpyHostToDevice));
    ex.pattern_ready = true;
  }
  HIP_TRY(c, ex.goverflow.ensure(16));
  HIP_TRY(c, ex.total.ensure(16));
  if (!ex.part_n_chosen) {
    // partitions: enough that a partition's groups load its table to about one half (the direct path's run feedback
    // left an estimate of the group count); one partition per CU or more keeps phase 2's single wave of workgroups full
    ex.part_n_chosen = true;
    if (c->part_n > 0) ex.part_n = (uint32_t)c->part_n;
    else {
      uint32_t pn = 256;
      // (the estimate is a lower bound: keep the load under one half.  The plain scatter gets faster with fewer partitions --
      //  fewer lines open per L2 -- and phase 2 does not mind a fuller table: it may load its tables a little more.)
      const double load = st.plain.ok && c->part_plain ? 0.4 : 0.3;
      while (ex.part_groups_est > load * (double)pn * (double)C && pn < 8192) pn *= 2;
      ex.part_n = pn;
    }
  }
  auto fill_plain_source = [&](PlainScatterParams& S) {
    memset(&S, 0, sizeof(S));
    S.n_rows = (unsigned long long)in.rows;
    S.n_keys = (uint32_t)st.plain.keys.size(); S.n_fields = (uint32_t)st.plain.fields.size(); S.n_preds = (uint32_t)st.plain.preds.size();
    for (size_t k = 0; k < st.plain.keys.size(); ++k) {
      const auto& K = st.plain.keys[k];
      S.keys[k].data = in.cols[K.col].data; S.keys[k].nulls = K.nullable ? in.cols[K.col].is_null : nullptr;
      S.keys[k].width = K.width; S.keys[k].shift = K.shift; S.keys[k].bits = K.bits; S.keys[k].nullbit = K.nullbit;
    }
    for (size_t f = 0; f < st.plain.fields.size(); ++f) {
      const auto& F = st.plain.fields[f];
      S.fields[f].src = F.is_null_mask ? (const void*)in.cols[F.col].is_null : in.cols[F.col].data; S.fields[f].width = F.width; S.fields[f].off = F.off;
    }
    for (size_t q = 0; q < st.plain.preds.size(); ++q) {
      const auto& Q = st.plain.preds[q];
      S.preds[q].data = in.cols[Q.col].data; S.preds[q].nulls = Q.nullable ? in.cols[Q.col].is_null : nullptr;
      S.preds[q].kind = (uint32_t)Q.kind; S.preds[q].cmp = (uint32_t)Q.cmp; S.preds[q].col_on_left = Q.col_on_left ? 1u : 0u; S.preds[q].bits = Q.bits;
    }
  };
  for (int attempt = 0; attempt < 8; ++attempt) {
    const bool slab = ex.part_slab;
    // plain stages, slab form: no scatter at all -- the aggregation workgroups read the input columns (ssgpu_group_resident_kernel)
    const bool resident = slab && st.plain.ok && c->part_plain != 0 && c->group_resident != 0;
    const uint32_t NP = slab ? 1u : ex.part_n;
    ex.last_group_shape = resident ? 3 : slab ? 2 : 1; if (attempt) ++ex.last_reruns;
    ex.last_plain_scatter = false;
    uint32_t capacity = NP * C;
    if (slab && !dense) { capacity = 1024; while (capacity < 4u * C) capacity *= 2; }   // the merge inserts by hash: a power of two, never full
    // heavy hitters (found when a segment overflowed, below): their groups live in SSGPU_HOT_SLOTS dense slots behind the special one
    const bool hot = !slab && !dense && ex.hot_n > 0 && st.plain.ok && c->part_plain != 0 && st.part_rec_bytes <= 128u;
    const uint32_t extra = hot ? SSGPU_HOT_SLOTS : 0u;
    const size_t slots = (size_t)capacity + 1 + extra;
    VmParams Ps;
    fill_params(&Ps, st.part_scatter, ex.lay_pscatter, ex.prog_pscatter, ex.n_instr_pscatter, in, row_id_base);
    apply_joins(p, ex, st.part_scatter, &Ps);
    Ps.part_n = NP;
    // behind the program's registers: the workgroup's NP segment fill counters, the tile's record index by staging
    // position, and the staging area where the tile's records are assembled (see VM_PART_RANK)
    Ps.part_lds_off = (Ps.lds_bytes + 15u) & ~15u;
    Ps.lds_bytes = Ps.part_lds_off + NP * 4u + (uint32_t)Ps.tile_rows * 4u + 16u + (uint32_t)Ps.tile_rows * st.part_rec_bytes;
    // plain stages: the scatter is a kernel of its own over (partition, XCD) segments (ssgpu_part_scatter_plain_kernel)
    const uint32_t W0 = st.part_rec_bytes / 8u;
    const bool plain = !slab && st.plain.ok && c->part_plain != 0 && !Ps.debug_pc && NP >= 2u && (dense || in.rows >= (1 << 16)) &&
                       ssgpu_part_scatter_plain_lds(NP, W0, 1) <= 156u * 1024u;
    if (dense && !plain && !resident) { if (trace_on()) fprintf(stderr, "[ssgpu trace] dense: neither the plain scatter nor the resident kernel can run (NP %u)\n", NP); *fallback = true; return SSGPU_OK; }   // (dense slots exist in the plain scatter and the resident kernel only)
    if (W0 > 16u && !plain) { if (trace_on()) fprintf(stderr, "[ssgpu trace] wide records (%u words) without the plain scatter: slab %d plain.ok %d NP %u rows %lld lds %u\n", W0, (int)slab, (int)st.plain.ok, NP, (long long)in.rows, ssgpu_part_scatter_plain_lds(NP, W0, 1)); *fallback = true; return SSGPU_OK; }     // (17 .. 20-word records: the plain scatter + ssgpu_part_agg_kernel<20> only)
    if (!resident && !plain && Ps.lds_bytes > 160u * 1024u) { *fallback = true; return SSGPU_OK; }
    if (plain && Ps.lds_bytes > 160u * 1024u) Ps.lds_bytes = 160u * 1024u;   // (the VM form's LDS is not used: only its tile shape sizes the grid below)
    ProgramLayout Ls = ex.lay_pscatter; Ls.lds_bytes = Ps.lds_bytes;
    int grid;
    {
      const int64_t saved = c->wgs_per_cu;
      if (c->part_wgs_per_cu > 0) c->wgs_per_cu = c->part_wgs_per_cu;
      grid = std::min(grid_for(c, Ls, Ps.n_tiles), 1024);   // phase 2 scans a partition's segment counts with one thread each
      c->wgs_per_cu = saved;
    }
    const int scatter_grid = grid;
    if (plain) grid = SSGPU_PSCAT_XCDS;   // from here on `grid` is the number of segments per partition
    ex.last_plain_scatter = plain;
    // records a (partition, workgroup) segment holds: the expected share of the INPUT rows (an upper bound of the
    // selected ones) with head room for the spread of a uniform hash, times the growth factor of earlier overflows
    const double expect = (double)std::max<int64_t>(in.rows, 1) / ((double)NP * (double)grid);
    uint64_t seg_cap = (uint64_t)((expect * 1.25 + 8.0 * std::sqrt(expect) + 32.0) * (double)ex.part_seg_growth);
    if (plain) {
      // the plain scatter deals tiles of 2048 (1024) rows round-robin to one workgroup per CU, and a workgroup appends to the segments of
      // ITS XCD: with few tiles the XCDs' shares differ by whole tiles (one tile: every row in XCD 0's segments)
      const PscatGeom geom = ssgpu_part_scatter_plain_geom(NP, W0, (int)c->pscat_threads, (int)c->pscat_rows, (int)c->pscat_wgs);
      const uint64_t T = (uint64_t)geom.threads * geom.rows;
      const uint64_t tiles = ((uint64_t)std::max<int64_t>(in.rows, 1) + T - 1) / T;
      const uint64_t pg = (uint64_t)std::min<int64_t>(std::max(c->cu_count, 1), std::max<int64_t>(1, (in.rows + 1023) / 1024));
      const uint64_t xcds = std::min<uint64_t>(std::min<uint64_t>(SSGPU_PSCAT_XCDS, pg), tiles);
      const double per_xcd = (double)std::min<uint64_t>((uint64_t)std::max<int64_t>(in.rows, 1), (tiles + xcds - 1) / xcds * T);
      const double expect_x = per_xcd / (double)NP;
      seg_cap = (uint64_t)((expect_x * 1.3 + 8.0 * std::sqrt(expect_x) + 64.0) * (double)ex.part_seg_growth);   // (partitions differ by their group counts, too)
    }
    if (slab) seg_cap = (uint64_t)((Ps.n_tiles + grid - 1) / grid) * (uint64_t)Ps.tile_rows;   // all rows a workgroup can see: never full
    if (resident) seg_cap = 1;                                                      // (no records are written)
    const uint64_t n_segs = resident ? 1ull : (uint64_t)NP * (uint64_t)grid;
    if (n_segs * seg_cap >= 0xFFFFFFFFull) { *fallback = true; return SSGPU_OK; }   // record indices are 32-bit
    unsigned long long* tkeys; unsigned long long* tacc; unsigned int* tcnt;   // the global table of this run
    DenseKeyMap dmap; memset(&dmap, 0, sizeof(dmap));
    if (dense) dmap = dense_map(st, ex, tabled);
    if (tabled) {
      char* base = static_cast<char*>(ex.dense_table);
      tkeys = reinterpret_cast<unsigned long long*>(base + SSGPU_DENSE_HEADER);
      tacc = tkeys + ((size_t)dmap.chunk_slots + 1);
      tcnt = reinterpret_cast<unsigned int*>(tacc + ((size_t)dmap.chunk_slots + 1) * ng);
    } else {
      HIP_TRY(c, ex.gkeys.ensure(slots * 8));
      HIP_TRY(c, ex.gacc.ensure(slots * ng * 8));
      HIP_TRY(c, ex.gcnt.ensure(slots * ng * 4));
      tkeys = ex.gkeys.as<unsigned long long>(); tacc = ex.gacc.as<unsigned long long>(); tcnt = ex.gcnt.as<unsigned int>();
    }
    if (ex.part_recs.ensure(n_segs * seg_cap * (size_t)st.part_rec_bytes + 16) != hipSuccess) { (void)hipGetLastError(); *fallback = true; return SSGPU_OK; }
    HIP_TRY(c, ex.part_hist.ensure(n_segs * 4));
    {
      GroupInitParams I; memset(&I, 0, sizeof(I));
      I.pattern = ex.gpattern.as<unsigned long long>(); I.ng = ng;
      if (slab) {   // the aggregation workgroups merge into the table: all of it starts empty
        I.keys = tkeys; I.n_keys = slots;
        I.acc = tacc; I.n_acc = (unsigned long long)slots * ng;
        I.cnt = tcnt; I.n_cnt = (unsigned long long)slots * ng;
      } else if (tabled) {   // the special slot of every chunk (phase 2 writes every regular slot of every chunk)
        I.keys = tkeys + dmap.chunk_slots; I.n_keys = 1;
        I.acc = tacc + (size_t)dmap.chunk_slots * ng; I.n_acc = ng;
        I.cnt = tcnt + (size_t)dmap.chunk_slots * ng; I.n_cnt = any_cnt ? ng : 0;
        I.n_rep = ex.dense.n_chunks - 1u; I.rep_stride = ex.dense.chunk_bytes;
      } else {      // only the reserved slot of the EMPTY-valued key (and the heavy hitters' slots behind it) need initialising: phase 2 writes every other slot
        I.keys = tkeys + capacity; I.n_keys = 1 + extra;
        I.acc = tacc + (size_t)capacity * ng; I.n_acc = (unsigned long long)(1 + extra) * ng;
        I.cnt = tcnt + (size_t)capacity * ng; I.n_cnt = (unsigned long long)(1 + extra) * ng;
      }
      I.z[0] = ex.goverflow.as<unsigned int>(); I.nz[0] = 4;
      I.z[1] = ex.error_flag.as<unsigned int>(); I.nz[1] = 1;
      if (plain) { I.z[2] = ex.part_hist.as<unsigned int>(); I.nz[2] = n_segs; }     // the plain scatter's segment counters
      I.z[3] = ex.total.as<unsigned int>(); I.nz[3] = 4;                             // the extraction's row count, ticket and gave-up flag
      HIP_TRY(c, ssgpu_launch_group_init(I, c->stream));
    }
    Ps.error_flag = ex.error_flag.as<unsigned int>();
    Ps.tile_counts = ex.part_hist.as<unsigned int>();
    Ps.part_seg_cap = (uint32_t)seg_cap;
    Ps.part_overflow = ex.goverflow.as<unsigned int>() + 1;
    Ps.outputs[0].dst = ex.part_recs.p; Ps.outputs[0].width = st.part_rec_bytes;
    if (!plain && !resident) { int rc = attach_pc_profile(c, ex, &Ps); if (rc != SSGPU_OK) return rc; }
    if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
    if (hot && plain) {
      // The heavy hitters' rows: aggregated by the resident kernel in its hot_only form -- every workgroup holds a small table
      // seeded with the hot keys, reads the input columns, skips every row of another key, and merges its entries into the
      // dense slots capacity + 1 + e.  The scatter below skips exactly these rows.
      PlainScatterParams S; fill_plain_source(S);
      S.rec_words = W;
      S.n_hot = ex.hot_n; for (uint32_t h = 0; h < ex.hot_n; ++h) S.hot_keys[h] = ex.hot_keys[h];
      PartAggParams H; memset(&H, 0, sizeof(H));
      H.rec_words = W; H.slab_segs = 1; H.n_segs = 0; H.seg_cap = 1;
      H.local_capacity = SSGPU_HOT_SLOTS; H.n_gaggs = ng; H.n_aggs = (unsigned int)st.part_aggs.size(); H.any_cnt = any_cnt ? 1u : 0u;
      H.T.keys = ex.gkeys.as<unsigned long long>(); H.T.acc = ex.gacc.as<unsigned long long>(); H.T.cnt = ex.gcnt.as<unsigned int>();
      H.T.overflow = ex.goverflow.as<unsigned int>() + 2; H.T.capacity_mask = capacity - 1u; H.T.n_gaggs = ng;
      H.T.acc_init = ex.gpattern.as<unsigned long long>(); H.T.merge_op = ex.gmergeop.as<unsigned int>();
      H.nan_flag = ex.error_flag.as<unsigned int>();
      H.hot_only = 1u; H.hot_base = capacity + 1u;
      for (size_t j = 0; j < st.part_aggs.size(); ++j) {
        const Stage::PartAgg& a = st.part_aggs[j];
        H.desc[j] = (uint64_t)(uint16_t)a.op | ((uint64_t)(uint8_t)a.word << 16) | ((uint64_t)(uint8_t)(a.val_off < 0 ? 0xFF : a.val_off) << 24) |
                    ((uint64_t)(uint8_t)a.val_width << 32) | ((uint64_t)(uint8_t)(a.null_off < 0 ? 0xFF : a.null_off) << 40) | ((uint64_t)(a.has_cnt ? 1 : 0) << 48);
      }
      const uint32_t hot_lds = fixed + SSGPU_HOT_SLOTS * entry;
      const int hgrid = (int)std::min<int64_t>(std::max(c->cu_count, 1), std::max<int64_t>(1, (in.rows + 2047) / 2048));
      H.n_parts = (unsigned int)hgrid;
      if (p->specialize && !(ex.rtc_hot.tried && ex.rtc_hot.static_lds == hot_lds && !ex.rtc_hot.ask_again() && !ex.rtc_hot.stronger_mode_now())) {
        if (ex.rtc_hot.h) { HIP_TRY(c, hipStreamSynchronize(c->stream)); ex.rtc_hot.drop(); }
        ex.rtc_hot.tried = true; ex.rtc_hot.static_lds = hot_lds;
        std::string why;
        ex.rtc_hot.h = ssgpu_rtc_specialize_part_agg(c->device, H.desc, (int)H.n_aggs, W, ng, any_cnt, hot_lds, &why, &S);
        ex.rtc_hot.asked();
        if (!ex.rtc_hot.h && ex.rtc_why.empty()) ex.rtc_why = "heavy-hitter aggregation: " + why;
      }
      if (p->specialize && ex.rtc_hot.h && ex.rtc_hot.static_lds == hot_lds) HIP_TRY(c, ssgpu_launch_group_resident_rtc(ex.rtc_hot.h, H, S, hgrid, c->stream));
      else HIP_TRY(c, ssgpu_launch_group_resident(H, S, hot_lds, hgrid, c->stream));
      p->counters.n_launches += 1;
    }
    if (resident) {
      // nothing to scatter
    } else if (plain) {
      PlainScatterParams S; fill_plain_source(S);
      if (hot) { S.n_hot = ex.hot_n; for (uint32_t h = 0; h < ex.hot_n; ++h) S.hot_keys[h] = ex.hot_keys[h]; }   // their rows are aggregated by the resident kernel below
      S.dense = dmap;
      S.n_parts = NP; S.seg_cap = (uint32_t)seg_cap; S.rec_words = W0; S.rec_inv = (uint32_t)(0x100000000ull / W0 + 1ull);
      S.recs = ex.part_recs.as<unsigned long long>(); S.counts = ex.part_hist.as<unsigned int>(); S.overflow = ex.goverflow.as<unsigned int>() + 1;
      // one fat workgroup per CU: every workgroup more multiplies the open lines and the per-tile atomics
      PscatGeom geom = ssgpu_part_scatter_plain_geom(NP, W0, (int)c->pscat_threads, (int)c->pscat_rows, (int)c->pscat_wgs);
      // (the pipelined form -- specialised builds -- keeps a second array of per-partition counters behind the staging area)
      geom.pipe = (c->pscat_pipe != 0 && p->specialize && geom.lds + NP * 4u <= 156u * 1024u) ? 1u : 0u;
      if (geom.pipe) geom.lds += NP * 4u;
      const int pgrid = (int)std::min<int64_t>((int64_t)std::max(c->cu_count, 1) * geom.wgs_per_cu, std::max<int64_t>(1, (in.rows + 1023) / 1024));
      // the specialised build (plans that asked): one per (descriptor, partition count) -- the LDS carve-up is static in it
      void* hs = nullptr;
      if (p->specialize) {
        const uint32_t lds = geom.lds;
        const uint32_t tag = NP * 128u + (geom.pipe ? 64u : 0u) + (geom.threads == 512u ? 32u : 0u) + geom.rows * 4u + (dense ? 1u : 0u);
        if (!(ex.rtc_plain.tried && ex.rtc_plain.static_lds == lds && ex.rtc_plain.tag == tag && !ex.rtc_plain.ask_again() && !ex.rtc_plain.stronger_mode_now())) {
          if (ex.rtc_plain.h) { HIP_TRY(c, hipStreamSynchronize(c->stream)); ex.rtc_plain.drop(); }
          ex.rtc_plain.tried = true; ex.rtc_plain.static_lds = lds; ex.rtc_plain.tag = tag;
          std::string why;
          ex.rtc_plain.h = ssgpu_rtc_specialize_pscat(c->device, S, geom, &why);
          ex.rtc_plain.asked();
          if (!ex.rtc_plain.h && ex.rtc_why.empty()) ex.rtc_why = "plain partition scatter: " + why;
        }
        hs = ex.rtc_plain.h;
      }
      const int g = (int)std::min<int64_t>(pgrid, std::max<int64_t>(1, ((int64_t)S.n_rows + 1023) / 1024));
      if (hs) HIP_TRY(c, ssgpu_launch_part_scatter_plain_rtc(hs, S, geom, g, c->stream));
      else HIP_TRY(c, ssgpu_launch_part_scatter_plain(S, geom, g, c->stream));
      (void)scatter_grid;
    } else {
      void* h = Ps.debug_pc ? nullptr : rtc_for(p, ex, ex.rtc_pscatter, st.part_scatter, ex.lay_pscatter, ex.host_prog_pscatter, ex.n_instr_pscatter, Ps.lds_bytes, "partition scatter: ");
      if (h) HIP_TRY(c, ssgpu_launch_pipeline_rtc(h, Ps, grid, ex.rtc_pscatter.static_lds != 0, c->stream));
      else HIP_TRY(c, ssgpu_launch_pipeline(Ps, ex.lay_pscatter.K, grid, c->stream));
    }
    if (!plain && !resident) { int rc = print_pc_profile(c, ex, st.part_scatter, Ps.n_instr); if (rc != SSGPU_OK) return rc; }
    PartAggParams A;
    memset(&A, 0, sizeof(A));
    A.recs = ex.part_recs.as<unsigned long long>();
    A.counts = ex.part_hist.as<unsigned int>();
    A.n_segs = (unsigned int)grid; A.seg_cap = (unsigned int)seg_cap; A.rec_words = W; A.n_parts = NP;
    if (slab) {   // one aggregation workgroup per CU, each over a run of the scatter workgroups' segments
      const unsigned int wgs = (unsigned int)std::min<int>(grid, std::max(c->cu_count, 1));
      A.slab_segs = ((unsigned int)grid + wgs - 1u) / wgs;
      A.n_parts = ((unsigned int)grid + A.slab_segs - 1u) / A.slab_segs;
    }
    A.local_capacity = C; A.n_gaggs = ng; A.n_aggs = (unsigned int)st.part_aggs.size(); A.any_cnt = any_cnt ? 1u : 0u;
    A.T.keys = tkeys; A.T.acc = tacc; A.T.cnt = tcnt;
    A.dense = dmap;
    A.T.overflow = ex.goverflow.as<unsigned int>(); A.T.capacity_mask = capacity - 1u; A.T.n_gaggs = ng;
    A.T.acc_init = ex.gpattern.as<unsigned long long>(); A.T.merge_op = ex.gmergeop.as<unsigned int>();
    A.nan_flag = ex.error_flag.as<unsigned int>();
    for (size_t j = 0; j < st.part_aggs.size(); ++j) {
      const Stage::PartAgg& a = st.part_aggs[j];
      A.desc[j] = (uint64_t)(uint16_t)a.op | ((uint64_t)(uint8_t)a.word << 16) | ((uint64_t)(uint8_t)(a.val_off < 0 ? 0xFF : a.val_off) << 24) |
                  ((uint64_t)(uint8_t)a.val_width << 32) | ((uint64_t)(uint8_t)(a.null_off < 0 ? 0xFF : a.null_off) << 40) | ((uint64_t)(a.has_cnt ? 1 : 0) << 48);
    }
    const uint32_t agg_lds = fixed + C * entry;
    if (resident) {
      PlainScatterParams S; fill_plain_source(S);
      S.rec_words = W; S.dense = dmap;
      A.slab_segs = 1; A.n_segs = 0;
      // one whole-LDS workgroup per CU; tiles of 2048 rows dealt round-robin
      const int rgrid = (int)std::min<int64_t>(std::max(c->cu_count, 1), std::max<int64_t>(1, (in.rows + 2047) / 2048));
      A.n_parts = (unsigned int)rgrid;
      if (p->specialize && !(ex.rtc_resident.tried && ex.rtc_resident.static_lds == agg_lds && ex.rtc_resident.tag == (dense ? 1u : 0u) && !ex.rtc_resident.ask_again() && !ex.rtc_resident.stronger_mode_now())) {
        if (ex.rtc_resident.h) { HIP_TRY(c, hipStreamSynchronize(c->stream)); ex.rtc_resident.drop(); }
        ex.rtc_resident.tried = true; ex.rtc_resident.static_lds = agg_lds; ex.rtc_resident.tag = dense ? 1u : 0u;
        std::string why;
        ex.rtc_resident.h = ssgpu_rtc_specialize_part_agg(c->device, A.desc, (int)A.n_aggs, W, ng, any_cnt, agg_lds, &why, &S, dense);
        ex.rtc_resident.asked();
        if (!ex.rtc_resident.h && ex.rtc_why.empty()) ex.rtc_why = "resident group aggregation: " + why;
      }
      if (p->specialize && ex.rtc_resident.h && ex.rtc_resident.static_lds == agg_lds) HIP_TRY(c, ssgpu_launch_group_resident_rtc(ex.rtc_resident.h, A, S, rgrid, c->stream));
      else HIP_TRY(c, ssgpu_launch_group_resident(A, S, agg_lds, rgrid, c->stream));
    } else
    if (p->specialize && !(ex.rtc_part.tried && ex.rtc_part.static_lds == agg_lds && ex.rtc_part.tag == (dense ? 1u : 0u) + (c->part_prefetch ? 4u : 0u) && !ex.rtc_part.ask_again() && !ex.rtc_part.stronger_mode_now())) {
      // one kernel per LDS size (hash partitions and the slab form differ in it): compiled when that shape is first run
      if (ex.rtc_part.h) { HIP_TRY(c, hipStreamSynchronize(c->stream)); ex.rtc_part.drop(); }
      ex.rtc_part.tried = true; ex.rtc_part.static_lds = agg_lds; ex.rtc_part.tag = (dense ? 1u : 0u) + (c->part_prefetch ? 4u : 0u);
      std::string why;
      ex.rtc_part.h = ssgpu_rtc_specialize_part_agg(c->device, A.desc, (int)A.n_aggs, W, ng, any_cnt, agg_lds, &why, nullptr, dense, c->part_prefetch != 0);
      ex.rtc_part.asked();
      if (!ex.rtc_part.h && ex.rtc_why.empty()) ex.rtc_why = "partition aggregation: " + why;
    }
    if (resident) { /* launched above */ }
    else if (p->specialize && ex.rtc_part.h && ex.rtc_part.static_lds == agg_lds) HIP_TRY(c, ssgpu_launch_part_agg_rtc(ex.rtc_part.h, A, c->stream));
    else HIP_TRY(c, ssgpu_launch_part_agg(A, agg_lds, c->stream));
    if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
    p->counters.n_launches += 6;
    p->counters.tile_rows = Ps.tile_rows; p->counters.grid = grid; p->counters.lds_bytes = (int32_t)Ps.lds_bytes;
    if (tabled) {
      // a sharded job's partial table: its flags (segment overflow, a key outside the ranges, the evaluation-error word) travel in the
      // chunks' headers to every rank, which all see them after the exchange (ssgpu_plan_fold_dense); nothing is read back here
      HIP_TRY(c, ssgpu_launch_dense_headers(ex.dense_table, ex.dense.n_chunks, ex.dense.chunk_bytes, ex.goverflow.as<unsigned int>(), ex.error_flag.as<unsigned int>(), c->stream));
      p->counters.n_launches += 1;
      ex.out_rows = 0;
      return SSGPU_OK;
    }
    HIP_TRY(c, ex.fb_host.ensure(16));
    uint32_t* fb = static_cast<uint32_t*>(ex.fb_host.p);   // [0] a partition outgrew its LDS table, [1] a segment ran full
    HIP_TRY(c, hipMemcpyAsync(fb, ex.goverflow.p, 16, hipMemcpyDeviceToHost, c->stream));
    if (attempt == 0 && ex.steady >= 2 && p->lazy_feedback && !c->debug_timing && tail_runs_without_host(p, si)) {
      // steady state: this shape held the last runs -- the flags are looked at lazily (settle_plan), no synchronise here
      { const int rc = record_feedback(c, ex); if (rc != SSGPU_OK) return rc; }
      ex.fb_pending = 2; p->deferred = true;
      return extract_groups(p, st, ex, capacity, ng, in, row_id_base, extra);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (attempt == 0 && !fb[0] && !fb[1] && !fb[3]) ++ex.steady; else ex.steady = 0;
    if (dense && trace_on()) fprintf(stderr, "[ssgpu trace] dense run: rows %lld slots %llu np %u cap %u resident %d plain %d seg_cap %llu fb %u %u %u %u\n", (long long)in.rows, (unsigned long long)ex.dense.slots, NP, C, (int)resident, (int)plain, (unsigned long long)seg_cap, fb[0], fb[1], fb[2], fb[3]);
    if (dense && fb[3]) {
      // a key outside the ranges the table was laid out for: look at THIS input's ranges, widen to the union, lay the table out again
      ++ex.dense.widened; ++ex.last_reruns;
      bool ok = !ex.dense.fixed && ex.dense.widened <= 8;
      if (ok) { const int rc = dense_find_ranges(p, st, ex, in); if (rc != SSGPU_OK) return rc; ok = dense_configure(c, st, ex, 1, false, in.rows); }
      if (!ok) { ex.dense.on = false; ex.dense.failed = !ex.dense.fixed; *fallback = true; if (ex.dense.fixed) { c->err = "a group key lies outside the dense ranges this plan was given (ssgpu_plan_set_dense)"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; } return SSGPU_OK; }
      return run_group_agg_partitioned(p, si, in, row_id_base, fallback);
    }
    if (dense && fb[0]) { ex.dense.on = false; ex.dense.failed = true; *fallback = true; return SSGPU_OK; }
    // (dense && fb[1]: rows pile up on a few slots -- a key's NULLs, a popular value.  The segments grow to what this input needs, below,
    //  up to x16; beyond that the hashed shapes take over, which aggregate heavy hitters apart)
    if (c->debug_timing) fprintf(stderr, "[ssgpu debug] group stage: partitioned, %u partitions x %u entries, grid %d, segments of %llu records (%u B), table overflow=%u segment overflow=%u\n",
                                 NP, C, grid, (unsigned long long)seg_cap, st.part_rec_bytes, fb[0], fb[1]);
    if (slab && (fb[0] || fb[1])) {   // more groups than one LDS table holds after all: hash partitions
      ex.part_slab = false; ex.part_slab_failed = true; ++ex.last_reruns;
      return run_group_agg_partitioned(p, si, in, row_id_base, fallback);
    }
    if (fb[1]) {   // skewed keys: larger segments (memory permitting), else the direct path
      if (ex.part_seg_growth >= 64) { *fallback = true; return SSGPU_OK; }
      if (plain && !dense && ex.hot_sampled_run != p->n_runs) {
        // Skewed keys?  Look at a sample of the rows before making every segment larger: a few keys that hold a large share of
        // the rows (each would fill ONE partition) are taken out of the partitions altogether and aggregated on their own
        // (ssgpu_hot_keys_kernel -> hot_only resident pass + a scatter that skips them), and the rest fits the segments as sized.
        ex.hot_sampled_run = p->n_runs;
        PlainScatterParams S; fill_plain_source(S);
        HIP_TRY(c, ex.hot_out.ensure((1 + 2 * SSGPU_HOT_MAX) * 8));
        const uint64_t n_sample = (uint64_t)std::min<int64_t>(in.rows, (int64_t)1 << 18);
        // "hot": at least a quarter of a partition's expected share of the sample
        const uint32_t min_count = (uint32_t)std::max<uint64_t>(n_sample / (4ull * NP), 16);
        HIP_TRY(c, ssgpu_launch_hot_keys(S, n_sample, min_count, ex.hot_out.as<unsigned long long>(), c->stream));
        uint64_t found[1 + 2 * SSGPU_HOT_MAX];
        HIP_TRY(c, hipMemcpyAsync(found, ex.hot_out.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        ex.hot_n = (uint32_t)std::min<uint64_t>(found[0], SSGPU_HOT_MAX);
        for (uint32_t h = 0; h < ex.hot_n; ++h) ex.hot_keys[h] = found[1 + 2 * h];
        if (c->debug_timing) fprintf(stderr, "[ssgpu debug] group stage: %u heavy-hitter key(s) in a sample of %llu rows (threshold %u)\n", ex.hot_n, (unsigned long long)n_sample, min_count);
        if (ex.hot_n > 0) continue;   // again, with the heavy hitters (of THIS input: an earlier run's list is replaced) handled apart
      }
      if (plain) {
        // the plain scatter's segment counters kept counting past the end: the fullest one says what this input needs.
        // One step to that size -- or, when such segments would not fit in a quarter of the free memory (one group holds
        // a large part of the rows), straight to the direct shape instead of three ever larger attempts (measured on 100 M
        // rows with 30 % in one group: 1.1 s of reruns and an 85 GB allocation before this, 35 ms now)
        std::vector<uint32_t> counts(n_segs);
        HIP_TRY(c, hipMemcpy(counts.data(), ex.part_hist.p, n_segs * 4, hipMemcpyDeviceToHost));
        uint32_t fullest = 0;
        for (uint32_t v : counts) fullest = std::max(fullest, v);
        uint32_t growth = ex.part_seg_growth;
        while (growth < 64u && (double)seg_cap / (double)ex.part_seg_growth * (double)growth < (double)fullest * 1.1) growth *= 4u;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        free_b += g_pool.parked(c->device);        // parked blocks are given back when an allocation needs them (DevBuf::ensure)
        const double need = (double)n_segs * ((double)seg_cap / (double)ex.part_seg_growth * (double)growth) * (double)st.part_rec_bytes;
        if ((double)seg_cap / (double)ex.part_seg_growth * (double)growth < (double)fullest * 1.1 || need > ((double)free_b + (double)ex.part_recs.cap) * 0.25 || (dense && growth > 16u)) {
          if (dense) { ex.dense.on = false; ex.dense.failed = true; ex.part_seg_growth = 1; }
          *fallback = true; return SSGPU_OK;
        }
        ex.part_seg_growth = std::max(growth, ex.part_seg_growth * 4u);
        continue;
      }
      ex.part_seg_growth *= 4;
      continue;
    }
    if (!fb[0]) return extract_groups(p, st, ex, capacity, ng, in, row_id_base, extra);
    if (ex.part_n >= 8192) break;
    ex.part_n *= 2;   // a partition held more groups than its LDS table: partition finer and rerun
  }
  *fallback = true;
  return SSGPU_OK;
}

int run_group_agg(ssgpu_plan* p, size_t si, const InCols& in, int64_t row_id_base, bool scout = false) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  const uint32_t ng = (uint32_t)std::max(st.n_gaggs, 1);
  if (!scout) ex.last_reruns = 0;
  // The execution shape follows run feedback, and the shape a plan starts in (the direct one) is the wrong one for a large
  // input with many groups: 54 ms for BASELINE config #3, whose steady shape takes 3.  A cursor that is drained once never
  // sees the steady shape -- so the first large run is preceded by a scout: the direct shape over a 1/64 prefix of the
  // rows (>= 1 M; an eighth of a smaller input, >= 128 K), only for its feedback (group-count estimate -> direct / partitioned /
  // one-table form).  Its result is thrown away; a prefix that is not representative (input sorted by key) just leaves the old
  // behaviour.  "Large" = group_scout_rows, 8 M rows.  With 1 M the first runs of 2 - 6 M-row inputs get 30 - 60 % faster (they
  // take the direct shape otherwise: 1.5 - 4.8 ms), but a prefix of an eighth over-estimates the group count of such inputs up
  // to eightfold and the plan then keeps too many partitions (or the one-table form where partitions are faster): steady runs
  // 1.5 - 3 x slower (profiles/r04_first_run.json).  A plan that is run once may set it lower; the default favours the plan that is run again.
  // Dense slots first: a plain stage whose key columns span small value ranges indexes its tables by the keys themselves -- no
  // hashing, no probe, no group-count estimate (the ranges bound it), the same slot for a group in every run and on every rank.
  // The ranges cost one pass over the key columns, once per plan (again only when a later input leaves them).
  if (!scout && !ex.dense.on && !ex.dense.failed && !ex.dense.checked && !ex.dense.fixed && in.rows >= std::max<int64_t>(c->dense_min_rows, 1) && dense_eligible(c, st)) {
    ex.dense.checked = true;
    { const int rc = dense_find_ranges(p, st, ex, in); if (rc != SSGPU_OK) return rc; }
    if (dense_configure(c, st, ex, 1, false, in.rows)) ex.dense.on = true; else ex.dense.failed = true;
    if (c->debug_timing) fprintf(stderr, "[ssgpu debug] group stage: key ranges span %llu dense slots -> %s\n", (unsigned long long)ex.dense.slots, ex.dense.on ? (ex.dense.resident ? "dense, one table" : "dense partitions") : "hashed");
  }
  if (!scout && ex.dense.on) {
    bool not_dense = false;
    const int rc = run_group_agg_partitioned(p, si, in, row_id_base, &not_dense);
    if (rc != SSGPU_OK || !not_dense) return rc;
    // the ranges did not make a usable table after all (keys too unevenly spread, a segment that would not fit): the hashed shapes
    ex.dense.on = false; if (!ex.dense.fixed) ex.dense.failed = true;
    ex.part_n_chosen = false; ex.part_slab = false; ex.steady = 0;
  }
  if (!scout && !ex.scouted && c->group_scout != 0 && c->group_partition == 1 && !ex.group_partitioned && !st.part_scatter.empty() &&
      in.rows >= std::max<int64_t>(c->group_scout_rows, (int64_t)1 << 18)) {
    ex.scouted = true; ex.scout_full_rows = in.rows;
    InCols prefix = in;
    prefix.rows = in.rows >= ((int64_t)8 << 20) ? std::max<int64_t>(in.rows / 64, (int64_t)1 << 20) : std::max<int64_t>(in.rows / 8, (int64_t)1 << 17);
    const int rc = run_group_agg(p, si, prefix, row_id_base, true);
    if (rc != SSGPU_OK) return rc;
    ex.steady = 0;
  }
  if ((ex.group_partitioned || c->group_partition == 2) && !st.part_scatter.empty()) {
    bool fallback = false;
    const int rc = run_group_agg_partitioned(p, si, in, row_id_base, &fallback);
    if (rc != SSGPU_OK || !fallback) return rc;
    // heavily skewed keys / too many groups per partition: the direct path (global table behind the LDS table) always works
    ex.group_partitioned = false; ex.group_local = true; ex.part_failed = true; ex.steady = 0;
  }
  if (ex.capacity == 0) ex.capacity = p->group_capacity_hint ? p->group_capacity_hint : (uint32_t)c->group_capacity;
  ex.last_group_shape = 0; ex.last_plain_scatter = false;
  for (int attempt = 0; attempt < 8; ++attempt) {
    if (attempt) ++ex.last_reruns;
    const size_t slots = (size_t)ex.capacity + 1;
    HIP_TRY(c, ex.gkeys.ensure(slots * 8));
    HIP_TRY(c, ex.gacc.ensure(slots * ng * 8));
    HIP_TRY(c, ex.gcnt.ensure(slots * ng * 4));
    HIP_TRY(c, ex.goverflow.ensure(16));
    HIP_TRY(c, ex.total.ensure(16));
    HIP_TRY(c, ex.gpattern.ensure(ng * 8));
    HIP_TRY(c, ex.gmergeop.ensure(ng * 4));
    if (!ex.pattern_ready) {
      std::vector<uint64_t> pattern(ng, 0);
      std::vector<uint32_t> mop(ng, VM_MERGE_ADD_U64);
      for (size_t i = 0; i < st.group_acc_init.size(); ++i) pattern[i] = st.group_acc_init[i];
      for (size_t i = 0; i < st.group_merge_op.size(); ++i) mop[i] = st.group_merge_op[i];
      HIP_TRY(c, hipMemcpy(ex.gpattern.p, pattern.data(), ng * 8, hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(ex.gmergeop.p, mop.data(), ng * 4, hipMemcpyHostToDevice));
      ex.pattern_ready = true;
    }
    {
      GroupInitParams I; memset(&I, 0, sizeof(I));
      I.keys = ex.gkeys.as<unsigned long long>(); I.n_keys = slots;
      I.acc = ex.gacc.as<unsigned long long>(); I.pattern = ex.gpattern.as<unsigned long long>(); I.ng = ng; I.n_acc = (unsigned long long)slots * ng;
      I.cnt = ex.gcnt.as<unsigned int>(); I.n_cnt = (unsigned long long)slots * ng;
      I.z[0] = ex.goverflow.as<unsigned int>(); I.nz[0] = 4;
      I.z[1] = ex.error_flag.as<unsigned int>(); I.nz[1] = 1;
      I.z[3] = ex.total.as<unsigned int>(); I.nz[3] = 4;   // the extraction's row count, ticket and gave-up flag
      HIP_TRY(c, ssgpu_launch_group_init(I, c->stream));
    }
    VmParams P;
    fill_params(&P, st.main, ex.lay, ex.prog_main, ex.n_instr_main, in, row_id_base);
    apply_joins(p, ex, st.main, &P);
    P.error_flag = ex.error_flag.as<unsigned int>();
    P.group.keys = ex.gkeys.as<unsigned long long>();
    P.group.acc = ex.gacc.as<unsigned long long>();
    P.group.cnt = ex.gcnt.as<unsigned int>();
    P.group.overflow = ex.goverflow.as<unsigned int>();
    P.group.stats = ex.goverflow.as<unsigned int>() + 1;
    P.group.capacity_mask = ex.capacity - 1;
    P.group.n_gaggs = ng;
    P.group.acc_init = ex.gpattern.as<unsigned long long>();
    P.group.merge_op = ex.gmergeop.as<unsigned int>();
    // workgroup-private pre-aggregation table behind the program's LDS registers: as many
    // entries as the LDS share of `group_wgs` resident workgroups per CU leaves room for
    bool any_cnt = false;
    for (auto& a : st.aggs) any_cnt = any_cnt || a.has_cnt;
    const uint32_t lstride = ng | 1u;   // odd word stride between LDS entries (bank conflicts, see VmGroupTable)
    const uint32_t entry = 8u + lstride * 8u + (any_cnt ? lstride * 4u : 0u);
    const uint32_t base = (ex.lay.lds_bytes + 15u) & ~15u;
    auto local_capacity_for = [&](int wgs) -> uint32_t {
      const uint32_t share = (160u * 1024u) / (uint32_t)wgs;
      if (share < base + 64u + 16u * entry) return 0u;
      return std::min<uint32_t>((share - base - 64u) / entry, 8192u);
    };
    uint32_t lcap = (c->group_local && ex.group_local) ? local_capacity_for(ex.group_wgs) : 0u;
    const uint32_t lsub = (uint32_t)std::max(ex.group_sub, 1);
    lcap = lcap / lsub * lsub;
    P.group.local_capacity = lcap;
    P.group.local_sub = lsub;
    P.group.local_sub_capacity = lcap / lsub;
    P.group.local_stride = lstride;
    if (lcap) {
      P.group.local_keys_off = base;
      P.group.local_acc_off = base + lcap * 8u;
      P.group.local_cnt_off = any_cnt ? base + lcap * 8u + lcap * lstride * 8u : VM_NONE;
      P.lds_bytes = base + lcap * entry;
    }
    int grid;
    {
      ProgramLayout Lg = ex.lay; Lg.lds_bytes = P.lds_bytes;
      const int64_t saved = c->wgs_per_cu;
      if (lcap) c->wgs_per_cu = std::min<int64_t>(saved, ex.group_wgs);
      grid = grid_for(c, Lg, P.n_tiles);
      c->wgs_per_cu = saved;
    }
    ex.grid = grid;
    p->counters.tile_rows = P.tile_rows; p->counters.grid = grid; p->counters.lds_bytes = (int32_t)P.lds_bytes;
    { int rc = attach_pc_profile(c, ex, &P); if (rc != SSGPU_OK) return rc; }
    if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
    HIP_TRY(c, launch_main(p, st, ex, P, ex.lay.K, grid));
    if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
    { int rc = print_pc_profile(c, ex, st.main, P.n_instr); if (rc != SSGPU_OK) return rc; }
    if (c->debug_timing) fprintf(stderr, "[ssgpu debug] group stage: wgs/CU=%d local entries=%u sub-tables=%u grid=%d lds=%u\n", ex.group_wgs, lcap, lsub, grid, P.lds_bytes);
    p->counters.n_launches += 5;
    HIP_TRY(c, ex.fb_host.ensure(16));
    uint32_t* fb = static_cast<uint32_t*>(ex.fb_host.p);   // overflow flag, rows that bypassed the local table, max local occupancy
    HIP_TRY(c, hipMemcpyAsync(fb, ex.goverflow.p, 16, hipMemcpyDeviceToHost, c->stream));
    if (!scout && attempt == 0 && ex.steady >= 2 && p->lazy_feedback && !c->debug_timing && tail_runs_without_host(p, si)) {   // (a scout run exists for its feedback: always read)
      { const int rc = record_feedback(c, ex); if (rc != SSGPU_OK) return rc; }
      ex.fb_pending = 1; p->deferred = true;   // steady state: looked at lazily (settle_plan)
      break;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint32_t overflow = fb[0];
    if (trace_on()) fprintf(stderr, "[ssgpu trace] group run: rows %lld lcap %u overflow %u misses %u occupancy %u grid %d tiles %lld tile_rows %d steady %d scout %d\n", (long long)in.rows, lcap, overflow, fb[1], fb[2], grid, (long long)P.n_tiles, (int)P.tile_rows, ex.steady, (int)scout);
    const int shape_before[5] = {ex.group_wgs, ex.group_local ? 1 : 0, ex.group_partitioned ? 1 : 0, (int)ex.part_slab, ex.group_sub};
    if (!lcap && !overflow && !scout && c->group_partition && !st.part_scatter.empty() && !ex.part_failed && st.plain.ok && c->part_plain != 0 && in.rows >= (1 << 16)) {
      // No table on chip at all (an entry of this stage's many aggregates is too wide for one): every row is an entry's worth of
      // global atomics -- the merge of a sharded job's partial tables: 1e5 rows x 16 values, 0.10 ms.  Partitions' LDS tables take
      // the same rows in a fraction of that; nothing is known about the group count, so they are sized for one group per row
      // -- an upper bound, which may load the tables to twice the usual share (0.8): half the bound goes in as the estimate.
      ex.group_partitioned = true; ex.part_groups_est = (double)in.rows * 0.5; ex.part_slab = false;
    }
    if (lcap && !overflow) {
      // feedback for the next run of this plan: the largest residency whose table still holds
      // every group of a workgroup at <= 75% load; a table most rows bypass is switched off
      if (fb[1] == 0) {
        const uint32_t groups = std::max<uint32_t>((fb[2] + lsub - 1u) / lsub, 1u);  // per workgroup
        int best = 1;
        for (int w = 4; w >= 1; --w) if (local_capacity_for(w) * 3u >= 4u * groups) { best = w; break; }
        ex.group_wgs = best;
        // (splitting the table into per-lane-group sub-tables was measured: 1.5 -> 2.1 ms on an
        //  8-group query; same-address LDS atomics are not the bottleneck, so group_sub stays 1)
        // No row missed its table -- but a table that ends up holding (nearly) one group per row the workgroup saw has reduced
        // nothing: every row goes on to the global table as an entry's worth of atomics (the merge of a sharded job's partial
        // tables: 1e5 rows, every one its own group, 0.10 ms of atomics).  Partitions' LDS tables do that merge on chip.
        const double rows_per_wg = (double)((P.n_tiles + grid - 1) / grid) * (double)P.tile_rows;
        if ((double)fb[2] * 2.0 >= rows_per_wg && c->group_partition && !st.part_scatter.empty() && !ex.part_failed && st.plain.ok && c->part_plain != 0 &&
            in.rows >= (1 << 16)) {
          const double groups_est = std::min((double)in.rows, (double)fb[2] * (double)grid);
          const uint32_t full = (159u * 1024u - (entry + 1025u * 4u + 128u)) / entry;
          ex.group_partitioned = true; ex.part_groups_est = groups_est;
          ex.part_slab = c->group_slab != 0 && groups_est * 1.08 <= (double)full;
        }
      } else {
        // some rows missed the (full) table.  With G >> C uniformly hit groups a fraction C/G of
        // the rows finds its group in the table, so G ~= C * rows / (rows - bypassed): size the
        // next run for that estimate in one step -- a bigger table at a lower residency if the
        // groups fit on chip, hash partitioning of the rows if not.
        const double rows = (double)std::max<int64_t>(in.rows, 1);
        const double hit = std::max(rows - (double)fb[1], 1.0);
        const double groups = std::max<double>((double)std::max(fb[2], lcap) * rows / hit, (double)fb[2]);
        int best = 0;
        for (int w = 4; w >= 1; --w) if ((double)local_capacity_for(w) * 0.9 >= groups) { best = w; break; }
        if (trace_on()) fprintf(stderr, "[ssgpu trace] group feedback: rows %lld misses %u groups %u est %.0f best %d wgs %d part_scatter %d part_failed %d partitioned %d\n", (long long)in.rows, fb[1], fb[2], groups, best, ex.group_wgs, (int)!st.part_scatter.empty(), (int)ex.part_failed, (int)ex.group_partitioned);
        if (best > 0 && best != ex.group_wgs) ex.group_wgs = best;
        else if (best == 0 || (best == ex.group_wgs && (double)fb[1] * 4.0 >= rows)) {
          // (a plain stage's scatter is its own kernel, worth it from 64 K rows: the merge of a sharded job's partial tables --
          //  1e5 rows, every one its own group -- takes 150 us through the global atomics and 25 us through partitions)
          if (c->group_partition && !st.part_scatter.empty() && !ex.part_failed && in.rows >= (st.plain.ok && c->part_plain ? (1 << 16) : (1 << 20))) {
            ex.group_partitioned = true; ex.part_groups_est = groups;
            // few enough groups for ONE whole-LDS table (with head room for the estimate): slabs of rows instead of hash partitions
            const uint32_t full = (159u * 1024u - (entry + 1025u * 4u + 128u)) / entry;
            ex.part_slab = c->group_slab != 0 && groups * 1.08 <= (double)full;   // (a nearly full table probes longer; it still beats re-partitioning)
          }
          else if ((double)fb[1] * 2.0 >= rows) ex.group_local = false;
        }
      }
    }
    {
      const int shape_after[5] = {ex.group_wgs, ex.group_local ? 1 : 0, ex.group_partitioned ? 1 : 0, (int)ex.part_slab, ex.group_sub};
      if (attempt == 0 && !overflow && memcmp(shape_before, shape_after, sizeof(shape_before)) == 0) { ++ex.steady; ex.steady_bypass = fb[1]; }
      else ex.steady = 0;
    }
    if (scout) {
      // The scout's own answer: every group of the prefix sits in the global table now (rows that missed the LDS table
      // were inserted there, the LDS tables were merged into it), so the prefix's group count is exact -- the hit-rate
      // estimate above assumes that a workgroup sees many more rows than there are groups, which a prefix does not give.
      double est;
      if (overflow) est = (double)ex.capacity * 4.0;
      else {
        const size_t nslots = (size_t)ex.capacity + 1;
        const int ntile = (int)((nslots + 511) / 512);
        HIP_TRY(c, ex.tile_counts.ensure((size_t)ntile * 4));
        HIP_TRY(c, ex.tile_offsets.ensure((size_t)ntile * 4));
        HIP_TRY(c, ex.total.ensure(16));
        GroupExtractParams G;
        memset(&G, 0, sizeof(G));
        G.keys = ex.gkeys.as<unsigned long long>(); G.acc = ex.gacc.as<unsigned long long>(); G.cnt = ex.gcnt.as<unsigned int>();
        G.capacity = ex.capacity; G.n_gaggs = ng; G.tile_offsets = ex.tile_offsets.as<unsigned int>();
        HIP_TRY(c, ssgpu_launch_group_count(G, ex.tile_counts.as<uint32_t>(), c->stream));
        HIP_TRY(c, ssgpu_launch_scan_counts(ex.tile_counts.as<uint32_t>(), ex.tile_offsets.as<uint32_t>(), ntile, ex.total.as<uint64_t>(), c->stream));
        uint64_t seen = 0;
        HIP_TRY(c, hipMemcpyAsync(&seen, ex.total.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // most prefix rows brought a new group: the groups grow with the rows -- scale to the whole input (an upper bound)
        est = (double)seen * 8.0 >= (double)in.rows ? (double)seen * ((double)ex.scout_full_rows / (double)std::max<int64_t>(in.rows, 1)) : (double)seen;
      }
      // (a stage without a table on chip -- entries too wide -- has only the partitions to go to, and only in the plain form)
      const bool only_partitions = !lcap && st.plain.ok && c->part_plain != 0 && !st.part_scatter.empty();
      if ((lcap || only_partitions) && c->group_partition && !ex.part_failed) {
        if (est > (lcap ? (double)local_capacity_for(1) * 0.75 : 0.0)) {
          uint32_t full = 0;
          { const uint32_t stw = ng | 1u, pentry = 8u + stw * 8u + (any_cnt ? stw * 4u : 0u); full = (159u * 1024u - (pentry + 1025u * 4u + 128u)) / pentry; }
          ex.group_partitioned = true; ex.part_groups_est = est;
          ex.part_slab = c->group_slab != 0 && est * 1.08 <= (double)full;
        } else {
          ex.group_partitioned = false;
          for (int w = 4; w >= 1; --w) if ((double)local_capacity_for(w) * 0.75 >= est) { ex.group_wgs = w; break; }
        }
      }
      if (c->debug_timing) fprintf(stderr, "[ssgpu debug] group stage scout: %lld of %lld rows, estimate %.0f groups -> %s\n", (long long)in.rows, (long long)ex.scout_full_rows, est,
                                   ex.group_partitioned ? (ex.part_slab ? "one-table form" : "hash partitions") : "direct");
      if (overflow && (uint64_t)ex.capacity < (1ull << 30)) ex.capacity *= 4;
      return SSGPU_OK;
    }
    if (!overflow) break;
    // table too small for this input: regrow x4 and run again (the reference grows its
    // Aggregator x2 on demand, aggregate_groups.cc:372-402)
    if ((uint64_t)ex.capacity >= (1ull << 30)) { c->err = "group table overflow"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
    ex.capacity *= 4;
  }
  return extract_groups(p, st, ex, ex.capacity, ng, in, row_id_base);
}

int sort_kind_of(int dtype) {   // 0 unsigned, 1 signed, 2 float32, 3 float64
  switch (dtype) {
    case SSGPU_INT32: case SSGPU_INT64: case SSGPU_DATE: case SSGPU_DATETIME: return 1;
    case SSGPU_FLOAT: return 2;
    case SSGPU_DOUBLE: return 3;
    default: return 0;
  }
}

int run_sort(ssgpu_plan* p, size_t si, const InCols& in) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  const uint64_t n = (uint64_t)in.rows;
  if (n >= (1ull << 32)) { c->err = "Sort: more than 2^32 rows per GPU is not supported yet"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  int rc = ensure_out_cols(c, st, ex, in.rows);
  if (rc != SSGPU_OK) return rc;
  const uint32_t nt = ssgpu_sort_tiles(n);
  HIP_TRY(c, ex.skeys_a.ensure(std::max<uint64_t>(n, 1) * 8)); HIP_TRY(c, ex.skeys_b.ensure(std::max<uint64_t>(n, 1) * 8));
  HIP_TRY(c, ex.sidx_a.ensure(std::max<uint64_t>(n, 1) * 4)); HIP_TRY(c, ex.sidx_b.ensure(std::max<uint64_t>(n, 1) * 4));
  HIP_TRY(c, ex.total2.ensure(16));
  // one-sweep scratch: digit histograms + their scans, per-(tile, digit) status words (zeroed when (re)allocated: an
  // all-zero word reads as "not ready" in every epoch), one tile ticket per pass, the "look-back gave up" flag
  HIP_TRY(c, ex.shist.ensure(8 * 256 * 4)); HIP_TRY(c, ex.soffs.ensure(8 * 256 * 4));
  {
    const size_t need = (size_t)std::max<uint32_t>(nt, 1) * 256 * 8;
    if (need > ex.sstatus.cap || !ex.sstatus.p) { HIP_TRY(c, ex.sstatus.ensure(need)); HIP_TRY(c, hipMemsetAsync(ex.sstatus.p, 0, ex.sstatus.cap, c->stream)); }
  }
  HIP_TRY(c, ex.sticket.ensure(64 * 4));
  HIP_TRY(c, hipMemsetAsync(ex.sticket.p, 0, 64 * 4, c->stream));
  uint32_t n_pass = 0;   // tickets [0, 61], "a tie run was too long" flag at [62], "look-back gave up" flag at [63]
  int sort_mode = 0;     // 0 plain LSD passes, 1 high digits + tie fix-up, 2 one-word (high half | row id) keys; +16: tie runs too long, all digits after all
  uint64_t* ka = ex.skeys_a.as<uint64_t>(); uint64_t* kb = ex.skeys_b.as<uint64_t>();
  uint32_t* ia = ex.sidx_a.as<uint32_t>(); uint32_t* ib = ex.sidx_b.as<uint32_t>();
  // The major key's column can be read back from the sorted keys when its transform is a bijection (integer
  // kinds, no NULLs): no gather for it -- and when it is the ONLY output column, no row ids at all.
  const SortKey major = st.sort_keys.empty() ? SortKey{0, 0} : st.sort_keys[0];
  const int major_kind = st.sort_keys.empty() ? 99 : sort_kind_of(st.in_schema[major.col].dtype);
  const bool major_direct0 = !st.sort_keys.empty() && major_kind <= 1 && dtype_width(st.in_schema[major.col].dtype) >= 4 &&
                             !(st.in_schema[major.col].nullable && in.cols[major.col].is_null);
  bool major_direct = major_direct0;
  bool keys_only = major_direct0 && st.sort_keys.size() == 1;
  for (int col : st.sort_out_cols) keys_only = keys_only && col == major.col;
  if (keys_only) ia = ib = nullptr;
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
  // ONE read of a key column: transformed keys, OR / AND of all keys (digits on which every key agrees are skipped) and
  // the histograms of all digits with their exclusive scans
  auto load_key = [&](int k, int kind, int null_pass, const uint32_t* idx, uint64_t* varying, uint64_t* compact_out = nullptr) -> int {
    const SortKey& sk = st.sort_keys[k];
    const unsigned long long init[2] = {0ull, ~0ull};
    HIP_TRY(c, hipMemcpyAsync(ex.total2.p, init, 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(ex.shist.p, 0, 8 * 256 * 4, c->stream));
    HIP_TRY(c, ssgpu_launch_sort_load_keys_hist(ka, idx, in.cols[sk.col].data, in.cols[sk.col].is_null, (uint32_t)dtype_width(st.in_schema[sk.col].dtype), kind,
                                                sk.order == SSGPU_DESCENDING, null_pass, n, ex.total2.as<unsigned long long>(), ex.shist.as<uint32_t>(),
                                                ex.soffs.as<uint32_t>(), c->stream, compact_out));
    unsigned long long bits[2];
    HIP_TRY(c, hipMemcpyAsync(bits, ex.total2.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *varying = bits[0] ^ bits[1];
    p->counters.n_launches += 2;
    return SSGPU_OK;
  };
  // The first key processed (the least significant one) is loaded before the payload layout is fixed: a wide key whose
  // high half separates almost all rows is sorted as ONE word per row -- (high half << 32 | row id), see
  // ssgpu_sort_load_keys_hist_kernel's compact_out -- which needs the key column inside the payload records (its low half is not in the
  // sorted words) when it is also the major key.
  const int k_first = (int)st.sort_keys.size() - 1;
  bool first_loaded = false, compact = false;
  uint64_t first_varying = 0;
  if (k_first >= 0 && n >= (1u << 16) && !keys_only && c->sort_hybrid && c->sort_compact && c->sort_records && c->sort_hi_digits == 4) {
    const SortKey& sk = st.sort_keys[k_first];
    if (dtype_width(st.in_schema[sk.col].dtype) == 8 && !(in.cols[sk.col].is_null && st.in_schema[sk.col].nullable)) {
      // (the load also writes the one-word keys, into the second key buffer: cheaper than a pass of their own when they are used)
      rc = load_key(k_first, sort_kind_of(st.in_schema[sk.col].dtype), 0, nullptr, &first_varying, kb); if (rc != SSGPU_OK) return rc;
      first_loaded = true;
      compact = (first_varying & 0xFFFFFFFFull) != 0;
      for (uint32_t pass = 4; pass < 8; ++pass) compact = compact && ((first_varying >> (pass * 8)) & 0xFFull) != 0;
      if (compact && k_first == 0) major_direct = false;
    }
  }
  // Payload: with three or more gathered columns the rows travel as fixed-stride records (ssgpu_sort_pack_kernel):
  // the sorted order then fetches one record per row instead of one 64-byte sector per row PER COLUMN.
  SortRecParams R;
  bool use_records = false;
  auto build_layout = [&]() {
    memset(&R, 0, sizeof(R));
    uint32_t off = 0, nf = 0, gathered = 0;
    for (uint32_t wsel : {8u, 4u, 1u}) {
      for (size_t i = 0; i < st.sort_out_cols.size(); ++i) {
        const int col = st.sort_out_cols[i];
        if (major_direct && col == major.col) continue;
        if (ex.out[i].width == wsel && nf < SSGPU_SORT_MAX_FIELDS) {
          R.fields[nf].src = in.cols[col].data; R.fields[nf].dst = ex.out[i].data.p; R.fields[nf].off = off; R.fields[nf].width = wsel; ++nf; off += wsel;
          if (wsel == 8 || ex.out[i].width == wsel) ++gathered;
        }
        if (wsel == 1 && ex.out[i].nullable && nf < SSGPU_SORT_MAX_FIELDS) {   // NULL flags ride with the 1-byte fields
          R.fields[nf].src = in.cols[col].is_null; R.fields[nf].dst = ex.out[i].nulls.p; R.fields[nf].off = off; R.fields[nf].width = 1; ++nf; off += 1;
        }
      }
    }
    uint32_t payload_cols = 0;
    for (size_t i = 0; i < st.sort_out_cols.size(); ++i) if (!(major_direct && st.sort_out_cols[i] == major.col)) ++payload_cols;
    R.stride = (off + 15u) & ~15u; R.n_fields = nf; R.n = n;
    use_records = !keys_only && payload_cols >= 3 && R.stride <= 224u && nf < SSGPU_SORT_MAX_FIELDS && n > 0 && c->sort_records != 0;
    (void)gathered;
  };
  build_layout();
  if (compact && !use_records) { compact = false; major_direct = major_direct0; build_layout(); }   // the one-word form gathers through records
  if (use_records) {
    HIP_TRY(c, ex.srecs.ensure((size_t)n * R.stride + 16));
    R.recs = ex.srecs.p;
    HIP_TRY(c, ssgpu_launch_sort_pack(R, c->stream));
    p->counters.n_launches += 1;
  }
  if (!keys_only && !compact) HIP_TRY(c, ssgpu_launch_sort_iota(ia, n, c->stream));
  const uint64_t* compact_sorted = nullptr;   // the sorted (high half << 32 | row id) words when the record gather reads row ids from them
  // least significant key first; each key: value digits, then the NULL-order bit on top
  for (int k = (int)st.sort_keys.size() - 1; k >= 0 && n > 0; --k) {
    const SortKey& sk = st.sort_keys[k];
    const int dtype = st.in_schema[sk.col].dtype;
    const uint32_t w = (uint32_t)dtype_width(dtype);
    const uint8_t* nulls = in.cols[sk.col].is_null;
    // ONE read of the key column: transformed keys, OR / AND of all keys (digits on which every key agrees are
    // skipped) and the histograms of all digits with their exclusive scans
    auto load_and_profile = [&](int kind, int null_pass, uint64_t* varying) -> int { return load_key(k, kind, null_pass, ia, varying); };
    auto one_pass = [&](uint32_t digit) -> int {
      if (n_pass >= 62) { c->err = "Sort: too many radix passes in one stage"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
      HIP_TRY(c, ssgpu_launch_sort_onesweep(ka, ia, kb, ib, digit * 8, n, ex.soffs.as<uint32_t>() + digit * 256, ex.sstatus.as<unsigned long long>(),
                                            ex.sticket.as<uint32_t>() + n_pass, ++ex.sort_epoch, ex.sticket.as<uint32_t>() + 63, c->stream));
      ++n_pass;
      std::swap(ka, kb); std::swap(ia, ib);
      p->counters.n_launches += 1;
      return SSGPU_OK;
    };
    uint64_t varying = 0;
    if (k == k_first && first_loaded) varying = first_varying;   // loaded above, in row order (what iota row ids would have read)
    else { rc = load_and_profile(sort_kind_of(dtype), 0, &varying); if (rc != SSGPU_OK) return rc; }
    // A wide key (all eight digits vary) that is the FIRST key processed (the rows are still in input order, which the
    // stable tie-break relies on): sort by its high half and fix up the rare, short runs of equal high halves -- see
    // ssgpu_sort_fix_ties_kernel -- instead of the four low-digit passes.
    bool done = false, tie_runs_too_long = false;
    if (compact && k == k_first) {
      // one word per row: the four high digits with the keys-only kernel, then the tie runs by the low halves
      HIP_TRY(c, ex.skeys_c.ensure(std::max<uint64_t>(n, 1) * 8));
      uint64_t* kc = kb; uint64_t* kd = ex.skeys_c.as<uint64_t>();   // kb: written by the load above
      for (uint32_t digit = 4; digit < 8; ++digit) {
        if (n_pass >= 62) { c->err = "Sort: too many radix passes in one stage"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
        HIP_TRY(c, ssgpu_launch_sort_onesweep(kc, nullptr, kd, nullptr, digit * 8, n, ex.soffs.as<uint32_t>() + digit * 256, ex.sstatus.as<unsigned long long>(),
                                              ex.sticket.as<uint32_t>() + n_pass, ++ex.sort_epoch, ex.sticket.as<uint32_t>() + 63, c->stream));
        ++n_pass;
        std::swap(kc, kd);
      }
      uint32_t* flag = ex.sticket.as<uint32_t>() + 62;
      HIP_TRY(c, ssgpu_launch_sort_fix_ties_compact(kc, ka, n, flag, c->stream));
      uint32_t too_long = 0;
      HIP_TRY(c, hipMemcpyAsync(&too_long, flag, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      p->counters.n_launches += 6;
      if (!too_long) {
        done = true; sort_mode = 2;
        if (k > 0) HIP_TRY(c, ssgpu_launch_sort_extract_idx(ia, kc, n, c->stream));   // more significant keys follow: they permute (key, row id) pairs
        else compact_sorted = kc;
      } else {
        // long runs of equal high halves: the plain LSD order over all digits (the key array and the digit offsets are untouched)
        HIP_TRY(c, hipMemsetAsync(flag, 0, 4, c->stream));
        HIP_TRY(c, ssgpu_launch_sort_iota(ia, n, c->stream));
        compact = false; tie_runs_too_long = true; sort_mode = 2 + 16;
      }
    }
    if (!done && !tie_runs_too_long && c->sort_hybrid && w == 8 && k == (int)st.sort_keys.size() - 1 && (varying & 0xFFFFFFFFull) && !(nulls && st.in_schema[sk.col].nullable) &&
        n >= (1u << 16)) {
      // how many high digits: as few as keep the expected run of equal high parts short (n / 256^d <= 8 rows for
      // uniform keys: 3 digits up to 134 M rows), never fewer than 2 nor more than 4
      uint32_t hi_digits = 4;
      if (c->sort_hi_digits >= 2 && c->sort_hi_digits <= 4) hi_digits = (uint32_t)c->sort_hi_digits;
      else if (c->sort_hi_digits == 0) { hi_digits = 2; while (hi_digits < 4 && (double)n / std::pow(256.0, (double)hi_digits) > 8.0) ++hi_digits; }
      const uint32_t first_pass = 8 - hi_digits;
      bool high_busy = true;
      for (uint32_t pass = first_pass; pass < 8; ++pass) high_busy = high_busy && ((varying >> (pass * 8)) & 0xFFull) != 0;
      if (high_busy) {
        for (uint32_t pass = first_pass; pass < 8; ++pass) { rc = one_pass(pass); if (rc != SSGPU_OK) return rc; }
        uint32_t* flag = ex.sticket.as<uint32_t>() + 62;
        HIP_TRY(c, ssgpu_launch_sort_fix_ties(ka, ia, n, first_pass * 8, flag, c->stream));
        uint32_t too_long = 0;
        HIP_TRY(c, hipMemcpyAsync(&too_long, flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        p->counters.n_launches += 1;
        if (!too_long) {
          done = true; sort_mode = 1;
        } else {
          sort_mode = 1 + 16;
          // long runs of equal high halves: the plain LSD order over all digits, from scratch (the four passes used
          // both buffers as targets: reload the row ids and the keys)
          if (!keys_only) HIP_TRY(c, ssgpu_launch_sort_iota(ia, n, c->stream));
          uint64_t v2 = 0;
          rc = load_and_profile(sort_kind_of(dtype), 0, &v2); if (rc != SSGPU_OK) return rc;
        }
      }
    }
    for (uint32_t pass = 0; pass < w && !done; ++pass)
      if ((varying >> (pass * 8)) & 0xFFull) { rc = one_pass(pass); if (rc != SSGPU_OK) return rc; }
    if (nulls && st.in_schema[sk.col].nullable) {
      rc = load_and_profile(0, 1, &varying); if (rc != SSGPU_OK) return rc;
      if (varying & 1ull) { rc = one_pass(0); if (rc != SSGPU_OK) return rc; }
    }
  }
  for (size_t i = 0; i < st.sort_out_cols.size(); ++i) {
    const int col = st.sort_out_cols[i];
    if (major_direct && col == major.col && n > 0) {
      HIP_TRY(c, ssgpu_launch_sort_unkey(ex.out[i].data.p, ka, ex.out[i].width, major_kind, major.order == SSGPU_DESCENDING, n, c->stream));
      if (ex.out[i].nullable) HIP_TRY(c, hipMemsetAsync(ex.out[i].nulls.p, 0, n, c->stream));
      continue;
    }
    if (use_records) continue;
    HIP_TRY(c, ssgpu_launch_sort_gather(ex.out[i].data.p, ex.out[i].nullable ? ex.out[i].nulls.as<uint8_t>() : nullptr,
                                        in.cols[col].data, in.cols[col].is_null, ex.out[i].width, ia, n, c->stream));
  }
  if (use_records) {
    if (compact_sorted) HIP_TRY(c, ssgpu_launch_sort_gather_rec(R, reinterpret_cast<const uint32_t*>(compact_sorted), 2, c->stream));   // row id = low word
    else HIP_TRY(c, ssgpu_launch_sort_gather_rec(R, ia, 1, c->stream));
    p->counters.n_launches += 1;
  }
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
  ex.last_sort_passes = (int)n_pass; ex.last_sort_mode = sort_mode;
  if (n_pass) {   // the look-back never gives up on a healthy device; if it did, the order is wrong: fail loudly
    uint32_t stuck = 0;
    HIP_TRY(c, hipMemcpyAsync(&stuck, ex.sticket.as<uint32_t>() + 63, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stuck) { c->err = "Sort: a radix pass timed out waiting for a predecessor tile"; return SSGPU_ERROR_HIP; }
  }
  ex.out_rows = in.rows;
  return SSGPU_OK;
}

int run_clusters(ssgpu_plan* p, size_t si, const InCols& in, int64_t row_id_base) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  const uint64_t n = (uint64_t)in.rows;
  const uint32_t nk = (uint32_t)st.sort_keys.size();
  const uint32_t ng = (uint32_t)std::max(st.n_gaggs, 1);
  const void* kdata[16] = {nullptr}; const uint8_t* knulls[16] = {nullptr}; uint32_t kwidth[16] = {0};
  for (uint32_t k = 0; k < nk; ++k) {
    const int col = st.sort_keys[k].col;
    kdata[k] = in.cols[col].data; knulls[k] = in.cols[col].is_null; kwidth[k] = (uint32_t)dtype_width(st.in_schema[col].dtype);
  }
  const int ntile = (int)((n + 511) / 512);
  HIP_TRY(c, ex.tile_counts.ensure((size_t)std::max(ntile, 1) * 4)); HIP_TRY(c, ex.tile_offsets.ensure((size_t)std::max(ntile, 1) * 4));
  HIP_TRY(c, ex.total.ensure(8)); HIP_TRY(c, ex.seg_id.ensure(std::max<uint64_t>(n, 1) * 4));
  HIP_TRY(c, hipMemsetAsync(ex.total.p, 0, 8, c->stream));
  HIP_TRY(c, ssgpu_launch_cluster_count(kdata, knulls, kwidth, nk, n, ex.tile_counts.as<uint32_t>(), c->stream));
  HIP_TRY(c, ssgpu_launch_scan_counts(ex.tile_counts.as<uint32_t>(), ex.tile_offsets.as<uint32_t>(), ntile, ex.total.as<uint64_t>(), c->stream));
  uint64_t nseg = 0;
  HIP_TRY(c, hipMemcpyAsync(&nseg, ex.total.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int rc = ensure_out_cols(c, st, ex, (int64_t)nseg);
  if (rc != SSGPU_OK) return rc;
  void* okdata[16] = {nullptr}; uint8_t* oknulls[16] = {nullptr};
  for (uint32_t k = 0; k < nk; ++k) { okdata[k] = ex.out[k].data.p; oknulls[k] = ex.out[k].nullable ? ex.out[k].nulls.as<uint8_t>() : nullptr; }
  HIP_TRY(c, ssgpu_launch_cluster_assign(kdata, knulls, kwidth, nk, okdata, oknulls, n, ex.tile_offsets.as<uint32_t>(), ex.seg_id.as<uint32_t>(), c->stream));
  const size_t slots = (size_t)std::max<uint64_t>(nseg, 1);
  HIP_TRY(c, ex.gacc.ensure(slots * ng * 8)); HIP_TRY(c, ex.gcnt.ensure(slots * ng * 4)); HIP_TRY(c, ex.gpattern.ensure(ng * 8));
  if (!ex.pattern_ready) {
    std::vector<uint64_t> pattern(ng, 0);
    for (size_t i = 0; i < st.group_acc_init.size(); ++i) pattern[i] = st.group_acc_init[i];
    HIP_TRY(c, hipMemcpy(ex.gpattern.p, pattern.data(), ng * 8, hipMemcpyHostToDevice));
    ex.pattern_ready = true;
  }
  HIP_TRY(c, ssgpu_launch_fill_pattern_u64(ex.gacc.as<uint64_t>(), ex.gpattern.as<uint64_t>(), ng, slots * ng, c->stream));
  HIP_TRY(c, hipMemsetAsync(ex.gcnt.p, 0, slots * ng * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(ex.error_flag.p, 0, 4, c->stream));
  InCols ext = in;
  ssgpu_column segcol; segcol.data = ex.seg_id.p; segcol.is_null = nullptr;
  ext.cols.push_back(segcol);
  if (!st.distinct_cols.empty()) {
    ssgpu_column f; const int frc = distinct_flags(c, st, ex, in, &f); if (frc != SSGPU_OK) return frc;
    ext.cols.push_back(f);
  }
  VmParams P;
  fill_params(&P, st.main, ex.lay, ex.prog_main, ex.n_instr_main, ext, row_id_base);
  apply_joins(p, ex, st.main, &P);
  P.error_flag = ex.error_flag.as<unsigned int>();
  P.group.acc = ex.gacc.as<unsigned long long>();
  P.group.cnt = ex.gcnt.as<unsigned int>();
  const int grid = grid_for(c, ex.lay, P.n_tiles);
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
  HIP_TRY(c, launch_main(p, st, ex, P, ex.lay.K, grid));
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
  rc = ensure_rowid_tmp(c, st, ex, nseg);
  if (rc != SSGPU_OK) return rc;
  std::vector<GroupAggOut> outs(st.aggs.size());
  for (size_t j = 0; j < st.aggs.size(); ++j) {
    outs[j].data = st.aggs[j].gather_col >= 0 ? ex.rowid_tmp[j].p : ex.out[nk + j].data.p;
    outs[j].is_null = ex.out[nk + j].nullable ? ex.out[nk + j].nulls.as<uint8_t>() : nullptr;
    outs[j].s = st.aggs[j].slot; outs[j].out_kind = st.aggs[j].emit_kind; outs[j].has_cnt = st.aggs[j].has_cnt ? 1 : 0;
  }
  HIP_TRY(c, ssgpu_launch_dense_extract(ex.gacc.as<uint64_t>(), ex.gcnt.as<uint32_t>(), ng, nseg, outs.data(), (uint32_t)outs.size(), c->stream));
  rc = gather_first_last(p, st, ex, nk, in, row_id_base, nullptr, nseg);
  if (rc == SSGPU_OK && !st.seq_sums.empty()) rc = run_seq_sums(p, st, ex, in, ex.seg_id.as<uint32_t>());
  if (rc != SSGPU_OK) return rc;
  p->counters.n_launches += 6;
  ex.out_rows = (int64_t)nseg;
  return SSGPU_OK;
}

// NOT_UNIQUE hash join, second half (the previous stage materialised the kept lhs columns plus every
// row's run of matching rhs rows): scan the run counts, expand to (lhs row, rhs row) pairs, gather.
int run_join_expand(ssgpu_plan* p, size_t si, const InCols& in) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  if (si == 0 || p->exec[si - 1].jrows_sorted.empty()) { c->err = "join expansion without its index"; return SSGPU_ERROR_UNKNOWN; }
  StageExec& bx = p->exec[si - 1];
  const size_t join_id = bx.jrows_sorted.size() - 1;   // the multi join is the last join of the lhs pipeline
  const uint64_t n = (uint64_t)in.rows;
  const size_t n_in = in.cols.size();
  const uint32_t* run_start = static_cast<const uint32_t*>(in.cols[n_in - 2].data);
  const uint32_t* run_count = static_cast<const uint32_t*>(in.cols[n_in - 1].data);
  HIP_TRY(c, ex.jx_offsets.ensure(std::max<uint64_t>(n, 1) * 4)); HIP_TRY(c, ex.total.ensure(8));
  HIP_TRY(c, hipMemsetAsync(ex.total.p, 0, 8, c->stream));
  uint64_t n_out = 0;
  if (n > 0) {
    if (n >= (1ull << 31)) { c->err = "hash join: more than 2^31 lhs rows per GPU is not supported yet"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    HIP_TRY(c, ssgpu_launch_scan_counts(run_count, ex.jx_offsets.as<uint32_t>(), (int)n, ex.total.as<uint64_t>(), c->stream));
    HIP_TRY(c, hipMemcpyAsync(&n_out, ex.total.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (n_out >= (uint64_t)VM_NONE) { c->err = "hash join: the result has more than 2^32 rows"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  int rc = ensure_out_cols(c, st, ex, (int64_t)n_out);
  if (rc != SSGPU_OK) return rc;
  HIP_TRY(c, ex.jx_lhs_idx.ensure(std::max<uint64_t>(n_out, 1) * 4)); HIP_TRY(c, ex.jx_rhs_row.ensure(std::max<uint64_t>(n_out, 1) * 4));
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
  HIP_TRY(c, ssgpu_launch_join_expand(ex.jx_offsets.as<uint32_t>(), run_start, bx.jrows_sorted[join_id].as<uint32_t>(), n, n_out,
                                      ex.jx_lhs_idx.as<uint32_t>(), ex.jx_rhs_row.as<uint32_t>(), c->stream));
  for (size_t q = 0; q < st.join_out.size(); ++q) {
    const Stage::JoinOut& f = st.join_out[q];
    const void* src; const uint8_t* src_null; const uint32_t* idx;
    if (f.from_rhs) {
      src = p->aux_cols[f.col].data; src_null = p->desc.aux_schema[f.col].nullable ? p->aux_cols[f.col].is_null : nullptr;
      idx = ex.jx_rhs_row.as<uint32_t>();
    } else {
      src = in.cols[f.col].data; src_null = in.cols[f.col].is_null; idx = ex.jx_lhs_idx.as<uint32_t>();
    }
    HIP_TRY(c, ssgpu_launch_sort_gather(ex.out[q].data.p, ex.out[q].nullable ? ex.out[q].nulls.as<uint8_t>() : nullptr, src, src_null,
                                        ex.out[q].width, idx, n_out, c->stream));
  }
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
  p->counters.n_launches += 2 + (int)st.join_out.size();
  ex.out_rows = (int64_t)n_out;
  return SSGPU_OK;
}

// GroupAggregateOptions::max_unique_keys_in_result, last stage: the group table, sorted by first-seen row id (its last
// column), keeps rows [0, limit] and has every later row merged into row `limit` (Stage::fold_op)
int run_fold_tail(ssgpu_plan* p, size_t si, const InCols& in) {
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  if (st.fold_cut) {
    // BestEffortGroupAggregate: the first `capacity` groups in first-seen order ARE the view -- copied as they are -- and the
    // first-seen row id of the next group, the first input row whose key found no room (aggregate_groups.cc:362: the reference
    // truncates its input view there), is where the next view starts (ssgpu_plan_run_best_effort)
    const int64_t keep = std::min<int64_t>(in.rows, p->be_capacity);
    int rc = ensure_out_cols(c, st, ex, keep);
    if (rc != SSGPU_OK) return rc;
    if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
    for (size_t i = 0; i < st.out_schema.size() && keep > 0; ++i) {
      HIP_TRY(c, hipMemcpyAsync(ex.out[i].data.p, in.cols[i].data, (size_t)keep * ex.out[i].width, hipMemcpyDeviceToDevice, c->stream));
      if (ex.out[i].nullable) {
        if (st.in_schema[i].nullable && in.cols[i].is_null) HIP_TRY(c, hipMemcpyAsync(ex.out[i].nulls.p, in.cols[i].is_null, (size_t)keep, hipMemcpyDeviceToDevice, c->stream));
        else HIP_TRY(c, hipMemsetAsync(ex.out[i].nulls.p, 0, (size_t)keep, c->stream));
      }
    }
    if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
    p->be_cut = -1;
    if (in.rows > keep) {
      unsigned long long next = 0;
      HIP_TRY(c, hipMemcpyAsync(&next, static_cast<const unsigned long long*>(in.cols[st.in_schema.size() - 1].data) + keep, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      p->be_cut = (int64_t)next + p->be_base;
    }
    ex.out_rows = keep;
    return SSGPU_OK;
  }
  const int64_t keep = std::min<int64_t>(in.rows, st.fold_limit + 1);
  int rc = ensure_out_cols(c, st, ex, keep);
  if (rc != SSGPU_OK) return rc;
  auto kind_of = [](int dtype) {
    switch (dtype) {
      case SSGPU_INT32: case SSGPU_DATE: case SSGPU_STRING: return 0u; case SSGPU_UINT32: return 1u;
      case SSGPU_INT64: case SSGPU_DATETIME: return 2u; case SSGPU_UINT64: return 3u;
      case SSGPU_FLOAT: return 4u; case SSGPU_DOUBLE: return 5u; default: return 6u;
    }
  };
  std::vector<FoldTailColumn> cols(st.out_schema.size());
  for (size_t i = 0; i < cols.size(); ++i) {
    cols[i].src = in.cols[i].data; cols[i].src_nulls = st.in_schema[i].nullable ? in.cols[i].is_null : nullptr;
    cols[i].dst = ex.out[i].data.p; cols[i].dst_nulls = ex.out[i].nullable ? ex.out[i].nulls.as<uint8_t>() : nullptr;
    cols[i].op = (unsigned)st.fold_op[i]; cols[i].kind = kind_of(st.out_schema[i].dtype);
    const int by = i < st.fold_by.size() ? st.fold_by[i] : -1;
    cols[i].by = by >= 0 ? (const unsigned long long*)in.cols[by].data : nullptr;
    cols[i].by_nulls = by >= 0 && st.in_schema[by].nullable ? in.cols[by].is_null : nullptr;
  }
  HIP_TRY(c, ex.emit_descs.ensure(std::max<size_t>(cols.size(), 1) * sizeof(FoldTailColumn)));
  HIP_TRY(c, hipMemcpyAsync(ex.emit_descs.p, cols.data(), cols.size() * sizeof(FoldTailColumn), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (`cols` is a host temporary)
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom0, c->stream));
  HIP_TRY(c, ssgpu_launch_fold_tail(ex.emit_descs.as<FoldTailColumn>(), (unsigned)cols.size(), (unsigned long long)in.rows, (unsigned long long)st.fold_limit, c->stream));
  if (c->profile) HIP_TRY(c, hipEventRecord(p->ev_dom1, c->stream));
  p->counters.n_launches += 1;
  ex.out_rows = keep;
  return SSGPU_OK;
}

static const void* rows_word(const StageExec& ex) { return ex.out_rows_dev ? ex.out_rows_dev : ex.total.p; }
int stage_rows(ssgpu_plan* p, size_t si, int64_t* rows) {
  ssgpu_ctx* c = p->ctx; StageExec& ex = p->exec[si];
  if (ex.out_rows < 0) {
    uint64_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, rows_word(ex), 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ex.out_rows = (int64_t)total;
  }
  *rows = ex.out_rows;
  return SSGPU_OK;
}

int check_error_flags(ssgpu_plan* p);

int check_error_flags(ssgpu_plan* p) {
  ssgpu_ctx* c = p->ctx;
  // The flags are written by kernels on c->stream, which is a non-blocking stream: a null-stream
  // hipMemcpy is NOT ordered behind it and can read a flag before the run that sets (or clears) it.
  std::vector<uint32_t> flags(p->exec.size(), 0);
  for (size_t i = 0; i < p->exec.size(); ++i)
    if (p->exec[i].error_flag.p)
      HIP_TRY(c, hipMemcpyAsync(&flags[i], p->exec[i].error_flag.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint32_t& f : flags) {
    if (f & SSGPU_FLAG_NAN_IN_MINMAX) p->nan_seen = true;   // not an error: see fix_nan_minmax
    f &= 0xFFu;
  }
  for (uint32_t f : flags) {
    if (f == 3) { c->err = "decoupled look-back: a tile waited for an earlier tile's row count for too long and gave up"; return SSGPU_ERROR_HIP; }
    if (f == SSGPU_EVAL_ERROR_FOREIGN_KEY) {   // VM_JOIN_ROWID: the message of rowid_merge_join.cc:99-102, the right table's row count in it
      c->err = "No parent record with ID > " + std::to_string(std::max<int64_t>(p->aux_rows, 0));
      return SSGPU_ERROR_FOREIGN_KEY_INVALID;
    }
    if (f) {
      c->err = f == 2 ? "Evaluation error: invalid argument of a signaling math expression (negative input of SQRT)"
                      : "Evaluation error: division by zero in a signaling expression";
      return SSGPU_ERROR_EVALUATION_ERROR;
    }
  }
  return SSGPU_OK;
}

// block uploads since the last run (ssgpu_ctx::copy_pending): whatever is launched on the compute stream from here on comes after them
static int order_after_uploads(ssgpu_ctx* c) {
  if (!c->copy_pending.exchange(false, std::memory_order_acq_rel)) return SSGPU_OK;
  if (!c->copy_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->copy_ev, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(c->copy_ev, c->copy_stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->copy_ev, 0));
  return SSGPU_OK;
}
int run_plan(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, int64_t row_id_base, bool partial);

// Looks at run feedback that was left on the stream (StageExec::fb_pending).  A run that overflowed a table or a segment
// after all produced an incomplete result: it is repeated here, synchronously (the stage is no longer "steady"), from the
// columns the caller passed -- which it keeps alive until it has its result, as for every asynchronous run.
int settle_plan(ssgpu_plan* p) {
  if (!p->deferred) return SSGPU_OK;
  ssgpu_ctx* c = p->ctx;
  p->deferred = false;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  bool rerun = false;
  for (auto& ex : p->exec) {
    if (!ex.fb_pending) continue;
    const uint32_t* fb = static_cast<const uint32_t*>(ex.fb_host.p);
    const int kind = ex.fb_pending; ex.fb_pending = 0;
    if (fb[0] || (kind == 2 && (fb[1] || fb[3]))) { rerun = true; ex.steady = 0; }
    else if (kind == 1 && (uint64_t)fb[1] > 2ull * ex.steady_bypass + (uint64_t)(p->last_rows >> 6)) ex.steady = 0;   // the data moved: the next run adapts again
  }
  if (!rerun) return SSGPU_OK;
  std::vector<ssgpu_column> cols = p->last_cols;
  return run_plan(p, cols.data(), (int32_t)cols.size(), p->last_rows, p->last_base, p->last_partial);
}

// Floating MIN / MAX and NaN.  The kernels skip NaN inputs, which is the reference's answer unless a NaN is a group's FIRST
// non-NULL value -- then the reference's result is that NaN (aggregation_operators.h:189-228: the first value is assigned,
// and "val < result" never replaces a NaN).  A run that met a NaN in such an aggregate (flagged by the kernels, seen by
// check_error_flags) is therefore repeated once with the plan lowered in its NaN-exact form; the plan keeps that form.
int fix_nan_minmax(ssgpu_plan* p) {
  if (!p->nan_seen) return SSGPU_OK;
  p->nan_seen = false;
  if (p->desc.nan_exact || p->partial_pending) return SSGPU_OK;   // already exact (or a partial run: the shards' merge is not order-aware)
  ssgpu_ctx* c = p->ctx;
  p->desc.nan_exact = true;
  std::vector<Stage> stages; Schema schema; std::string describe;
  Status s = lower_plan(p->desc, &stages, &schema, &describe);
  if (!s.ok()) { p->desc.nan_exact = false; return SSGPU_OK; }   // (a shape the exact form cannot take keeps the order-independent answer)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (auto& ex : p->exec) { ex.rtc_main.drop(); ex.rtc_pscatter.drop(); ex.rtc_plain.drop(); ex.rtc_part.drop(); ex.rtc_resident.drop(); ex.rtc_hot.drop(); }
  for (auto& ex : p->exec) if (ex.fb_event) { (void)hipEventDestroy(ex.fb_event); ex.fb_event = nullptr; g_events.fetch_sub(1); }
  p->exec.clear();
  p->stages = stages; p->describe = describe;
  p->exec.resize(p->stages.size());
  std::vector<ssgpu_column> cols = p->last_cols;
  int rc = run_plan(p, cols.data(), (int32_t)cols.size(), p->last_rows, p->last_base, false);
  if (rc != SSGPU_OK) return rc;
  rc = settle_plan(p);
  if (rc != SSGPU_OK) return rc;
  rc = check_error_flags(p);
  p->nan_seen = false;
  return rc;
}

int run_plan(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, int64_t row_id_base, bool partial) {
  ssgpu_ctx* c = p->ctx;
  if (!c || c->device < 0) { if (c) c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  ssgpu_rtc_mode(!p->cached_only ? 0 : p->background && rows >= p->background_min_rows ? 2 : 1);   // (this thread's kernel requests during the run)
  p->run_row_end = row_id_base + rows;
  p->nan_seen = false;
  if (p->deferred) {   // the previous run's feedback first: an overflow there puts the stage back into its adapting, synchronous form
    p->deferred = false;   // (that run's result is being replaced by this run: nothing to repeat)
    for (auto& ex : p->exec) {
      if (!ex.fb_pending) continue;
      // only the copy of the words has to be done -- not the work queued behind it (a stepping job keeps the stream busy)
      if (ex.fb_event) HIP_TRY(c, hipEventSynchronize(ex.fb_event)); else HIP_TRY(c, hipStreamSynchronize(c->stream));
      const uint32_t* fb = static_cast<const uint32_t*>(ex.fb_host.p);
      const int kind = ex.fb_pending; ex.fb_pending = 0;
      if (fb[0] || (kind == 2 && (fb[1] || fb[3]))) ex.steady = 0;
      else if (kind == 1 && (uint64_t)fb[1] > 2ull * ex.steady_bypass + (uint64_t)(p->last_rows >> 6)) ex.steady = 0;
    }
  }
  if (n_cols != (int)p->desc.input_schema.size()) { c->err = "column count does not match the plan's input schema"; return SSGPU_ERROR_ATTRIBUTE_COUNT_MISMATCH; }
  if (rows < 0) { c->err = "negative row count"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  if (p->interrupted.exchange(0)) { c->err = "interrupted"; return SSGPU_INTERRUPTED; }
  QuotaScope quota_scope(&p->quota);
  HIP_TRY(c, hipSetDevice(c->device));
  { const int orc = order_after_uploads(c); if (orc != SSGPU_OK) return orc; }
  // blocks are staged on the copy stream: kernels must wait for those copies
  memset(&p->counters, 0, sizeof(p->counters));
  { const int trc = ensure_dict_tables(p); if (trc != SSGPU_OK) return trc; }
  p->counters.rows_in = rows;
  p->result.fetched.assign(p->result.fetched.size(), false);
  for (ssgpu_dict*& cd : p->result.concat_dicts) { if (cd) ssgpu_dict_destroy(cd); cd = nullptr; }
  InCols in; in.cols.assign(cols, cols + n_cols); in.rows = rows;
  if (partial && !(p->stages.size() == 1 && p->stages[0].kind == STAGE_SCALAR_AGG)) {
    c->err = "partial runs need a plan whose only stage is a ScalarAggregate"; return SSGPU_ERROR_NOT_IMPLEMENTED;
  }
  for (size_t si = 0; si < p->stages.size(); ++si) {
    if (si == 0) ++p->n_runs;
    int rc = prepare_stage(p, si);
    if (rc != SSGPU_OK) return rc;
  }
  if (c->profile) {
    const int slot = (int)(p->profiled_runs % ssgpu_plan::kEventRing);
    if (!p->ring0[slot]) { HIP_TRY(c, hipEventCreate(&p->ring0[slot])); HIP_TRY(c, hipEventCreate(&p->ring1[slot])); g_events.fetch_add(2); }
    p->ev_dom0 = p->ring0[slot]; p->ev_dom1 = p->ring1[slot];
    ++p->profiled_runs;
    p->events_valid = false;
    if (c->profile_total) HIP_TRY(c, hipEventRecord(p->ev_begin, c->stream));
  }
  // every stage's evaluation-error word starts clear: the flags of ALL stages are read at each hand-off and at fetch
  // (a GroupAggregate that is the plan's FIRST stage clears its word in its own init launch -- one fill launch less per run; later
  //  stages' words are read at the hand-offs before those stages run, so they are cleared here)
  for (size_t si = 0; si < p->exec.size(); ++si)
    if (p->exec[si].error_flag.p && !p->keep_error_flags && !(si == 0 && p->stages[si].kind == STAGE_GROUP_AGG)) HIP_TRY(c, hipMemsetAsync(p->exec[si].error_flag.p, 0, sizeof(uint32_t), c->stream));
  int64_t alg_bytes = 0;
  for (size_t si = 0; si < p->stages.size(); ++si) {
    if (p->interrupted.exchange(0)) { c->err = "interrupted"; return SSGPU_INTERRUPTED; }
    Stage& st = p->stages[si];
    int rc = SSGPU_OK;
    alg_bytes += st.algorithmic_bytes_per_row * in.rows;
    rc = build_joins(p, st, p->exec[si]);
    if (rc != SSGPU_OK) return rc;
    switch (st.kind) {
      case STAGE_SCALAR_AGG:
        rc = run_scalar_agg(p, si, in, row_id_base, partial);
        if (rc == SSGPU_OK && !partial) rc = emit_scalar_agg(p, si);
        if (rc == SSGPU_OK && !partial && !st.seq_sums.empty()) rc = run_seq_sums(p, st, p->exec[si], in, nullptr);
        break;
      case STAGE_MATERIALIZE: rc = run_materialize(p, si, in, row_id_base); break;
      case STAGE_GROUP_AGG: rc = run_group_agg(p, si, in, row_id_base); break;
      case STAGE_SORT: rc = run_sort(p, si, in); break;
      case STAGE_CLUSTERS: rc = run_clusters(p, si, in, row_id_base); break;
      case STAGE_JOIN_EXPAND: rc = run_join_expand(p, si, in); break;
      case STAGE_FOLD_TAIL: rc = run_fold_tail(p, si, in); break;
      default: c->err = "stage kind not executable yet"; rc = SSGPU_ERROR_NOT_IMPLEMENTED; break;
    }
    if (rc != SSGPU_OK) return rc;
    if (si + 1 < p->stages.size()) {
      // next stage reads this stage's materialised result
      StageExec& ex = p->exec[si];
      const Stage& nx = p->stages[si + 1];
      // A filter-less materialising stage (Compute / Project over a blocking stage's result, e.g. the COUNT -> NOT NULL and
      // sum + residual columns of a sharded merge) takes the row count FROM THE DEVICE: no stream synchronise between the two
      // stages, the kernel reads the count where the producer left it and runs over the buffers' capacity at most.  Every
      // stage's error word is still looked at when the result is touched (check_error_flags); rows beyond the count are
      // never computed, so a signaling operator cannot fail on them.
      const bool device_rows = c->async_handoff != 0 && !c->debug_timing && ex.out_rows < 0 && ex.out_capacity > 0 && nx.kind == STAGE_MATERIALIZE &&
                               !nx.has_filter && nx.distinct_cols.empty() && !nx.has_segment && !nx.has_rank && nx.joins.empty();
      int64_t r = 0;
      in.rows_dev = nullptr;
      if (device_rows) {
        r = ex.out_capacity;
        in.rows_dev = static_cast<const unsigned long long*>(rows_word(ex));
      } else {
        rc = stage_rows(p, si, &r);
        if (rc != SSGPU_OK) return rc;
        // a stage that hit an evaluation error must not feed the next one (the hand-off already waits for the row count)
        rc = check_error_flags(p);
        if (rc != SSGPU_OK) return rc;
      }
      in.cols.clear();
      for (auto& oc : ex.out) { ssgpu_column col; col.data = oc.data.p; col.is_null = oc.nullable ? oc.nulls.as<uint8_t>() : nullptr; in.cols.push_back(col); }
      in.rows = r;
      row_id_base = 0;
    }
  }
  if (c->profile && c->profile_total) { HIP_TRY(c, hipEventRecord(p->ev_end, c->stream)); p->events_valid = true; }
  p->counters.algorithmic_bytes = alg_bytes;
  p->last_rows = rows;
  p->last_cols.assign(cols, cols + n_cols); p->last_base = row_id_base; p->last_partial = partial;
  p->partial_pending = partial;
  return SSGPU_OK;
}

}  // namespace

extern "C" {

int ssgpu_plan_run(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, ssgpu_result** out) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  int rc = run_plan(p, cols, n_cols, rows, 0, false);
  if (rc != SSGPU_OK) return rc;
  if (!p->lazy_feedback) {
    // the safe mode (default): everything that could make the library read the input columns again is decided HERE, while the
    // caller still holds them -- run feedback is never deferred in this mode, and the NaN-exact repeat of a floating MIN / MAX
    // happens now instead of when the result is first touched.  (An evaluation error still surfaces where it always did: when
    // the result is touched -- its flag stays set until the next run.)
    rc = settle_plan(p);
    if (rc != SSGPU_OK) return rc;
    (void)check_error_flags(p);      // synchronises; sets nan_seen
    rc = fix_nan_minmax(p);
    if (rc != SSGPU_OK) return rc;
  }
  if (out) *out = &p->result;
  return SSGPU_OK;
}

// BestEffortGroupAggregate (cursor/core/aggregate.h:230-250; GroupAggregateCursor::Next / ProcessInput with best_effort_,
// aggregate_groups.cc:211-222,332-433).  One call = one ProcessInput: the plan's GroupAggregate over the LONGEST run of input rows
// that starts at `start_row` and holds at most `capacity` distinct keys (the operation's option0; the reference's verdict comes from
// its allocator, deterministic under GuaranteeMemory -- here the result block's row capacity).  The result is key-unique; *next_row
// is where the next call starts (== rows: the input is exhausted).  How: the aggregate runs over a window of input rows with the
// hidden first-seen row id; if more than `capacity` keys turn up, the first-seen id of key number `capacity` IS the end of the run,
// and the aggregate runs again over exactly [start_row, end).  A window in which every key fitted and that is not the end of the
// input is widened (x 4).  ERROR_MEMORY_EXCEEDED is never the answer to a large input: a run that does not fit the plan's memory
// limit is repeated over half the window with the capacity lowered to match (the reference emits what it has and starts anew,
// :375-393); only a single row that does not fit fails (:405-412).
int ssgpu_plan_run_best_effort(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, int64_t start_row, int64_t* next_row, ssgpu_result** out) {
  if (!p || !next_row) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (!p->best_effort) { if (c) c->err = "ssgpu_plan_run_best_effort needs a plan whose root is a BestEffortGroupAggregate"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  if (n_cols != (int)p->desc.input_schema.size()) { c->err = "column count does not match the plan's input schema"; return SSGPU_ERROR_ATTRIBUTE_COUNT_MISMATCH; }
  if (start_row < 0 || start_row > rows) { c->err = "start_row outside the input"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  std::vector<ssgpu_column> win((size_t)n_cols);
  auto window = [&](int64_t s) {
    for (int i = 0; i < n_cols; ++i) {
      const size_t w = (size_t)dtype_width(p->desc.input_schema[i].dtype);
      win[i].data = cols[i].data ? static_cast<const char*>(cols[i].data) + (size_t)s * w : nullptr;
      win[i].is_null = cols[i].is_null ? cols[i].is_null + s : nullptr;
    }
  };
  auto run_range = [&](int64_t s, int64_t n) -> int {
    window(s);
    p->be_base = s;      // (row ids count from the window's first row -- FIRST / LAST fetch their values by them --; the cut stage adds the base back)
    int rc = run_plan(p, win.data(), n_cols, n, 0, false);
    if (rc != SSGPU_OK) return rc;
    rc = settle_plan(p);
    if (rc != SSGPU_OK) return rc;
    rc = check_error_flags(p);
    if (rc != SSGPU_OK) return rc;
    return fix_nan_minmax(p);
  };
  const int64_t left = rows - start_row;
  int64_t W = p->be_window > 0 ? p->be_window : std::max<int64_t>(1 << 16, p->be_capacity < (INT64_MAX >> 4) ? p->be_capacity * 8 : INT64_MAX);
  for (;;) {
    W = std::max<int64_t>(1, std::min(W, left));
    if (left == 0) W = 0;
    int rc = run_range(start_row, W);
    if (rc == SSGPU_ERROR_MEMORY_EXCEEDED && W > 1) {
      // what fits is emitted and the aggregation starts anew: half the window, and no more groups than that many rows can hold
      p->be_window_fail = W;       // (no later window of this plan is widened to this size again)
      W = std::max<int64_t>(1, W / 2); p->be_window = W; p->be_capacity = std::min(p->be_capacity, W);
      // the stages start over with buffers sized for the smaller window: what they hold was sized for the run that did not fit
      // (tables only grow while a plan lives), and a direct-shape table starts at 4 slots per possible group instead of the context's default
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (auto& ex : p->exec) { ex.rtc_main.drop(); ex.rtc_pscatter.drop(); ex.rtc_plain.drop(); ex.rtc_part.drop(); ex.rtc_resident.drop(); ex.rtc_hot.drop(); }
      for (auto& ex : p->exec) if (ex.fb_event) { (void)hipEventDestroy(ex.fb_event); ex.fb_event = nullptr; g_events.fetch_sub(1); }
      p->exec.clear(); p->exec.resize(p->stages.size());
      p->deferred = false;
      { uint32_t cap = 1024; while ((int64_t)cap < 4 * W && cap < (1u << 30)) cap *= 2; p->group_capacity_hint = cap; }
      continue;
    }
    if (rc != SSGPU_OK) return rc;
    if (p->be_cut >= 0) {
      const int64_t end = p->be_cut;
      if (end <= start_row || end > start_row + W) { c->err = "best-effort cut outside the window"; return SSGPU_ERROR_HIP; }
      rc = run_range(start_row, end - start_row);
      if (rc != SSGPU_OK) return rc;
      if (p->be_cut >= 0) { c->err = "best-effort run over its own cut still overflows"; return SSGPU_ERROR_HIP; }
      *next_row = end;
      break;
    }
    if (W >= left) { *next_row = rows; break; }
    // every key of the window fitted: the run goes on over a wider one -- unless a window of that size has already failed to fit the
    // memory limit: then this window is the view (widening and halving would alternate for ever)
    int64_t wider = W > (INT64_MAX >> 2) ? INT64_MAX : W * 4;
    if (p->be_window_fail > 0 && wider >= p->be_window_fail) wider = std::max(W, p->be_window_fail / 2);
    if (wider <= W) { *next_row = start_row + W; break; }
    W = wider; p->be_window = W;
  }
  if (out) *out = &p->result;
  return SSGPU_OK;
}

int32_t ssgpu_plan_specialized(const ssgpu_plan* p) {
  if (!p) return 0;
  int32_t n = 0;
  for (auto& ex : p->exec) n += (ex.rtc_main.h ? 1 : 0) + (ex.rtc_pscatter.h ? 1 : 0) + (ex.rtc_plain.h ? 1 : 0) + (ex.rtc_part.h ? 1 : 0) + (ex.rtc_resident.h ? 1 : 0) + (ex.rtc_hot.h ? 1 : 0);
  return n;
}
const char* ssgpu_plan_specialize_reason(const ssgpu_plan* p) {
  if (!p) return "";
  for (auto& ex : p->exec) {
    if (ex.rtc_why.empty()) continue;
    // "being compiled": true while one of the stage's slots is still waiting for its kernel
    if (ex.rtc_why.find("being compiled") != std::string::npos && !(ex.rtc_main.pending || ex.rtc_pscatter.pending || ex.rtc_plain.pending || ex.rtc_part.pending ||
                                                                    ex.rtc_resident.pending || ex.rtc_hot.pending)) continue;
    return ex.rtc_why.c_str();
  }
  return "";
}
// Ask for specialised kernels NOW: the deterministic compile point.  Stages whose launch shape is known without a run
// (scalar aggregates, materialising stages, clustered aggregation) are compiled here; a GroupAggregate's kernels depend
// on the execution shape its first runs settle on and are compiled when that shape is first launched.
int ssgpu_plan_specialize(ssgpu_plan* p) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (!c || c->device < 0) { if (c) c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  HIP_TRY(c, hipSetDevice(c->device));
  p->specialize = true;
  if (p->cached_only) {          // kernels this plan looked for and did not find are compiled from now on (one the worker is at: waited for)
    p->cached_only = false; p->background = false;
    for (auto& ex : p->exec) {
      for (StageExec::RtcSlot* sl : {&ex.rtc_main, &ex.rtc_pscatter, &ex.rtc_plain, &ex.rtc_part, &ex.rtc_resident, &ex.rtc_hot}) if (!sl->h) sl->tried = false;
      ex.rtc_why.clear();
    }
  }
  ssgpu_rtc_cached_only(false);
  for (size_t si = 0; si < p->stages.size(); ++si) {
    const int rc = prepare_stage(p, si);
    if (rc != SSGPU_OK) return rc;
    Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
    if (st.main.empty() || st.kind == STAGE_GROUP_AGG) continue;
    (void)rtc_for(p, ex, ex.rtc_main, st.main, ex.lay, ex.host_prog_main, ex.n_instr_main, ex.lay.lds_bytes, "");
  }
  return SSGPU_OK;
}
int32_t ssgpu_plan_stage_count(const ssgpu_plan* p) { return p ? (int32_t)p->stages.size() : 0; }
int ssgpu_plan_stage_info(const ssgpu_plan* p, int32_t stage, ssgpu_stage_info* out) {
  if (!p || !out || stage < 0 || stage >= (int32_t)p->stages.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  const StageExec& ex = p->exec[stage];
  memset(out, 0, sizeof(*out));
  out->kind = (int32_t)p->stages[stage].kind;
  out->group_shape = ex.last_group_shape; out->part_n = (int32_t)ex.part_n; out->part_seg_growth = (int32_t)ex.part_seg_growth;
  out->group_wgs_per_cu = ex.group_wgs; out->reruns = ex.last_reruns;
  out->sort_passes = ex.last_sort_passes; out->sort_mode = ex.last_sort_mode;
  out->specialized = (ex.rtc_main.h ? 1 : 0) + (ex.rtc_pscatter.h ? 2 : 0) + (ex.rtc_part.h ? 4 : 0) + (ex.rtc_plain.h ? 8 : 0) + (ex.rtc_resident.h ? 16 : 0);
  out->plain_scatter = ex.last_plain_scatter ? 1 : 0;
  out->hot_keys = (int32_t)ex.hot_n;
  out->dense_slots = ex.dense.on ? (int32_t)ex.dense.slots : 0;
  return SSGPU_OK;
}
void ssgpu_specialized_kernels_trim(int32_t keep) { ssgpu_rtc_trim(keep); }
int ssgpu_memory_stats(ssgpu_memory_stats_t* out) {
  if (!out) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  memset(out, 0, sizeof(*out));
  out->device_bytes = g_dev_bytes.load(); out->pinned_bytes = g_pinned_bytes.load();
  out->live_plans = g_live_plans.load(); out->live_blocks = g_live_blocks.load(); out->events = g_events.load();
  long long m = 0, b = 0, n = 0, d = 0;
  ssgpu_rtc_stats(&m, &b, &n, &d);
  out->rtc_modules = m; out->rtc_code_bytes = b; out->rtc_compilations = n; out->rtc_disk_hits = d;
  return SSGPU_OK;
}
int ssgpu_plan_set_memory_limit(ssgpu_plan* p, int64_t bytes) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  p->quota.limit = bytes < 0 ? -1 : bytes;
  return SSGPU_OK;
}
int64_t ssgpu_plan_memory_in_use(const ssgpu_plan* p) { return p ? p->quota.used : 0; }

// Expression::Bind + BoundExpressionTree::Evaluate (expression/base/expression.h:46-167): the bound tree is a plan that
// computes the expression over a scan of the schema it was bound against
int ssgpu_expr_bind(ssgpu_ctx* c, const ssgpu_attr* schema, int32_t n_attrs, const ssgpu_expr* exprs, int32_t n_exprs,
                    const int32_t* expr_args, int32_t n_expr_args, int32_t root, int64_t max_row_count, ssgpu_plan** out) {
  if (!c || !schema || !exprs || !out || root < 0 || root >= n_exprs) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_op ops[2]; memset(ops, 0, sizeof(ops));
  ops[0].kind = SSGPU_OP_SCAN; ops[0].child = -1; ops[0].expr = -1;
  ops[1].kind = SSGPU_OP_COMPUTE; ops[1].child = 0; ops[1].expr = root;
  ssgpu_plan_desc d; memset(&d, 0, sizeof(d));
  d.input_schema = schema; d.n_attrs = n_attrs; d.ops = ops; d.n_ops = 2;
  d.exprs = exprs; d.n_exprs = n_exprs; d.expr_args = expr_args; d.n_expr_args = n_expr_args;
  int rc = ssgpu_plan_create(c, &d, out);
  if (rc == SSGPU_OK) (*out)->expr_row_capacity = max_row_count > 0 ? max_row_count : INT64_MAX;
  return rc;
}
int64_t ssgpu_expr_row_capacity(const ssgpu_plan* bound) { return bound ? bound->expr_row_capacity : 0; }
int ssgpu_expr_evaluate(ssgpu_plan* bound, const ssgpu_column* cols, int32_t n_cols, int64_t rows, ssgpu_result** out) {
  if (!bound) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (rows > bound->expr_row_capacity) {
    bound->ctx->err = "Trying to evaluate an expression with number of rows: " + std::to_string(rows) +
                      ", while the expression has capacity for less rows: " + std::to_string(bound->expr_row_capacity);
    return SSGPU_ERROR_TOO_MANY_ROWS;
  }
  return ssgpu_plan_run(bound, cols, n_cols, rows, out);
}

// BoundExpression::DoEvaluate(const View& input, const BoolView& skip_vectors) (expression/base/expression.h:46-92; how the reference's
// operations call into a bound node: bound_expression_factory.cc:44-107 hands every child the rows it may skip).  One skip vector per
// result attribute, in and out: a row whose skip byte is set on entry is not evaluated -- its result is NULL and no failing operator
// fails on it -- and on return the vector holds the result's NULLs (entry skips included).  Here: the tree re-bound once as
// Compute(IF($skip_i, NULL, e_i) AS name_i) over the input plus one BOOL column per result attribute -- IF evaluates its branches
// guardedly (lower.cpp), which is exactly the skip-vector contract -- and the result's NULL masks copied back into the caller's vectors.
int ssgpu_expr_evaluate_skip(ssgpu_plan* bound, const ssgpu_column* cols, int32_t n_cols, int64_t rows, uint8_t* const* skip, int32_t n_skip, ssgpu_result** out) {
  if (!bound || !skip) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = bound->ctx;
  const PlanDesc& D = bound->desc;
  const int n_out = (int)bound->result_schema.size();
  if (n_skip != n_out) { c->err = "skip vectors: one per result attribute (" + std::to_string(n_out) + ")"; return SSGPU_ERROR_ATTRIBUTE_COUNT_MISMATCH; }
  if (D.ops.size() != 2 || D.ops[1].kind != SSGPU_OP_COMPUTE) { c->err = "ssgpu_expr_evaluate_skip needs a tree bound by ssgpu_expr_bind"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  if (rows > bound->expr_row_capacity) {
    c->err = "Trying to evaluate an expression with number of rows: " + std::to_string(rows) + ", while the expression has capacity for less rows: " + std::to_string(bound->expr_row_capacity);
    return SSGPU_ERROR_TOO_MANY_ROWS;
  }
  if (!bound->skip_plan) {
    const ssgpu_expr& root = D.exprs[(size_t)D.ops[1].expr];
    std::vector<int32_t> kids;
    if (root.kind == SSGPU_EXPR_COMPOUND) for (int i = 0; i < root.nargs; ++i) kids.push_back(D.expr_args[(size_t)(root.first_arg + i)]);
    else kids.push_back(D.ops[1].expr);
    if ((int)kids.size() != n_out) { c->err = "skip vectors: a nested compound expression has no node-level form"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    std::deque<std::string> names;
    std::vector<ssgpu_attr> attrs;
    for (auto& a : D.input_schema) attrs.push_back(ssgpu_attr{a.name.c_str(), a.dtype, a.nullable ? 1 : 0});
    for (int i = 0; i < n_out; ++i) { names.push_back("$skip" + std::to_string(i)); attrs.push_back(ssgpu_attr{names.back().c_str(), SSGPU_BOOL, 0}); }
    std::vector<ssgpu_expr> exprs(D.exprs.begin(), D.exprs.end());
    std::vector<int32_t> args(D.expr_args.begin(), D.expr_args.end());
    auto add = [&](int kind, int op, int dtype, const char* name, std::initializer_list<int32_t> kk) -> int32_t {
      ssgpu_expr e; memset(&e, 0, sizeof(e));
      e.kind = kind; e.op = op; e.dtype = dtype; e.first_arg = (int32_t)args.size(); e.nargs = (int32_t)kk.size(); e.name = name ? name : "";
      for (int32_t k : kk) args.push_back(k);
      exprs.push_back(e);
      return (int32_t)exprs.size() - 1;
    };
    std::vector<int32_t> outs;
    for (int i = 0; i < n_out; ++i) {
      int32_t inner = kids[(size_t)i];
      if (exprs[(size_t)inner].kind == SSGPU_EXPR_ALIAS && exprs[(size_t)inner].nargs == 1) inner = args[(size_t)exprs[(size_t)inner].first_arg];
      const int dtype = bound->result_schema[(size_t)i].dtype;
      if (dtype_width(dtype) == 0) { c->err = "skip vectors: variable-length results have no node-level form"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
      const int32_t cond = add(SSGPU_EXPR_ATTR_NAMED, 0, 0, names[(size_t)i].c_str(), {});
      const int32_t null = add(SSGPU_EXPR_NULL, 0, dtype, "", {});
      const int32_t sel = add(SSGPU_EXPR_OP, 204 /* OPERATOR_IF */, 0, "", {cond, null, inner});
      outs.push_back(add(SSGPU_EXPR_ALIAS, 0, 0, bound->result_schema[(size_t)i].name.c_str(), {sel}));
    }
    int32_t new_root;
    { ssgpu_expr e; memset(&e, 0, sizeof(e)); e.kind = SSGPU_EXPR_COMPOUND; e.first_arg = (int32_t)args.size(); e.nargs = (int32_t)outs.size(); e.name = "";
      for (int32_t k : outs) args.push_back(k);
      exprs.push_back(e); new_root = (int32_t)exprs.size() - 1; }
    ssgpu_plan* q = nullptr;
    const int rc = ssgpu_expr_bind(c, attrs.data(), (int32_t)attrs.size(), exprs.data(), (int32_t)exprs.size(), args.data(), (int32_t)args.size(), new_root,
                                   bound->expr_row_capacity == INT64_MAX ? 0 : bound->expr_row_capacity, &q);
    if (rc != SSGPU_OK) return rc;
    bound->skip_plan = q;
  }
  ssgpu_plan* q = bound->skip_plan;
  q->dict = bound->dict; q->dict_gen = bound->dict_gen; q->quota.limit = bound->quota.limit;
  if (n_cols != (int)D.input_schema.size()) { c->err = "column count does not match the plan's input schema"; return SSGPU_ERROR_ATTRIBUTE_COUNT_MISMATCH; }
  if (!c || c->device < 0) { if (c) c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  HIP_TRY(c, hipSetDevice(c->device));
  // a vector the caller does not have (NULL) skips nothing: a zeroed one of the library's own
  HIP_TRY(c, q->host_states.ensure((size_t)std::max<int64_t>(rows, 1)));
  bool need_zero = false;
  for (int i = 0; i < n_out; ++i) need_zero = need_zero || !skip[i];
  if (need_zero) HIP_TRY(c, hipMemsetAsync(q->host_states.p, 0, (size_t)std::max<int64_t>(rows, 1), c->stream));
  std::vector<ssgpu_column> all(cols, cols + n_cols);
  for (int i = 0; i < n_out; ++i) { ssgpu_column k; k.data = skip[i] ? (const void*)skip[i] : (const void*)q->host_states.p; k.is_null = nullptr; all.push_back(k); }
  ssgpu_result* res = nullptr;
  int rc = ssgpu_plan_run(q, all.data(), (int32_t)all.size(), rows, &res);
  if (rc != SSGPU_OK) return rc;
  for (int i = 0; i < n_out && rows > 0; ++i) {
    if (!skip[i]) continue;
    ssgpu_column col;
    rc = ssgpu_result_device_column(res, i, &col);
    if (rc != SSGPU_OK) return rc;
    if (col.is_null) HIP_TRY(c, hipMemcpyAsync(skip[i], col.is_null, (size_t)rows, hipMemcpyDeviceToDevice, c->stream));
  }
  if (out) *out = res;
  return SSGPU_OK;
}

int ssgpu_plan_run_block(ssgpu_plan* p, const ssgpu_block* b, ssgpu_result** out) {
  if (!p || !b) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (!c || c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  // uploads were issued on the copy stream; order the compute stream after them
  hipEvent_t ev;
  HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(ev, c->copy_stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, ev, 0));
  (void)hipEventDestroy(ev);
  std::vector<ssgpu_column> cols(b->schema.size());
  for (size_t i = 0; i < cols.size(); ++i) ssgpu_block_column(b, (int32_t)i, &cols[i]);
  return ssgpu_plan_run(p, cols.data(), (int32_t)cols.size(), b->rows, out);
}


// ---- chunked execution beyond the ScalarAggregate shape (ssgpu_plan::StreamJob) ------------------------------------------------
// The reference pulls 1024-row blocks from any child for every operation (aggregate_groups.cc:212,282 ProcessInput, filter.cc:96-128);
// here a HOST input of any size crosses PCIe in chunks while the device works on the chunk before it.
static void stream_job_reset_out(ssgpu_plan* q) {     // the last stage's result buffers: views of an accumulation are dropped, a fresh run allocates its own
  if (q->exec.empty()) return;
  StageExec& ex = q->exec.back();
  bool any_view = false;
  for (auto& oc : ex.out) any_view = any_view || oc.data.view || oc.nulls.view;
  if (!any_view || ex.out_arena.p) return;            // (views into the stage's own arena stay)
  for (auto& oc : ex.out) { oc.data.release(); oc.nulls.release(); }
  ex.out_capacity = 0; ex.out_rows = 0;
}
static int lookup_name(const Schema& s, const char* name) {
  for (size_t i = 0; i < s.size(); ++i) if (s[i].name == (name ? name : "")) return (int)i;
  return -1;
}
// the row-local operations whose `child2` is a scan of the auxiliary input
static bool op_has_aux_side(int kind) { return kind == SSGPU_OP_HASH_JOIN || kind == SSGPU_OP_FOREIGN_FILTER || kind == SSGPU_OP_ROWID_MERGE_JOIN; }
// kind 3: the derived plans.  iB = the GroupAggregate in p->desc.ops
static int stream_job_build_group(ssgpu_plan* p, int iB, ssgpu_plan** head_out, ssgpu_plan** tail_out) {
  ssgpu_ctx* c = p->ctx; const PlanDesc& D = p->desc;
  std::vector<ssgpu_attr> in_attrs, aux_attrs;
  for (auto& a : D.input_schema) in_attrs.push_back(ssgpu_attr{a.name.c_str(), a.dtype, a.nullable ? 1 : 0});
  for (auto& a : D.aux_schema) aux_attrs.push_back(ssgpu_attr{a.name.c_str(), a.dtype, a.nullable ? 1 : 0});
  ssgpu_plan_desc base; memset(&base, 0, sizeof(base));
  base.input_schema = in_attrs.data(); base.n_attrs = (int32_t)in_attrs.size();
  base.ops = D.ops.data(); base.n_ops = (int32_t)D.ops.size();
  base.exprs = D.exprs.data(); base.n_exprs = (int32_t)D.exprs.size();
  base.expr_args = D.expr_args.data(); base.n_expr_args = (int32_t)D.expr_args.size();
  base.projs = D.projs.data(); base.n_projs = (int32_t)D.projs.size();
  base.aggs = D.aggs.data(); base.n_aggs = (int32_t)D.aggs.size();
  base.sortkeys = D.sortkeys.data(); base.n_sortkeys = (int32_t)D.sortkeys.size();
  base.aux_schema = aux_attrs.empty() ? nullptr : aux_attrs.data(); base.n_aux_attrs = (int32_t)aux_attrs.size();
  const ssgpu_op B = D.ops[(size_t)iB];
  // the schema the GroupAggregate reads: the plan cut below it, bound
  Schema child_schema;
  {
    ssgpu_plan_desc d1 = base; d1.n_ops = B.child + 1;
    ssgpu_plan* child = nullptr;
    const int rc = ssgpu_plan_create(c, &d1, &child);
    if (rc != SSGPU_OK) return rc;
    child_schema = child->result_schema;
    ssgpu_plan_destroy(child);
  }
  // head: the plan up to and including the GroupAggregate; behind every DOUBLE sum its residual (SSGPU_SUM_RESIDUAL: the partial sum
  // travels as the exact pair (s, e), as between shards -- supersonic_amd/distributed.py _shard_spec)
  std::deque<std::string> names;
  std::vector<ssgpu_agg> haggs(D.aggs.begin(), D.aggs.end());
  const size_t hfirst = haggs.size();
  enum { COL_RESIDUAL = 1000, COL_FIRST = 1001 };
  std::vector<int> col_fn;                      // per aggregate column of the head's result: its aggregation, or COL_RESIDUAL
  for (int j = 0; j < B.agg_n; ++j) {
    const ssgpu_agg a = D.aggs[(size_t)(B.agg_first + j)];
    if (a.distinct || a.aggregation == SSGPU_CONCAT || a.aggregation == SSGPU_SUM_RESIDUAL) {
      c->err = "chunked execution: DISTINCT / CONCAT aggregates are not partial results (their GroupAggregate takes device columns: ssgpu_plan_run)"; return SSGPU_ERROR_NOT_IMPLEMENTED;
    }
    const int pos = lookup_name(child_schema, a.input);
    const int in_type = pos >= 0 ? child_schema[(size_t)pos].dtype : -1;
    const bool int_out = a.output_type == SSGPU_INT32 || a.output_type == SSGPU_UINT32 || a.output_type == SSGPU_INT64 || a.output_type == SSGPU_UINT64;
    if (a.aggregation == SSGPU_SUM && (in_type == SSGPU_FLOAT || in_type == SSGPU_DOUBLE) && int_out) {
      // the reference adds and truncates row after row (aggregation_operators.h:173-185): a chunk's result is not a partial sum
      c->err = "chunked execution: SUM of a floating input into an integer result is a row-after-row fold, not a partial result"; return SSGPU_ERROR_NOT_IMPLEMENTED;
    }
    haggs.push_back(a); col_fn.push_back(a.aggregation);
    if ((a.aggregation == SSGPU_MIN || a.aggregation == SSGPU_MAX) && (in_type == SSGPU_FLOAT || in_type == SSGPU_DOUBLE)) {
      // a NaN that is a group's FIRST value stays its MIN / MAX in the reference (aggregation_operators.h:189-228); the kernels skip NaNs,
      // so the group's first value travels next to the partial result and the merged one becomes IF(IS_NAN(first), first, min) -- the
      // plan's own NaN-exact form (lower.cpp), spelled out over the chunks
      names.push_back(std::string(a.output ? a.output : "") + "$first");
      ssgpu_agg r; memset(&r, 0, sizeof(r));
      r.aggregation = SSGPU_FIRST; r.output_type = -1; r.input = a.input; r.output = names.back().c_str();
      haggs.push_back(r); col_fn.push_back(COL_FIRST);
    }
    if (a.aggregation == SSGPU_SUM && in_type == SSGPU_DOUBLE && (a.output_type == -1 || a.output_type == SSGPU_DOUBLE)) {
      names.push_back(std::string(a.output ? a.output : "") + "$res");
      ssgpu_agg r; memset(&r, 0, sizeof(r));
      r.aggregation = SSGPU_SUM_RESIDUAL; r.output_type = -1; r.input = a.input; r.output = names.back().c_str();
      haggs.push_back(r); col_fn.push_back(COL_RESIDUAL);
    }
  }
  std::vector<ssgpu_op> hops(D.ops.begin(), D.ops.begin() + iB + 1);
  hops[(size_t)iB].agg_first = (int32_t)hfirst; hops[(size_t)iB].agg_n = (int32_t)(haggs.size() - hfirst);
  ssgpu_plan* head = nullptr;
  {
    ssgpu_plan_desc dh = base; dh.ops = hops.data(); dh.n_ops = iB + 1; dh.aggs = haggs.data(); dh.n_aggs = (int32_t)haggs.size();
    const int rc = ssgpu_plan_create(c, &dh, &head);
    if (rc != SSGPU_OK) return rc;
  }
  // tail: Scan(partial tables) -> GroupAggregate(the merge functions: COUNT merges as SUM) -> Compute(COUNT back to NOT NULL, every
  // DOUBLE sum = merged sum + merged residual, residuals projected away: the GroupAggregate's own schema) -> the operations above
  const Schema& hs = head->result_schema;
  const size_t nk = hs.size() - col_fn.size();
  std::vector<ssgpu_attr> t_in;
  for (auto& a : hs) t_in.push_back(ssgpu_attr{a.name.c_str(), a.dtype, a.nullable ? 1 : 0});
  std::vector<ssgpu_expr> texprs(D.exprs.begin(), D.exprs.end());
  std::vector<int32_t> targs(D.expr_args.begin(), D.expr_args.end());
  std::vector<ssgpu_proj> tprojs(D.projs.begin(), D.projs.end());
  std::vector<ssgpu_agg> taggs(D.aggs.begin(), D.aggs.end());
  const int32_t kp_first = (int32_t)tprojs.size();
  for (size_t k = 0; k < nk; ++k) { ssgpu_proj pr; memset(&pr, 0, sizeof(pr)); pr.kind = SSGPU_PROJ_AT; pr.position = (int32_t)k; pr.name = ""; pr.alias = ""; tprojs.push_back(pr); }
  const int32_t ma_first = (int32_t)taggs.size();
  for (size_t j = 0; j < col_fn.size(); ++j) {
    ssgpu_agg m; memset(&m, 0, sizeof(m));
    m.aggregation = (col_fn[j] == SSGPU_COUNT || col_fn[j] == COL_RESIDUAL) ? SSGPU_SUM : col_fn[j] == COL_FIRST ? SSGPU_FIRST : col_fn[j];
    m.output_type = -1; m.input = hs[nk + j].name.c_str(); m.output = hs[nk + j].name.c_str();
    taggs.push_back(m);
  }
  auto add_expr = [&](int kind, int op, int dtype, const char* name, std::initializer_list<int32_t> kids, int64_t i64 = 0) -> int32_t {
    ssgpu_expr e; memset(&e, 0, sizeof(e));
    e.kind = kind; e.op = op; e.dtype = dtype; e.first_arg = (int32_t)targs.size(); e.nargs = (int32_t)kids.size(); e.i64 = i64; e.name = name ? name : "";
    for (int32_t k : kids) targs.push_back(k);
    texprs.push_back(e);
    return (int32_t)texprs.size() - 1;
  };
  std::vector<int32_t> outs;
  for (size_t k = 0; k < nk; ++k) outs.push_back(add_expr(SSGPU_EXPR_ATTR_NAMED, 0, 0, hs[k].name.c_str(), {}));
  for (size_t j = 0; j < col_fn.size(); ++j) {
    const char* nm = hs[nk + j].name.c_str();
    if (col_fn[j] == COL_RESIDUAL || col_fn[j] == COL_FIRST) continue;
    const int32_t self = add_expr(SSGPU_EXPR_ATTR_NAMED, 0, 0, nm, {});
    if (j + 1 < col_fn.size() && col_fn[j + 1] == COL_FIRST) {
      const char* fn = hs[nk + j + 1].name.c_str();
      const int32_t f1 = add_expr(SSGPU_EXPR_ATTR_NAMED, 0, 0, fn, {}), f2 = add_expr(SSGPU_EXPR_ATTR_NAMED, 0, 0, fn, {});
      const int32_t isnan = add_expr(SSGPU_EXPR_OP, 156 /* OPERATOR_IS_NAN */, 0, "", {f1});
      const int32_t pick = add_expr(SSGPU_EXPR_OP, 204 /* OPERATOR_IF */, 0, "", {isnan, f2, self});
      outs.push_back(add_expr(SSGPU_EXPR_ALIAS, 0, 0, nm, {pick}));
      continue;
    }
    if (col_fn[j] == SSGPU_COUNT) {
      const int32_t zero = add_expr(SSGPU_EXPR_CONST, 0, hs[nk + j].dtype, "", {}, 0);
      const int32_t ifnull = add_expr(SSGPU_EXPR_OP, 220 /* OPERATOR_IFNULL */, 0, "", {self, zero});
      outs.push_back(add_expr(SSGPU_EXPR_ALIAS, 0, 0, nm, {ifnull}));
    } else if (j + 1 < col_fn.size() && col_fn[j + 1] == COL_RESIDUAL) {
      const int32_t res = add_expr(SSGPU_EXPR_ATTR_NAMED, 0, 0, hs[nk + j + 1].name.c_str(), {});
      const int32_t sum = add_expr(SSGPU_EXPR_OP, 0 /* OPERATOR_ADD */, 0, "", {self, res});
      outs.push_back(add_expr(SSGPU_EXPR_ALIAS, 0, 0, nm, {sum}));
    } else outs.push_back(self);
  }
  int32_t root;
  { ssgpu_expr e; memset(&e, 0, sizeof(e)); e.kind = SSGPU_EXPR_COMPOUND; e.first_arg = (int32_t)targs.size(); e.nargs = (int32_t)outs.size(); e.name = "";
    for (int32_t k : outs) targs.push_back(k);
    texprs.push_back(e); root = (int32_t)texprs.size() - 1; }
  std::vector<ssgpu_op> tops;
  { ssgpu_op o; memset(&o, 0, sizeof(o)); o.kind = SSGPU_OP_SCAN; o.child = -1; o.expr = -1; o.child2 = -1; tops.push_back(o); }
  { ssgpu_op o; memset(&o, 0, sizeof(o)); o.kind = SSGPU_OP_GROUP_AGGREGATE; o.child = 0; o.expr = -1; o.child2 = -1; o.proj_first = kp_first; o.proj_n = (int32_t)nk; o.agg_first = ma_first; o.agg_n = (int32_t)col_fn.size(); tops.push_back(o); }
  { ssgpu_op o; memset(&o, 0, sizeof(o)); o.kind = SSGPU_OP_COMPUTE; o.child = 1; o.expr = root; o.child2 = -1; tops.push_back(o); }
  std::vector<int32_t> remap(D.ops.size(), -1);
  remap[(size_t)iB] = 2;
  bool tail_has_aux = false;
  for (size_t j = (size_t)iB + 1; j < D.ops.size(); ++j) {
    ssgpu_op o = D.ops[j];
    auto ref = [&](int32_t k) -> int32_t {
      if (k < 0) return k;
      if (remap[(size_t)k] >= 0) return remap[(size_t)k];
      const ssgpu_op& r = D.ops[(size_t)k];
      if (r.kind == SSGPU_OP_SCAN && r.option0 == 1) { tops.push_back(r); tail_has_aux = true; remap[(size_t)k] = (int32_t)tops.size() - 1; return remap[(size_t)k]; }
      return -2;
    };
    o.child = ref(o.child); if (op_has_aux_side(o.kind)) o.child2 = ref(o.child2);
    if (o.child == -2 || o.child2 == -2) { ssgpu_plan_destroy(head); c->err = "chunked execution: the operations above the GroupAggregate read more than its result"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    tops.push_back(o); remap[j] = (int32_t)tops.size() - 1;
  }
  ssgpu_plan* tail = nullptr;
  {
    ssgpu_plan_desc dt; memset(&dt, 0, sizeof(dt));
    dt.input_schema = t_in.data(); dt.n_attrs = (int32_t)t_in.size();
    dt.ops = tops.data(); dt.n_ops = (int32_t)tops.size();
    dt.exprs = texprs.data(); dt.n_exprs = (int32_t)texprs.size();
    dt.expr_args = targs.data(); dt.n_expr_args = (int32_t)targs.size();
    dt.projs = tprojs.data(); dt.n_projs = (int32_t)tprojs.size();
    dt.aggs = taggs.data(); dt.n_aggs = (int32_t)taggs.size();
    dt.sortkeys = D.sortkeys.data(); dt.n_sortkeys = (int32_t)D.sortkeys.size();
    if (tail_has_aux) { dt.aux_schema = aux_attrs.data(); dt.n_aux_attrs = (int32_t)aux_attrs.size(); }
    const int rc = ssgpu_plan_create(c, &dt, &tail);
    if (rc != SSGPU_OK) { ssgpu_plan_destroy(head); return rc; }
  }
  if (tail->result_schema.size() != p->result_schema.size()) { ssgpu_plan_destroy(head); ssgpu_plan_destroy(tail); c->err = "chunked execution: the merged plan's schema differs from the plan's"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  for (size_t i = 0; i < p->result_schema.size(); ++i)
    if (tail->result_schema[i].dtype != p->result_schema[i].dtype || tail->result_schema[i].name != p->result_schema[i].name) {
      ssgpu_plan_destroy(head); ssgpu_plan_destroy(tail); c->err = "chunked execution: the merged plan's schema differs from the plan's (column '" + p->result_schema[i].name + "')"; return SSGPU_ERROR_NOT_IMPLEMENTED;
    }
  *head_out = head; *tail_out = tail;
  return SSGPU_OK;
}
// Which chunked form serves the plan (and the derived plans of kind 3, made once per plan): 1 = ScalarAggregate state fold (the caller's own code)
static int stream_job_prepare(ssgpu_plan* p, int* kind_out, bool for_run = true) {
  ssgpu_ctx* c = p->ctx;
  if (p->stages.size() == 1 && p->stages[0].kind == STAGE_SCALAR_AGG) { *kind_out = 1; return SSGPU_OK; }
  if (!p->stream_job) {
    int kind = 0, iB = -1;
    bool row_local = !p->stages.empty();
    for (auto& st : p->stages)
      row_local = row_local && ((st.kind == STAGE_MATERIALIZE && st.distinct_cols.empty() && !st.has_segment && !st.has_rank && st.concat.empty()) || st.kind == STAGE_JOIN_EXPAND);
    if (row_local) kind = 2;
    else {
      // the path from the root down to the scan of the plan's input; its lowest operation that is not row-local
      std::vector<int> path;
      for (int i = (int)p->desc.ops.size() - 1; i >= 0; i = p->desc.ops[(size_t)i].child) path.push_back(i);
      for (size_t k = path.size(); k-- > 0;) {
        const ssgpu_op& o = p->desc.ops[(size_t)path[k]];
        if (o.kind == SSGPU_OP_SCAN || o.kind == SSGPU_OP_COMPUTE || o.kind == SSGPU_OP_FILTER || o.kind == SSGPU_OP_PROJECT || op_has_aux_side(o.kind)) continue;
        if (o.kind == SSGPU_OP_GROUP_AGGREGATE && o.option0 == 0) { kind = 3; iB = path[k]; }
        break;
      }
    }
    if (!kind) {
      c->err = "chunked staging serves plans of row-local operations (Filter / Compute / Project / HashJoin / ForeignFilter / RowidMergeJoin), ScalarAggregates over them, and plans whose "
               "first blocking operation is a GroupAggregate without a key limit; other plans take device columns (ssgpu_block_upload + ssgpu_plan_run_block)";
      return SSGPU_ERROR_NOT_IMPLEMENTED;
    }
    ssgpu_plan* head = p; ssgpu_plan* tail = nullptr;
    if (kind == 3) { const int rc = stream_job_build_group(p, iB, &head, &tail); if (rc != SSGPU_OK) return rc; }
    p->stream_job = new ssgpu_plan::StreamJob;
    p->stream_job->kind = kind; p->stream_job->head = head; p->stream_job->tail = tail;
  }
  *kind_out = p->stream_job->kind;
  if (!for_run) return SSGPU_OK;
  ssgpu_plan::StreamJob& J = *p->stream_job;
  J.acc_rows = 0;
  for (ssgpu_plan* q : {J.head, J.tail}) {
    if (!q || q == p) continue;
    q->aux_cols = p->aux_cols; q->aux_rows = p->aux_rows; q->dict = p->dict; q->dict_gen = p->dict_gen; q->quota.limit = p->quota.limit;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  stream_job_reset_out(J.head);
  *kind_out = J.kind;
  return SSGPU_OK;
}
// one staged chunk (device columns, `n` rows, the chunk's first row id `base`) through the head plan; its result rows join the accumulation
static int stream_job_chunk(ssgpu_plan* p, const ssgpu_column* dev, int32_t n_cols, int64_t n, int64_t base) {
  ssgpu_ctx* c = p->ctx; ssgpu_plan::StreamJob& J = *p->stream_job; ssgpu_plan* h = J.head;
  if (h != p && p->interrupted.exchange(0)) { c->err = "interrupted"; return SSGPU_INTERRUPTED; }   // (Cursor::Interrupt reaches the plan the caller holds; the derived plans run on its behalf)
  int rc = run_plan(h, dev, n_cols, n, base, false);
  if (rc == SSGPU_OK) rc = settle_plan(h);
  if (rc == SSGPU_OK) rc = check_error_flags(h);
  if (rc != SSGPU_OK) return rc;
  if (J.kind == 3) h->nan_seen = false;   // (NaNs a floating MIN / MAX skipped: the group's FIRST value travels next to it and the tail decides -- stream_job_build_group)
  if (J.kind == 2) { rc = fix_nan_minmax(h); if (rc != SSGPU_OK) return rc; }
  int64_t rows = 0;
  rc = stage_rows(h, h->exec.size() - 1, &rows);
  if (rc != SSGPU_OK) return rc;
  StageExec& ex = h->exec.back();
  const size_t nc = ex.out.size();
  if (J.acc_data.size() != nc) {
    if (!J.acc_data.empty()) { c->err = "chunked execution: result shape changed"; return SSGPU_ERROR_HIP; }
    J.acc_data = std::vector<DevBuf>(nc); J.acc_nulls = std::vector<DevBuf>(nc); J.acc_cap = 0;
  }
  if (J.acc_rows + rows > J.acc_cap) {      // grow: twice what is needed, the rows so far move over
    QuotaScope quota_scope(&p->quota);
    int64_t cap = std::max<int64_t>((J.acc_rows + rows) * 2, 1 << 16);
    if (J.kind == 2 && J.rows_hint > cap) {
      size_t row_bytes = 0, free_b = 0, total_b = 0;
      for (size_t i = 0; i < nc; ++i) row_bytes += ex.out[i].width + (ex.out[i].nullable ? 1u : 0u);
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (size_t)J.rows_hint * row_bytes <= free_b / 4) cap = J.rows_hint;
      else (void)hipGetLastError();
    }
    for (size_t i = 0; i < nc; ++i) {
      DevBuf bigger;
      if (bigger.ensure((size_t)cap * ex.out[i].width + 16) != hipSuccess) { (void)hipGetLastError(); c->err = "chunked execution: the accumulated result does not fit the device"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
      if (J.acc_rows) HIP_TRY(c, hipMemcpyAsync(bigger.p, J.acc_data[i].p, (size_t)J.acc_rows * ex.out[i].width, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      std::swap(bigger.p, J.acc_data[i].p); std::swap(bigger.cap, J.acc_data[i].cap); std::swap(bigger.q, J.acc_data[i].q);
      if (!ex.out[i].nullable) continue;
      DevBuf bn;
      if (bn.ensure((size_t)cap + 16) != hipSuccess) { (void)hipGetLastError(); c->err = "chunked execution: the accumulated result does not fit the device"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
      if (J.acc_rows) HIP_TRY(c, hipMemcpyAsync(bn.p, J.acc_nulls[i].p, (size_t)J.acc_rows, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      std::swap(bn.p, J.acc_nulls[i].p); std::swap(bn.cap, J.acc_nulls[i].cap); std::swap(bn.q, J.acc_nulls[i].q);
    }
    J.acc_cap = cap;
  }
  for (size_t i = 0; i < nc && rows > 0; ++i) {
    HIP_TRY(c, hipMemcpyAsync(J.acc_data[i].as<char>() + (size_t)J.acc_rows * ex.out[i].width, ex.out[i].data.p, (size_t)rows * ex.out[i].width, hipMemcpyDeviceToDevice, c->stream));
    if (ex.out[i].nullable) HIP_TRY(c, hipMemcpyAsync(J.acc_nulls[i].as<char>() + J.acc_rows, ex.out[i].nulls.p, (size_t)rows, hipMemcpyDeviceToDevice, c->stream));
  }
  J.acc_rows += rows;
  return SSGPU_OK;
}
// the end of the input: kind 2 -- the accumulation IS the result (installed as the last stage's columns); kind 3 -- the tail plan over it
static int stream_job_finish(ssgpu_plan* p, ssgpu_result** out) {
  ssgpu_ctx* c = p->ctx; ssgpu_plan::StreamJob& J = *p->stream_job;
  if (J.kind == 3) {
    if (p->interrupted.exchange(0)) { c->err = "interrupted"; return SSGPU_INTERRUPTED; }
    std::vector<ssgpu_column> cols(J.acc_data.size());
    StageExec& hx = J.head->exec.back();
    for (size_t i = 0; i < cols.size(); ++i) { cols[i].data = J.acc_data[i].p; cols[i].is_null = hx.out[i].nullable ? J.acc_nulls[i].as<uint8_t>() : nullptr; }
    int rc = run_plan(J.tail, cols.data(), (int32_t)cols.size(), J.acc_rows, 0, false);
    if (rc == SSGPU_OK) rc = settle_plan(J.tail);
    if (rc == SSGPU_OK) rc = check_error_flags(J.tail);
    if (rc == SSGPU_OK) rc = fix_nan_minmax(J.tail);
    if (rc != SSGPU_OK) return rc;
    if (out) *out = &J.tail->result;
    return SSGPU_OK;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  StageExec& ex = p->exec.back();
  for (size_t i = 0; i < ex.out.size(); ++i) {
    ex.out[i].data.release(); ex.out[i].nulls.release();
    ex.out[i].data.set_view(J.acc_data[i].p, J.acc_data[i].cap);
    if (ex.out[i].nullable) ex.out[i].nulls.set_view(J.acc_nulls[i].p, J.acc_nulls[i].cap);
  }
  ex.out_arena.release();
  ex.out_rows = J.acc_rows; ex.out_rows_dev = nullptr; ex.out_capacity = J.acc_cap;
  p->result.fetched.assign(p->result.fetched.size(), false);
  if (out) *out = &p->result;
  return SSGPU_OK;
}

int ssgpu_plan_chunked_form(ssgpu_plan* p, int32_t* kind, const char** head, const char** tail) {
  if (!p || !kind) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  int k = 0;
  const int rc = stream_job_prepare(p, &k, false);
  if (rc != SSGPU_OK) return rc;
  *kind = k;
  if (head) *head = (k == 3 && p->stream_job) ? p->stream_job->head->describe.c_str() : p->describe.c_str();
  if (tail) *tail = (k == 3 && p->stream_job) ? p->stream_job->tail->describe.c_str() : "";
  return SSGPU_OK;
}

// Chunked staging of a HOST input (ssgpu.h).  Chunk k + 1 is copied on the copy stream while the plan's kernel reads chunk k on the
// compute stream; a staging set is written again only after the run that read it has finished (events, no host wait); every chunk
// leaves its partial state (the multi-GPU form: run_plan(partial)), and ONE launch folds the states in chunk (= row) order and emits.
int ssgpu_plan_run_host(ssgpu_plan* p, const ssgpu_column* host_cols, int32_t n_cols, int64_t rows, int64_t chunk_rows, ssgpu_result** out) {
  if (!p || (!host_cols && n_cols)) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (!c || c->device < 0) { if (c) c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  if (n_cols != (int)p->desc.input_schema.size() || rows < 0) { c->err = "ssgpu_plan_run_host: column count / row count do not fit the plan's input"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  HIP_TRY(c, hipSetDevice(c->device));
  int job_kind = 0;
  { const int jrc = stream_job_prepare(p, &job_kind); if (jrc != SSGPU_OK) return jrc; }
  if (p->stream_job) p->stream_job->rows_hint = rows;
  if (chunk_rows <= 0) chunk_rows = 1 << 24;
  const int64_t n_chunks = std::max<int64_t>(1, (rows + chunk_rows - 1) / chunk_rows);
  const Schema& schema = p->desc.input_schema;
  for (int b = 0; b < 2; ++b) { p->host_stage_data[b].resize((size_t)n_cols); p->host_stage_nulls[b].resize((size_t)n_cols); }
  for (int32_t i = 0; i < n_cols; ++i) {
    if (dtype_width(schema[i].dtype) == 0) { c->err = "ssgpu_plan_run_host: variable-length columns travel as dictionary codes (INT32)"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
    if (!host_cols[i].data && rows) { c->err = "ssgpu_plan_run_host: a column without data"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  }
  const size_t state_bytes = job_kind == 1 ? (size_t)SSGPU_STATE_ARRAYS * (size_t)std::max(p->stages[0].main.n_slots, 1) * 8 : 0;
  if (job_kind == 1) HIP_TRY(c, p->host_states.ensure((size_t)n_chunks * state_bytes));
  hipEvent_t uploaded[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
  auto drop_events = [&]() { for (int b = 0; b < 2; ++b) { if (uploaded[b]) (void)hipEventDestroy(uploaded[b]); if (consumed[b]) (void)hipEventDestroy(consumed[b]); } };
  for (int b = 0; b < 2; ++b)
    if (hipEventCreateWithFlags(&uploaded[b], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&consumed[b], hipEventDisableTiming) != hipSuccess) {
      drop_events(); c->err = "hipEventCreate failed"; return SSGPU_ERROR_HIP;
    }
  const int64_t cap = std::min<int64_t>(chunk_rows, std::max<int64_t>(rows, 1));
  auto upload = [&](int64_t k) -> int {     // chunk k into staging set k & 1, on the copy stream
    const int b = (int)(k & 1);
    const int64_t lo = k * chunk_rows, n = std::min<int64_t>(chunk_rows, rows - lo);
    if (k >= 2) HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, consumed[b], 0));   // (the run over chunk k - 2 read this set)
    for (int32_t i = 0; i < n_cols; ++i) {
      const size_t w = (size_t)dtype_width(schema[i].dtype);
      HIP_TRY(c, p->host_stage_data[b][(size_t)i].ensure((size_t)cap * w));
      if (n > 0) HIP_TRY(c, hipMemcpyAsync(p->host_stage_data[b][(size_t)i].p, static_cast<const char*>(host_cols[i].data) + (size_t)lo * w, (size_t)n * w, hipMemcpyHostToDevice, c->copy_stream));
      if (!schema[i].nullable) continue;
      HIP_TRY(c, p->host_stage_nulls[b][(size_t)i].ensure((size_t)cap));
      if (n <= 0) continue;
      if (host_cols[i].is_null) HIP_TRY(c, hipMemcpyAsync(p->host_stage_nulls[b][(size_t)i].p, host_cols[i].is_null + lo, (size_t)n, hipMemcpyHostToDevice, c->copy_stream));
      else HIP_TRY(c, hipMemsetAsync(p->host_stage_nulls[b][(size_t)i].p, 0, (size_t)n, c->copy_stream));
    }
    HIP_TRY(c, hipEventRecord(uploaded[b], c->copy_stream));
    return SSGPU_OK;
  };
  int rc = upload(0);
  std::vector<ssgpu_column> dev((size_t)n_cols);
  for (int64_t k = 0; rc == SSGPU_OK && k < n_chunks; ++k) {
    const int b = (int)(k & 1);
    const int64_t lo = k * chunk_rows, n = std::max<int64_t>(0, std::min<int64_t>(chunk_rows, rows - lo));
    if (k + 1 < n_chunks) { rc = upload(k + 1); if (rc != SSGPU_OK) break; }     // (queued BEFORE this chunk's run: the copy overlaps the kernel)
    if (hipStreamWaitEvent(c->stream, uploaded[b], 0) != hipSuccess) { c->err = "hipStreamWaitEvent failed"; rc = SSGPU_ERROR_HIP; break; }
    for (int32_t i = 0; i < n_cols; ++i) {
      dev[(size_t)i].data = p->host_stage_data[b][(size_t)i].p;
      dev[(size_t)i].is_null = schema[i].nullable ? p->host_stage_nulls[b][(size_t)i].as<uint8_t>() : nullptr;
    }
    if (job_kind != 1) {     // the chunk through the head plan, its result rows appended (stream_job_chunk)
      rc = stream_job_chunk(p, dev.data(), n_cols, n, lo);
      if (rc != SSGPU_OK) break;
      if (hipEventRecord(consumed[b], c->stream) != hipSuccess) { c->err = "ssgpu_plan_run_host: queueing a chunk failed"; rc = SSGPU_ERROR_HIP; break; }
      continue;
    }
    p->keep_error_flags = k > 0;
    rc = run_plan(p, dev.data(), n_cols, n, lo, true);
    p->keep_error_flags = false;
    if (rc != SSGPU_OK) break;
    if (hipMemcpyAsync(p->host_states.as<char>() + (size_t)k * state_bytes, p->exec[0].state.p, state_bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipEventRecord(consumed[b], c->stream) != hipSuccess) { c->err = "ssgpu_plan_run_host: queueing a chunk failed"; rc = SSGPU_ERROR_HIP; break; }
  }
  if (rc != SSGPU_OK) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamSynchronize(c->stream); drop_events(); return rc; }
  drop_events();
  if (job_kind != 1) {
    rc = stream_job_finish(p, out);
    if (rc != SSGPU_OK) return rc;
    p->last_cols.clear(); p->last_rows = rows;
    return SSGPU_OK;
  }
  rc = ssgpu_plan_fold_finalize(p, p->host_states.p, (int32_t)n_chunks, out);
  if (rc != SSGPU_OK) return rc;
  p->last_cols.clear(); p->last_rows = rows;     // (nothing of this run can be repeated from device columns: they were staging sets)
  return settle_plan(p) == SSGPU_OK ? check_error_flags(p) : SSGPU_ERROR_HIP;
}

// ---- the push form of chunked staging: begin / push / push ... / finish (ssgpu.h) --------------------------------------------------------
static int stream_abort(ssgpu_plan* p, int rc) {
  ssgpu_ctx* c = p->ctx;
  (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamSynchronize(c->stream);
  p->host_stream.drop_events(); p->host_stream.open = false; p->host_stream.rc = rc; p->keep_error_flags = false;
  return rc;
}
// the filled part of pinned set b -> device set b -> one partial run -> its state appended to host_states
static int stream_flush(ssgpu_plan* p, int b, int64_t n) {
  ssgpu_ctx* c = p->ctx; ssgpu_plan::HostStream& hs = p->host_stream;
  const Schema& schema = p->desc.input_schema;
  const int32_t n_cols = (int32_t)schema.size();
  if (hs.in_flight[b]) HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, hs.consumed[b], 0));   // (the run that read device set b)
  for (int32_t i = 0; i < n_cols; ++i) {
    const size_t w = (size_t)dtype_width(schema[i].dtype);
    HIP_TRY(c, p->host_stage_data[b][(size_t)i].ensure((size_t)hs.chunk_rows * w));
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(p->host_stage_data[b][(size_t)i].p, hs.pin_data[b][(size_t)i].p, (size_t)n * w, hipMemcpyHostToDevice, c->copy_stream));
    if (!schema[i].nullable) continue;
    HIP_TRY(c, p->host_stage_nulls[b][(size_t)i].ensure((size_t)hs.chunk_rows));
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(p->host_stage_nulls[b][(size_t)i].p, hs.pin_nulls[b][(size_t)i].p, (size_t)n, hipMemcpyHostToDevice, c->copy_stream));
  }
  HIP_TRY(c, hipEventRecord(hs.uploaded[b], c->copy_stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, hs.uploaded[b], 0));
  std::vector<ssgpu_column> dev((size_t)n_cols);
  for (int32_t i = 0; i < n_cols; ++i) {
    dev[(size_t)i].data = p->host_stage_data[b][(size_t)i].p;
    dev[(size_t)i].is_null = schema[i].nullable ? p->host_stage_nulls[b][(size_t)i].as<uint8_t>() : nullptr;
  }
  if (hs.kind != 1) {
    const int jrc = stream_job_chunk(p, dev.data(), n_cols, n, hs.pushed - n);
    if (jrc != SSGPU_OK) return jrc;
    HIP_TRY(c, hipEventRecord(hs.consumed[b], c->stream));
    hs.in_flight[b] = true;
    ++hs.chunks;
    return SSGPU_OK;
  }
  p->keep_error_flags = hs.chunks > 0;
  const int rc = run_plan(p, dev.data(), n_cols, n, hs.pushed - n, true);
  p->keep_error_flags = false;
  if (rc != SSGPU_OK) return rc;
  const size_t state_bytes = (size_t)SSGPU_STATE_ARRAYS * (size_t)std::max(p->stages[0].main.n_slots, 1) * 8;
  if ((size_t)(hs.chunks + 1) * state_bytes > p->host_states.cap) {     // the states so far move into a larger buffer (they are a few hundred bytes each)
    DevBuf bigger;
    HIP_TRY(c, bigger.ensure(std::max<size_t>((size_t)(hs.chunks + 1) * state_bytes * 2, 64 * state_bytes)));
    if (hs.chunks) HIP_TRY(c, hipMemcpyAsync(bigger.p, p->host_states.p, (size_t)hs.chunks * state_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::swap(bigger.p, p->host_states.p); std::swap(bigger.cap, p->host_states.cap); std::swap(bigger.q, p->host_states.q);
  }
  HIP_TRY(c, hipMemcpyAsync(p->host_states.as<char>() + (size_t)hs.chunks * state_bytes, p->exec[0].state.p, state_bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(hs.consumed[b], c->stream));
  hs.in_flight[b] = true;
  ++hs.chunks;
  return SSGPU_OK;
}
int ssgpu_plan_stream_begin(ssgpu_plan* p, int64_t chunk_rows) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (!c || c->device < 0) { if (c) c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  const Schema& schema = p->desc.input_schema;
  for (auto& a : schema) if (dtype_width(a.dtype) == 0) { c->err = "ssgpu_plan_stream_begin: variable-length columns travel as dictionary codes (INT32)"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  HIP_TRY(c, hipSetDevice(c->device));
  ssgpu_plan::HostStream& hs = p->host_stream;
  if (hs.open) (void)stream_abort(p, SSGPU_OK);     // (an unfinished stream is dropped)
  { int kind = 0; const int jrc = stream_job_prepare(p, &kind); if (jrc != SSGPU_OK) return jrc; hs.kind = kind; }
  if (p->stream_job) p->stream_job->rows_hint = 0;      // (a pushed stream's length is not known)
  hs.chunk_rows = chunk_rows > 0 ? chunk_rows : (1 << 22); hs.fill = 0; hs.pushed = 0; hs.chunks = 0; hs.cur = 0; hs.rc = SSGPU_OK;
  for (int b = 0; b < 2; ++b) {
    p->host_stage_data[b].resize(schema.size()); p->host_stage_nulls[b].resize(schema.size());
    hs.pin_data[b].resize(schema.size()); hs.pin_nulls[b].resize(schema.size());
    for (size_t i = 0; i < schema.size(); ++i) {
      HIP_TRY(c, hs.pin_data[b][i].ensure((size_t)hs.chunk_rows * (size_t)dtype_width(schema[i].dtype)));
      if (schema[i].nullable) HIP_TRY(c, hs.pin_nulls[b][i].ensure((size_t)hs.chunk_rows));
    }
    if (hipEventCreateWithFlags(&hs.uploaded[b], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&hs.consumed[b], hipEventDisableTiming) != hipSuccess) {
      hs.drop_events(); c->err = "hipEventCreate failed"; return SSGPU_ERROR_HIP;
    }
  }
  hs.open = true;
  return SSGPU_OK;
}
int ssgpu_plan_stream_push(ssgpu_plan* p, const ssgpu_column* host_cols, int32_t n_cols, int64_t rows) {
  if (!p || !p->host_stream.open) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx; ssgpu_plan::HostStream& hs = p->host_stream;
  const Schema& schema = p->desc.input_schema;
  if (n_cols != (int32_t)schema.size() || rows < 0 || (!host_cols && rows)) { c->err = "ssgpu_plan_stream_push: column count / row count do not fit the plan's input"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  for (int64_t done = 0; done < rows;) {
    if (hs.fill == 0 && hs.in_flight[hs.cur]) HIP_TRY(c, hipEventSynchronize(hs.uploaded[hs.cur]));   // (the copy that last read this pinned set)
    const int64_t n = std::min<int64_t>(rows - done, hs.chunk_rows - hs.fill);
    for (int32_t i = 0; i < n_cols; ++i) {
      const size_t w = (size_t)dtype_width(schema[i].dtype);
      memcpy(static_cast<char*>(hs.pin_data[hs.cur][(size_t)i].p) + (size_t)hs.fill * w, static_cast<const char*>(host_cols[i].data) + (size_t)done * w, (size_t)n * w);
      if (!schema[i].nullable) continue;
      if (host_cols[i].is_null) memcpy(static_cast<char*>(hs.pin_nulls[hs.cur][(size_t)i].p) + hs.fill, host_cols[i].is_null + done, (size_t)n);
      else memset(static_cast<char*>(hs.pin_nulls[hs.cur][(size_t)i].p) + hs.fill, 0, (size_t)n);
    }
    hs.fill += n; hs.pushed += n; done += n;
    if (hs.fill == hs.chunk_rows) {
      const int rc = stream_flush(p, hs.cur, hs.fill);
      if (rc != SSGPU_OK) return stream_abort(p, rc);
      hs.cur ^= 1; hs.fill = 0;
    }
  }
  return SSGPU_OK;
}
int ssgpu_plan_stream_finish(ssgpu_plan* p, ssgpu_result** out) {
  if (!p || !p->host_stream.open) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_plan::HostStream& hs = p->host_stream;
  if (hs.fill > 0 || hs.chunks == 0) {     // the last, partly filled set (or no row at all: the one row of an empty input)
    const int rc = stream_flush(p, hs.cur, hs.fill);
    if (rc != SSGPU_OK) return stream_abort(p, rc);
  }
  const int64_t n_chunks = hs.chunks, rows = hs.pushed;
  hs.drop_events(); hs.open = false;
  if (hs.kind != 1) {
    const int jrc = stream_job_finish(p, out);
    if (jrc != SSGPU_OK) return jrc;
    p->last_cols.clear(); p->last_rows = rows;
    return SSGPU_OK;
  }
  int rc = ssgpu_plan_fold_finalize(p, p->host_states.p, (int32_t)n_chunks, out);
  if (rc != SSGPU_OK) return rc;
  p->last_cols.clear(); p->last_rows = rows;
  return settle_plan(p) == SSGPU_OK ? check_error_flags(p) : SSGPU_ERROR_HIP;
}

int ssgpu_plan_set_aux_input(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (n_cols != (int)p->desc.aux_schema.size()) { p->ctx->err = "column count does not match the plan's auxiliary schema"; return SSGPU_ERROR_ATTRIBUTE_COUNT_MISMATCH; }
  if (rows < 0 || rows >= (int64_t)VM_NONE) { p->ctx->err = "auxiliary input: bad row count"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  p->aux_cols.assign(cols, cols + n_cols);
  p->aux_rows = rows;
  return SSGPU_OK;
}

int ssgpu_plan_run_partial(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, int64_t base) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  return run_plan(p, cols, n_cols, rows, base, true);
}

// ---- dense-slot GroupAggregate across ranks (ssgpu.h) -----------------------------------------------------------------------
static int dense_stage_of(ssgpu_plan* p, bool need_device) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (need_device && (!c || c->device < 0)) { if (c) c->err = "no gfx950 device bound to this context (bind-only context)"; return SSGPU_ERROR_NO_DEVICE; }
  if (p->stages.size() != 1 || p->stages[0].kind != STAGE_GROUP_AGG || !dense_eligible(c, p->stages[0])) {
    c->err = "dense slots need a plan that is ONE plain GroupAggregate stage over integer-like key columns"; return SSGPU_ERROR_NOT_IMPLEMENTED;
  }
  for (auto& a : p->stages[0].aggs) if (a.gather_col >= 0) { c->err = "FIRST / LAST aggregates take their values from the shard that saw the row: not in the dense exchange"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  return SSGPU_OK;
}
int ssgpu_plan_key_ranges(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, int32_t* n_keys, uint64_t* lo, uint64_t* hi) {
  int rc = dense_stage_of(p, true);
  if (rc != SSGPU_OK) return rc;
  ssgpu_ctx* c = p->ctx;
  if (n_cols != (int)p->desc.input_schema.size() || rows < 0 || !n_keys || !lo || !hi) { c->err = "key ranges: bad arguments"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  HIP_TRY(c, hipSetDevice(c->device));
  InCols in; in.cols.assign(cols, cols + n_cols); in.rows = rows;
  StageExec& ex = p->exec[0];
  rc = order_after_uploads(c);
  if (rc != SSGPU_OK) return rc;
  rc = dense_find_ranges(p, p->stages[0], ex, in);
  if (rc != SSGPU_OK) return rc;
  *n_keys = (int32_t)ex.dense.n_keys;
  for (uint32_t k = 0; k < ex.dense.n_keys; ++k) { lo[k] = ex.dense.lo[k]; hi[k] = ex.dense.hi[k]; }
  return SSGPU_OK;
}
int ssgpu_plan_set_dense(ssgpu_plan* p, int32_t n_keys, const uint64_t* lo, const uint64_t* hi, int32_t n_chunks, ssgpu_dense_layout* out) {
  int rc = dense_stage_of(p, false);
  if (rc != SSGPU_OK) return rc;
  ssgpu_ctx* c = p->ctx; const Stage& st = p->stages[0]; StageExec& ex = p->exec[0];
  if (n_keys != (int32_t)st.plain.keys.size() || !lo || !hi || n_chunks < 1) { c->err = "dense ranges: one (lo, hi) pair per group key and at least one chunk"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  ex.dense.n_keys = (uint32_t)n_keys;
  for (int32_t k = 0; k < n_keys; ++k) { ex.dense.lo[k] = lo[k]; ex.dense.hi[k] = hi[k]; }
  if (!dense_configure(c, st, ex, (uint32_t)n_chunks, true, 0)) {
    ex.dense.on = false; ex.dense.fixed = false;
    c->err = "dense ranges: the table of these ranges would exceed 2^21 slots (or 4096 partitions)"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  }
  ex.dense.on = true; ex.dense.fixed = true; ex.dense.failed = false; ex.dense.widened = 0;
  ex.part_seg_growth = std::max(ex.part_seg_growth, 1u);
  if (out) {
    uint32_t entry, fixed, slot_bytes;
    dense_entry_bytes(st, &entry, &fixed, &slot_bytes);
    memset(out, 0, sizeof(*out));
    out->slots = (int64_t)ex.dense.slots; out->n_parts = (int32_t)ex.dense.np; out->part_cap = (int32_t)ex.dense.cap;
    out->chunk_slots = (int64_t)(ex.dense.np / ex.dense.n_chunks) * ex.dense.cap; out->chunk_bytes = (int64_t)ex.dense.chunk_bytes;
    out->n_gaggs = std::max(st.n_gaggs, 1); out->has_counts = slot_bytes > 8u + (uint32_t)out->n_gaggs * 8u ? 1 : 0;
  }
  return SSGPU_OK;
}
int ssgpu_plan_run_dense(ssgpu_plan* p, const ssgpu_column* cols, int32_t n_cols, int64_t rows, void* table) {
  int rc = dense_stage_of(p, true);
  if (rc != SSGPU_OK) return rc;
  StageExec& ex = p->exec[0];
  if (!ex.dense.on || !ex.dense.fixed || !table) { p->ctx->err = "ssgpu_plan_run_dense: set the ranges first (ssgpu_plan_set_dense) and pass a table buffer"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  ex.dense_table = table;
  rc = run_plan(p, cols, n_cols, rows, 0, false);
  ex.dense_table = nullptr;
  if (rc == SSGPU_OK && !ex.dense.on) { p->ctx->err = "the dense table could not be laid out for this input (a partition's segments would not fit)"; rc = SSGPU_ERROR_MEMORY_EXCEEDED; ex.dense.on = true; }
  return rc;
}
int ssgpu_plan_fold_dense(ssgpu_plan* p, const void* chunks, int32_t n_chunks, ssgpu_result** out) {
  int rc = dense_stage_of(p, true);
  if (rc != SSGPU_OK) return rc;
  ssgpu_ctx* c = p->ctx; Stage& st = p->stages[0]; StageExec& ex = p->exec[0];
  if (!ex.dense.on || !ex.dense.fixed || !chunks || n_chunks < 1) { c->err = "ssgpu_plan_fold_dense: set the ranges first (ssgpu_plan_set_dense)"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  QuotaScope quota_scope(&p->quota);
  HIP_TRY(c, hipSetDevice(c->device));
  rc = prepare_stage(p, 0);
  if (rc != SSGPU_OK) return rc;
  const uint32_t ng = (uint32_t)std::max(st.n_gaggs, 1);
  bool any_cnt = false;
  for (auto& a : st.aggs) any_cnt = any_cnt || a.has_cnt;
  const uint32_t slots = (ex.dense.np / ex.dense.n_chunks) * ex.dense.cap;
  HIP_TRY(c, ex.gkeys.ensure(((size_t)slots + 1) * 8));
  HIP_TRY(c, ex.gacc.ensure(((size_t)slots + 1) * ng * 8));
  HIP_TRY(c, ex.gcnt.ensure(((size_t)slots + 1) * ng * 4));
  HIP_TRY(c, ex.total.ensure(16));
  HIP_TRY(c, ex.dense_flags.ensure(16));
  HIP_TRY(c, ex.gmergeop.ensure(ng * 4));
  HIP_TRY(c, ex.gpattern.ensure(ng * 8));
  if (!ex.pattern_ready) {
    std::vector<uint64_t> pattern(ng, 0);
    std::vector<uint32_t> mop(ng, VM_MERGE_ADD_U64);
    for (size_t i = 0; i < st.group_acc_init.size(); ++i) pattern[i] = st.group_acc_init[i];
    for (size_t i = 0; i < st.group_merge_op.size(); ++i) mop[i] = st.group_merge_op[i];
    HIP_TRY(c, hipMemcpy(ex.gpattern.p, pattern.data(), ng * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(ex.gmergeop.p, mop.data(), ng * 4, hipMemcpyHostToDevice));
    ex.pattern_ready = true;
  }
  DenseFoldParams F; memset(&F, 0, sizeof(F));
  F.chunks = chunks; F.n_chunks = (unsigned int)n_chunks; F.n_gaggs = ng; F.any_cnt = any_cnt ? 1u : 0u; F.slots = slots; F.chunk_bytes = ex.dense.chunk_bytes;
  F.keys = ex.gkeys.as<unsigned long long>(); F.acc = ex.gacc.as<unsigned long long>(); F.cnt = ex.gcnt.as<unsigned int>();
  F.merge_op = ex.gmergeop.as<unsigned int>(); F.flags_out = ex.dense_flags.as<unsigned int>();
  F.clear[0] = ex.total.as<unsigned int>(); F.n_clear[0] = 4;   // the extraction's row count, ticket and gave-up flag
  HIP_TRY(c, ssgpu_launch_dense_fold(F, c->stream));
  p->counters.n_launches += 1;
  p->result.fetched.assign(p->result.fetched.size(), false);
  InCols none;
  rc = extract_groups(p, st, ex, slots, ng, none, 0);
  if (rc != SSGPU_OK) return rc;
  if (out) *out = &p->result;
  return SSGPU_OK;
}
int ssgpu_plan_dense_flags(ssgpu_plan* p, uint32_t* flags, uint32_t* error) {
  int rc = dense_stage_of(p, true);
  if (rc != SSGPU_OK) return rc;
  ssgpu_ctx* c = p->ctx; StageExec& ex = p->exec[0];
  uint32_t w[2] = {0, 0};
  if (ex.dense_flags.p) {
    HIP_TRY(c, hipMemcpyAsync(w, ex.dense_flags.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (flags) *flags = w[0];
  if (error) *error = w[1] & 0xFFu;   // (the NaN-in-MIN/MAX bit is not an error: the fold skips NaNs like every order-independent shape)
  return SSGPU_OK;
}
// A rank whose shard run failed (memory quota, interrupt, anything ssgpu_plan_run_dense returned) must still take part in the
// step's collective, or the other ranks wait in it forever: it sends its table with every chunk header flagged "failed" +
// the return code, and every rank's ssgpu_plan_dense_flags reports it after the fold.
int ssgpu_plan_dense_fail(ssgpu_plan* p, void* table, int32_t code) {
  int rc = dense_stage_of(p, true);
  if (rc != SSGPU_OK) return rc;
  ssgpu_ctx* c = p->ctx; StageExec& ex = p->exec[0];
  if (!ex.dense.fixed || !table || code <= 0) { c->err = "ssgpu_plan_dense_fail: no table layout (ssgpu_plan_set_dense), or no failure code"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, ssgpu_launch_dense_headers(table, ex.dense.n_chunks, ex.dense.chunk_bytes, nullptr, nullptr, c->stream, 8u | ((uint32_t)code << 8)));
  return SSGPU_OK;
}
int ssgpu_plan_dense_grow(ssgpu_plan* p) {
  int rc = dense_stage_of(p, false);
  if (rc != SSGPU_OK) return rc;
  StageExec& ex = p->exec[0];
  if (ex.part_seg_growth >= 64u) { p->ctx->err = "a partition's record segments cannot grow any further (one group holds most of the rows)"; return SSGPU_ERROR_MEMORY_EXCEEDED; }
  ex.part_seg_growth *= 4u;
  return SSGPU_OK;
}

int32_t ssgpu_plan_partial_segments(ssgpu_plan* p, ssgpu_partial_segment* out, int32_t max_segments) {
  if (!p || !p->partial_pending || p->stages.empty()) return 0;
  StageExec& ex = p->exec[0];
  const int ns = p->stages[0].main.n_slots;
  static const int reduce[SSGPU_STATE_ARRAYS] = {0, 0, 0, 0, 1, 2, 1, 2};
  static const int dtype[SSGPU_STATE_ARRAYS] = {SSGPU_INT64, SSGPU_INT64, SSGPU_DOUBLE, SSGPU_DOUBLE, SSGPU_INT64, SSGPU_INT64, SSGPU_DOUBLE, SSGPU_DOUBLE};
  int n = 0;
  for (int i = 0; i < SSGPU_STATE_ARRAYS && n < max_segments; ++i, ++n) {
    out[n].device_ptr = ex.state.as<uint64_t>() + (size_t)i * ns;
    out[n].count = ns; out[n].dtype = dtype[i]; out[n].reduce = reduce[i];
  }
  return n;
}

int32_t ssgpu_plan_recent_kernel_ms(ssgpu_plan* p, double* out_ms, int32_t max) {
  if (!p || !out_ms || max <= 0 || !p->ctx || p->ctx->device < 0) return 0;
  ssgpu_ctx* c = p->ctx;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
  const uint64_t have = std::min<uint64_t>(p->profiled_runs, (uint64_t)ssgpu_plan::kEventRing);
  const uint64_t n = std::min<uint64_t>(have, (uint64_t)max);
  int32_t written = 0;
  for (uint64_t i = p->profiled_runs - n; i < p->profiled_runs; ++i) {
    const int slot = (int)(i % ssgpu_plan::kEventRing);
    float ms = 0.f;
    if (p->ring0[slot] && hipEventElapsedTime(&ms, p->ring0[slot], p->ring1[slot]) == hipSuccess) out_ms[written++] = ms;
  }
  return written;
}

int ssgpu_plan_fold_partials(ssgpu_plan* p, const void* images, int32_t n_images) {
  if (!p || !p->partial_pending || p->stages.empty() || !images || n_images < 1) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  StageExec& ex = p->exec[0];
  const int ns = p->stages[0].main.n_slots;
  HIP_TRY(c, ssgpu_launch_fold_state(static_cast<const uint64_t*>(images), n_images, ex.state.as<uint64_t>(), ns, ex.slot_kind.as<int>(), c->stream));
  return SSGPU_OK;
}

int ssgpu_plan_fold_finalize(ssgpu_plan* p, const void* images, int32_t n_images, ssgpu_result** out) {
  if (!p || !p->partial_pending || p->stages.empty() || !images || n_images < 1) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  StageExec& ex = p->exec[0];
  const int ns = p->stages[0].main.n_slots;
  int n_out = 0;
  const int rc = prepare_scalar_emit(p, 0, &n_out);
  if (rc != SSGPU_OK) return rc;
  HIP_TRY(c, ssgpu_launch_fold_emit(static_cast<const uint64_t*>(images), n_images, ex.state.as<uint64_t>(), ns, ex.slot_kind.as<int>(),
                                    ex.slot_recs.as<VmAccRec>(), ex.emit_descs.as<EmitDesc>(), n_out, c->stream));
  p->counters.n_launches += 1;
  ex.out_rows = 1;
  p->partial_pending = false;
  if (out) *out = &p->result;
  return SSGPU_OK;
}

int ssgpu_plan_finalize(ssgpu_plan* p, ssgpu_result** out) {
  if (!p || !p->partial_pending) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  StageExec& ex = p->exec[0];
  const int ns = p->stages[0].main.n_slots;
  HIP_TRY(c, ssgpu_launch_state_to_slots(ex.state.as<uint64_t>(), ns, ex.slot_kind.as<int>(), ex.slot_recs.as<VmAccRec>(), c->stream));
  int rc = emit_scalar_agg(p, 0);
  if (rc != SSGPU_OK) return rc;
  p->partial_pending = false;
  if (out) *out = &p->result;
  return SSGPU_OK;
}

void ssgpu_result_destroy(ssgpu_result* r) { (void)r; /* owned by the plan: valid until the next run */ }

int ssgpu_result_write_file(ssgpu_result* r, const char* path) {
  if (!r || !r->plan || r->plan->exec.empty()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_plan* p = r->plan; ssgpu_ctx* c = p->ctx;
  int rc = settle_plan(p);
  if (rc != SSGPU_OK) return rc;
  rc = check_error_flags(p);
  if (rc == SSGPU_OK) rc = fix_nan_minmax(p);
  if (rc != SSGPU_OK) return rc;
  const int64_t rows = ssgpu_result_row_count(r);
  if (rows < 0) return SSGPU_ERROR_HIP;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  StageExec& ex = p->exec.back();
  const int n = (int)ex.out.size();
  std::vector<const void*> d(n); std::vector<const uint8_t*> z(n); std::vector<int> w(n); std::vector<bool> nl(n);
  for (int i = 0; i < n; ++i) { d[i] = ex.out[i].data.p; z[i] = ex.out[i].nullable ? ex.out[i].nulls.as<uint8_t>() : nullptr; w[i] = (int)ex.out[i].width; nl[i] = ex.out[i].nullable; }
  return write_view_file(c, path, n, rows, d, z, w, nl);
}

int64_t ssgpu_result_row_count(ssgpu_result* r) {
  if (!r || !r->plan || r->plan->exec.empty()) return -1;
  if (settle_plan(r->plan) != SSGPU_OK) return -1;
  int64_t rows = -1;
  if (stage_rows(r->plan, r->plan->exec.size() - 1, &rows) != SSGPU_OK) return -1;
  r->plan->counters.rows_out = rows;
  return rows;
}
int32_t ssgpu_result_column_count(const ssgpu_result* r) { return r && r->plan ? (int32_t)r->plan->result_schema.size() : 0; }

int ssgpu_result_device_column(ssgpu_result* r, int32_t i, ssgpu_column* out) {
  if (!r || !r->plan) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  // device-resident consumers (the sharded sort / group aggregate) must not pass on the result of a run that hit a
  // signaling division or SQRT error (or that overflowed a table: settled first)
  { int rc = settle_plan(r->plan); if (rc != SSGPU_OK) return rc; rc = check_error_flags(r->plan); if (rc == SSGPU_OK) rc = fix_nan_minmax(r->plan); if (rc != SSGPU_OK) return rc; }
  StageExec& ex = r->plan->exec.back();
  if (i < 0 || i >= (int)ex.out.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  if (concat_of(r->plan, i)) { r->plan->ctx->err = "a CONCAT column exists on the host only (ssgpu_result_column)"; return SSGPU_ERROR_NOT_IMPLEMENTED; }
  out->data = ex.out[i].data.p;
  out->is_null = ex.out[i].nullable ? ex.out[i].nulls.as<uint8_t>() : nullptr;
  return SSGPU_OK;
}

}  // extern "C"

namespace {
// the calendar date of a day count since 1970-01-01 (proleptic Gregorian calendar, any year: 400-year eras of 146097 days)
static void civil_from_days(int64_t z, int64_t* year, unsigned* month, unsigned* day) {
  z += 719468;                                            // days since 0000-03-01
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const unsigned doe = (unsigned)(z - era * 146097);      // day of the era [0, 146096]
  const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const unsigned mp = (5 * doy + 2) / 153;                // month counted from March
  *day = doy - (153 * mp + 2) / 5 + 1;
  *month = mp < 10 ? mp + 3 : mp - 9;
  *year = (int64_t)yoe + era * 400 + (*month <= 2 ? 1 : 0);
}
// PrintTyped<DATE / DATETIME> (types_infrastructure.cc:36-39,92-114): strftime of gmtime, "%Y/%m/%d" resp. "%Y/%m/%d-%H:%M:%S" (glibc's %Y:
// the year as it is, no padding, '-' for years before 0); microseconds are dropped (`value / 1000000`, toward zero)
static void print_time(int64_t seconds, bool with_time, std::string* out) {
  int64_t days = seconds / 86400, sod = seconds % 86400;
  if (sod < 0) { sod += 86400; days -= 1; }
  int64_t y; unsigned m, d; civil_from_days(days, &y, &m, &d);
  char buf[64];
  if (with_time) snprintf(buf, sizeof(buf), "%lld/%02u/%02u-%02d:%02d:%02d", (long long)y, m, d, (int)(sod / 3600), (int)(sod / 60 % 60), (int)(sod % 60));
  else snprintf(buf, sizeof(buf), "%lld/%02u/%02u", (long long)y, m, d);
  *out += buf;
}
// PrintTyped (base/infrastructure/types_infrastructure.cc:45-114): integers in decimal, BOOL as TRUE / FALSE, FLOAT / DOUBLE as
// SimpleFtoa / SimpleDtoa (the shortest of %.6g / %.9g resp. %.15g / %.17g that reads back as the same value), STRING as is
void print_typed(int dtype, const char* cell, const ssgpu_dict* dict, std::string* out) {
  char buf[64];
  switch (dtype) {
    // DATE: `const time_t time = value * (24 * 3600)` is an int32 product in the reference (:105): it leaves the int range beyond
    // +-24855 days (the years 1901 .. 2038) -- undefined there, the wrapped product here
    case SSGPU_DATE: { int32_t v; memcpy(&v, cell, 4); print_time((int64_t)(int32_t)((uint32_t)v * 86400u), false, out); } break;
    case SSGPU_DATETIME: { int64_t v; memcpy(&v, cell, 8); print_time(v / 1000000, true, out); } break;
    case SSGPU_INT32: { int32_t v; memcpy(&v, cell, 4); *out += std::to_string(v); } break;
    case SSGPU_UINT32: { uint32_t v; memcpy(&v, cell, 4); *out += std::to_string(v); } break;
    case SSGPU_INT64: { int64_t v; memcpy(&v, cell, 8); *out += std::to_string((long long)v); } break;
    case SSGPU_UINT64: { uint64_t v; memcpy(&v, cell, 8); *out += std::to_string((unsigned long long)v); } break;
    case SSGPU_BOOL: *out += *cell ? "TRUE" : "FALSE"; break;
    case SSGPU_FLOAT: {
      float v; memcpy(&v, cell, 4);
      if (std::isnan(v)) { *out += "nan"; break; }
      if (std::isinf(v)) { *out += v < 0 ? "-inf" : "inf"; break; }
      snprintf(buf, sizeof(buf), "%.*g", 6, (double)v);
      if (strtof(buf, nullptr) != v) snprintf(buf, sizeof(buf), "%.*g", 9, (double)v);
      *out += buf;
    } break;
    case SSGPU_DOUBLE: {
      double v; memcpy(&v, cell, 8);
      if (std::isnan(v)) { *out += "nan"; break; }
      if (std::isinf(v)) { *out += v < 0 ? "-inf" : "inf"; break; }
      snprintf(buf, sizeof(buf), "%.*g", 15, v);
      if (strtod(buf, nullptr) != v) snprintf(buf, sizeof(buf), "%.*g", 17, v);
      *out += buf;
    } break;
    case SSGPU_STRING: {
      int32_t code; memcpy(&code, cell, 4);
      const char* bytes = nullptr; int32_t len = 0;
      if (dict && ssgpu_dict_decode(dict, code, &bytes, &len) == SSGPU_OK) out->append(bytes, (size_t)len);
    } break;
    default: break;
  }
}

// The STRINGs of a CONCAT column (Stage::ConcatCol): the stage's input rows -- materialised and, for a group aggregate, sorted
// by the keys, so a group's rows are adjacent and in input order -- come to the host with their segment ids; every non-NULL
// value is printed and appended to its group's string, ',' between values (aggregation_operators.h:236-283; the first value
// is assigned, column_aggregator.cc:108-124).  A group without a non-NULL value is NULL.  The strings become a dictionary
// of the result; the column holds its codes.
int build_concat_column(ssgpu_result* r, int32_t col, const Stage::ConcatCol& cc, int64_t out_rows) {
  ssgpu_plan* p = r->plan; ssgpu_ctx* c = p->ctx;
  const size_t si = cc.stage >= 0 ? (size_t)cc.stage : p->stages.size() - 1;
  const Stage& st = p->stages[si]; StageExec& ex = p->exec[si];
  if (cc.src_dtype == SSGPU_STRING && !p->dict) { c->err = "CONCAT of a STRING column needs the plan's dictionary (ssgpu_plan_set_dict)"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  int64_t n = p->last_rows;
  const void* dev_x = nullptr; const uint8_t* dev_z = nullptr;
  if (si == 0) {
    if (cc.src_col >= (int)p->last_cols.size()) return SSGPU_ERROR_UNKNOWN;
    dev_x = p->last_cols[cc.src_col].data; dev_z = p->desc.input_schema[cc.src_col].nullable ? p->last_cols[cc.src_col].is_null : nullptr;
  } else {
    int rc = stage_rows(p, si - 1, &n); if (rc != SSGPU_OK) return rc;
    StageExec& px = p->exec[si - 1];
    dev_x = px.out[cc.src_col].data.p; dev_z = px.out[cc.src_col].nullable ? px.out[cc.src_col].nulls.as<uint8_t>() : nullptr;
  }
  const size_t w = (size_t)dtype_width(cc.src_dtype);
  std::vector<char> x((size_t)n * w); std::vector<uint8_t> z; std::vector<uint32_t> seg;
  if (n) HIP_TRY(c, hipMemcpyAsync(x.data(), dev_x, x.size(), hipMemcpyDeviceToHost, c->stream));
  if (dev_z && n) { z.resize((size_t)n); HIP_TRY(c, hipMemcpyAsync(z.data(), dev_z, z.size(), hipMemcpyDeviceToHost, c->stream)); }
  if (st.kind == STAGE_CLUSTERS && n) { seg.resize((size_t)n); HIP_TRY(c, hipMemcpyAsync(seg.data(), ex.seg_id.p, seg.size() * 4, hipMemcpyDeviceToHost, c->stream)); }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<std::string> text((size_t)out_rows); std::vector<uint8_t> has((size_t)out_rows, 0);
  // DISTINCT CONCAT: the DistinctAggregator in front of the CONCAT lets a value through at its first occurrence in the result row
  // (column_aggregator.cc:308-376: one set per result index; NULLs never count).  Values compare as the device's other DISTINCT
  // aggregates compare them: by their bits, -0.0 as +0.0.  A group's rows are adjacent here, so ONE set, emptied at every new group.
  std::unordered_set<uint64_t> seen; size_t seen_group = (size_t)-1;
  for (int64_t i = 0; i < n; ++i) {
    if (!z.empty() && z[(size_t)i]) continue;
    const size_t g = seg.empty() ? 0 : seg[(size_t)i];
    if (g >= (size_t)out_rows) continue;
    if (cc.distinct) {
      if (g != seen_group) { seen.clear(); seen_group = g; }
      uint64_t bits = 0; memcpy(&bits, x.data() + (size_t)i * w, w);
      if (cc.src_dtype == SSGPU_DOUBLE && bits == 0x8000000000000000ull) bits = 0;
      if (cc.src_dtype == SSGPU_FLOAT && bits == 0x80000000ull) bits = 0;
      if (!seen.insert(bits).second) continue;
    }
    if (has[g]) text[g] += ','; else has[g] = 1;
    print_typed(cc.src_dtype, x.data() + (size_t)i * w, p->dict, &text[g]);
  }
  std::vector<const char*> ptrs; std::vector<int32_t> lens;
  for (size_t g = 0; g < text.size(); ++g) if (has[g]) { ptrs.push_back(text[g].data()); lens.push_back((int32_t)text[g].size()); }
  ssgpu_dict* dict = nullptr;
  int rc = ssgpu_dict_create(ptrs.data(), lens.data(), (int64_t)ptrs.size(), &dict);
  if (rc != SSGPU_OK) return rc;
  ptrs.clear(); lens.clear();
  for (size_t g = 0; g < text.size(); ++g) { ptrs.push_back(text[g].data()); lens.push_back((int32_t)text[g].size()); }
  HIP_TRY(c, r->host_data[col].ensure((size_t)std::max<int64_t>(out_rows, 1) * 4)); HIP_TRY(c, r->host_nulls[col].ensure((size_t)std::max<int64_t>(out_rows, 1)));
  std::vector<uint8_t> isnull((size_t)out_rows);
  for (size_t g = 0; g < isnull.size(); ++g) isnull[g] = has[g] ? 0 : 1;
  if (out_rows) {
    rc = ssgpu_dict_encode(dict, ptrs.data(), lens.data(), isnull.data(), out_rows, static_cast<int32_t*>(r->host_data[col].p));
    if (rc != SSGPU_OK) { ssgpu_dict_destroy(dict); return rc; }
    memcpy(r->host_nulls[col].p, isnull.data(), isnull.size());
  }
  if (r->concat_dicts.size() < r->host_data.size()) r->concat_dicts.resize(r->host_data.size(), nullptr);
  if (r->concat_dicts[col]) ssgpu_dict_destroy(r->concat_dicts[col]);
  r->concat_dicts[col] = dict;
  return SSGPU_OK;
}
}  // namespace

extern "C" {

int ssgpu_plan_set_dict(ssgpu_plan* p, const ssgpu_dict* dict) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  p->dict = dict;
  p->dict_gen = g_dict_gen.fetch_add(1) + 1;   // tables over the previous dictionary are rebuilt before the next run (ensure_dict_tables)
  return SSGPU_OK;
}

int32_t ssgpu_plan_string_steps(const ssgpu_plan* p, ssgpu_string_step* out, int32_t cap) {
  if (!p) return 0;
  std::vector<ssgpu_string_step> steps;
  plan_string_steps(p, &steps);
  for (size_t i = 0; out && i < steps.size() && (int64_t)i < (int64_t)cap; ++i) out[i] = steps[i];
  return (int32_t)steps.size();
}

const ssgpu_dict* ssgpu_result_column_dict(ssgpu_result* r, int32_t i) {
  if (!r || !r->plan || !concat_of(r->plan, i)) return nullptr;
  if ((size_t)i >= r->concat_dicts.size() || !r->concat_dicts[i]) { const void* d; const uint8_t* z; if (ssgpu_result_column(r, i, &d, &z) != SSGPU_OK) return nullptr; }
  return (size_t)i < r->concat_dicts.size() ? r->concat_dicts[i] : nullptr;
}

int ssgpu_result_column(ssgpu_result* r, int32_t i, const void** data, const uint8_t** is_null) {
  if (!r || !r->plan) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_plan* p = r->plan; ssgpu_ctx* c = p->ctx;
  int rc = settle_plan(p);
  if (rc != SSGPU_OK) return rc;
  rc = check_error_flags(p);
  if (rc == SSGPU_OK) rc = fix_nan_minmax(p);
  if (rc != SSGPU_OK) return rc;
  StageExec& ex = p->exec.back();   // (the NaN-exact form replaces the plan's stages)
  if (i < 0 || i >= (int)ex.out.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  int64_t rows = ssgpu_result_row_count(r);
  if (rows < 0) return SSGPU_ERROR_HIP;
  const size_t n = ex.out.size();
  if (r->host_data.size() != n) { r->host_data = std::vector<PinnedBuf>(n); r->host_nulls = std::vector<PinnedBuf>(n); r->fetched.assign(n, false); }
  if (!r->fetched[i] && concat_of(p, i)) {   // a CONCAT column: its strings are built here, from the stage's ordered input
    rc = build_concat_column(r, i, *concat_of(p, i), rows);
    if (rc != SSGPU_OK) return rc;
    r->fetched[i] = true;
  }
  if (concat_of(p, i)) {
    if (data) *data = r->host_data[i].p;
    if (is_null) *is_null = (const uint8_t*)r->host_nulls[i].p;
    return SSGPU_OK;
  }
  if (!r->fetched[i]) {
    const size_t bytes = (size_t)rows * ex.out[i].width;
    HIP_TRY(c, r->host_data[i].ensure(bytes));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(r->host_data[i].p, ex.out[i].data.p, bytes, hipMemcpyDeviceToHost, c->stream));
    if (ex.out[i].nullable) {
      HIP_TRY(c, r->host_nulls[i].ensure((size_t)rows));
      if (rows) HIP_TRY(c, hipMemcpyAsync(r->host_nulls[i].p, ex.out[i].nulls.p, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    r->fetched[i] = true;
  }
  if (data) *data = r->host_data[i].p;
  if (is_null) *is_null = ex.out[i].nullable ? (const uint8_t*)r->host_nulls[i].p : nullptr;
  return SSGPU_OK;
}

int ssgpu_plan_counters(ssgpu_plan* p, ssgpu_counters* out) {
  if (!p || !out) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (c->device >= 0 && c->profile && p->profiled_runs > 0) {
    float ms = 0;
    if (p->events_valid) {
      HIP_TRY(c, hipEventSynchronize(p->ev_end));
      if (hipEventElapsedTime(&ms, p->ev_begin, p->ev_end) == hipSuccess) p->counters.kernel_ms = ms;
    } else if (p->ev_dom1) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (p->ev_dom0 && hipEventElapsedTime(&ms, p->ev_dom0, p->ev_dom1) == hipSuccess) p->counters.dominant_ms = ms;
  }
  *out = p->counters;
  return SSGPU_OK;
}

}  // extern "C"

// ---- result images (ssgpu.h "result images"): layout shared by pack, unpack and the host mirrors ----
namespace {
struct ImageLayout {
  int64_t image_bytes = 0, unpacked_bytes = 0, valid_off = 0, trailer_off = 0;
  std::vector<int64_t> img_data, img_null, unp_data, unp_null;   // per attribute; -1 = no NULL mask
  std::vector<uint32_t> width;
};
int64_t align16(int64_t v) { return (v + 15) & ~int64_t(15); }
bool image_layout(const Schema& schema, int64_t cap, int32_t n_images, ImageLayout* L) {
  if (cap < 0 || n_images < 1 || schema.size() * 2 > SSGPU_IMAGE_MAX_PIECES) return false;
  const size_t n = schema.size();
  L->img_data.assign(n, -1); L->img_null.assign(n, -1); L->unp_data.assign(n, -1); L->unp_null.assign(n, -1); L->width.assign(n, 0);
  int64_t io = SSGPU_IMAGE_HEADER, uo = 0;
  for (size_t i = 0; i < n; ++i) {
    const int w = dtype_width(schema[i].dtype);
    if (w == 0) return false;
    L->width[i] = (uint32_t)w;
    L->img_data[i] = io; io = align16(io + cap * w);
    L->unp_data[i] = uo; uo = align16(uo + (int64_t)n_images * cap * w);
    if (schema[i].nullable) {
      L->img_null[i] = io; io = align16(io + cap);
      L->unp_null[i] = uo; uo = align16(uo + (int64_t)n_images * cap);
    }
  }
  L->image_bytes = io;
  L->valid_off = uo; uo = align16(uo + (int64_t)n_images * cap);
  L->trailer_off = uo; uo += 32;
  L->unpacked_bytes = uo;
  return true;
}
}  // namespace

extern "C" {

int ssgpu_plan_image_layout(const ssgpu_plan* p, int64_t capacity_rows, int32_t n_images, int64_t* image_bytes,
                            int64_t* unpacked_bytes, int64_t* offsets) {
  if (!p) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ImageLayout L;
  if (!image_layout(p->result_schema, capacity_rows, n_images, &L)) {
    p->ctx->err = "result images need fixed-width columns, at most 46 of them, and a non-negative capacity";
    return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  }
  if (image_bytes) *image_bytes = L.image_bytes;
  if (unpacked_bytes) *unpacked_bytes = L.unpacked_bytes;
  if (offsets) {
    const size_t n = p->result_schema.size();
    for (size_t i = 0; i < n; ++i) { offsets[4 * i] = L.img_data[i]; offsets[4 * i + 1] = L.img_null[i]; offsets[4 * i + 2] = L.unp_data[i]; offsets[4 * i + 3] = L.unp_null[i]; }
    offsets[4 * n] = -1; offsets[4 * n + 1] = -1; offsets[4 * n + 2] = L.valid_off; offsets[4 * n + 3] = -1;
  }
  return SSGPU_OK;
}

int ssgpu_result_pack_image(ssgpu_result* r, int64_t capacity_rows, void* image) {
  if (!r || !r->plan || r->plan->exec.empty() || !image) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_plan* p = r->plan; ssgpu_ctx* c = p->ctx;
  if (c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  ImageLayout L;
  if (!image_layout(p->result_schema, capacity_rows, 1, &L)) { c->err = "result images need fixed-width columns and a non-negative capacity"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  StageExec& ex = p->exec.back();
  ImagePackParams P; memset(&P, 0, sizeof(P));
  P.image = image; P.capacity = (unsigned long long)capacity_rows;
  if (ex.out_rows >= 0) P.rows_host = (unsigned long long)ex.out_rows; else P.rows_dev = static_cast<const unsigned long long*>(rows_word(ex));
  for (auto& sx : p->exec) if (sx.error_flag.p && P.n_flags < 8) P.error_flags[P.n_flags++] = sx.error_flag.as<unsigned int>();
  // a group stage whose overflow words have not been looked at yet (lazy feedback): they travel in the header, and a set
  // word makes the receiver repeat the step -- by then the next run has settled the stage
  for (auto& sx : p->exec) if (sx.fb_pending && sx.goverflow.p && P.n_retry + 2 <= 4) {
    P.retry_flags[P.n_retry++] = sx.goverflow.as<unsigned int>();
    if (sx.fb_pending == 2) P.retry_flags[P.n_retry++] = sx.goverflow.as<unsigned int>() + 1;
  }
  for (size_t i = 0; i < ex.out.size(); ++i) {
    ImagePiece& d = P.pieces[P.n_pieces++];
    d.src = ex.out[i].data.p; d.image_off = (unsigned long long)L.img_data[i]; d.width = L.width[i];
    if (L.img_null[i] >= 0) {
      ImagePiece& z = P.pieces[P.n_pieces++];
      z.src = ex.out[i].nullable ? ex.out[i].nulls.p : nullptr; z.image_off = (unsigned long long)L.img_null[i]; z.width = 1;
    }
  }
  HIP_TRY(c, ssgpu_launch_pack_image(P, c->stream));
  return SSGPU_OK;
}

int ssgpu_result_route_images(ssgpu_result* r, int32_t n_keys, int32_t n_dest, int64_t capacity_rows, void* images) {
  if (!r || !r->plan || r->plan->exec.empty() || !images || n_dest < 1 || n_dest > 256 || n_keys < 0 || n_keys > 16) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_plan* p = r->plan; ssgpu_ctx* c = p->ctx;
  if (c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  if (n_keys > (int32_t)p->result_schema.size()) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ImageLayout L;
  if (!image_layout(p->result_schema, capacity_rows, 1, &L)) { c->err = "result images need fixed-width columns and a non-negative capacity"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  StageExec& ex = p->exec.back();
  ImagePackParams P; memset(&P, 0, sizeof(P));
  ImageRoutePieces R; memset(&R, 0, sizeof(R));
  P.image = images; P.capacity = (unsigned long long)capacity_rows;
  const uint64_t rows_max = ex.out_rows >= 0 ? (uint64_t)ex.out_rows : (uint64_t)std::max<int64_t>(ex.out_capacity, 1);
  P.rows_host = rows_max;   // the routing kernels' bound on the row count; the count itself is on the device when the stage left it there
  if (ex.out_rows < 0) P.rows_dev = static_cast<const unsigned long long*>(rows_word(ex));
  for (auto& sx : p->exec) if (sx.error_flag.p && P.n_flags < 8) P.error_flags[P.n_flags++] = sx.error_flag.as<unsigned int>();
  for (auto& sx : p->exec) if (sx.fb_pending && sx.goverflow.p && P.n_retry + 2 <= 4) {
    P.retry_flags[P.n_retry++] = sx.goverflow.as<unsigned int>();
    if (sx.fb_pending == 2) P.retry_flags[P.n_retry++] = sx.goverflow.as<unsigned int>() + 1;
  }
  for (size_t i = 0; i < ex.out.size(); ++i) {
    if ((int32_t)i < n_keys) { R.key_piece[i] = P.n_pieces; R.key_null_piece[i] = -1; }
    ImagePiece& d = P.pieces[P.n_pieces++];
    d.src = ex.out[i].data.p; d.image_off = (unsigned long long)L.img_data[i]; d.width = L.width[i];
    if (L.img_null[i] >= 0) {
      if ((int32_t)i < n_keys) R.key_null_piece[i] = (int)P.n_pieces;
      ImagePiece& z = P.pieces[P.n_pieces++];
      z.src = ex.out[i].nullable ? ex.out[i].nulls.p : nullptr; z.image_off = (unsigned long long)L.img_null[i]; z.width = 1;
    }
  }
  R.n_keys = (unsigned)n_keys; R.n_dest = (unsigned)n_dest; R.image_bytes = (unsigned long long)L.image_bytes;
  {
    // the per-destination counters are left clear by the routing's own last kernel: filled only when the buffer is new
    const void* had = ex.route_scratch.p; const size_t had_cap = ex.route_scratch.cap;
    HIP_TRY(c, ex.route_scratch.ensure((256 + 2 * rows_max) * 4));
    if (ex.route_scratch.p != had || ex.route_scratch.cap != had_cap) HIP_TRY(c, hipMemsetAsync(ex.route_scratch.p, 0, 256 * 4, c->stream));
  }
  R.counters = ex.route_scratch.as<unsigned int>();
  HIP_TRY(c, ssgpu_launch_route_images(P, R, c->stream));
  return SSGPU_OK;
}

int ssgpu_images_unpack(ssgpu_plan* p, const void* images, int32_t n_images, int64_t capacity_rows, void* unpacked, ssgpu_column* cols) {
  if (!p || !images || !unpacked || !cols) return SSGPU_ERROR_INVALID_ARGUMENT_VALUE;
  ssgpu_ctx* c = p->ctx;
  if (c->device < 0) return SSGPU_ERROR_NO_DEVICE;
  ImageLayout L;
  if (!image_layout(p->result_schema, capacity_rows, n_images, &L)) { c->err = "result images need fixed-width columns and a non-negative capacity"; return SSGPU_ERROR_INVALID_ARGUMENT_VALUE; }
  ImageUnpackParams P; memset(&P, 0, sizeof(P));
  P.images = images; P.unpacked = unpacked; P.image_bytes = (unsigned long long)L.image_bytes; P.capacity = (unsigned long long)capacity_rows;
  P.valid_off = (unsigned long long)L.valid_off; P.trailer_off = (unsigned long long)L.trailer_off; P.n_images = (unsigned)n_images;
  char* base = static_cast<char*>(unpacked);
  const size_t n = p->result_schema.size();
  for (size_t i = 0; i < n; ++i) {
    ImagePiece& d = P.pieces[P.n_pieces++];
    d.image_off = (unsigned long long)L.img_data[i]; d.unpacked_off = (unsigned long long)L.unp_data[i]; d.width = L.width[i];
    cols[i].data = base + L.unp_data[i]; cols[i].is_null = nullptr;
    if (L.img_null[i] >= 0) {
      ImagePiece& z = P.pieces[P.n_pieces++];
      z.image_off = (unsigned long long)L.img_null[i]; z.unpacked_off = (unsigned long long)L.unp_null[i]; z.width = 1;
      cols[i].is_null = reinterpret_cast<const uint8_t*>(base + L.unp_null[i]);
    }
  }
  cols[n].data = base + L.valid_off; cols[n].is_null = nullptr;
  HIP_TRY(c, ssgpu_launch_unpack_images(P, c->stream));
  return SSGPU_OK;
}

}  // extern "C"

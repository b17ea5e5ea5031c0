"""The pipeline kernel's geometry restated, an independent reference for Filter / Compute / ScalarAggregate, and the inputs that put
the tile loop, the finish, the count / scan / store passes and the device row count on their edges
(tests/test_pipeline_reference_cpu.py checks all of it without a GPU; tests/test_sizes_pipeline_forms_gpu.py runs the device over it).

The reference shares no algorithm with the device or the oracle: NumPy boolean indexing selects, integer sums are Python integers
reduced mod 2^64 (2^32 for INT32 results), DOUBLE sums are `math.fsum`, MIN / MAX are Python's `min` / `max` over the non-NULL,
non-NaN values under the reference's "a leading NaN stays" rule, FIRST / LAST are the first and the last
selected non-NULL value (the oracle's fold assigns the first value it is given and skips NULLs), COUNT counts the selected non-NULL
rows; a ScalarAggregate result is one row, every column but COUNT nullable and NULL when nothing contributed.

Data rules: every DOUBLE input is a multiple of 0.25 whose sums stay far inside 2^53, so every comparison is bit for bit (the one
inexact case, `inexact_sum_case`, says so); INT64 inputs include the weight column w[r] = r + 1 and w * w (wrapping), so a dropped
or doubled row anywhere changes a SUM.

The mirrors (`parse_programs`, `tile_k`, `lds_bytes`, `grid_size`, `first_tile`, `locate`) restate layout_program (lower.cpp),
grid_for (runtime.cpp) and the tile / lane mapping of ssgpu_pipeline_kernel (pipeline_kernels.hip, vm.h).  They only STATE each
case's `facts` -- what plan.counters() must report -- and place planted rows; expected rows never come from them."""
import math
import re

import numpy as np

U64 = np.uint64
TILE_UNIT = 512              # vm.h: VM_TILE_UNIT, the rows of a K = 1 tile (256 threads x one row pair)
THREADS = 256                # vm.h: VM_THREADS
PF_UNITS = 8                 # vm.h: VM_PF_UNITS, 16-byte-per-lane units of the register prefetch file
FAST_SLOTS = 8               # vm.h: VM_FAST_SLOTS, aggregate slots kept in registers
MAX_SLOTS = 64               # vm.h: VM_MAX_AGG_SLOTS
ACC_STRIDE = 128             # vm.h: VM_ACC_STRIDE, LDS bytes of one aggregate slot
LDS_TARGET = 48 * 1024       # engine.h: LowerOptions::lds_target_bytes
LDS_MAX = 160 * 1024         # layout_program: a tile must fit one CU
SCAN_CHUNK = 8192            # ssgpu_scan_counts_kernel: 1024 threads x 8 counts per trip
ARENA_MIN = 32 << 20         # runtime.cpp: kBlockArenaMin

NP_OF = {"INT32": np.int32, "INT64": np.int64, "UINT64": np.uint64, "DOUBLE": np.float64, "FLOAT": np.float32, "BOOL": np.bool_}
TYPE_CODE = {"INT32": 1, "INT64": 2, "UINT64": 3, "DOUBLE": 5, "BOOL": 6, "FLOAT": 9}       # supersonic.proto DataType


# ---- mirrors -----------------------------------------------------------------------------------------------------------------------
def parse_programs(text):
    """The programs of plan.describe(): [{stage, name, n_staged, bytes_per_row, n_slots, n_instr}] in the order they are printed
    ("main" is a stage's own program, "count pass" the materialising Filter's)."""
    out, stage, name, cur = [], -1, "main", None
    for line in text.splitlines():
        m = re.match(r"stage (\d+) kind=", line)
        if m:
            stage, name, cur = int(m.group(1)), "main", None
            continue
        m = re.match(r" (\S[^:]*):\s*$", line)
        if m:
            name = m.group(1)
            continue
        m = re.match(r"  staged:(.*)$", line)
        if m and stage >= 0:
            cur = {"stage": stage, "name": name, "n_staged": len(m.group(1).split()), "n_instr": 0}
            out.append(cur)
            continue
        m = re.match(r"  lds bytes/row: (\d+), slots: (\d+), outputs: (\d+)", line)
        if m and cur is not None:
            cur["bytes_per_row"], cur["n_slots"] = int(m.group(1)), int(m.group(2))
            continue
        if cur is not None and re.match(r"  \d+: [A-Z]", line):
            cur["n_instr"] += 1
    return out


def lds_bytes(prog, K):
    """lds_for of layout_program: registers, slot records, 256 bytes of scratch, the constant pool, the two mask arrays of a tile."""
    regs = prog["bytes_per_row"] * TILE_UNIT * K
    return ((regs + 15) & ~15) + prog["n_slots"] * ACC_STRIDE + 256 + 16 * prog["n_instr"] + 2 * TILE_UNIT * K


def tile_k(prog, tile_rows=0, lds_target=LDS_TARGET):
    """K of layout_program: the tile_rows option rounded to 1 / 2 / 4 units and halved until it fits a CU, or -- option 0 -- the
    largest tile within the LDS target whose staged units fit the register prefetch file (else one unit)."""
    if tile_rows > 0:
        K = max(1, tile_rows // TILE_UNIT)
        K = 4 if K >= 4 else 2 if K >= 2 else 1
        while K > 1 and lds_bytes(prog, K) > LDS_MAX:
            K //= 2
        return K
    for K in (4, 2, 1):
        if lds_bytes(prog, K) <= lds_target and prog["n_staged"] * K <= PF_UNITS:
            break
    return K


def count_pass_k(count_prog, main_k):
    """prepare_stage (runtime.cpp): the count pass takes the largest tile that fits, never a smaller one than the store pass."""
    K = tile_k(count_prog, 4 * TILE_UNIT)
    return K if K >= main_k else tile_k(count_prog, main_k * TILE_UNIT)


def ceil_div(a, b):
    return -(-a // b)


def grid_size(n_tiles, grid_limit, lds, cu_count=256, wgs_per_cu=3):
    """grid_for (runtime.cpp)."""
    per_cu = max(min(wgs_per_cu, LDS_MAX // max(lds, 1)), 1)
    g = cu_count * per_cu
    if grid_limit > 0:
        g = min(g, grid_limit)
    return max(min(g, max(1, n_tiles)), 1)


def first_tile(block, grid, chunks):
    """vm_first_tile of ssgpu_pipeline_kernel: under VM_FLAG_XCD_CHUNKS a grid that is a multiple of 8 hands every XCD (block % 8)
    a contiguous eighth of each round's tiles; any other grid takes tile = block."""
    if chunks and grid % 8 == 0:
        return (block & 7) * (grid >> 3) + (block >> 3)
    return block


def tiles_of(block, grid, n_tiles, chunks):
    """The tiles a workgroup runs over, in the order of its trips: first_tile + it * grid."""
    return list(range(first_tile(block, grid, chunks), n_tiles, grid))


def uses_chunks(tile_map, writes_rows):
    """run_scalar_agg / the count pass set VM_FLAG_XCD_CHUNKS from tile_map 2, the store pass of run_materialize from 1."""
    return tile_map >= (1 if writes_rows else 2)


def locate(row, tile_rows):
    """Where a row sits in the kernel: (tile, sub-tile k, lane pair t, second row of the pair) -- vm.h: pair p = k * 256 + t of a tile
    holds the rows 2 p and 2 p + 1."""
    tile, within = divmod(int(row), tile_rows)
    k, t = divmod(within // 2, THREADS)
    return tile, k, t, within % 2


# ---- cases and their reference -------------------------------------------------------------------------------------------------------
class Col(object):
    """One input column.  nullable: the attribute's; nulls: the is_null vector the View carries (None: none, also for a nullable one)."""

    def __init__(self, name, type, data, nulls=None, nullable=None):
        self.name, self.type = name, type
        self.data = np.ascontiguousarray(data, dtype=NP_OF[type])
        self.nulls = None if nulls is None else np.ascontiguousarray(nulls, dtype=bool)
        self.nullable = (nulls is not None) if nullable is None else nullable


def wrap_mul(a, b):
    return (np.asarray(a, np.int64).view(U64) * np.asarray(b, np.int64).view(U64)).view(np.int64)


def wrap_add(a, b):
    return (np.asarray(a, np.int64).view(U64) + np.asarray(b, np.int64).view(U64)).view(np.int64)


def weights(n):
    """w[r] = r + 1 and w * w (wrapping)."""
    w = np.arange(n, dtype=np.int64) + 1
    return w, wrap_mul(w, w)


def signed(v, bits):
    v %= 1 << bits
    return v - (1 << bits) if v >> (bits - 1) else v


class PipeCase(object):
    """One plan over one input.  steps, innermost first: ("compute", [(out, name | (fn, x, y))]) with fn "plus" / "mul" over two columns
    of one type, ("filter", ("gt", column, constant) | ("true", BOOL column), None | [projected names]), ("agg", [(fn, input or "", out)]).
    options: the context's; facts: what plan.counters() reports (tile_rows, grid) and n_tiles = ceil(rows / tile_rows);
    notes: what the builder planted, for the geometry checks."""

    def __init__(self, name, cols, steps, options, facts, **notes):
        self.name, self.cols, self.steps, self.options, self.facts, self.notes = name, cols, steps, options, facts, notes
        self.rows = len(cols[0].data)
        self.data_key = notes.pop("data_key", name)      # cases that differ in context options only share it (and their expected rows)

    def schema(self):
        import supersonic_amd as ss
        return ss.TupleSchema([ss.Attribute(c.name, getattr(ss, c.type), ss.NULLABLE if c.nullable else ss.NOT_NULLABLE) for c in self.cols])

    def columns(self):
        import supersonic_amd as ss
        return [ss.Column(c.data, c.nulls) for c in self.cols]

    def view(self):
        import supersonic_amd as ss
        return ss.View(self.schema(), self.columns())

    def op(self, view):
        import supersonic_amd as ss
        NA = ss.NamedAttribute
        fns = {"plus": ss.Plus, "mul": ss.Multiply}
        node = ss.ScanView(view)
        for step in self.steps:
            if step[0] == "compute":
                e = ss.CompoundExpression()
                for out, ex in step[1]:
                    if isinstance(ex, str):
                        e.Add(NA(ex)) if ex == out else e.AddAs(out, NA(ex))
                    else:
                        e.AddAs(out, fns[ex[0]](NA(ex[1]), NA(ex[2])))
                node = ss.Compute(e, node)
            elif step[0] == "filter":
                pred = ss.Greater(NA(step[1][1]), ss.ConstInt64(step[1][2])) if step[1][0] == "gt" else NA(step[1][1])
                node = ss.Filter(pred, ss.ProjectAllAttributes() if step[2] is None else ss.ProjectNamedAttributes(list(step[2])), node)
            else:
                spec = ss.AggregationSpecification()
                for fn, col, out in step[1]:
                    spec.AddAggregation(getattr(ss, fn), col, out)
                node = ss.ScalarAggregate(spec, node)
        return node

    def kept(self):
        """The rows the plan's Filter keeps (all, without one)."""
        keep = np.ones(self.rows, bool)
        by_name = {c.name: c for c in self.cols}
        for step in self.steps:
            if step[0] == "filter":
                c = by_name[step[1][1]]
                k = c.data > step[1][2] if step[1][0] == "gt" else c.data.astype(bool)
                keep &= k if c.nulls is None else k & ~c.nulls
        return keep

    def expected(self):
        """(schema as [(name, type code, nullable)], [(data, is_null or None)]) by the rules of the module's docstring."""
        env = [[c.name, c.type, c.data, c.nulls, c.nullable] for c in self.cols]
        for step in self.steps:
            by_name = {e[0]: e for e in env}
            if step[0] == "compute":
                new = []
                for out, ex in step[1]:
                    if isinstance(ex, str):
                        _n, t, d, z, nb = by_name[ex]
                    else:
                        (_a, t, da, za, na), (_b, tb, db, zb, nb_) = by_name[ex[1]], by_name[ex[2]]
                        assert t == tb and t in ("INT64", "DOUBLE")
                        if t == "INT64":
                            d = wrap_add(da, db) if ex[0] == "plus" else wrap_mul(da, db)
                        else:
                            d = da + db if ex[0] == "plus" else da * db
                        z = za if zb is None else zb if za is None else za | zb
                        nb = na or nb_
                    new.append([out, t, d, z, nb])
                env = new
            elif step[0] == "filter":
                _n, t, d, z, _nb = by_name[step[1][1]]
                keep = d > step[1][2] if step[1][0] == "gt" else d.astype(bool)
                if z is not None:
                    keep = keep & ~z
                names = [e[0] for e in env] if step[2] is None else list(step[2])
                env = [[n, by_name[n][1], by_name[n][2][keep], None if by_name[n][3] is None else by_name[n][3][keep], by_name[n][4]] for n in names]
            else:
                env = [self._aggregate(fn, by_name.get(col), out, len(env[0][2])) for fn, col, out in step[1]]
        schema = [(n, TYPE_CODE[t], 1 if nb else 0) for n, t, _d, _z, nb in env]
        cols = [(d, (np.zeros(len(d), bool) if z is None else z) if nb else None) for _n, _t, d, z, nb in env]
        return schema, cols

    @staticmethod
    def _aggregate(fn, col, out, rows):
        if fn == "COUNT":
            n = rows if col is None or col[3] is None else int((~col[3]).sum())
            return [out, "UINT64", np.array([n], np.uint64), None, False]
        _n, t, d, z, _nb = col
        v = (d if z is None else d[~z]).tolist()
        if not v:
            return [out, t, np.zeros(1, NP_OF[t]), np.ones(1, bool), True]
        if fn == "SUM":
            assert t in ("INT64", "INT32", "DOUBLE")
            r = math.fsum(v) if t == "DOUBLE" else signed(sum(v), 64 if t == "INT64" else 32)
        elif fn in ("FIRST", "LAST"):
            r = v[0] if fn == "FIRST" else v[-1]
        elif t in ("DOUBLE", "FLOAT") and v[0] != v[0]:
            r = (d if z is None else d[~z])[0]          # a leading NaN stays (its own bits)
        else:
            r = (min if fn == "MIN" else max)(x for x in v if x == x)
        return [out, t, np.array([r], NP_OF[t]), np.zeros(1, bool), True]


def stated_facts(rows, tile_rows, grid_limit):
    n_tiles = ceil_div(rows, tile_rows)
    return {"tile_rows": tile_rows, "n_tiles": n_tiles, "grid": max(min(grid_limit, n_tiles), 1) if grid_limit else None}


# A. the tile loop of ScalarAggregate
TILES = (512, 1024, 2048)
GRID_LIMITS = (1, 2, 3, 8, 16)
POSITIONS = ("row_0", "full_tile_end", "partial_first", "pair_second", "last_row")
Z_KINDS = ("mixed", "first_in_last_tile", "last_in_tile_0", "all_null")
WIDE_AGGS = [("SUM", "s", "sum_s"), ("COUNT", "", "cnt"), ("SUM", "w", "sum_w"), ("MIN", "d", "min_d"), ("MAX", "d0", "max_d0"), ("SUM", "d1", "sum_d1"),
             ("SUM", "p", "sum_p"), ("FIRST", "z", "first_z"), ("LAST", "z", "last_z"), ("COUNT", "z", "cnt_z")]
WIDE_STEPS = [("compute", [("a", "a"), ("s", ("plus", "a", "b")), ("w", "w"), ("d", "d"), ("d0", "d0"), ("d1", "d1"), ("p", ("mul", "d2", "d3")), ("z", "z")]),
              ("filter", ("gt", "a", 499), None), ("agg", WIDE_AGGS)]


def tile_counts(g):
    return (g, g + 1, 2 * g, 2 * g + 1, 3 * g - 1)


def last_sizes(T):
    return (T, 1, 2, 3, T - 1)


def planted_row(kind, n, T, g):
    """The row a unique MIN / MAX is planted on.  full_tile_end: the last row of a full tile -- tile g, the second trip of workgroup 0,
    where there is one (row n - 1 where no tile is full); partial_first: the first row of the last tile; pair_second: an odd row a quarter or half way into
    tile g (or into the last tile; row 0 when that tile has one row)."""
    n_tiles = ceil_div(n, T)
    if kind == "row_0":
        return 0
    if kind == "last_row":
        return n - 1
    if kind == "partial_first":
        return (n_tiles - 1) * T
    if kind == "full_tile_end":
        n_full = n // T
        return n - 1 if n_full == 0 else min(g, n_full - 1) * T + T - 1
    tile = min(g, n_tiles - 1)
    valid = min(T, n - tile * T)
    off = (valid // (4 if n_tiles % 2 else 2)) | 1
    return tile * T + (off if off < valid else 1 if valid > 1 else 0)


def tile_loop_case(T, g, n_tiles, last, min_at, max_at, z_kind, tile_map=None):
    """A. Q-FPA-wide's shape (Compute a, s = a + b, w, d, d0, d1, p = d2 * d3 -> Filter a > 499 -> SUM s, COUNT(*), SUM w, MIN d, MAX d0,
    SUM d1, SUM p) plus FIRST z, LAST z and COUNT z of a NULLABLE INT32 -- FIRST on slot 7, the last register slot, LAST on slot 8, the
    first LDS slot -- over n_tiles tiles of T rows, the last one of `last` rows, on at most g workgroups.  b = w * w.  The Filter keeps two
    rows of three and every planted row; a dropped row carries a value below the MIN and one above the MAX, and a non-NULL z where z_kind
    leaves a single one."""
    n = (n_tiles - 1) * T + last
    r = np.arange(n, dtype=np.int64)
    w, ww = weights(n)
    min_row, max_row = planted_row(min_at, n, T, g), planted_row(max_at, n, T, g)
    z_row = None
    if z_kind == "first_in_last_tile":
        z_row = (n_tiles - 1) * T + (last - 1) // 2
    elif z_kind == "last_in_tile_0":
        z_row = 0 if (n_tiles + last) % 2 == 0 else min(n, T) - 1      # row id 0 is also LAST's identity in the kernel
    keep = r % 3 != 1
    keep[[x for x in (min_row, max_row, z_row) if x is not None]] = True
    dropped = np.nonzero(~keep)[0]
    d = (r * 2654435761) % (1 << 40) - (1 << 39)
    d0 = ((r * 37) % 4096) * 0.25 - 512.0
    d[min_row], d0[max_row] = -(1 << 50), 2.0 ** 30
    z = (r % 1000 + 1).astype(np.int32)
    zn = {"mixed": r % 5 < 2, "all_null": np.ones(n, bool)}.get(z_kind)
    if zn is None:
        zn = np.ones(n, bool)
        zn[z_row] = False
    if len(dropped):
        decoy = int(dropped[len(dropped) // 2])
        d[decoy], d0[decoy] = -(1 << 55), 2.0 ** 31
        if z_row is not None:
            zn[dropped[0] if z_kind == "first_in_last_tile" else dropped[-1]] = False   # ahead of the only kept one / behind it
    cols = [Col("a", "INT64", np.where(keep, 500 + r % 400, r % 500)), Col("b", "INT64", ww), Col("w", "INT64", w), Col("d", "INT64", d),
            Col("d0", "DOUBLE", d0), Col("d1", "DOUBLE", (r % 4000) * 0.25), Col("d2", "DOUBLE", (r % 64).astype(np.float64)),
            Col("d3", "DOUBLE", ((r * 5) % 64).astype(np.float64)), Col("z", "INT32", z, zn)]
    options = {"tile_rows": T, "grid_limit": g}
    if tile_map is not None:
        options["tile_map"] = tile_map
    key = ("tile loop", T, g, n_tiles, last, min_at, max_at, z_kind)
    return PipeCase("tile-loop-T%d-g%d-%dx-last%d-%s-%s-%s%s" % (T, g, n_tiles, last, min_at, max_at, z_kind, "" if tile_map is None else "-map%d" % tile_map),
                    cols, WIDE_STEPS, options, stated_facts(n, T, g), data_key=key, min_row=min_row, max_row=max_row, z_row=z_row, min_at=min_at, max_at=max_at,
                    z_kind=z_kind, grid_limit=g, last=last)


def tile_loop_sweep(T, g, tile_map=None):
    """The 5 x 5 (tile count, last-tile size) inputs of one (T, g): the positions of MIN and MAX and the z kinds take turns, every
    position five times and every kind six or seven times per (T, g)."""
    out, seen = [], set()
    for ic, n_tiles in enumerate(tile_counts(g)):
        for il, last in enumerate(last_sizes(T)):
            if (n_tiles, last) in seen:        # g = 1: 2 g = g + 1 = 3 g - 1
                continue
            seen.add((n_tiles, last))
            out.append(tile_loop_case(T, g, n_tiles, last, POSITIONS[(ic + il) % 5], POSITIONS[(ic + il + 2) % 5], Z_KINDS[(2 * ic + il) % 4], tile_map))
    return out


# B. the NaN flag across trips
NAN_KINDS = ("second_tile", "partial_tile", "row_0", "row_0_dropped", "none")
NAN_STEPS = [("filter", ("gt", "a", 499), None),
             ("agg", [("MIN", "x", "lo"), ("MAX", "x", "hi"), ("MIN", "f", "flo"), ("MAX", "f", "fhi"), ("SUM", "w", "sum_w")])]


def nan_case(kind, T):
    """B. grid_limit = 2 over ten tiles and a partial one (workgroup 0 takes six tiles, workgroup 1 five); MIN / MAX of a DOUBLE and a
    FLOAT column with ONE NaN each: in tile 2 (workgroup 0's second), in the partial tile, at row 0 (leading: it stays), at row 0 but
    dropped by the Filter (not leading: skipped), nowhere.  A run that meets a NaN is flagged and repeated in the plan's NaN-exact form
    (hidden FIRST, IF(IS_NAN(first), first, min) in a Compute behind the aggregate), which the plan keeps."""
    n = 10 * T + 100
    r = np.arange(n, dtype=np.int64)
    w, _ww = weights(n)
    keep = r % 3 != 1
    at = {"second_tile": 2 * T + 1, "partial_tile": 10 * T + 99, "row_0": 0, "row_0_dropped": 0, "none": None}[kind]
    if at is not None:
        keep[at] = kind != "row_0_dropped"
    x = ((r * 37) % 4096) * 0.25 - 300.25
    f = (((r * 11) % 512) * 0.5 - 100.25).astype(np.float32)
    if at is not None:
        x[at], f[at] = np.nan, np.nan
    cols = [Col("a", "INT64", np.where(keep, 500 + r % 400, r % 500)), Col("x", "DOUBLE", x), Col("f", "FLOAT", f), Col("w", "INT64", w)]
    facts = stated_facts(n, T, 2)
    flagged = at is not None and kind != "row_0_dropped"
    if flagged:
        facts["grid"] = 1       # counters() speak of a run's LAST stage: the NaN-exact repeat ends on a Compute over the one result row
    return PipeCase("nan-%s-T%d" % (kind, T), cols, NAN_STEPS, {"tile_rows": T, "grid_limit": 2}, facts, nan_at=at, leading=kind == "row_0", flagged=flagged, agg_grid=2)


# C. slots
SLOT_KINDS = ("SUM", "MIN", "MAX", "COUNT", "FIRST", "LAST")
SLOT_COUNTS = (8, 9, 64, 65)
SLOT_T, SLOT_GRID = 512, 2


def slot_case(n_aggs, rot, fuse_emit=None):
    """C. n_aggs aggregations over four tiles on two workgroups (two trips each, the last tile partial).  Aggregation i is of kind
    SLOT_KINDS[(i + rot) % 6], so over rot = 0 .. 5 every kind lands once on slot 7 and once on slot 8; its input is column i of a cycle
    over INT64, DOUBLE, INT32, a NULLABLE INT64, FLOAT and a NULLABLE DOUBLE (COUNT: a NULLABLE one -- it then owns its slot; SUM: never FLOAT)."""
    n = 3 * SLOT_T + 200
    r = np.arange(n, dtype=np.int64)
    w, ww = weights(n)
    keep = r % 3 != 1
    cols = [Col("a", "INT64", np.where(keep, 500 + r % 400, r % 500)), Col("w", "INT64", ww), Col("x", "DOUBLE", ((r * 37) % 4096) * 0.25 - 300.0),
            Col("i", "INT32", ((r * 7919) % 100000 - 50000).astype(np.int32)), Col("nz", "INT64", wrap_mul(w, 3), r % 4 == 1),
            Col("f", "FLOAT", (((r * 11) % 512) * 0.5 - 100.0).astype(np.float32)), Col("nd", "DOUBLE", ((r * 5) % 2048) * 0.25 - 7.0, r % 5 == 2)]
    pool = ("w", "x", "i", "nz", "f", "nd")
    aggs = []
    for i in range(n_aggs):
        kind, col = SLOT_KINDS[(i + rot) % 6], pool[i % 6]
        if kind == "COUNT":
            col = "nz" if i % 2 == 0 else "nd"
        elif kind == "SUM" and col == "f":
            col = "x"
        aggs.append((kind, col, "%s_%s_%d" % (kind.lower(), col, i)))
    options = {"tile_rows": SLOT_T, "grid_limit": SLOT_GRID}
    if fuse_emit is not None:
        options["fuse_emit"] = fuse_emit
    return PipeCase("slots-%d-rot%d%s" % (n_aggs, rot, "" if fuse_emit is None else "-fuse%d" % fuse_emit), cols, [("filter", ("gt", "a", 499), None), ("agg", aggs)],
                    options, stated_facts(n, SLOT_T, SLOT_GRID), data_key=("slots", n_aggs, rot), aggs=aggs)


# D. staging forms
STAGING_SHAPES = ((8, 512), (9, 512), (4, 1024), (5, 1024), (2, 2048), (3, 2048))     # staged arrays x tile: staged x K = 8 fits the prefetch file, one more does not
STAGING_FAMILIES = ("w8", "w4", "w1", "mixed")


def staging_columns(staged, family, n):
    """`staged` staged arrays, the Filter's BOOL column first: all further ones INT64 / INT32 / BOOL (w8 / w4 / w1), or mixed --
    widths 8, 4 and 1 in turn, ending on a NULLABLE INT32 whose View carries no is_null (two staged arrays: data and mask)."""
    r = np.arange(n, dtype=np.int64)
    w, ww = weights(n)
    cols = [Col("keep", "BOOL", r % 3 != 1)]
    make = {"w8": lambda j: Col("c%d" % j, "INT64", wrap_add(wrap_mul(ww, j + 1), j)),
            "w4": lambda j: Col("c%d" % j, "INT32", ((r * (7919 + 2 * j) + j) % 2000003 - 1000000).astype(np.int32)),
            "w1": lambda j: Col("c%d" % j, "BOOL", (r * (j + 3)) % (j + 5) < 2)}
    if family != "mixed":
        return cols + [make[family](j) for j in range(staged - 1)]
    if staged == 2:
        return cols + [make["w8"](0)]
    turn = ("w8", "w4", "w1")
    cols += [make[turn[j % 3]](j) for j in range(staged - 3)]
    return cols + [Col("nn", "INT32", (r % 1000 - 500).astype(np.int32), None, nullable=True)]


def staging_case(staged, T, family, grid_limit=1):
    """D. ScalarAggregate over three full tiles and a partial one on ONE workgroup: units 0 .. 7 of a full tile travel through the
    register prefetch file, further ones are fetched in place; the partial tile is fetched in place as a whole."""
    n = 3 * T + T // 2 + 3
    cols = staging_columns(staged, family, n)
    aggs = []
    for c in cols[1:]:
        aggs += [("MAX" if c.type == "BOOL" else "SUM", c.name, "s_" + c.name), ("MIN" if c.type == "BOOL" else "LAST", c.name, "l_" + c.name)]
    aggs.append(("COUNT", "", "cnt"))
    return PipeCase("staging-%d-T%d-%s" % (staged, T, family), cols, [("filter", ("true", "keep"), None), ("agg", aggs)],
                    {"tile_rows": T, "grid_limit": grid_limit}, stated_facts(n, T, grid_limit), staged=staged)


ODD_OFFSET_ROWS = 1


def odd_address_case():
    """D. A BOOL column at an odd device address: the case's block holds ODD_OFFSET_ROWS rows more than the plan reads, and the plan reads a
    DeviceView of the block whose column pointers are moved on by that many rows (the expected rows are those of the rows behind the
    offset).  The case itself describes the rows the plan sees; `block_columns` prepends the ones it skips."""
    T = 512
    n = 3 * T + 77
    r = np.arange(n, dtype=np.int64)
    w, ww = weights(n)
    cols = [Col("keep", "BOOL", r % 3 != 1), Col("w", "INT64", ww), Col("t", "BOOL", (r * 7) % 5 < 2)]
    aggs = [("SUM", "w", "sum_w"), ("MAX", "t", "max_t"), ("MIN", "t", "min_t"), ("LAST", "t", "last_t"), ("COUNT", "", "cnt")]
    return PipeCase("staging-odd-address", cols, [("filter", ("true", "keep"), None), ("agg", aggs)], {"tile_rows": T, "grid_limit": 1}, stated_facts(n, T, 1))


def block_columns(case, skipped=ODD_OFFSET_ROWS):
    """The columns of odd_address_case's block: `skipped` rows of ones (TRUE, kept: they would change every result) ahead of the case's."""
    return [np.concatenate([np.ones(skipped, c.data.dtype), c.data]) for c in case.cols]


# E. materialising Filter
STORE_NAMES = ("w", "x", "i", "f", "t", "nz", "nd", "ww")
SURVIVORS = ("all", "none", "last_row", "first_of_512", "every_other", "one_per_2048")
FILTER_ROWS = tuple(2048 * m + d for m in (1, 3) for d in (0, 1, 511, 512, 513, 1536, 1537, 2047))
FILTER_GRIDS, FILTER_MAPS = (1, 3, 8), (0, 1)
STORE_T, COUNT_T = 512, 2048      # 11 staged arrays leave the store pass one unit per tile; the count pass stages the predicate alone


def survivors(kind, n):
    r = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "last_row": r == n - 1, "first_of_512": r % 512 == 0, "every_other": r % 2 == 1,
            "one_per_2048": r % 2048 == ((r // 2048) * 577) % 2048}[kind]


def filter_case(n, kind, grid_limit, tile_map):
    """E. Filter on a BOOL column over 8 stored columns (INT64, DOUBLE, INT32, FLOAT, BOOL, NULLABLE INT64, NULLABLE DOUBLE, INT64): the
    store pass runs tiles of 512 rows, the count pass tiles of 2048 that publish four counts each."""
    r = np.arange(n, dtype=np.int64)
    w, ww = weights(n)
    cols = [Col("w", "INT64", w), Col("x", "DOUBLE", ((r * 37) % 4096) * 0.25 - 300.0), Col("i", "INT32", ((r * 7919) % 100000 - 50000).astype(np.int32)),
            Col("f", "FLOAT", (((r * 11) % 512) * 0.5 - 100.0).astype(np.float32)), Col("t", "BOOL", r % 3 == 0), Col("nz", "INT64", wrap_mul(w, 3), r % 4 == 1),
            Col("nd", "DOUBLE", ((r * 5) % 2048) * 0.25 - 7.0, r % 5 == 2), Col("ww", "INT64", ww), Col("keep", "BOOL", survivors(kind, n))]
    return PipeCase("filter-%d-%s-g%d-map%d" % (n, kind, grid_limit, tile_map), cols, [("filter", ("true", "keep"), STORE_NAMES)],
                    {"grid_limit": grid_limit, "tile_map": tile_map}, stated_facts(n, STORE_T, grid_limit), data_key=("filter", n, kind), count_tile=COUNT_T)


SCAN_CARRY_ROWS = 512 * SCAN_CHUNK + 1
SCAN_CARRY_STEPS, SCAN_CARRY_OPTIONS = [("filter", ("true", "keep"), ("v",))], {"tile_rows": 512}


def scan_carry_case():
    """E. 8193 store tiles of 512 rows: ssgpu_scan_counts_kernel makes a second trip, for ONE count behind the carry of 8192.  Every third
    row survives."""
    n = SCAN_CARRY_ROWS
    r = np.arange(n, dtype=np.int64)
    cols = [Col("v", "INT32", ((r * 7919) % 2000003 - 1000000).astype(np.int32)), Col("keep", "BOOL", r % 3 == 0)]
    return PipeCase("filter-scan-carry", cols, SCAN_CARRY_STEPS, SCAN_CARRY_OPTIONS, stated_facts(n, 512, 0), count_tile=COUNT_T)


ARENA_STEPS = [("filter", ("true", "keep"), tuple("c%d" % j for j in range(8)))]
ARENA_ROWS = (524288, 524287, 524288)      # 8 INT64 columns: 64 bytes per row, 32 MiB at 2^19 rows


def arena_case(run):
    """E. The three inputs of ONE plan of 8 NOT NULL INT64 columns: the result (sized by the INPUT's rows) is an arena, then buffers of
    its own, then an arena again.  One row in seven survives."""
    n = ARENA_ROWS[run]
    r = np.arange(n, dtype=np.int64)
    w, ww = weights(n)
    cols = [Col("c%d" % j, "INT64", wrap_add(wrap_mul(ww, j + 1 + run), j)) for j in range(8)] + [Col("keep", "BOOL", r % 7 == 3 + run)]
    return PipeCase("filter-arena-run%d-%d" % (run, n), cols, ARENA_STEPS, {}, stated_facts(n, 512, 0),
                    result_bytes=64 * n)


# F. device row count
HANDOFF_T = 512
HANDOFF_GROUPS = (0, 1, HANDOFF_T - 1, HANDOFF_T, HANDOFF_T + 1)


class HandoffCase(object):
    """F. Compute (k, q = sv / sn SIGNALING, s2 = sv + sn) over GroupAggregate(k: SUM v, SUM one) over a Filter: the stage pair run_plan
    hands off on the device -- the Compute runs over the group result's capacity and reads the group count there; the rows beyond it
    would divide by zero.  groups = 0: the Filter drops every row.  The expected rows are the oracle's (the GroupAggregate is not this
    module's to restate), sorted: `expected_sorted` restates them for the CPU test."""

    def __init__(self, groups):
        self.name, self.groups = "handoff-%d-groups" % groups, groups
        self.rows = 4 * max(groups, 1) + 3
        r = np.arange(self.rows, dtype=np.int64)
        self.k = (r % max(groups, 1)).astype(np.int32)
        self.v = wrap_mul(r + 1, 6)
        self.one = np.full(self.rows, 2, np.int64)   # SUM one is 8 or 10: never 0 for a group, and q = sv / sn is ONE correctly rounded IEEE division of two exact doubles
        self.a = np.full(self.rows, 1 if groups else 0, np.int64)

    def view(self):
        import supersonic_amd as ss
        schema = ss.TupleSchema([ss.Attribute("k", ss.INT32), ss.Attribute("v", ss.INT64), ss.Attribute("one", ss.INT64), ss.Attribute("a", ss.INT64)])
        return ss.View(schema, [self.k, self.v, self.one, self.a])

    def op(self, view):
        import supersonic_amd as ss
        NA = ss.NamedAttribute
        spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sv").AddAggregation(ss.SUM, "one", "sn")
        group = ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None,
                                  ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(0)), ss.ProjectAllAttributes(), ss.ScanView(view)))
        return ss.Compute(ss.CompoundExpression().Add(NA("k")).AddAs("q", ss.DivideSignaling(NA("sv"), NA("sn"))).AddAs("s2", ss.Plus(NA("sv"), NA("sn"))), group)

    def expected_sorted(self):
        g = self.groups
        sv = [sum(self.v[self.k == j].tolist()) for j in range(g)]
        sn = [sum(self.one[self.k == j].tolist()) for j in range(g)]
        no = np.zeros(g, bool)
        return [(np.arange(g, dtype=np.int32), None), (np.array([a / b for a, b in zip(sv, sn)], np.float64), no), (np.array([a + b for a, b in zip(sv, sn)], np.int64), no)]


# G. one inexact DOUBLE sum
def inexact_sum_case():
    """G. The ONE case whose DOUBLE sum is not exact: 6 tiles of 2048 rows and a partial one on three workgroups, doubles of mixed sign and
    of magnitudes 1e-8 .. 1e8; SUM x on slot 0 (registers) and on slot 8 (LDS), each within 1 ULP of math.fsum."""
    T, g = 2048, 3
    n = 6 * T + 1000
    rng = np.random.default_rng(7)
    w, _ww = weights(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    aggs = [("SUM", "x", "s0")] + [("MIN" if j % 2 else "MAX", "w", "m%d" % j) for j in range(1, 8)] + [("SUM", "x", "s8")]
    return PipeCase("inexact-sum", [Col("x", "DOUBLE", x), Col("w", "INT64", w)], [("agg", aggs)], {"tile_rows": T, "grid_limit": g}, stated_facts(n, T, g), inexact=("s0", "s8"))


def all_cases(max_rows=None):
    """Every PipeCase of the suite, one per distinct input (cases that differ in context options only are left out)."""
    seen = set()

    def fresh(cases):
        for c in cases:
            if c.data_key not in seen and (max_rows is None or c.rows <= max_rows):
                seen.add(c.data_key)
                yield c
    for T in TILES:
        for g in GRID_LIMITS:
            for c in fresh(tile_loop_sweep(T, g)):
                yield c
    for c in fresh(nan_case(kind, T) for kind in NAN_KINDS for T in (512, 2048)):
        yield c
    for c in fresh(slot_case(n, rot) for n in SLOT_COUNTS[:3] for rot in range(6)):
        yield c
    for c in fresh(staging_case(s, T, fam) for s, T in STAGING_SHAPES for fam in STAGING_FAMILIES):
        yield c
    for c in fresh([odd_address_case(), inexact_sum_case()]):
        yield c
    for c in fresh(filter_case(n, kind, 1, 0) for n in FILTER_ROWS for kind in SURVIVORS):
        yield c
    if max_rows is None or SCAN_CARRY_ROWS <= max_rows:
        for c in fresh([scan_carry_case()]):
            yield c
    if max_rows is None or max(ARENA_ROWS) <= max_rows:
        for c in fresh(arena_case(run) for run in range(3)):
            yield c

"""Every execution form of run_sort (supersonic_amd/csrc/runtime.cpp) at the sizes where it switches, against a stable reference.

run_sort chooses per run: plain LSD passes (sort_mode 0), high digits + tie fix-up on (key, row id) pairs (1:
ssgpu_sort_fix_ties_kernel), one-word (high half << 32 | row id) keys (2: ssgpu_sort_fix_ties_compact_kernel), either hybrid
falling back to all digits when a tie run is too long (17, 18); and for the payload: keys only, column gathers or fixed-stride
records.  Random keys reach these forms but not their edges: here `sort_reference.tie_layout` plants the runs of equal high
parts on workgroup and thread edges, at both ends of the array and next to each other, and `sort_reference.stable_order` --
the device sort is stable -- gives the expected row order bit for bit (tests/test_sort_reference_cpu.py checks both)."""
import ctypes
import functools

import numpy as np
import pytest

import supersonic_amd as ss
from sort_reference import (BOUNDARY_LENGTHS, LONG_RUNS, N_TIES, boundary_key, gather, geometry_key, long_run_key, stable_order)

pytestmark = pytest.mark.gpu

HYBRID, FELL_BACK = (1, 2), (17, 18)


def make_ctx(**options):
    ctx = ss.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])     # floats as integers


def run_sort_case(view, order, projection, options=None, context="", device_view=None, fetched=None, ctx=None):
    """Sort `view` (a host View) by `order` ([(name, descending), ...], major key first), keep `projection` (names, None = all),
    in a fresh context with `options`; two runs of one plan, each compared with the rows `stable_order` picks: data bit for bit
    (NULL rows included: the sort moves rows, it computes nothing) and NULL masks.  device_view: the same columns already on the
    device, scanned instead of `view`.  ctx: the context to use (it has the options already).  fetched: a list that receives the View fetched after the last run.  Returns stage_info()[0] of
    the last run."""
    schema = view.schema()
    names = [schema.attribute(i).name() for i in range(schema.attribute_count())]
    host = [(view.column(i).data, view.column(i).is_null) for i in range(view.column_count())]
    want = gather(host, stable_order(host, [(names.index(name), descending) for name, descending in order]))
    spec = ss.SortOrder()
    for name, descending in order:
        spec.add(name, ss.DESCENDING if descending else ss.ASCENDING)
    projector = None if projection is None else ss.ProjectNamedAttributes(list(projection))
    out_cols = [names.index(name) for name in (projection if projection is not None else names)]
    plan = ss.Plan(ss.Sort(spec, projector, 0, ss.ScanView(device_view if device_view is not None else view)), ctx if ctx is not None else make_ctx(**(options or {})))
    info = None
    for run in range(2):
        plan.run()
        got = plan.fetch()
        assert got.column_count() == len(out_cols) and got.row_count() == view.row_count(), (context, got.column_count(), got.row_count())
        for i, col in enumerate(out_cols):
            where = "%s: run %d, column %s" % (context, run, names[col])
            wd, wz = want[col]
            g, w = bits_of(got.column(i).data), bits_of(wd)
            assert g.dtype == w.dtype and len(g) == len(w), (where, g.dtype, w.dtype, len(g), len(w))
            bad = np.nonzero(g != w)[0]
            assert len(bad) == 0, "%s: %d rows differ, first at %s: got %s want %s" % (where, len(bad), bad[:8], g[bad[:8]], w[bad[:8]])
            if schema.attribute(col).is_nullable():
                gz = got.column(i).is_null
                assert gz is not None, where
                wz = np.zeros(len(wd), bool) if wz is None else wz
                bad = np.nonzero(gz != wz)[0]
                assert len(bad) == 0, "%s: NULL masks differ at %s" % (where, bad[:8])
        info = plan.stage_info()[0]
    if fetched is not None:
        fetched.append(got)
    return info


SS_TYPE = {"INT64": ss.INT64, "UINT64": ss.UINT64, "DOUBLE": ss.DOUBLE}


def tie_view(key, ktype, payload=2, nullability=ss.NOT_NULLABLE, key_nulls=None, extra=()):
    """k (the wide key), id (the row number: what tells duplicates apart), `payload` value columns, then `extra` (name, type, data)."""
    n = len(key)
    rng = np.random.default_rng(n + payload)
    attrs = [ss.Attribute("k", SS_TYPE[ktype], nullability), ss.Attribute("id", ss.INT64)]
    cols = [ss.Column(key, key_nulls), ss.Column(np.arange(n, dtype=np.int64))]
    for i in range(payload):
        attrs.append(ss.Attribute("p%d" % i, ss.DOUBLE if i % 2 == 0 else ss.INT64))
        cols.append(ss.Column(rng.integers(-9, 9, n) * 0.5 if i % 2 == 0 else rng.integers(-(1 << 40), 1 << 40, n)))
    for name, t, data in extra:
        attrs.append(ss.Attribute(name, t))
        cols.append(ss.Column(data))
    return ss.View(ss.TupleSchema(attrs), cols, n)


# the three forms a wide first key can take: (projection, options, sort_mode of the hybrid, of its fallback)
FORMS = {
    "compact": (["k", "id", "p0", "p1"], {}, 2, 18),                        # one-word keys, records with a row-id stride of 2
    "pairs_records": (["k", "id", "p0", "p1"], {"sort_compact": 0}, 1, 17),  # (key, row id) pairs: fix_ties<true>, records
    "pairs_keys_only": (["k"], {"sort_compact": 0}, 1, 17),                  # integer keys: no row ids, fix_ties<false> + unkey
}


# ---- a. tie-run geometry --------------------------------------------------------------------------------------------------
# (a DOUBLE key is never read back from the sorted keys: there is no keys-only form for it)
GEOMETRY_CASES = [(layout, ktype, descending, form) for layout in ("A", "B") for ktype in ("INT64", "UINT64", "DOUBLE") for descending in (False, True)
                  for form in FORMS if not (form == "pairs_keys_only" and ktype == "DOUBLE")]


@pytest.mark.parametrize("layout,ktype,descending,form", GEOMETRY_CASES, ids=["%s-%s-%s-%s" % (c[0], c[1], "desc" if c[2] else "asc", c[3]) for c in GEOMETRY_CASES])
def test_tie_runs_on_workgroup_and_thread_edges(layout, ktype, descending, form):
    projection, options, mode, _fallback = FORMS[form]
    view = tie_view(geometry_key(layout, 32, ktype, descending), ktype)
    info = run_sort_case(view, [("k", descending)], projection, options, "layout %s %s %s %s" % (layout, ktype, descending, form))
    assert info["sort_mode"] == mode and info["sort_passes"] == 4, info


# ---- b. the too-long boundary ---------------------------------------------------------------------------------------------
BOUNDARY_KEYS = {"int64_asc": ("INT64", False), "double_desc": ("DOUBLE", True)}


@functools.lru_cache(maxsize=None)
def boundary_case(form, keys, length):
    ktype, descending = BOUNDARY_KEYS[keys]
    projection, options, _mode, _fallback = FORMS[form]
    view = tie_view(boundary_key(length, ktype, descending), ktype)
    info = run_sort_case(view, [("k", descending)], projection, options, "one run of %d, %s %s" % (length, keys, form))
    return info["sort_mode"], info["sort_passes"]


@pytest.mark.parametrize("length", BOUNDARY_LENGTHS)
@pytest.mark.parametrize("keys", list(BOUNDARY_KEYS))
@pytest.mark.parametrize("form", list(FORMS))
def test_one_tie_run_of_any_length_is_sorted_exactly(form, keys, length):
    # (pairs_keys_only with the DOUBLE key: the key column is gathered like any other -- fix_ties<true> and column gathers)
    mode, passes = boundary_case(form, keys, length)
    assert mode in HYBRID + FELL_BACK, mode
    if mode in FELL_BACK:
        assert passes >= 8, passes


@pytest.mark.parametrize("keys", list(BOUNDARY_KEYS))
@pytest.mark.parametrize("form", list(FORMS))
def test_runs_up_to_one_length_stay_hybrid_and_longer_ones_fall_back(form, keys):
    _projection, _options, hybrid, fallback = FORMS[form]
    modes = [boundary_case(form, keys, length)[0] for length in BOUNDARY_LENGTHS]
    assert set(modes) <= {hybrid, fallback}, modes
    n_hybrid = sum(1 for m in modes if m == hybrid)
    assert modes == [hybrid] * n_hybrid + [fallback] * (len(modes) - n_hybrid), modes         # monotone in the length
    assert modes[BOUNDARY_LENGTHS.index(8)] == hybrid and modes[BOUNDARY_LENGTHS.index(1000)] == fallback, modes
    # T = the longest hybrid length of the list: T + 1 is in the list too, so both sides of the boundary -- wherever it is -- ran
    t = BOUNDARY_LENGTHS[n_hybrid - 1]
    assert t + 1 in BOUNDARY_LENGTHS and BOUNDARY_LENGTHS[n_hybrid] == t + 1, (t, modes)


# Longer runs that are in order already: the pairs kernel reads such a run once (up to 1024 rows) and leaves it alone; one row
# out of place, or one row more, and all digits are sorted after all.  The one-word form falls back for every run this long.
LONG_RUN_HYBRID = {(200, "asc"): True, (200, "rotated"): False, (722, "copies"): True, (1024, "asc"): True, (1025, "asc"): False, (1025, "copies"): False}
assert set(LONG_RUN_HYBRID) == set(LONG_RUNS)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("length,content", LONG_RUNS, ids=["%d-%s" % c for c in LONG_RUNS])
def test_long_tie_runs_that_are_in_order_already(length, content, form):
    projection, options, hybrid, fallback = FORMS[form]
    view = tie_view(long_run_key(length, content), "INT64")
    info = run_sort_case(view, [("k", False)], projection, options, "one run of %d, %s, %s" % (length, content, form))
    stays = LONG_RUN_HYBRID[(length, content)] and form != "compact"
    assert info["sort_mode"] == (hybrid if stays else fallback), info
    assert info["sort_passes"] == (4 if stays else 12), info


# ---- c. sort_hi_digits ------------------------------------------------------------------------------------------------------
def uniform_keys(n, seed, copies_every):
    """Uniform 64-bit INT64 keys; every `copies_every`-th row is a copy of row 5 (exact duplicates: input order must survive)."""
    key = np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=np.uint64).view(np.int64)
    key[::copies_every] = key[5]
    return key


def both_hybrid_and_plain(view, order, projection, options, context):
    info = run_sort_case(view, order, projection, options, context)
    plain = run_sort_case(view, order, projection, dict(options, sort_hybrid=0), context + ", sort_hybrid=0")      # the same rows
    assert plain["sort_mode"] == 0, plain
    return info


@pytest.mark.parametrize("payload", [0, 4])
@pytest.mark.parametrize("keys", list(BOUNDARY_KEYS))
@pytest.mark.parametrize("layout", ["A", "B"])
def test_three_high_digits_then_ties_of_the_high_24_bits(layout, keys, payload):
    ktype, descending = BOUNDARY_KEYS[keys]
    # payload 0: the key alone -- for INT64 no row ids at all (fix_ties<false> with a shift of 40, then unkey); a DOUBLE key is
    # never read back from the sorted keys, it is gathered by row id.  payload 4: k, id, p0..p3 as records
    view = tie_view(geometry_key(layout, 24, ktype, descending), ktype, payload=4)
    projection = ["k"] if payload == 0 else None
    info = both_hybrid_and_plain(view, [("k", descending)], projection, {"sort_hi_digits": 3}, "3 high digits, layout %s %s payload %d" % (layout, keys, payload))
    assert info["sort_mode"] == 1 and info["sort_passes"] == 3, info


@pytest.mark.parametrize("projection", [None, ["k"]], ids=["k_id_p0_p1", "keys_only"])
def test_two_high_digits_uniform_keys_with_722_copies_of_one_key(projection):
    # key[::97] = key[5]: 722 copies of one key are ONE tie run far beyond what ssgpu_sort_fix_ties_kernel sorts itself -- but
    # copies are in order as they stand (the passes are stable), so the kernel leaves them alone and nothing falls back
    view = tie_view(uniform_keys(N_TIES, 61, 97), "INT64", payload=2)
    info = both_hybrid_and_plain(view, [("k", False)], projection, {"sort_hi_digits": 2}, "2 high digits, 722 copies")
    assert info["sort_mode"] == 1 and info["sort_passes"] == 2, info


@pytest.mark.parametrize("projection", [None, ["k"]], ids=["k_id_p0_p1", "keys_only"])
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_two_high_digits_uniform_keys_with_47_copies_of_one_key(descending, projection):
    # 70001 uniform keys over 65536 high parts of 16 bits: most rows are in a run of 2..8; the 47 copies are one run below the limit
    view = tie_view(uniform_keys(N_TIES, 61, 1499), "INT64", payload=2)
    info = both_hybrid_and_plain(view, [("k", descending)], projection, {"sort_hi_digits": 2}, "2 high digits, 47 copies")
    assert info["sort_mode"] == 1 and info["sort_passes"] == 2, info


@pytest.mark.parametrize("projection", [None, ["k"]], ids=["k_id_p0_p1", "keys_only"])
@pytest.mark.parametrize("n,passes,copies_every", [(N_TIES, 2, 1499), (600011, 3, 9973)])
def test_high_digit_count_by_row_count(n, passes, copies_every, projection):
    # sort_hi_digits = 0: as few digits as keep n / 256^d <= 8 -- 2 digits at 70001 rows, 3 at 600011 (61 copies of one key: a run below the limit)
    view = tie_view(uniform_keys(n, 67, copies_every), "INT64", payload=2)
    info = both_hybrid_and_plain(view, [("k", False)], projection, {"sort_hi_digits": 0}, "digits by row count, %d rows" % n)
    assert info["sort_mode"] == 1 and info["sort_passes"] == passes, info


# ---- d. the row-count switch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("payload", [0, 2, 4])
@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_row_counts_around_the_hybrid_threshold(n, payload, descending):
    # payload 0: keys only; 2: column gathers; 4: records (and one-word keys from 65536 rows on)
    key = uniform_keys(n, 71, 2003)                                      # 33 copies of one key
    key[100:120:2] = key[101:121:2]                                      # and ten adjacent pairs
    view = tie_view(key, "INT64", payload=3)
    projection = {0: ["k"], 2: ["k", "id", "p0"], 4: ["k", "id", "p0", "p1", "p2"]}[payload]
    run_sort_case(view, [("k", descending)], projection, {}, "%d rows, payload %d" % (n, payload))


# ---- e. which key the shortcut may use ------------------------------------------------------------------------------------
def group_column(n):
    return (np.random.default_rng(5).integers(-3, 4, n)).astype(np.int32)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_wide_key_as_the_minor_of_two_keys(descending):
    # g INT32, k DOUBLE: k is processed first, as one-word keys; ssgpu_sort_extract_idx_kernel hands the row ids to the passes over g
    view = tie_view(geometry_key("A", 32, "DOUBLE", descending), "DOUBLE", extra=[("g", ss.INT32, group_column(N_TIES))])
    info = run_sort_case(view, [("g", descending), ("k", descending)], None, {}, "g, k")
    assert info["sort_mode"] == 2, info
    info = run_sort_case(view, [("g", descending), ("k", descending)], None, {"sort_compact": 0}, "g, k as pairs")
    assert info["sort_mode"] == 1, info


def test_wide_key_as_the_major_of_two_keys_takes_no_shortcut():
    view = tie_view(geometry_key("B", 32, "INT64", False), "INT64", extra=[("g", ss.INT32, group_column(N_TIES))])
    key = view.column(0).data
    key[::1499] = key[5]                                                 # ties in k, decided by g
    info = run_sort_case(view, [("k", False), ("g", True)], None, {}, "k, g")
    assert info["sort_mode"] == 0, info


@pytest.mark.parametrize("form", ["compact", "pairs_records"])
def test_nullable_wide_key_without_a_mask_may_take_the_shortcut(form):
    # declared NULLABLE, no NULL mask given (a NULL is_null pointer in the C ABI): the columns of a NOT NULL device block (it
    # has no masks), scanned under a schema that says NULLABLE, in the block's own context
    projection, options, mode, _fallback = FORMS[form]
    key = geometry_key("A", 32, "INT64", False)
    view = tie_view(key, "INT64", nullability=ss.NULLABLE)
    plain = tie_view(key, "INT64")
    ctx = make_ctx(**options)
    block = ss.DeviceBlock(plain.schema(), N_TIES, ctx)
    for i in range(plain.column_count()):
        ctx.check(ctx.lib.ssgpu_block_upload(block.handle, i, plain.column(i).data.ctypes.data_as(ctypes.c_void_p), None, 0, N_TIES))
    ctx.synchronize()
    pointers = [(block.column_ptr(i), block.null_ptr(i)) for i in range(plain.column_count())]
    assert all(null_ptr == 0 for _data_ptr, null_ptr in pointers)
    device_view = ss.DeviceView(view.schema(), pointers, N_TIES)
    info = run_sort_case(view, [("k", False)], projection, options, "NULLABLE, no mask, %s" % form, device_view=device_view, ctx=ctx)
    assert info["sort_mode"] == mode and info["sort_passes"] == 4, info
    del block
    # the same from the host: staging gives the column an all-zero mask -- whichever form runs, the same rows
    run_sort_case(view, [("k", False)], projection, options, "NULLABLE, no mask, host view, %s" % form)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_nullable_wide_key_with_nulls_sorts_all_digits(descending):
    key = geometry_key("B", 32, "DOUBLE", descending)
    nulls = np.random.default_rng(9).random(N_TIES) < 0.1
    view = tie_view(key, "DOUBLE", nullability=ss.NULLABLE, key_nulls=nulls)
    fetched = []
    info = run_sort_case(view, [("k", descending)], None, {}, "10 % NULLs", fetched=fetched)
    assert info["sort_mode"] == 0, info
    # the mask the device returned: NULLs first for ASCENDING, last for DESCENDING
    device_nulls = fetched[0].column(0).is_null
    n_null = int(nulls.sum())
    assert 0 < n_null < N_TIES and int(device_nulls.sum()) == n_null
    assert device_nulls[-n_null:].all() if descending else device_nulls[:n_null].all()


def test_wide_key_whose_low_words_are_all_equal():
    rng = np.random.default_rng(13)
    hi = rng.integers(0, 1 << 32, N_TIES, dtype=np.uint64)
    hi[::211] = hi[3]
    key = ((hi << np.uint64(32)) | np.uint64(0x9ABCDEF0)).view(np.int64)
    info = run_sort_case(tie_view(key, "INT64"), [("k", False)], None, {}, "equal low words")
    assert info["sort_mode"] == 0 and info["sort_passes"] == 4, info


def test_wide_key_with_one_constant_high_digit():
    key = uniform_keys(N_TIES, 17, 1499).view(np.uint64)
    key = ((key & ~np.uint64(0xFF << 48)) | np.uint64(0x5A << 48)).view(np.int64)         # digit 6 agrees in every key: it is skipped
    info = run_sort_case(tie_view(key, "INT64"), [("k", False)], None, {}, "constant digit 6")
    assert info["sort_mode"] == 0 and info["sort_passes"] == 7, info


# ---- f. payload layout matrix -----------------------------------------------------------------------------------------------
# a payload schema: type letters -- I INT64, D DOUBLE, i INT32, f FLOAT, u UINT32, b BOOL; "?" after a letter: NULLABLE with a
# mask, "!": NULLABLE without one.  Bytes of a record: 8 / 4 / 1 per column + 1 per NULLABLE column, rounded up to 16; the wide
# key's form carries its 8-byte key column in the record too (the INT32 key is read back from the sorted keys instead).
LETTER = {"I": ss.INT64, "D": ss.DOUBLE, "i": ss.INT32, "f": ss.FLOAT, "u": ss.UINT32, "b": ss.BOOL}


def eights(count):
    return " ".join("ID"[i % 2] for i in range(count)) + " "


PAYLOADS = [schema.split() for schema in (
    # schema                payload bytes -> record of the INT32-key form / of the wide-key form
    "i b b?",               # 7 -> 16 / 16: exactly three columns            gather_rec_fast<1>
    "I i? f u",             # 21 -> 32 / 32                                   fast<2>
    "I D I? D! i",          # 38 -> 48 / 48                                   fast<3>
    "I D I D I? D? u",      # 54 -> 64 / 64                                   fast<4>
    eights(8) + "f?",       # 69 -> 80 / 80                                   fast<5>
    eights(10) + "b i",     # 85 -> 96 / 96                                   fast<6>
    eights(12) + "u!",      # 101 -> 112 / 112                                fast<7>
    eights(14) + "f b?",    # 118 -> 128 / 128                                fast<8>
    eights(16) + "i b",     # 133 -> 144 / 144                                the generic kernel: 9 chunks of 16 bytes
    eights(18) + "f?",      # 149 -> 160 / 160                                10
    eights(20) + "u b!",    # 166 -> 176 / 176                                11
    eights(22) + "i? b",    # 182 -> 192 / 192                                12
    eights(24) + "f u",     # 200 -> 208 / 208                                13
    eights(26) + "i!",      # 213 -> 224 / 224                                14: the largest record
    "I " * 29,              # 232 -> 240 / 240: more than 224 bytes -- column gathers (the wide key: as pairs)
    "I D?",                 # exactly two columns: no records (with the wide key itself: three, 25 -> 32)
    "D i? b",               # 14 -> 16 / 22 -> 32: three columns, a NULLABLE one among them
)]


def payload_view(n, letters, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(-40, 40, n).astype(np.int32)                        # the INT32 key: duplicates from 81 rows on
    k = geometry_key("A", 32, "INT64", False) if n == N_TIES else rng.integers(-(1 << 62), 1 << 62, n)
    attrs, cols = [ss.Attribute("g", ss.INT32), ss.Attribute("k", ss.INT64)], [ss.Column(g), ss.Column(k)]
    for j, letter in enumerate(letters):
        t = LETTER[letter[0]]
        if t == ss.BOOL:
            data = rng.integers(0, 2, n).astype(bool)
        elif t in (ss.DOUBLE, ss.FLOAT):
            data = rng.integers(-1000, 1000, n) * 0.125
        elif t == ss.UINT32:
            data = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        elif t == ss.INT32:
            data = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
        else:
            data = rng.integers(-(1 << 63), (1 << 63) - 1, n)
        attrs.append(ss.Attribute("c%d" % j, t, ss.NULLABLE if len(letter) > 1 else ss.NOT_NULLABLE))
        cols.append(ss.Column(data, rng.random(n) < 0.3 if letter[1:] == "?" else None))
    return ss.View(ss.TupleSchema(attrs), cols, n), ["c%d" % j for j in range(len(letters))]


@pytest.mark.parametrize("case", range(len(PAYLOADS)), ids=["".join(p) if len(p) < 8 else "%dx8+%s" % (len(p) - 2, "".join(p[-2:])) for p in PAYLOADS])
def test_payload_layouts_by_an_int32_key(case):
    # row ids from the index array (stride 1); 256 rows = one workgroup of the pack and gather kernels
    for n in (1, 255, 256, 257, N_TIES):
        view, names = payload_view(n, PAYLOADS[case], 1000 + case)
        run_sort_case(view, [("g", case % 2 == 1)], ["g"] + names, {}, "INT32 key, %d rows, payload %s" % (n, " ".join(PAYLOADS[case])))


@pytest.mark.parametrize("case", range(len(PAYLOADS)), ids=["".join(p) if len(p) < 8 else "%dx8+%s" % (len(p) - 2, "".join(p[-2:])) for p in PAYLOADS])
def test_payload_layouts_by_a_wide_key_as_one_word_keys(case):
    # row ids in the low words of the sorted (high half << 32 | row id) keys (stride 2)
    view, names = payload_view(N_TIES, PAYLOADS[case], 2000 + case)
    info = run_sort_case(view, [("k", False)], names + ["k"], {}, "wide key, payload %s" % " ".join(PAYLOADS[case]))
    assert info["sort_passes"] == 4, info
    records = len(names) >= 2 and PAYLOADS[case] != ["I"] * 29            # (with k itself: three or more columns, at most 224 bytes)
    assert info["sort_mode"] == (2 if records else 1), info

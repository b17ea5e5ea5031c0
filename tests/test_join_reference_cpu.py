"""tests/join_reference.py without a GPU: the reference join against the oracle's nested loop (at sizes the loop can afford) and
against a plain Python double loop, the mirrors of the device's index geometry against second implementations, and every
layout's stated geometry -- chain length and wrap, run lengths, rows reaching the expand stage, result row counts.

What cannot be checked here is that the device hashes as `hash64` / `hash_wide` say: that takes a GPU.  The mirrors only place
keys (tests/join_reference.py); a wrong mirror would make the chain layouts of tests/test_sizes_join_forms_gpu.py ordinary inputs, never
a wrong expectation."""
import numpy as np
import pytest

import join_reference as jr
from helpers import assert_cols_equal
from oracle import oracle

JOIN_TYPES = (jr.INNER, jr.LEFT_OUTER)
SHAPES = list(jr.KEY_SHAPES)


# ---- the reference against the oracle and against a double loop -------------------------------------------------------------------
def small_cases(shape, unique):
    """Every kind of layout of the GPU tests, at n <= 2000 and m <= 300."""
    out = [("index m=%d" % m, jr.index_case(m, shape, unique, n=2000)) for m in (1, 9, 300)]
    out += [("chain %d" % length, jr.chain_case(length, shape, unique)) for length in (2, 64)]
    if shape in jr.ONE_WORD_SHAPES:
        out += [("reserved rhs=%d lhs=%d" % (r, l), jr.reserved_case(shape, r, l, run=1 if unique else 3)) for r in (0, 1) for l in (0, 1)]
    if shape == "i64":
        out += [("chunked n=%d" % n, jr.chunked_case(n, unique)) for n in (0, 1, 1001)]
        if not unique:
            out += [("expand", jr.expand_case(jr.expand_fan(500, jr.LEFT_OUTER, "mixed")))]
    return out


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "not_unique"])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_agrees_with_the_oracle(shape, join_type, unique):
    for name, case in small_cases(shape, unique):
        assert case.n <= 2000 and case.m <= 300, name
        if unique:
            assert not jr.has_duplicate_key(case.rhs_keys), name
        lview, rview = jr.views(case)
        _schema, want = oracle.run(jr.join_op(case, join_type, unique, lview, rview, lhs_names=("lid", "a")))
        _pairs, cols = jr.expected(case, join_type, lhs_names=("lid", "a"))
        assert_cols_equal(cols, want, context="%s %s %s %s" % (shape, join_type, "unique" if unique else "not unique", name))
        # NULL masks exactly where the schema has them: LEFT_OUTER makes ri and rs nullable, rw is nullable anyway
        assert [z is not None for _d, z in cols] == [False, False, join_type == jr.LEFT_OUTER, True, join_type == jr.LEFT_OUTER], name


def loop_join(lhs_keys, rhs_keys, join_type):
    def key(cols, i):
        if any(z is not None and z[i] for _d, z in cols):
            return None
        return tuple(np.asarray(d)[i:i + 1].tobytes() for d, _z in cols)
    out = []
    for i in range(len(lhs_keys[0][0])):
        k = key(lhs_keys, i)
        found = [j for j in range(len(rhs_keys[0][0])) if k is not None and key(rhs_keys, j) == k]
        out += [(i, j) for j in found] or ([(i, -1)] if join_type == jr.LEFT_OUTER else [])
    return np.array([p[0] for p in out], dtype=np.int64), np.array([p[1] for p in out], dtype=np.int64)


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_join_pairs_agrees_with_a_double_loop(join_type):
    rng = np.random.default_rng(3)
    for trial in range(60):
        n, m = int(rng.integers(0, 9)), int(rng.integers(0, 7))
        two = trial % 2 == 1
        def side(k):
            cols = [(rng.integers(-1, 3, k), rng.random(k) < 0.2 if trial % 3 else None)]
            if two:     # a DOUBLE second column: -0.0 and 0.0 differ bit for bit, as do two NaNs of different payload
                cols.append((rng.choice(np.array([0.0, -0.0, 1.5, np.nan]), k), rng.random(k) < 0.2))
            return cols
        lhs, rhs = side(n), side(m)
        got, want = jr.join_pairs(lhs, rhs, join_type), loop_join(lhs, rhs, join_type)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (trial, got, want)
        row, twin = loop_join(rhs, rhs, jr.INNER)                          # a row that finds another one: a duplicate key
        assert jr.has_duplicate_key(rhs) == bool((row != twin).any()), trial


def test_gather_join_masks_and_values():
    lhs_row, rhs_row = np.array([0, 0, 2, 3]), np.array([1, 2, -1, 0])
    lhs = [(np.array([10, 11, 12, 13]), None)]
    rhs = [(np.array([5.0, 6.0, 7.0]), np.array([False, True, False])), (np.array([b"x", b"y", b"z"], dtype=object), None)]
    (ld, lz), (d0, z0), (d1, z1) = jr.gather_join((lhs_row, rhs_row), lhs, rhs, jr.LEFT_OUTER)
    assert ld.tolist() == [10, 10, 12, 13] and lz is None
    assert d0.tolist() == [6.0, 7.0, 0.0, 5.0] and z0.tolist() == [True, False, True, False]
    assert d1.tolist() == [b"y", b"z", b"", b"x"] and z1.tolist() == [False, False, True, False]
    keep = rhs_row >= 0
    _l, (_d0, z0), (_d1, z1) = jr.gather_join((lhs_row[keep], rhs_row[keep]), lhs, rhs, jr.INNER)
    assert z0.tolist() == [True, False, False] and z1 is None


# ---- the mirrors -------------------------------------------------------------------------------------------------------------------
def hash64_int(k):
    mask = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & mask
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & mask
    k ^= k >> 33
    return k & 0xFFFFFFFF


def test_hash64_agrees_with_python_integers():
    rng = np.random.default_rng(11)
    keys = np.concatenate([rng.integers(0, 1 << 64, 5000, dtype=np.uint64), np.array([0, 1, (1 << 64) - 1, (1 << 64) - 2, 1 << 63, (1 << 33) - 1], dtype=np.uint64)])
    assert jr.hash64(keys).tolist() == [hash64_int(int(k)) for k in keys]
    his = rng.integers(0, 1 << 64, len(keys), dtype=np.uint64)
    assert jr.hash_wide(keys, his).tolist() == [hash64_int(int(lo) ^ hash64_int(int(hi))) for lo, hi in zip(keys, his)]
    for cap in (16, 1024, 1 << 17):
        assert jr.home_slot(cap, keys).tolist() == [hash64_int(int(k)) % cap for k in keys]


def test_capacity_at_the_sizes_of_the_index_cases():
    assert [jr.capacity(m) for m in (0, 1, 8, 9, 16, 17)] == [16, 16, 16, 32, 32, 64]
    assert {m: jr.capacity(m) for m in jr.INDEX_SIZES} == {1: 16, 8: 16, 9: 32, 4096: 8192, 4097: 16384, 16384: 32768, 16385: 65536,
                                                           32768: 65536, 32769: 131072}
    # the scan over cap + 1 run counts is one kernel up to 65536 elements and three (chunks of 8192) beyond:
    assert jr.capacity(16384) + 1 <= 65536 < jr.capacity(16385) + 1
    assert (jr.capacity(16385) + 1) % 8192 == 1                           # slot `cap` is alone in the last chunk


def test_packing_of_every_shape_and_the_keys_that_pack_to_all_ones():
    rng = np.random.default_rng(5)
    for shape in SHAPES:
        lo = rng.integers(0, 1 << 64, 100, dtype=np.uint64)
        hi = rng.integers(0, 1 << 64, 100, dtype=np.uint64) if jr.is_wide(shape) else None
        cols = jr.unpack_key(shape, lo, hi)
        assert [c.dtype for c in cols] == [np.dtype(jr.NP_OF[t]) for t in jr.KEY_SHAPES[shape]]
        back = jr.pack_key(shape, cols)
        assert np.array_equal(back[0], lo) and (hi is None) == (back[1] is None) and (hi is None or np.array_equal(back[1], hi))
    ones = jr.ALL_ONES
    assert jr.pack_key("i64", [np.array([-1])])[0][0] == ones and jr.pack_key("u64", [np.array([2 ** 64 - 1], dtype=np.uint64)])[0][0] == ones
    assert jr.pack_key("i32i32", [np.array([-1]), np.array([-1])])[0][0] == ones
    assert jr.pack_key("u32i32", [np.array([2 ** 32 - 1], dtype=np.uint32), np.array([-1])])[0][0] == ones
    # the near misses: all ones minus one, and (-1, -2)
    assert [c.tolist() for c in jr.unpack_key("i64", np.array(jr.NEAR_MISSES["i64"], dtype=np.uint64))] == [[-2]]
    assert [c.tolist() for c in jr.unpack_key("u64", np.array(jr.NEAR_MISSES["u64"], dtype=np.uint64))] == [[2 ** 64 - 2]]
    assert [c.tolist() for c in jr.unpack_key("i32i32", np.array(jr.NEAR_MISSES["i32i32"], dtype=np.uint64))] == [[-2, -1], [-1, -2]]
    assert [c.tolist() for c in jr.unpack_key("u32i32", np.array(jr.NEAR_MISSES["u32i32"], dtype=np.uint64))] == [[2 ** 32 - 2, 2 ** 32 - 1], [-1, -2]]


@pytest.mark.parametrize("wide", [False, True])
def test_keys_homing_at_every_key_homes_where_it_was_asked_to(wide):
    rng = np.random.default_rng(2)
    for cap, slots, count in ((16, [15], 5), (1024, [1021, 1022, 1023], 90), (2048, [0, 2047], 40)):
        keys, homes = jr.keys_homing_at(cap, slots, count, rng, wide)
        lo, hi = keys if wide else (keys, None)
        assert len(lo) == count * len(slots) and homes.tolist() == [s for s in slots for _ in range(count)]
        assert jr.home_slot(cap, lo, hi).tolist() == homes.tolist()                           # all of them
        assert [(hash64_int(int(a) ^ hash64_int(int(b))) if wide else hash64_int(int(a))) % cap for a, b in zip(lo, hi if wide else lo)] == homes.tolist()
        assert len(set(zip(lo.tolist(), hi.tolist())) if wide else set(lo.tolist())) == len(lo)   # distinct
        assert wide or not (lo == jr.ALL_ONES).any()


# ---- the layouts' stated geometry --------------------------------------------------------------------------------------------------
def packed(case, side):
    return jr.pack_key(case.shape, [d for d, _z in (case.lhs_keys if side == "lhs" else case.rhs_keys)])


def any_null(keys):
    out = np.zeros(len(keys[0][0]), bool)
    for _d, z in keys:
        if z is not None:
            out |= z
    return out


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "not_unique"])
@pytest.mark.parametrize("shape", ["i64", "i64i64"])
@pytest.mark.parametrize("m", jr.INDEX_SIZES)
def test_index_cases(m, shape, unique):
    case = jr.index_case(m, shape, unique)
    assert case.m == m and case.n == jr.N_LHS
    assert jr.has_duplicate_key(case.rhs_keys) == (not unique and m > 1)
    live = ~any_null(case.rhs_keys)
    assert int((~live).sum()) == jr.rhs_null_rows(m, unique) and (m == 1 or not unique or m & (m - 1) or live.all())
    lo, hi = packed(case, "rhs")
    keys = np.stack([lo[live], hi[live] if hi is not None else lo[live]], axis=1)
    _distinct, counts = np.unique(keys, axis=0, return_counts=True)
    assert len(counts) == case.notes["distinct"] and counts.max() == case.notes["max_run"]
    if unique:
        assert counts.max() == 1
        if m in (8, 32768):
            assert 2 * len(counts) == jr.capacity(m)                     # load exactly one half
    elif m >= 8:
        assert 1 <= counts.min() and 2 <= counts.max() <= 4
        assert m < 4096 or set(counts.tolist()) == {1, 2, 3, 4}
    if m > 1 and not jr.is_wide(shape):
        assert (lo[live] == jr.ALL_ONES).sum() >= 1                      # the reserved key is on a (non-NULL) rhs row
        assert packed(case, "lhs")[0][7] == jr.ALL_ONES and not any_null(case.lhs_keys)[7]
    matched, unmatched = case.matched_and_unmatched()
    assert matched > jr.N_LHS // 3 and unmatched > jr.N_LHS // 3
    assert 0 < any_null(case.lhs_keys).sum() < jr.N_LHS // 10
    if not unique and m >= 16384:                                        # rows of one key lie in different 4096-row tiles of the rhs-row sort
        order = np.lexsort([np.arange(m)[live], lo[live]] if hi is None else [np.arange(m)[live], lo[live], hi[live]])
        rows, same = np.arange(m)[live][order], np.all(keys[order][1:] == keys[order][:-1], axis=1)
        assert (same & (rows[1:] // 4096 != rows[:-1] // 4096)).sum() > 100


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "not_unique"])
@pytest.mark.parametrize("shape", ["i64", "i32i32", "i64i64"])
@pytest.mark.parametrize("length", jr.CHAIN_LENGTHS)
def test_chain_cases(length, shape, unique):
    case = jr.chain_case(length, shape, unique)
    cap, head = case.notes["cap"], case.notes["head"]
    assert cap == jr.capacity(case.m) and (not unique or case.m == {2: 8, 64: 70, 257: 300}[length])
    live = ~any_null(case.rhs_keys)
    lo, hi = packed(case, "rhs")
    homes = jr.home_slot(cap, lo[live], None if hi is None else hi[live]).astype(np.int64)
    assert set(homes.tolist()) == ({cap - 1} if length == 2 else {cap - 3, cap - 2, cap - 1})     # every indexed row homes on the last slots
    klo, khi = case.notes["keys"]
    assert len(klo) == length and len(set(zip(klo.tolist(), khi.tolist())) if khi is not None else set(klo.tolist())) == length
    assert jr.home_slot(cap, klo, khi).tolist() == case.notes["homes"].tolist()
    # the chain: `length` slots in a row from the head, across the table's end
    taken = jr.occupied_slots(cap, case.notes["homes"])
    assert taken == {(head + i) % cap for i in range(length)} and cap - 1 in taken and 0 in taken
    # the absent keys home at the head and are on no rhs row: a probe walks `length` slots to the first free one
    alo, ahi = case.notes["absent"]
    assert (jr.home_slot(cap, alo, ahi) == np.uint64(head)).all() and len(alo) == 8
    absent = jr.JoinCase(shape, jr._columns(shape, alo, ahi, None), case.rhs_keys)
    assert absent.matched_and_unmatched() == (0, 8)
    # the lhs probes every member (without a NULL over it) and every absent key
    plo, phi = packed(case, "lhs")
    ok = ~any_null(case.lhs_keys)
    probed = set(zip(plo[ok].tolist(), phi[ok].tolist())) if phi is not None else set(plo[ok].tolist())
    assert (set(zip(klo.tolist(), khi.tolist())) | set(zip(alo.tolist(), ahi.tolist())) if phi is not None else set(klo.tolist()) | set(alo.tolist())) <= probed
    matched, unmatched = case.matched_and_unmatched()
    assert matched >= length and unmatched >= 8
    assert jr.has_duplicate_key(case.rhs_keys) == (not unique)


@pytest.mark.parametrize("shape", jr.ONE_WORD_SHAPES)
def test_reserved_cases(shape):
    for rhs_has in (0, 1):
        for lhs_has in (0, 1):
            for run, m in ((1, 300), (3, 300), (300, 600), (3, 16385)):
                case = jr.reserved_case(shape, rhs_has, lhs_has, run=run, m=m)
                lo, live = packed(case, "rhs")[0], ~any_null(case.rhs_keys)
                assert case.m == m and ((lo == jr.ALL_ONES) & live).sum() == (run if rhs_has else 0)
                for near in jr.NEAR_MISSES[shape]:
                    assert ((lo == np.uint64(near)) & live).sum() == 1
                plo, ok = packed(case, "lhs")[0], ~any_null(case.lhs_keys)
                assert ((plo == jr.ALL_ONES) & ok).sum() == (4 if lhs_has else 0)
                assert all(((plo == np.uint64(near)) & ok).any() for near in jr.NEAR_MISSES[shape])
                pairs = case.pairs(jr.INNER)
                on_reserved = np.isin(pairs[0], np.flatnonzero(plo == jr.ALL_ONES))
                assert on_reserved.sum() == (4 * run if rhs_has and lhs_has else 0)
                matched, unmatched = case.matched_and_unmatched()
                assert matched > 500 and unmatched > 500
    absent = jr.reserved_case(shape, 1, 1, near_on_rhs=False)
    assert not np.isin(packed(absent, "rhs")[0], np.array(jr.NEAR_MISSES[shape], dtype=np.uint64)).any()


@pytest.mark.parametrize("shape", ["i64", "i32i32", "i64i64"])
def test_far_duplicate_cases(shape):
    for reserved in ([False, True] if shape != "i64i64" else [False]):
        case = jr.far_duplicate_case(shape, reserved)
        assert case.m == 16385 and jr.has_duplicate_key(case.rhs_keys)
        lo, hi = packed(case, "rhs")
        same = (lo == lo[0]) & (True if hi is None else hi == hi[0])
        assert np.flatnonzero(same).tolist() == [0, 16384] and (lo[0] == jr.ALL_ONES) == reserved
        once = [(d[1:], None) for d, _z in case.rhs_keys]
        assert not jr.has_duplicate_key(once)                            # nothing else repeats


def stage_rows(case, join_type):
    """lhs rows that reach the expand stage: INNER drops the unmatched ones ahead of it."""
    matched, _unmatched = case.matched_and_unmatched()
    return matched if join_type == jr.INNER else case.n


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_expansion_cases(join_type):
    for n_stage in jr.EXPAND_N:
        for fanout in ("ones", "mixed"):
            case = jr.expand_case(jr.expand_fan(n_stage, join_type, fanout))
            assert stage_rows(case, join_type) == n_stage
            lhs_row, rhs_row = case.pairs(join_type)
            per_row = np.bincount(lhs_row[rhs_row >= 0], minlength=case.n)
            assert np.array_equal(per_row, case.notes["fan"])              # every lhs row's fan-out is what the layout says
            assert per_row.max() == (1 if fanout == "ones" else 4) or n_stage == 1
            if n_stage > 1:
                assert per_row[0] == 0 and per_row[-1] == 0                # unmatched rows at both ends
            if join_type == jr.LEFT_OUTER and n_stage >= 65536:
                assert not per_row[20000:29000].any() and 29000 - 20000 > 8192
    for total in (65536, 65537):
        case = jr.expand_case(jr.fan_with_output(total, join_type))
        assert len(case.pairs(join_type)[0]) == total
        matched, unmatched = case.matched_and_unmatched()
        assert matched > 1000 and unmatched > 1000
    for where, at in (("first", [0]), ("last", [2999]), ("adjacent", [1500, 1501])):
        case = jr.expand_case(jr.big_run_fan(where), big=True)
        lhs_row, rhs_row = case.pairs(join_type)
        per_row = np.bincount(lhs_row[rhs_row >= 0], minlength=case.n)
        assert np.flatnonzero(per_row == jr.BIG_RUN).tolist() == at and case.n == 3000
        run = rhs_row[lhs_row == at[0]]
        assert len(run) == jr.BIG_RUN and (np.diff(run) > 0).all()         # ascending rhs row, interleaved with other keys' rows
        assert run[-1] - run[0] > jr.BIG_RUN


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "not_unique"])
def test_chunked_cases(unique):
    for n in jr.CHUNKED_N:
        case = jr.chunked_case(n, unique)
        assert case.n == n and case.m == 300 and jr.has_duplicate_key(case.rhs_keys) == (not unique)
        if n >= 1000:
            matched, unmatched = case.matched_and_unmatched()
            assert matched > n // 3 and unmatched > n // 4
    barren = jr.chunked_case(70001, False, barren=True)
    lhs_row, _rhs_row = barren.pairs(jr.INNER)
    for chunk in (1000, 4096):                                           # whole chunks without a result row
        with_rows = np.unique(lhs_row // chunk)
        assert len(with_rows) < -(-70001 // chunk) - 3
    assert not np.isin(np.arange(4096, 20480), lhs_row).any()

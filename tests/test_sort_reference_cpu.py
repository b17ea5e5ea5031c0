"""The reference of tests/test_sort_forms_gpu.py, checked where no GPU is needed: `sort_reference.stable_order` against the CPU
oracle's Sort, and `sort_reference.tie_layout` against its own contract -- the tie runs lie where they were designed and all
eight digits of the keys vary, which is what sends a GPU case to the execution form it is meant for."""
import numpy as np
import pytest

import supersonic_amd as ss
from helpers import assert_cols_equal, sort_rows
from oracle import oracle
from sort_reference import layouts_in_use, radix_image, stable_order, gather, tie_layout

TYPES = ["INT32", "UINT32", "INT64", "UINT64", "FLOAT", "DOUBLE", "BOOL", "DATE"]


def distinct_values(rng, tname, n):
    """n distinct values of the type, of both signs where it has two, in random order (BOOL: None, it has only two values)."""
    if tname == "BOOL":
        return None
    if tname in ("FLOAT", "DOUBLE"):
        return (rng.permutation(n) - n // 2 + 0.5) * 0.25           # exact in float32 too; no zero
    if tname in ("UINT32", "UINT64"):
        bits = 32 if tname == "UINT32" else 64
        return rng.permutation(np.unique(rng.integers(0, 1 << bits, 4 * n + 4, dtype=np.uint64)))[:n]      # (both halves of the range)
    bits = 31 if tname in ("INT32", "DATE") else 63
    return rng.permutation(np.unique(rng.integers(-(1 << bits), 1 << bits, 4 * n + 4)))[:n]


def few_values(rng, tname, n):
    if tname == "BOOL":
        return rng.integers(0, 2, n).astype(bool)
    pool = distinct_values(rng, tname, 7)
    return pool[rng.integers(0, 7, n)]


def sort_op(schema, cols, keys, n):
    order = ss.SortOrder()
    for col, descending in keys:
        order.add(schema.attribute(col).name(), ss.DESCENDING if descending else ss.ASCENDING)
    return ss.Sort(order, ss.ProjectAllAttributes(), 0, ss.ScanView(ss.View(schema, cols, n)))


def host_columns(schema, cols):
    view = ss.View(schema, cols)
    return [(view.column(i).data, view.column(i).is_null) for i in range(view.column_count())]


@pytest.mark.parametrize("n", [0, 1, 1000])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("tname", TYPES)
def test_stable_order_is_the_oracles_order_when_the_whole_key_is_unique(tname, descending, nulls, n):
    rng = np.random.default_rng(len(tname) * 1000 + n + descending)
    N = ss.NULLABLE if nulls else ss.NOT_NULLABLE
    t = getattr(ss, tname)
    schema = ss.TupleSchema([ss.Attribute("t", ss.BOOL, N), ss.Attribute("v", t, N), ss.Attribute("u", t), ss.Attribute("id", ss.INT64),
                             ss.Attribute("x", ss.DOUBLE, N)])
    mask = (lambda: rng.random(n) < 0.15) if nulls else (lambda: None)
    unique = distinct_values(rng, tname, n)
    cols = [ss.Column(rng.integers(0, 2, n).astype(bool), mask()), ss.Column(few_values(rng, tname, n), mask()),
            ss.Column(unique if unique is not None else few_values(rng, tname, n)), ss.Column(rng.permutation(n)), ss.Column(rng.integers(-9, 9, n) * 0.5, mask())]
    host = host_columns(schema, cols)
    key_sets = [[(1, descending), (3, not descending)],                       # two keys: duplicates and NULLs, then a unique one
                [(0, not descending), (1, descending), (3, False)]]            # three keys
    if unique is not None:
        key_sets.append([(2, descending)])                                     # one key, unique by itself
        key_sets.append([(1, descending), (2, descending)])
    else:
        key_sets.append([(3, descending)])
    for keys in key_sets:
        _schema, want = oracle.run(sort_op(schema, cols, keys, n))
        got = gather(host, stable_order(host, keys))
        assert_cols_equal(got, want, context="%s keys %s" % (tname, keys))


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("tname", TYPES)
def test_stable_order_with_duplicate_keys_agrees_in_key_columns_and_rows(tname, nulls):
    # the oracle's qsort_r is not stable: with ties only the key columns and the multiset of rows are determined
    n = 1000
    rng = np.random.default_rng(77 + len(tname))
    N = ss.NULLABLE if nulls else ss.NOT_NULLABLE
    schema = ss.TupleSchema([ss.Attribute("v", getattr(ss, tname), N), ss.Attribute("g", ss.INT32, N), ss.Attribute("id", ss.INT64)])
    mask = (lambda: rng.random(n) < 0.15) if nulls else (lambda: None)
    cols = [ss.Column(few_values(rng, tname, n), mask()), ss.Column(rng.integers(-2, 3, n), mask()), ss.Column(np.arange(n))]
    host = host_columns(schema, cols)
    for keys in ([(0, False)], [(0, True)], [(1, True), (0, False)], [(0, True), (1, True)]):
        _schema, want = oracle.run(sort_op(schema, cols, keys, n))
        order = stable_order(host, keys)
        got = gather(host, order)
        key_cols = [col for col, _d in keys]
        assert_cols_equal([got[c] for c in key_cols], [want[c] for c in key_cols], context="%s keys %s: key columns" % (tname, keys))
        assert_cols_equal(sort_rows(got), sort_rows(want), context="%s keys %s: rows" % (tname, keys))
        # and the reference itself is stable: inside a run of equal keys the row ids ascend
        same = np.ones(n - 1, bool)
        for c in key_cols:
            d, z = got[c]
            z = np.zeros(n, bool) if z is None else z
            same &= (z[1:] & z[:-1]) | (~z[1:] & ~z[:-1] & (d[1:] == d[:-1]))
        assert (np.diff(got[2][0])[same] > 0).all()


def test_stable_order_negative_zero_is_zero():
    d = np.array([0.0, -0.0, -1.0, -0.0, 0.0, 1.0])
    assert stable_order([(d, None)], [(0, False)]).tolist() == [2, 0, 1, 3, 4, 5]
    assert stable_order([(d, None)], [(0, True)]).tolist() == [5, 0, 1, 3, 4, 2]


def high_part_runs(image_sorted, hi_bits):
    """(start, length) of every run of two or more equal high parts."""
    hi = image_sorted >> np.uint64(64 - hi_bits)
    edge = np.concatenate([[True], hi[1:] != hi[:-1], [True]])
    starts = np.nonzero(edge)[0]
    return [(int(s), int(e - s)) for s, e in zip(starts[:-1], starts[1:]) if e - s >= 2]


LAYOUTS = layouts_in_use()


@pytest.mark.parametrize("case", range(len(LAYOUTS)), ids=[lay[0] for lay in LAYOUTS])
def test_tie_layout_puts_its_runs_where_they_were_designed(case):
    _name, runs, hi_bits, ktype, descending, key = LAYOUTS[case]
    n = len(key)
    assert key.dtype == {"INT64": np.int64, "UINT64": np.uint64, "DOUBLE": np.float64}[ktype]
    if ktype == "DOUBLE":
        assert np.isfinite(key).all() and (key != 0).all()
    order = stable_order([(key, None)], [(0, descending)])
    image = radix_image(key, ktype, descending)
    in_order = image[order]
    assert (in_order[1:] >= in_order[:-1]).all()                    # the radix image is the sort order
    assert high_part_runs(in_order, hi_bits) == sorted((s, l) for s, l, _c in runs)
    varying = np.bitwise_or.reduce(image) ^ np.bitwise_and.reduce(image)
    assert all((int(varying) >> (8 * b)) & 0xFF for b in range(8)), hex(int(varying))     # OR xor AND: every digit varies
    assert int(varying) & 0xFFFFFFFF
    if ktype == "INT64":
        assert (key < 0).any() and (key > 0).any()
    # what each run holds, in INPUT order (low words of the radix image)
    for start, length, content in runs:
        rows = np.sort(order[start:start + length])
        low = image[rows] & np.uint64(0xFFFFFFFF)
        if content not in ("straddle", "dups"):
            low = image[rows] & np.uint64((1 << (64 - hi_bits)) - 1)          # the whole low part decides
            if hi_bits < 32 and length > 2 and content != "copies":
                assert len(np.unique(low >> np.uint64(32))) > 1               # ... the bits above the low word among it
        assert len(np.unique(image[rows] >> np.uint64(64 - hi_bits))) == 1
        if content == "asc":
            assert (np.diff(low.astype(np.int64)) > 0).all()
        elif content == "desc":
            assert (np.diff(low.astype(np.int64)) < 0).all()
        elif content == "copies":
            assert len(np.unique(image[rows])) == 1
        elif content == "rotated":
            assert (np.diff(low[:-1].astype(np.int64)) > 0).all() and low[-1] < low[0]
        elif content == "dups":
            assert len(np.unique(image[rows])) < length and (length == 2 or low[0] > low[1])
        elif content == "straddle":
            assert (low >= 1 << 31).any() and (low < 1 << 31).any()
            # a signed compare of the low words gives another order than the unsigned one
            assert np.argsort(low, kind="stable").tolist() != np.argsort(low.astype(np.uint32).view(np.int32), kind="stable").tolist()
        else:
            assert len(np.unique(low)) == length
    # outside the designed runs every whole key is unique
    assert len(np.unique(image)) == n - sum(length - len(np.unique(image[order[start:start + length]])) for start, length, _c in runs)


def test_tie_layout_is_shuffled_and_repeatable():
    a = tie_layout(5000, [(10, 3, "random")], 32, "INT64", False, seed=1)
    b = tie_layout(5000, [(10, 3, "random")], 32, "INT64", False, seed=1)
    assert np.array_equal(a, b)
    order = stable_order([(a, None)], [(0, False)])
    assert not np.array_equal(order, np.arange(5000)) and (np.abs(np.diff(order)) > 1).mean() > 0.9

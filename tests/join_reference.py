"""A plain reference for HashJoin, mirrors of the device index's geometry, and the inputs that put index, probe and expansion on
their edges (tests/test_join_reference_cpu.py checks all three without a GPU; tests/test_sizes_join_forms_gpu.py compares the device
join with them).

`join_pairs` is no hash table: dense ids of the distinct keys of both sides (`np.unique(..., return_inverse=True)`, per column
over the columns' BITS), the rhs rows in a stable argsort by id, `searchsorted` for every lhs row's run and `repeat` for the
output.  The result is the reference's order (hash_join.cc:361-470): lhs order, one lhs row's matches in ascending rhs row, so
every comparison is in order and bit for bit.  A NULL in any key column matches nothing.  The oracle's join is a nested loop
that checks UNIQUE up to 4096 rhs rows only: it vouches for this reference at small sizes (tests/test_join_reference_cpu.py),
this reference for the device at the sizes that matter; `has_duplicate_key` is the UNIQUE declaration at any size.

`capacity`, `hash64`, `hash_wide`, `pack_key` and `home_slot` restate build_joins (supersonic_amd/csrc/runtime.cpp),
ssgpu_join_build_kernel and hash64 (pipeline_kernels.hip) and the key packing of lower.cpp (SSGPU_OP_HASH_JOIN): they are used
only to BUILD inputs (keys that share a home slot) and never by `join_pairs`.  Without a GPU they can be checked against a second
implementation in Python integers, not against the device: were the device to hash differently, the chain layouts would
degrade to ordinary random keys and their results would still be compared exactly.

Out of reach at test sizes: pass 3 of the rhs-row sort (sort_rows_by_u32 skips a digit in which all slots agree) sees more
than two digit values only with more than 2^24 slots, i.e. more than 8 M distinct rhs rows; here it runs with the digits 0x00
and 0xFF alone (the rows of NULL keys carry the slot VM_NONE)."""
import numpy as np

U64 = np.uint64
ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)                  # VM_KEY_EMPTY: the packed one-word key that owns the reserved slot `cap`
INNER, LEFT_OUTER = "INNER", "LEFT_OUTER"
NP_OF = {"INT64": np.int64, "UINT64": np.uint64, "INT32": np.int32, "UINT32": np.uint32}
# key shapes: the column types, in key order.  Fields fill word 0 while they fit (lower.cpp: first fit), then word 1
KEY_SHAPES = {"i64": ("INT64",), "u64": ("UINT64",), "i32i32": ("INT32", "INT32"), "u32i32": ("UINT32", "INT32"), "i64i64": ("INT64", "INT64")}
ONE_WORD_SHAPES = ("i64", "u64", "i32i32", "u32i32")
WIDE_SHAPE = "i64i64"


def is_wide(shape):
    return shape == WIDE_SHAPE


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _bits(data):
    a = np.asarray(data)
    if a.dtype == object:
        return a                                                        # STRING: byte strings compare as they are
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def key_ids(lhs_keys, rhs_keys):
    """(lhs id, rhs id, lhs any-NULL, rhs any-NULL): two rows of either side have the same id exactly when they agree bit for
    bit in every key column.  lhs_keys / rhs_keys: [(data, nulls or None), ...], one pair per key column."""
    n, m = len(lhs_keys[0][0]), len(rhs_keys[0][0])
    ids = np.zeros(n + m, dtype=np.int64)
    lnull, rnull = np.zeros(n, bool), np.zeros(m, bool)
    for (ld, lz), (rd, rz) in zip(lhs_keys, rhs_keys):
        lb, rb = _bits(ld), _bits(rd)
        assert lb.dtype == rb.dtype, (lb.dtype, rb.dtype)
        _values, inverse = np.unique(np.concatenate([lb, rb]), return_inverse=True)
        _pairs, ids = np.unique(ids * np.int64(n + m + 1) + inverse.reshape(-1), return_inverse=True)      # dense again: no overflow
        ids = ids.reshape(-1).astype(np.int64)
        if lz is not None:
            lnull |= np.asarray(lz, dtype=bool)
        if rz is not None:
            rnull |= np.asarray(rz, dtype=bool)
    return ids[:n], ids[n:], lnull, rnull


def join_pairs(lhs_keys, rhs_keys, join_type):
    """(lhs_row, rhs_row) of every result row of HashJoin(join_type), int64; rhs_row = -1 for the NULL-extended row of an
    unmatched lhs row (LEFT_OUTER).  lhs order; the matches of one lhs row in ascending rhs row."""
    assert join_type in (INNER, LEFT_OUTER), join_type
    lid, rid, lnull, rnull = key_ids(lhs_keys, rhs_keys)
    n = len(lid)
    rows = np.flatnonzero(~rnull)                                       # a NULL key is never found
    by_key = rows[np.argsort(rid[rows], kind="stable")]                 # rhs rows by key; ascending row inside a key
    sorted_ids = rid[by_key]
    first = np.searchsorted(sorted_ids, lid, side="left")
    count = np.where(lnull, 0, np.searchsorted(sorted_ids, lid, side="right") - first)
    out_count = np.maximum(count, 1) if join_type == LEFT_OUTER else count
    lhs_row = np.repeat(np.arange(n, dtype=np.int64), out_count)
    out_start = np.cumsum(out_count) - out_count
    within = np.arange(len(lhs_row), dtype=np.int64) - np.repeat(out_start, out_count)
    matched = np.repeat(count > 0, out_count)
    at = np.minimum(np.repeat(first, out_count) + within, max(len(by_key) - 1, 0))
    rhs_row = np.where(matched, by_key[at], -1) if len(by_key) else np.full(len(lhs_row), -1, dtype=np.int64)
    return lhs_row, rhs_row.astype(np.int64)


def gather_join(pairs, lhs_cols, rhs_cols, join_type):
    """The result columns [(data, nulls or None), ...]: `lhs_cols` then `rhs_cols` ([(data, nulls or None), ...]) at the rows of
    `pairs`.  LEFT_OUTER makes every rhs column nullable (hash_join.h:39-40); the data of a NULL-extended row is zero / b""
    (the reference leaves it unspecified: compare it nowhere)."""
    lhs_row, rhs_row = pairs
    out = [(np.asarray(d)[lhs_row], None if z is None else np.asarray(z, dtype=bool)[lhs_row]) for d, z in lhs_cols]
    none = rhs_row < 0
    at = np.where(none, 0, rhs_row)
    for d, z in rhs_cols:
        d = np.asarray(d)
        if len(d) == 0:                                                 # an empty rhs table: nothing but NULL-extended rows
            data = np.zeros(len(rhs_row), dtype=d.dtype) if d.dtype != object else np.full(len(rhs_row), b"", dtype=object)
        else:
            data = d[at].copy()
            data[none] = b"" if d.dtype == object else 0
        nulls = None
        if z is not None or join_type == LEFT_OUTER:
            nulls = none.copy()
            if z is not None and len(d):
                nulls |= np.asarray(z, dtype=bool)[at] & ~none
        out.append((data, nulls))
    return out


def has_duplicate_key(rhs_keys):
    """Whether a (non-NULL) key occurs on more than one rhs row: what a UNIQUE declaration must not meet."""
    _lid, rid, _lnull, rnull = key_ids([(np.asarray(d)[:0], None) for d, _z in rhs_keys], rhs_keys)
    ids = rid[~rnull]
    return len(np.unique(ids)) < len(ids)


# ---- mirrors of the device's geometry ----------------------------------------------------------------------------------------------
def capacity(m):
    """Slots of the index over an rhs table of m rows (NULL-key rows count): the smallest power of two >= 2 m, at least 16."""
    cap = 16
    while cap < 2 * max(int(m), 1):
        cap <<= 1
    return cap


def hash64(k):
    """hash64 of pipeline_kernels.hip over a uint64 array: the low 32 bits of the 64-bit finaliser, as uint64."""
    k = np.asarray(k, dtype=U64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> U64(33)
        k *= U64(0xff51afd7ed558ccd)
        k ^= k >> U64(33)
        k *= U64(0xc4ceb9fe1a85ec53)
        k ^= k >> U64(33)
    return k & U64(0xFFFFFFFF)


def hash_wide(lo, hi):
    """The mix of a two-word key: hash64(lo ^ hash64(hi)), the inner hash zero-extended from its 32 bits."""
    return hash64(np.asarray(lo, dtype=U64) ^ hash64(hi))


def home_slot(cap, lo, hi=None):
    """The slot a packed key is looked for first (the all-ones one-word key has none: it owns slot `cap`)."""
    return (hash64(lo) if hi is None else hash_wide(lo, hi)) & U64(cap - 1)


def pack_key(shape, cols):
    """(word 0, word 1 or None) of the key columns `cols` (arrays, in key order) as the index build packs them."""
    words = [np.zeros(len(cols[0]), dtype=U64), np.zeros(len(cols[0]), dtype=U64)]
    fill = [0, 0]
    for t, col in zip(KEY_SHAPES[shape], cols):
        bits = np.dtype(NP_OF[t]).itemsize * 8
        word = 0 if fill[0] + bits <= 64 else 1
        v = _bits(np.ascontiguousarray(col, dtype=NP_OF[t])).astype(U64)
        words[word] |= v << U64(fill[word])
        fill[word] += bits
    return words[0], (words[1] if fill[1] else None)


def unpack_key(shape, lo, hi=None):
    """The key columns (arrays of the shape's types) whose packed key is (lo, hi): the inverse of pack_key."""
    lo = np.asarray(lo, dtype=U64)
    types = KEY_SHAPES[shape]
    if is_wide(shape):
        return [lo.view(np.int64).copy(), np.asarray(hi, dtype=U64).view(np.int64).copy()]
    if len(types) == 1:
        return [lo.view(NP_OF[types[0]]).copy()]
    return [(lo & U64(0xFFFFFFFF)).astype(np.uint32).view(NP_OF[types[0]]).copy(), (lo >> U64(32)).astype(np.uint32).view(NP_OF[types[1]]).copy()]


def keys_homing_at(cap, slots, count, rng, wide=False):
    """`count` distinct random packed keys -- a uint64 array, or (lo, hi) for a two-word table -- per slot of `slots`, every one
    homing on its slot of a table of `cap` slots: random keys are drawn until enough of them do.  Never the all-ones word.
    Returns (keys, homes) in slot-major order."""
    slots = [int(s) for s in slots]
    found = {s: [] for s in slots}
    seen = set()
    while any(len(found[s]) < count for s in slots):
        lo = rng.integers(0, 1 << 64, 1 << 16, dtype=U64)
        hi = rng.integers(0, 1 << 64, 1 << 16, dtype=U64) if wide else None
        home = home_slot(cap, lo, hi)
        for s in slots:
            for j in np.flatnonzero(home == U64(s)):
                key = (int(lo[j]), int(hi[j])) if wide else int(lo[j])
                if len(found[s]) < count and key not in seen and (wide or lo[j] != ALL_ONES):
                    seen.add(key)
                    found[s].append(key)
    flat = [key for s in slots for key in found[s]]
    homes = np.array([s for s in slots for _ in found[s]], dtype=np.int64)
    if wide:
        return (np.array([k[0] for k in flat], dtype=U64), np.array([k[1] for k in flat], dtype=U64)), homes
    return np.array(flat, dtype=U64), homes


def occupied_slots(cap, homes):
    """The slots linear probing fills for keys with these home slots (the set does not depend on the insertion order)."""
    taken = set()
    for h in homes:
        s = int(h)
        while s in taken:
            s = (s + 1) & (cap - 1)
        taken.add(s)
    return taken


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
class JoinCase(object):
    """One join input: the key columns of both sides ([(data, nulls or None), ...]) under a key shape, plus whatever the layout
    wants to tell its checks (`notes`)."""

    def __init__(self, shape, lhs_keys, rhs_keys, **notes):
        self.shape, self.lhs_keys, self.rhs_keys, self.notes = shape, lhs_keys, rhs_keys, notes
        self.n, self.m = len(lhs_keys[0][0]), len(rhs_keys[0][0])

    def pairs(self, join_type):
        return join_pairs(self.lhs_keys, self.rhs_keys, join_type)

    def matched_and_unmatched(self):
        """(lhs rows with a match, lhs rows without one), from the reference alone."""
        lhs_row, rhs_row = self.pairs(LEFT_OUTER)
        unmatched = int((rhs_row < 0).sum())
        return self.n - unmatched, unmatched


def _columns(shape, lo, hi, nulls):
    """Key columns from packed words; `nulls` (bool per row or None) is spread over the key columns in turn, and the data under
    a NULL is left as it is (it must not matter)."""
    cols = unpack_key(shape, lo, hi)
    if nulls is None:
        return [(c, None) for c in cols]
    nulls = np.asarray(nulls, dtype=bool)
    which = np.arange(len(nulls)) % len(cols)
    return [(c, nulls & (which == j) if len(cols) > 1 else nulls.copy()) for j, c in enumerate(cols)]


def _distinct_words(rng, count, wide):
    """`count` distinct random packed keys, none of them all ones in word 0.  Two-word keys share their first word in pairs and
    their second word among four values: both words decide."""
    if not wide:
        out = np.zeros(0, U64)
        while len(out) < count:
            out = np.unique(np.concatenate([out, rng.integers(0, 1 << 64, count + 8, dtype=U64)]))
            out = out[out != ALL_ONES]
        return rng.permutation(out)[:count], None
    first, _ = _distinct_words(rng, (count + 3) // 4, False)
    seconds = np.array([0, 1, 0xFFFFFFFFFFFFFFFF, 1 << 32], dtype=U64)
    g = np.arange(count)
    return first[g // 4], seconds[g % 4]


def _miss_words(rng, count, lo, hi):
    """`count` packed keys that are on no rhs row: fresh random words, and -- two-word keys -- rhs first words under a second word no
    rhs key has."""
    wide = hi is not None
    out_lo = rng.integers(0, 1 << 64, count, dtype=U64)
    taken = np.isin(out_lo, lo) | (out_lo == ALL_ONES)
    while taken.any():                                                  # (one chance in 2^40: drawn again)
        out_lo[taken] = rng.integers(0, 1 << 64, int(taken.sum()), dtype=U64)
        taken = np.isin(out_lo, lo) | (out_lo == ALL_ONES)
    if not wide:
        return out_lo, None
    out_hi = rng.integers(0, 4, count).astype(U64)
    if len(lo):
        half = np.arange(count) % 2 == 0
        out_lo[half] = lo[rng.integers(0, len(lo), int(half.sum()))]     # a first word that IS there ...
        out_hi[half] = U64(77)                                           # ... under a second word that is not
    return out_lo, out_hi


def _take(words, rows):
    lo, hi = words
    return lo[rows], (None if hi is None else hi[rows])


def _concat(*words):
    lo = np.concatenate([w[0] for w in words])
    hi = None if words[0][1] is None else np.concatenate([w[1] for w in words])
    return lo, hi


N_LHS = 20000
INDEX_SIZES = (1, 8, 9, 4096, 4097, 16384, 16385, 32768, 32769)


def rhs_null_rows(m, unique):
    """NULL-key rows of the index layouts.  UNIQUE at a power of two: none, so that the load is exactly one half."""
    if m == 1 or (unique and m & (m - 1) == 0):
        return 0
    return max(1, m // 64)


def index_case(m, shape, unique, n=N_LHS):
    """a. An rhs table of `m` rows in random row order: distinct keys (UNIQUE) or keys on 1..4 rows each, the all-ones key among them
    (m > 1), NULL-key rows; `n` lhs rows, half of them drawn from the rhs keys, half on no rhs row, 5 % NULL, row 7 the all-ones key."""
    wide = is_wide(shape)
    rng = np.random.default_rng(1000 * m + 10 * len(shape) + unique)
    n_null = rhs_null_rows(m, unique)
    live = m - n_null
    if unique:
        reps = np.ones(live, dtype=np.int64)
    else:
        reps = rng.integers(1, 5, live)
        reps = reps[:int(np.searchsorted(np.cumsum(reps), live, side="left")) + 1]
        reps[-1] -= reps.sum() - live
        assert reps.sum() == live and reps.min() >= 1
    lo, hi = _distinct_words(rng, len(reps), wide)
    if m > 1:
        lo[0] = ALL_ONES                                                # one word: the reserved key; two words: (all ones, ...), an ordinary key
    of_row = rng.permutation(np.concatenate([np.repeat(np.arange(len(reps)), reps), np.full(n_null, -1)]))   # rhs row -> key, -1 = NULL
    rnull = of_row < 0
    r_lo, r_hi = _take((lo, hi), np.maximum(of_row, 0))
    r_lo[rnull] = lo[0]                                                  # under a NULL: a key that is there (it must not be found through it)
    hit = np.arange(n) % 2 == 0
    pick = rng.integers(0, len(reps), n)
    miss = _miss_words(rng, n, lo, hi)
    l_lo = np.where(hit, lo[pick], miss[0])
    l_hi = None if not wide else np.where(hit, hi[pick], miss[1])
    if m > 1 and n > 7:
        l_lo[7] = lo[0]
        if wide:
            l_hi[7] = hi[0]
    lnull = rng.random(n) < 0.05
    lnull[:8] = False
    return JoinCase(shape, _columns(shape, l_lo, l_hi, lnull), _columns(shape, r_lo, r_hi, rnull if n_null else None),
                    distinct=len(reps), max_run=int(reps.max()), load=len(reps) / float(capacity(m)))


# b. the reserved key
NEAR_MISSES = {   # packed one-word keys next to all ones: all ones minus one; (-1, -2) of a two-column shape = the high field minus one
    "i64": (0xFFFFFFFFFFFFFFFE,), "u64": (0xFFFFFFFFFFFFFFFE,),
    "i32i32": (0xFFFFFFFFFFFFFFFE, 0xFFFFFFFEFFFFFFFF), "u32i32": (0xFFFFFFFFFFFFFFFE, 0xFFFFFFFEFFFFFFFF),
}


def reserved_case(shape, rhs_has, lhs_has, run=1, m=300, rows=None, near_on_rhs=True):
    """An rhs table of `m` rows where the all-ones key is on `run` rows (rhs_has; at `rows` if given, else spread evenly) and every
    near miss on one row each (near_on_rhs); other keys distinct.  The lhs (2000 rows) probes the all-ones key (lhs_has), every near
    miss, rhs keys, misses and NULLs."""
    rng = np.random.default_rng(7 * m + run + 2 * rhs_has + lhs_has + len(shape))
    near = np.array(NEAR_MISSES[shape], dtype=U64)
    lo, _ = _distinct_words(rng, m, False)
    lo = lo[~np.isin(lo, near)][:m]
    assert len(lo) == m
    if rhs_has:
        where = np.asarray(rows) if rows is not None else np.linspace(0, m - 1, run).astype(np.int64) if run > 1 else np.array([m // 2])
        assert len(where) == run and len(np.unique(where)) == run
        lo[where] = ALL_ONES
    if near_on_rhs:
        lo[np.flatnonzero(lo != ALL_ONES)[1:1 + len(near)]] = near
    rnull = np.zeros(m, bool)
    if m >= 16:
        rnull[np.flatnonzero(lo != ALL_ONES)[5::37]] = True
    n = 2000
    l_lo = np.where(np.arange(n) % 2 == 0, lo[rng.integers(0, m, n)], _miss_words(rng, n, np.concatenate([lo, near]), None)[0])
    l_lo[l_lo == ALL_ONES] = lo[np.flatnonzero(lo != ALL_ONES)[0]]       # the reserved key is probed only where the case says so
    l_lo[3:3 + 3 * len(near):3] = near
    if lhs_has:
        l_lo[[0, 1, 700, n - 1]] = ALL_ONES
    lnull = rng.random(n) < 0.05
    lnull[:16] = False
    lnull[[700, n - 1]] = False
    return JoinCase(shape, _columns(shape, l_lo, None, lnull), _columns(shape, lo, None, rnull), run=run if rhs_has else 0)


def far_duplicate_case(shape, reserved, m=16385):
    """A key on rhs rows 0 and m - 1 and on no other: the all-ones key (reserved, one-word shapes) or an ordinary one."""
    wide = is_wide(shape)
    rng = np.random.default_rng(m + reserved + len(shape))
    lo, hi = _distinct_words(rng, m, wide)
    lo[0] = ALL_ONES if reserved else lo[0]
    lo[m - 1] = lo[0]
    if wide:
        hi[m - 1] = hi[0]
    l_lo, l_hi = _take((lo, hi), rng.integers(0, m, 1000))
    return JoinCase(shape, _columns(shape, l_lo, l_hi, None), _columns(shape, lo, hi, None))


# c. probe chains
CHAIN_LENGTHS = (2, 64, 257)


def chain_case(length, shape, unique):
    """rhs keys that all home on the last three slots of the table, so that the chain of `length` distinct keys wraps past the table's end
    (2: both on the last slot); NOT_UNIQUE: every key on 1..3 rows.  NULL-key rows pad the table (m = 8, 70 and 300 for UNIQUE).
    The lhs probes every member, absent keys homing at the chain's head -- they walk the whole chain across the wrap to the first free
    slot --, absent keys homing elsewhere and NULLs.  notes: cap, head, homes (per distinct key), keys (packed), absent (packed, at head)."""
    wide = is_wide(shape)
    rng = np.random.default_rng(31 * length + len(shape) + unique)
    reps = np.ones(length, dtype=np.int64) if unique else rng.integers(1, 4, length)
    reps[0] = 1 if unique else 3
    m = int(reps.sum()) + {2: 6, 64: 6, 257: 43}[length]
    cap = capacity(m)
    slots = [cap - 1] if length == 2 else [cap - 3, cap - 2, cap - 1]
    per_slot = -(-length // len(slots))
    keys, homes = keys_homing_at(cap, slots, per_slot + 8, rng, wide)    # 8 more per slot: the absent ones
    keys = keys if wide else (keys, None)
    by_slot = np.arange(len(homes)).reshape(len(slots), per_slot + 8)
    members = by_slot[:, :per_slot].T.reshape(-1)[:length]              # round-robin over the slots: each of them is some key's home
    absent = by_slot[0, per_slot:]                                      # homing at the head, on no rhs row
    of_row = rng.permutation(np.concatenate([np.repeat(members, reps), np.full(m - int(reps.sum()), -1)]))
    rnull = of_row < 0
    r_lo, r_hi = _take(keys, np.where(rnull, members[0], of_row))
    elsewhere = _miss_words(rng, 200, keys[0], keys[1])
    probes = _concat(_take(keys, members), _take(keys, absent), elsewhere, _take(keys, members[::-1]))
    lnull = np.zeros(len(probes[0]), bool)
    lnull[length + 8 + 3::11] = True
    return JoinCase(shape, _columns(shape, probes[0], probes[1], lnull), _columns(shape, r_lo, r_hi, rnull),
                    cap=cap, head=slots[0], homes=homes[members], keys=_take(keys, members), absent=_take(keys, absent), length=length)


# d. expansion
EXPAND_N = (1, 8192, 8193, 65536, 65537, 73729)
BIG_RUN = 20000
_FAN_KEYS = {1: 101, 2: 102, 3: 103, 4: 104, BIG_RUN: 105}              # fan-out -> the (INT64) key with that many rhs rows


def expand_rhs(big):
    """The rhs of the expansion cases (INT64 key): key 100 + f on f rows for f = 1..4 (and 105 on 20 000 rows: big), rows interleaved."""
    keys = np.concatenate([np.full(f, k, dtype=np.int64) for f, k in _FAN_KEYS.items() if big or f != BIG_RUN] + [np.array([7, 8, 9], dtype=np.int64)])
    keys = np.random.default_rng(len(keys)).permutation(keys)
    return [(keys, None)]


def expand_case(fan, big=False):
    """lhs row i matches fan[i] rhs rows (0: none; 1..4 or 20 000)."""
    fan = np.asarray(fan, dtype=np.int64)
    key = np.full(len(fan), -5, dtype=np.int64)                          # on no rhs row
    for f, k in _FAN_KEYS.items():
        key[fan == f] = k
    assert np.isin(fan, [0] + list(_FAN_KEYS)).all()
    return JoinCase("i64", [(key, None)], expand_rhs(big), fan=fan)


def expand_fan(n_stage, join_type, fanout, seed=0):
    """The fan-outs of an lhs of which `n_stage` rows reach the expand stage: INNER counts matched rows only (unmatched ones are
    interleaved and dropped ahead of it), LEFT_OUTER all rows -- unmatched at both ends and, from 65536 rows on, in a stretch of
    9000.  fanout: "ones" or "mixed" (1..4)."""
    rng = np.random.default_rng(n_stage + seed)
    draw = (lambda k: np.ones(k, dtype=np.int64)) if fanout == "ones" else (lambda k: rng.integers(1, 5, k))
    if join_type == INNER:
        fan = np.zeros(n_stage + n_stage // 4 + 2, dtype=np.int64)
        matched = np.sort(rng.permutation(len(fan) - 2)[:n_stage] + 1) if n_stage > 1 else np.array([1])    # rows 0 and the last: unmatched
        fan[matched] = draw(n_stage)
        return fan
    fan = draw(n_stage)
    if n_stage > 1:
        fan[[0, n_stage - 1]] = 0
        fan[rng.integers(0, n_stage, n_stage // 10)] = 0
    if n_stage >= 65536:
        fan[20000:29000] = 0
    return fan


def fan_with_output(total, join_type):
    """Mixed fan-outs (and unmatched rows) whose join has exactly `total` result rows."""
    rng = np.random.default_rng(total)
    fan = rng.integers(0, 5, total)
    rows = np.where(fan == 0, 1 if join_type == LEFT_OUTER else 0, fan)
    keep = int(np.searchsorted(np.cumsum(rows), total - 4, side="right"))
    fan, short = fan[:keep], total - int(rows[:keep].sum())
    assert 4 <= short < 8
    return np.concatenate([fan, [short - 4, 4] if short > 4 else [short]])


def big_run_fan(where, n=3000):
    """`n` mixed lhs rows with one row (two adjacent ones: where = "adjacent") that matches 20 000 rhs rows: "first", "last"."""
    fan = np.random.default_rng(len(where)).integers(0, 5, n)
    at = {"first": [0], "last": [n - 1], "adjacent": [n // 2, n // 2 + 1]}[where]
    fan[at] = BIG_RUN
    return fan


# e. chunked forms
CHUNKED_N = (0, 1, 1000, 1001, 70001)


def chunked_case(n, unique, barren=False):
    """An rhs of 300 rows (INT64 key; NOT_UNIQUE: on 1..4 rows each) and `n` lhs rows: 60 % on rhs keys.  barren: rows [4096, 20480) and
    [50000, 56000) match nothing -- whole chunks of 1000 and of 4096 rows without a match."""
    rng = np.random.default_rng(n + 3 * unique)
    m = 300
    keys = rng.permutation(2 * m)[:m].astype(np.int64) - 5 if unique else rng.integers(-1, 100, m)      # -1: the reserved key, too
    rnull = np.arange(m) % 29 == 3
    lkey = np.where(rng.random(n) < 0.6, keys[rng.integers(0, m, n)], rng.integers(1000, 2000, n))
    if barren:
        lkey[4096:20480] = 5000
        lkey[50000:56000] = 5001
    return JoinCase("i64", [(lkey.astype(np.int64), rng.random(n) < 0.05)], [(keys, rnull)])


# ---- views and plans (host only: nothing here touches a device) --------------------------------------------------------------------------
RHS_NAMES = ["ri", "rw", "rs"]


def payload(case):
    """lhs: lid INT64 (the row id), a INT64 in [0, 1000); rhs: ri INT64 (the row id), rw DOUBLE NULLABLE (20 % NULL), rs STRING."""
    rng = np.random.default_rng(case.n + case.m)
    lhs = [(np.arange(case.n, dtype=np.int64), None), (rng.integers(0, 1000, case.n), None)]
    strings = np.empty(case.m, dtype=object)
    strings[:] = [b"s%d" % (i % 41) for i in range(case.m)]
    rhs = [(np.arange(case.m, dtype=np.int64), None), (rng.integers(-100, 100, case.m) * 0.25, rng.random(case.m) < 0.2), (strings, None)]
    return lhs, rhs


def views(case):
    """(lhs View, rhs View): the key columns lk0.. / rk0.. (NULLABLE where the case has a mask), then the payload."""
    import supersonic_amd as ss
    types = {"INT64": ss.INT64, "UINT64": ss.UINT64, "INT32": ss.INT32, "UINT32": ss.UINT32}
    lhs, rhs = payload(case)

    def view(prefix, keys, names_types, cols):
        attrs = [ss.Attribute("%s%d" % (prefix, j), types[t], ss.NULLABLE if z is not None else ss.NOT_NULLABLE)
                 for j, (t, (_d, z)) in enumerate(zip(KEY_SHAPES[case.shape], keys))]
        attrs += [ss.Attribute(name, t, ss.NULLABLE if z is not None else ss.NOT_NULLABLE) for (name, t), (_d, z) in zip(names_types, cols)]
        return ss.View(ss.TupleSchema(attrs), [ss.Column(d, z) for d, z in list(keys) + list(cols)], len(cols[0][0]))
    return (view("lk", case.lhs_keys, [("lid", ss.INT64), ("a", ss.INT64)], lhs),
            view("rk", case.rhs_keys, [("ri", ss.INT64), ("rw", ss.DOUBLE), ("rs", ss.STRING)], rhs))


def join_op(case, join_type, unique, lview, rview, lhs_names=("lid",)):
    """HashJoin over the case's views keeping `lhs_names` and ri, rw, rs."""
    import supersonic_amd as ss
    k = len(KEY_SHAPES[case.shape])
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(list(lhs_names))).add(1, ss.ProjectNamedAttributes(RHS_NAMES))
    return ss.HashJoin(ss.INNER if join_type == INNER else ss.LEFT_OUTER, ss.ProjectNamedAttributes(["lk%d" % j for j in range(k)]),
                       ss.ProjectNamedAttributes(["rk%d" % j for j in range(k)]), proj, ss.UNIQUE if unique else ss.NOT_UNIQUE,
                       ss.ScanView(lview), ss.ScanView(rview))


def expected(case, join_type, lhs_names=("lid",)):
    """(pairs, result columns) of join_op(case, join_type, ...) by the reference."""
    lhs, rhs = payload(case)
    pairs = case.pairs(join_type)
    return pairs, gather_join(pairs, [lhs[("lid", "a").index(name)] for name in lhs_names], rhs, join_type)

"""A plain reference for Sort and a generator of wide keys with designed tie runs (tests/test_sort_reference_cpu.py checks
both without a GPU; tests/test_sort_forms_gpu.py compares every execution form of run_sort with them).

`stable_order` knows nothing of radix digits: dense ranks per key column, NULLs ranked below every value, DESCENDING as
negated ranks, `np.lexsort` with the row id as the last tie-break.  The device sort is stable (its passes and run_sort rely
on it), so this is the expected row order bit for bit, duplicates included.

`tie_layout` plants runs of rows that agree in the high `hi_bits` bits of their radix image (the word whose unsigned order is
the sort order: see `radix_image`) at chosen OUTPUT positions -- the rows the tie fix-up kernels permute -- and nowhere else.
`radix_image` is used only to build and to inspect such keys, never by `stable_order`."""
import numpy as np

U64 = np.uint64
TOP = U64(1) << U64(63)
CONTENTS = ("random", "asc", "desc", "straddle", "dups", "copies", "rotated")
NP_OF = {"INT64": np.int64, "UINT64": np.uint64, "DOUBLE": np.float64}


def stable_order(columns, keys):
    """Row order of Sort over `columns` ([(data, nulls_or_None), ...]) by `keys` ([(col, descending), ...], major key first):
    NULLs first for ASCENDING and last for DESCENDING (oracle/ss_oracle.c: sort_cmp), ties in input order."""
    n = len(columns[0][0]) if columns else 0
    ranks = []
    for col, descending in keys:
        data, nulls = columns[col]
        _values, inverse = np.unique(np.asarray(data), return_inverse=True)     # (-0.0 == 0.0: one rank for both)
        rank = inverse.reshape(-1).astype(np.int64)
        if nulls is not None:
            rank[np.asarray(nulls, dtype=bool)] = -1
        ranks.append(-rank if descending else rank)
    # np.lexsort: the LAST array is the primary key
    return np.lexsort([np.arange(n, dtype=np.int64)] + ranks[::-1])


def gather(columns, order):
    """The rows of `columns` in `order`."""
    return [(np.asarray(d)[order], None if z is None else np.asarray(z, dtype=bool)[order]) for d, z in columns]


# ---- wide keys with designed tie runs ---------------------------------------------------------------------------------
def radix_image(key, ktype, descending):
    """The 64-bit word of every key whose UNSIGNED order is the sort order (ascending = output order)."""
    bits = np.ascontiguousarray(key, dtype=NP_OF[ktype]).view(U64)
    if ktype == "INT64":
        img = bits ^ TOP
    elif ktype == "DOUBLE":
        img = np.where(bits & TOP != 0, ~bits, bits | TOP)
    else:
        img = bits.copy()
    return ~img if descending else img


def _from_radix_image(img, ktype, descending):
    img = ~img if descending else img
    if ktype == "INT64":
        bits = img ^ TOP
    elif ktype == "DOUBLE":
        bits = np.where(img & TOP != 0, img ^ TOP, ~img)
    else:
        bits = img
    return np.ascontiguousarray(bits).view(NP_OF[ktype]).copy()


def _distinct(rng, count, bits):
    """`count` distinct random integers below 2**bits, in random order."""
    out = np.zeros(0, U64)
    while len(out) < count:
        out = np.unique(np.concatenate([out, rng.integers(0, 1 << bits, 2 * count + 8, dtype=U64)]))
    return rng.permutation(out)[:count]


def _run_lows(rng, length, content, low_bits):
    """The low parts of one run in INPUT order, as parts of the radix image (so "asc" is a run already in place and "desc" one
    that has to be reversed, whatever the key's type and direction)."""
    top = U64(rng.integers(0, 1 << (low_bits - 32))) << U64(32) if low_bits > 32 else U64(0)     # bits above the low word ("dups", "straddle": one value per run)
    if content == "dups":                       # exact duplicates of the whole key, interleaved: [b, a, b, a, ...] with a < b
        a, b = np.sort(_distinct(rng, 2, 32))
        low = np.where(np.arange(length) % 2 == 0, b, a).astype(U64)
        if length == 2:
            low[:] = a
    elif content == "straddle":                 # alternately above and below 2**31 (= 2**63 >> 32): a signed compare misorders them
        small = _distinct(rng, length, 20)
        low = np.where(np.arange(length) % 2 == 0, (U64(1) << U64(31)) + small, (U64(1) << U64(31)) - U64(1) - small).astype(U64)
    else:
        # the whole low part varies inside the run: with more than 32 low bits the bits above the low word decide too
        low, top = _distinct(rng, length, low_bits), U64(0)
        if content == "asc":
            low = np.sort(low)
        elif content == "copies":               # one key, `length` times: in order as it stands
            low[:] = low[0]
        elif content == "rotated":              # ascending but for the LAST row, which belongs first
            low = np.roll(np.sort(low), -1)
        elif content == "desc":
            low = np.sort(low)[::-1].copy()
        elif content != "random":
            raise ValueError(content)
    return top | low


def tie_layout(n, runs, hi_bits, ktype, descending, seed):
    """A shuffled 8-byte key column of `n` rows (dtype of `ktype`: "INT64", "UINT64" or "DOUBLE").  In the expected output
    order of Sort(key, DESCENDING if `descending`), the rows at positions [start, start + length) of every (start, length,
    content) in `runs` agree in the high `hi_bits` bits of their radix image; every other row has a high part of its own.
    High parts are spread over the whole range of the type (INT64: both signs; DOUBLE: both signs, every exponent but 0x7FF,
    neither zero), so every high digit varies; low parts are random outside the runs and as `content` says inside them."""
    rng = np.random.default_rng(seed)
    low_bits = 64 - hi_bits
    assert 12 <= hi_bits <= 32
    new_part = np.ones(n, dtype=np.int64)           # 1 where an output position starts a new high part
    covered = np.zeros(n, dtype=bool)
    for start, length, content in runs:
        assert 0 <= start and start + length <= n and length >= 2 and content in CONTENTS, (start, length, content)
        assert not covered[start:start + length].any(), "runs overlap at %d" % start
        covered[start:start + length] = True
        new_part[start + 1:start + length] = 0
    part_of = np.cumsum(new_part) - 1               # output position -> index into the sorted distinct high parts
    n_parts = int(part_of[-1]) + 1 if n else 0
    # the distinct high parts, in output order = ascending in the radix image
    parts = np.zeros(0, U64)
    while len(parts) < n_parts:
        cand = rng.integers(0, 1 << hi_bits, 2 * n_parts + 64, dtype=U64)
        if ktype == "DOUBLE":
            # built in value order: the image's top 12 bits are the sign and the exponent (complemented for negative values) --
            # 0xFFF and 0x000 are the exponent 0x7FF (infinities, NaN); the two parts next to the middle hold +0.0 and -0.0
            top12 = cand >> U64(hi_bits - 12)
            mid = U64(1) << U64(hi_bits - 1)
            cand = cand[(top12 != U64(0)) & (top12 != U64(0xFFF)) & (cand != mid) & (cand != mid - U64(1))]
        parts = np.unique(np.concatenate([parts, cand]))
    parts = np.sort(rng.permutation(parts)[:n_parts])
    image = (parts[part_of] << U64(low_bits)) | rng.integers(0, 1 << low_bits, n, dtype=U64)      # by output position
    where = rng.permutation(n)                      # output position -> input row (of the rows outside the runs; runs: see below)
    key_image = np.zeros(n, dtype=U64)
    key_image[where] = image
    for start, length, content in runs:
        rows = np.sort(where[start:start + length])                 # the run's rows, in input order
        key_image[rows] = (parts[part_of[start]] << U64(low_bits)) | _run_lows(rng, length, content, low_bits)
    return _from_radix_image(key_image, ktype, descending)


# ---- the layouts the GPU tests use (checked on their own in tests/test_sort_reference_cpu.py) ----------------------------
N_TIES = 70001
# Workgroup edges: 2048 rows (ssgpu_sort_fix_ties_compact_kernel), 1024 rows (ssgpu_sort_fix_ties_kernel: 256 threads x 4 rows);
# a thread of the latter looks at 4 rows.  (start, length, content), by output position:
GEOMETRY_RUNS = {
    "A": [(0, 2, "random"),                       # starts at output row 0
          (1023, 2, "desc"),                      # one row before an edge of 1024
          (2047, 3, "random"),                    # one row before an edge of 2048
          (4095, 5, "straddle"),                  # one row before an edge of both
          (6140, 4, "random"),                    # ends exactly at 6143
          (8180, 40, "random"),                   # a long run across 8192
          (10003, 2, "random"),                   # start = 3 (mod 4), the last row of a thread
          (10007, 6, "desc"),                     # start = 3 (mod 4), across two threads
          (12000, 3, "asc"), (12003, 4, "dups"),  # two adjacent runs
          (N_TIES - 5, 5, "dups")],               # ends at row n - 1
    "B": [(0, 5, "straddle"),
          (1024, 2, "desc"),                      # starts exactly at an edge of 1024
          (2046, 2, "dups"), (2048, 3, "random"),  # two rows before an edge of 2048, and adjacent to it a run that starts exactly there
          (4096, 4, "asc"),                       # starts exactly at an edge of both
          (6142, 2, "random"),                    # ends exactly at 6143
          (8190, 40, "straddle"),
          (10003, 6, "random"), (10011, 2, "desc"),
          (N_TIES - 2, 2, "desc")],
}
BOUNDARY_LENGTHS = (2, 3, 8, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 1000)
BOUNDARY_EDGE = 17 * 2048                           # the planted run straddles this multiple of 2048, in mid-array


def boundary_runs(length):
    return [(BOUNDARY_EDGE - length // 2, length, "random")]


# runs beyond the length the tie kernels sort themselves; ssgpu_sort_fix_ties_kernel leaves one alone when it is in order already
LONG_RUNS = ((200, "asc"), (200, "rotated"), (722, "copies"), (1024, "asc"), (1025, "asc"), (1025, "copies"))


def long_run_key(length, content):
    return tie_layout(N_TIES, [(BOUNDARY_EDGE - length // 2, length, content)], 32, "INT64", False, seed=900 + length)


def geometry_key(which, hi_bits, ktype, descending):
    return tie_layout(N_TIES, GEOMETRY_RUNS[which], hi_bits, ktype, descending, seed=101 + hi_bits + (which == "B"))


def boundary_key(length, ktype, descending):
    return tie_layout(N_TIES, boundary_runs(length), 32, ktype, descending, seed=500 + length)


def layouts_in_use():
    """(name, runs, hi_bits, ktype, descending, key) of every tie_layout call of tests/test_sort_forms_gpu.py."""
    out = []
    for which in ("A", "B"):
        for ktype in ("INT64", "UINT64", "DOUBLE"):
            for descending in (False, True):
                out.append(("geometry %s %s %s" % (which, ktype, "desc" if descending else "asc"), GEOMETRY_RUNS[which], 32, ktype, descending,
                            geometry_key(which, 32, ktype, descending)))
        for ktype, descending in (("INT64", False), ("DOUBLE", True)):
            out.append(("geometry %s, 24 high bits, %s" % (which, ktype), GEOMETRY_RUNS[which], 24, ktype, descending, geometry_key(which, 24, ktype, descending)))
    for length in BOUNDARY_LENGTHS:
        for ktype, descending in (("INT64", False), ("DOUBLE", True)):
            out.append(("boundary L=%d %s" % (length, ktype), boundary_runs(length), 32, ktype, descending, boundary_key(length, ktype, descending)))
    for length, content in LONG_RUNS:
        out.append(("long run L=%d %s" % (length, content), [(BOUNDARY_EDGE - length // 2, length, content)], 32, "INT64", False, long_run_key(length, content)))
    return out

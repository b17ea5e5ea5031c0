"""What the STRING_REPLACE tests share (no test lives here): the Python restatement of the reference's StringReplace, the literal
transcription of its loop, the pool of values the kernels are checked on and the needle -> substitute pairs."""
import numpy as np

LONG = 128                       # string_map_kernels.hip STRMAP_LONG: up to this length one lane maps a value, beyond it a whole wave
STRING_REPLACE = 480


def replace(h, n, s):
    """string_evaluators.h:76-90 -> util.cc:201-222 with replace_all: bytes.replace is leftmost and non-overlapping for a non-empty needle."""
    return h if n == b"" else h.replace(n, s)


def reference_loop(s, oldsub, newsub):
    """utils/strings/util.cc:201-222, statement by statement (replace_all = true)."""
    res = b""
    if len(oldsub) == 0:
        res += s
        return res
    start_pos = 0
    while True:
        pos = s.find(oldsub, start_pos)
        if pos == -1:
            break
        res += s[start_pos:pos]
        res += newsub
        start_pos = pos + len(oldsub)
    res += s[start_pos:]
    return res


def _rnd(rng, n, alphabet):
    return bytes(alphabet[rng.integers(0, len(alphabet), n)])


ALPHABET = np.frombuffer(b"ab\x00\xe4 ", np.uint8)
_rng0 = np.random.default_rng(480)
V1300 = _rnd(_rng0, 1300, ALPHABET)
V2100 = _rnd(_rng0, 2100, ALPHABET)
NEEDLE17 = b"ab\x00\xe4 b\xe4a \x00\x00ba\xe4 ab"
NEEDLE130 = V1300[500:630]
NEEDLE_HUGE = b"ab" * 1500                                   # longer than every value of the pool
SUB200 = b"\xe4b" * 100
RUN100 = b"a" * 100
LAST_A = b"a" + b"\xe4" * 45 + b"a"                          # the largest value that starts with 'a'; b"b" follows it in sorted order
assert len(NEEDLE17) == 17 and len(NEEDLE130) == 130


def pool():
    """The interesting values first (a dictionary of the first n keeps them), then random ones over `a b 0x00 0xe4 space`."""
    rng = np.random.default_rng(4800)
    vals = [b"", b"a", b"b", b"ababababa", V1300, b"a" * 129, LAST_A, b"ab" * 600, b"aba" * 50, V2100,
            _rnd(rng, 127, ALPHABET), _rnd(rng, 128, ALPHABET), _rnd(rng, 129, ALPHABET), b"a" * 1030, b"a" * 250 + b"b", b"b" + b"a" * 100, b" " + b"a" * 199 + b" " + b"a" * 100,
            NEEDLE17, b"b" + NEEDLE17 + b" a", NEEDLE17 * 3, NEEDLE17[:16] + NEEDLE17, (b" " * 50 + NEEDLE17) * 9, NEEDLE17[1:] + b"a" * 130,
            b"\x00", b"\x00\x00a\x00", b"\xe4\x00" * 70, b"aab", b"baa", b"aaab aab", b"abab", b"ba", b"bab", b" aba", b"abaaba", b"ababa" * 30]
    vals += [b"a" * k for k in range(2, 21)]
    # the ONLY match of "aba" at every offset of a 24-byte stretch -- wherever the value starts in the heap, one of them straddles an
    # aligned 8-byte and one an aligned 16-byte word --, at the value's very end, and around the wave form's boundaries: the 64 starts
    # of a sub-step and the 1 KiB of a step (the step's base is the value's start rounded down to 16)
    vals += [b" " * k + b"aba" + b" " * (23 - k) for k in range(24)]
    vals += [b" " * 5 + b"aba", b" " * 300 + b"aba", b"\x00" * 125 + b"aba", b" " * 126 + b"aba"]
    vals += [b" " * k + b"aba" + b"\x00" * (200 - k) for k in range(44, 70)]
    vals += [b"\xe4" * k + b"aba" + b" " * (1100 - k) for k in range(1003, 1029)]
    seen = set()
    out = []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    while len(out) < len(vals) + 200:
        v = _rnd(rng, int(rng.integers(0, 41)), ALPHABET)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


PAIRS = [(b"a", b"b"), (b"a", b""), (b"a", b"aa"), (b"aa", b"b"), (b"aa", b"a"), (b"aba", b"X"), (b"ab", b"ba"), (b"", b"zzz"), (b"\x00", b"\xe4\xe4"),
         (NEEDLE17, b""), (NEEDLE130, b"Q"), (NEEDLE_HUGE, b"never"), (b"ababababa", b""), (b"a", SUB200), (RUN100, b"")]
PAIR_IDS = ["a-b", "a-empty", "a-aa", "aa-b", "aa-a", "aba-X", "ab-ba", "empty-zzz", "nul-e4e4", "17-empty", "130-Q", "huge", "whole-value", "a-200", "run100-empty"]

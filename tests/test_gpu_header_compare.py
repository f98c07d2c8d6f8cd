"""The exact 256-bit compare of the three block-header kernels, word by word,
against hashlib and never against the library itself.

For a hash h with words h[0..7], most significant first, three targets per
word k (the "ladder"):

  up(k)    words above k as h's, word k = h[k] + 1, words below k all zero:
           T > h, every lower word of h is above T's, only word k makes a hit;
  down(k)  word k = h[k] - 1, words below k all 0xFFFFFFFF: T < h, every lower
           word of h is below T's, only word k makes a miss;
  flip(k)  word k = h[k] ^ 0x80000000, words below all 0xFFFFFFFF when bit 31
           of h[k] is set (T < h) and all zero otherwise (T > h): a signed
           compare of word k inverts the result.

A compare that skipped a word, visited the words in the wrong order or took a
word as signed fails here for that word; the host recheck can only turn a
false hit into BM_EINTERNAL, it cannot see a missed one.  Every rung asserts
its own preconditions (no word of h is 0 or 0xFFFFFFFF, and the target lies
on the intended side of h as an integer); no word is left out.

The windows are tests/test_gpu_header.py's and tests/test_gpu_header_versions.py's
LOW (2^16 nonces, under VERS4 the 2^18 pairs those files already hold),
computed once and shared."""
import pytest

from test_gpu_header import GENESIS, H, expect as expect_first, window
from test_gpu_header_hits import check, expect as expect_hits
from test_gpu_header_versions import H as HV, VERS4, expect as expect_versions, smallest

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
LOW = (0, 65535)
NMIN = 8603  # the nonce of LOW's smallest hash under the genesis header
NONCES = (4200, 8603, U32)
VERSION_NONCES = NONCES + (65535,)


def words(h):
    return [(h >> (32 * (7 - k))) & U32 for k in range(8)]


def join(ws):
    assert len(ws) == 8 and all(0 <= w <= U32 for w in ws)
    t = 0
    for w in ws:
        t = (t << 32) | w
    return t


def up(h, k):
    ws = words(h)
    assert all(w not in (0, U32) for w in ws)
    t = join(ws[:k] + [ws[k] + 1] + [0] * (7 - k))
    assert t > h and all(a > b for a, b in zip(ws[k + 1:], words(t)[k + 1:]))
    return t


def down(h, k):
    ws = words(h)
    assert all(w not in (0, U32) for w in ws)
    t = join(ws[:k] + [ws[k] - 1] + [U32] * (7 - k))
    assert t < h and all(a < b for a, b in zip(ws[k + 1:], words(t)[k + 1:]))
    return t


def flip(h, k):
    ws = words(h)
    assert all(w not in (0, U32) for w in ws)
    neg = ws[k] >> 31
    t = join(ws[:k] + [ws[k] ^ 0x80000000] + [U32 if neg else 0] * (7 - k))
    assert (t < h) if neg else (t > h)
    # as signed 32-bit words the order of word k is the other way round
    signed = lambda w: w - (1 << 32) if w >> 31 else w
    assert (signed(words(t)[k]) > signed(ws[k])) if neg else (signed(words(t)[k]) < signed(ws[k]))
    return t


def ladder(h):
    """[(name, k, T)]: the 24 targets of h."""
    return [(f.__name__, k, f(h, k)) for k in range(8) for f in (up, down, flip)]


def test_ladder_shape():
    """The ladder itself, on a hash whose words are known: 24 targets, on the
    sides the docstring says, differing from h from word k on."""
    h = join([0x00000010, 0x80000001, 0x7FFFFFFE, 5, 0xFFFFFFF0, 0x80000000, 0x7FFFFFFF, 2])
    rungs = ladder(h)
    assert len(rungs) == 24 and len({t for _, _, t in rungs}) == 24
    for name, k, t in rungs:
        assert words(t)[:k] == words(h)[:k] and words(t)[k] != words(h)[k]
        if name == "up":
            assert t > h
        elif name == "down":
            assert t < h
        else:
            assert (t < h) == bool(words(h)[k] >> 31)
    assert up(h, 7) == h + 1 and down(h, 7) == h - 1
    # the sign bits of the words used below are mixed in every position
    hs = [HV(v, n) for n in VERSION_NONCES for v in VERS4]
    for k in range(8):
        assert {words(x)[k] >> 31 for x in hs} == {0, 1}, k


# ---- 1. single-nonce ranges: nothing but the compare decides -------------------

@pytest.mark.parametrize("n", NONCES)
def test_single_nonce_header(gpu_ctx, n):
    h = H(GENESIS, n)
    for name, k, T in ladder(h):
        assert gpu_ctx.search_header(GENESIS, n, n, T) == (T >= h, h, n), (name, k)


@pytest.mark.parametrize("n", NONCES)
def test_single_nonce_hits(gpu_ctx, n):
    h = H(GENESIS, n)
    for name, k, T in ladder(h):
        want = (1, [(h, n)], (h, n)) if T >= h else (0, [], (h, n))
        assert gpu_ctx.search_header_hits(GENESIS, n, n, T) == want, (name, k)
        assert gpu_ctx.search_header_hits(GENESIS, n, n, T, 0)[0] == want[0], (name, k)  # count mode


def _single_versions(versions, n, T):
    """What search_header_versions must return over [n, n], from hashlib."""
    hs = [HV(v, n) for v in versions]
    i = next((i for i, x in enumerate(hs) if x <= T), None)
    if i is not None:
        return (True, hs[i], n, i)
    _, i = min((x >> 192, i) for i, x in enumerate(hs))
    return (False, hs[i], n, i)


def _observable(versions, n):
    """The slots whose own compare shows in the result over [n, n] at targets
    that share their hash's top word: those with no smaller hash at a lower
    index (a lower index that hits wins whatever the slot's compare says)."""
    hs = [HV(v, n) for v in versions]
    return {s for s in range(len(hs)) if all(hs[j] > hs[s] for j in range(s))}


@pytest.mark.parametrize("n", VERSION_NONCES)
@pytest.mark.parametrize("nver", [4, 2, 1])
def test_single_nonce_versions(gpu_ctx, nver, n):
    """The ladder of every slot's own hash, the others' hashes standing where
    they fall.  Over the nonces used, every slot of every kernel (M = 4, 2, 1)
    is observable at least once; slot 3 of M = 4 only at 65535, which is why
    that nonce is here."""
    vs = VERS4[:nver]
    assert set().union(*(_observable(vs, m) for m in VERSION_NONCES)) == set(range(nver))
    assert _observable(VERS4, 65535) >= {3} and all(3 not in _observable(VERS4, m) for m in NONCES)
    for slot in range(nver):
        h = HV(vs[slot], n)
        for name, k, T in ladder(h):
            want = _single_versions(vs, n, T)
            assert want == expect_versions(vs, n, n, T)
            if k >= 1 and slot in _observable(vs, n):  # this slot's compare alone decides the answer
                assert (want[0] and want[3] == slot) == (T >= h)
            assert gpu_ctx.search_header_versions(GENESIS, vs, n, n, T) == want, (slot, name, k)
        assert gpu_ctx.last_stats().launches == 1


# ---- 2. inside a window: the filter, the running minimum, other lanes ----------

def _window_ladder():
    hmin, nmin = min(window(GENESIS, *LOW))
    assert nmin == NMIN and hmin == H(GENESIS, NMIN)
    return hmin, ladder(hmin)


def test_window_header_and_hits(gpu_ctx):
    hmin, rungs = _window_ladder()
    for name, k, T in rungs:
        want = check(gpu_ctx, GENESIS, *LOW, T, single=gpu_ctx)  # the whole list, and search_header beside it
        assert want == expect_hits(GENESIS, *LOW, T) and want[2] == (hmin, NMIN)
        first = expect_first(GENESIS, *LOW, T)
        if k >= 1 and name == "up":  # words 0..k-1 are the minimum's: nothing else is that low
            assert first == (True, hmin, NMIN) and want[:2] == (1, [(hmin, NMIN)]), (name, k)
        if k >= 1 and name == "down":
            assert first == (False, hmin, NMIN) and want[:2] == (0, []), (name, k)
        assert gpu_ctx.search_header(GENESIS, *LOW, T) == first, (name, k)


@pytest.mark.parametrize("of", ["genesis_minimum", "pair_minimum"])
def test_window_versions(gpu_ctx, of):
    """Over VERS4 the expectation covers all 2^18 pairs.  The ladder of the
    genesis header's own minimum (slot 2 at nonce 8603), and the ladder of
    the smallest hash of all pairs, below which nothing is found."""
    if of == "genesis_minimum":
        hmin, rungs = _window_ladder()
        assert HV(VERS4[2], NMIN) == hmin
    else:
        hmin, n0, i0 = smallest(VERS4, *LOW)[0]
        rungs = ladder(hmin)
    for name, k, T in rungs:
        want = expect_versions(VERS4, *LOW, T)
        if of == "pair_minimum" and k >= 1 and name == "up":
            assert want == (True, hmin, n0, i0), k
        if of == "pair_minimum" and k >= 1 and name == "down":
            assert want == (False, hmin, n0, i0), k
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, T) == want, (name, k)

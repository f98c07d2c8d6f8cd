"""The session table's multiword arithmetic on the host (no GPU), without the table:
tests/cpp/sessions_arith.cpp includes bm_sessions_args.hpp -- the header the kernels
and the CPU table compile -- and prints mul_64x64, div_128by64, target_words_fx,
vardiff_evaluated and vardiff_new for the cases on its stdin.  Built on demand with
the host compiler, the flags and include paths of bm_sessions.cpp, and the address and
undefined-behaviour sanitizers.  Every line is compared with Python's big integers
(tests/sessions_ref.py for the rule): about 2000 generated cases of every bit length,
the directed rows of sessions_ref.directed_rows(), and what the C ABI cannot reach --
`accepted` at and above 2^32 - 1 (rule 3's clamp) and div_128by64 with hi = d - 1.
The argument block the retarget kernel is launched with is pinned field by field."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import sessions_ref as sref
from sessions_ref import U32, U64

CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "sessions_arith.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "sessions_arith")
POLICY_FIELDS = ("target_ms", "window_ms", "min_difficulty_fx", "max_difficulty_fx", "burst", "band_permille", "max_up",
                 "max_down")


@pytest.fixture(scope="module")
def arith():
    """lines -> the program's answers, one list of integers per line."""
    deps = [SRC, os.path.join(ROOT, "include", "btcminer.h")] + [os.path.join(CSRC, h) for h in
                                                                 ("bm_sessions_args.hpp", "bm_sha256.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-I",
                               os.path.join(ROOT, "include"), SRC, "-o", EXE])

    def run(lines):
        text = "".join(" ".join([line[0]] + [format(v, "x") for v in line[1:]]) + "\n" for line in lines)
        r = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines) and "error" not in out
        return [[int(f, 16) for f in line.split()] for line in out]

    return run


def bits(rng, lo=1, hi=64):
    return sref.random_bits(rng, lo, hi)


def edgy(rng):
    """A 64-bit value: of a random bit length, or at an edge of a 32-bit half."""
    pick = rng.randrange(8)
    if pick == 0:
        return rng.choice((0, 1, U32 - 1, U32, U32 + 1, 1 << 63, (1 << 63) - 1, U64 - 1, U64, U32 << 32, (U32 << 32) + 1))
    if pick == 1:  # all ones in one half, anything in the other
        return (U32 << 32) | rng.getrandbits(32) if rng.getrandbits(1) else (rng.getrandbits(32) << 32) | U32
    return bits(rng)


def test_argument_block(arith):
    """sizeof(SessionsRetargetArgs) and the offsets of now_ms, target_ms, window_ms, min_fx,
    max_fx, burst, band_permille, max_up, max_down, count, cap, apply, pad."""
    assert arith([("args",)]) == [[72, 0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68]]


def test_mul_64x64(arith):
    rng = random.Random(31)
    cases = [(a, b) for a in (0, 1, U32, U32 + 1, 1 << 63, U64) for b in (0, 1, U32, U32 + 1, 1 << 63, U64)]
    cases += [(edgy(rng), edgy(rng)) for _ in range(600)]
    # the carries of the middle column: all-ones halves on either side
    cases += [((U32 << 32) | rng.getrandbits(32), (rng.getrandbits(32) << 32) | U32) for _ in range(50)]
    got = arith([("mul", a, b) for a, b in cases])
    for (a, b), g in zip(cases, got):
        assert g == [a * b >> 64, a * b & U64], (hex(a), hex(b))


def test_div_128by64(arith):
    """hi < d: random operands of every bit length, a divisor above 2^63 (the carry out
    of the remainder's shift), and hi = d - 1 with lo = 2^64 - 1, the largest dividend."""
    rng = random.Random(32)
    cases = [(d - 1, U64, d) for d in (1, 2, 1 << 63, (1 << 63) + 1, U64)]
    cases += [(d - 1, lo, d) for d in (1, 2, 3, U32, U32 + 1, U32 + 2, 1 << 63, (1 << 63) + 1, U64 - 1, U64)
              for lo in (0, 1, 1 << 63, U64 - 1, U64)]
    for _ in range(600):
        d = max(edgy(rng), 1)
        cases.append((rng.choice((0, d - 1, d // 2, rng.randrange(d))), edgy(rng), d))
    for _ in range(100):
        d = (1 << 63) | rng.getrandbits(63)
        cases.append((rng.randrange(d), rng.getrandbits(64), d))
    got = arith([("div",) + c for c in cases])
    for (hi, lo, d), g in zip(cases, got):
        assert g == list(divmod((hi << 64) | lo, d)), (hex(hi), hex(lo), hex(d))


def test_target_words_fx(arith):
    rng = random.Random(33)
    cases = list(sref.DIFFICULTIES) + [U32 - 1, U32, (1 << 63) + 1, U64 - 1] + [max(edgy(rng), 1) for _ in range(200)]
    got = arith([("tgt", d) for d in cases])
    for d, g in zip(cases, got):
        t = sref.target_fx(d)
        assert g == [t >> 192, t >> 128 & U64, t >> 64 & U64, t & U64], hex(d)


def policy(rng):
    lo, hi = sorted((bits(rng), bits(rng)))
    wide = rng.getrandbits(1)
    return dict(target_ms=rng.choice((1, 1000, U32 - 1, U32, bits(rng, 1, 32))),
                window_ms=rng.choice((0, 0, 1, bits(rng), U64)), min_difficulty_fx=1 if wide else lo,
                max_difficulty_fx=U64 if wide else hi, burst=rng.choice((0, 0, 1, 6, U32, bits(rng, 1, 32))),
                band_permille=rng.choice((0, 1, 100, 999, 1000)), max_up=rng.choice((1, 2, 4, U32, bits(rng, 1, 32))),
                max_down=rng.choice((1, 2, 4, U32, bits(rng, 1, 32))))


def check_rule(arith, cases):
    """cases: [(policy, now_ms, old, since_ms, accepted)] against sessions_ref.vardiff and the rule's trace."""
    got = arith([("var", now) + tuple(p[f] for f in POLICY_FIELDS) + (old, since, accepted)
                 for p, now, old, since, accepted in cases])
    for (p, now, old, since, accepted), (evaluated, new) in zip(cases, got):
        state = (old, since, accepted, 0)
        assert evaluated == sref.vardiff(p, now, state)[0], (p, now, state)
        # vardiff_new is the rule of an evaluated slot, whatever rule 2 says
        assert new == sref.vardiff(dict(p, window_ms=0), now, state)[1], (p, now, state)


def test_vardiff_generated(arith):
    """700 cases: policies, difficulties, clocks and counts of every bit length."""
    rng = random.Random(34)
    cases = []
    for _ in range(700):
        now = edgy(rng)
        since = rng.choice((now, max(now - 1, 0), max(now - rng.randrange(1000, 20000), 0), rng.randrange(now + 1),
                            rng.randrange(1000), min(now + bits(rng, 1, 40), U64), edgy(rng)))
        accepted = rng.choice((0, 1, 2, rng.randrange(7), rng.randrange(7), bits(rng, 1, 32), bits(rng)))
        cases.append((policy(rng), now, max(edgy(rng), 1), since, accepted))
    check_rule(arith, cases)
    assert sum(1 for p, now, old, since, a in cases if old >> 32 and min(a, U32) * p["target_ms"] >> 32) >= 100


def test_vardiff_directed(arith):
    """The directed rows of the table's scenario, at a small clock and at one above 2^63."""
    cases = [(sref.DIRECTED[k], now, old, now - elapsed, accepted) for k in range(len(sref.DIRECTED))
             for old, accepted, elapsed in sref.directed_rows(k) for now in (U32, U64)]
    for p, now, old, accepted, since in ((sref.POLICY, sref.NOW, e[0], e[1], e[2]) for e in sref.EDGES):
        cases.append((p, now, old, since, accepted))
    assert len(cases) > 80
    check_rule(arith, cases)


def test_accepted_is_cut_at_32_bits(arith):
    """Rule 3: min(accepted, 2^32 - 1).  No table reaches these counts; a policy whose
    clamps are wide open makes the cut visible in the new difficulty."""
    rng = random.Random(35)
    cases, cut = [], 0
    for accepted in (U32 - 1, U32, U32 + 1, 1 << 63, U64):
        for target_ms in (1, 1000, U32):
            for old in (1, 7, U32, bits(rng, 33, 64)):
                for elapsed in (0, 1, bits(rng, 20, 40), bits(rng, 41, 63)):
                    p = dict(sref.POLICY, target_ms=target_ms, window_ms=0, band_permille=0, max_up=U32, max_down=U32)
                    cases.append((p, U64, old, U64 - elapsed, accepted))
                    # the rule without the cut, in 64-bit words: N = accepted * target_ms mod 2^64
                    wrapped = dict(p, target_ms=accepted * target_ms & U64)
                    cut += (sref.vardiff(p, U64, (old, U64 - elapsed, accepted, 0)) !=
                            sref.vardiff(wrapped, U64, (old, U64 - elapsed, 1, 0)))
    check_rule(arith, cases)
    assert cut >= 20  # so many of the cases tell the cut from its absence

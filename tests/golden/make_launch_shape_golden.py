"""Generator of tests/golden/launch_shape.json: what a fixed table of calls
returns and how the library shaped their launches (bm_launch_stat_t: layout,
task size, grid, tasks per thread), recorded from ONE build so that another
build can be held against it (tests/test_gpu_launch_shape.py replays the table
and asserts equality).  Nothing else pins launch geometry: a slip in the sizing
arithmetic changes speed, not results.

Run it on an MI355X against the build whose behaviour is the reference, e.g. a
checkout of the parent commit built beside the tree:

    BTCMINER_LIB=/path/to/parent/libbtcminer.so \
        python tests/golden/make_launch_shape_golden.py --made-from <commit> [--out FILE]

The geometry depends on the CU count, so the file records the one it was made
on (the grid of the saturating blocks_per_cu = 1 launch); the test skips on a
device with another count.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

BRADFITZ = dict(msg=b"bradfitz".hex(), lo=10**10, hi=10**10 + 2**28 - 1)
R20 = dict(lo=10**9, hi=10**9 + 2**20 - 1)
M50 = (b"a" * 50).hex()  # "msg nonce" ends at byte 60 of one block: a padding block, folded for a search
M46 = (b"a" * 46).hex()  # P = 56: P % 4 == 0, the two-word inner loop (100-nonce tasks need a big launch)
M59 = (b"a" * 59).hex()  # the digits straddle two blocks; over more than 64 windows of 10^6: NBV = 2
SPLIT3 = dict(devices=[0, 0, 0], split=[1, 5, 2])
T_SOME = (1 << 64) >> 12  # about 256 of 2^20 nonces meet it
T_FEW = (1 << 64) >> 16   # about 16 of 2^20
H_SOME = (1 << 244) - 1   # about 1 nonce in 2^12 meets it
HDR3 = dict(devices=[0, 0, 0], lo=393216, hi=393216 + 3 * 2**15 - 1)
ONE_NONCE3 = dict(devices=[0, 0, 0], lo=8603, hi=8603)  # one nonce and two empty pieces
R18 = dict(lo=0, hi=2**18 - 1)
# seven versions (groups 4 + 2 + 1), one of them twice: tools/header_versions_hits_check.cpp's
VERSIONS7 = [0x20000000, 0x20002000, 1, 0x3FFFE000, 0, 0x20002000, 0xFFFFFFFF]

# name -> the call.  kind: search | target | hits | header | header_hits | header_versions |
# header_versions_hits; knobs are Context setters.
CASES = [
    dict(name="search_digit_boundaries", kind="search", msg=b"msg".hex(), lo=0, hi=99999),
    dict(name="search_tail_split_bpc1", kind="search", blocks_per_cu=1, **BRADFITZ),
    dict(name="search_tail_split", kind="search", **BRADFITZ),
    dict(name="search_tail_split_task_digits1", kind="search", task_digits=1, **BRADFITZ),
    dict(name="search_tail_split_task_digits2", kind="search", task_digits=2, **BRADFITZ),
    dict(name="search_folded_pad", kind="search", msg=M50, **R20),
    dict(name="target_generic_pad_found", kind="target", msg=M50, target=T_SOME, **R20),
    dict(name="target_generic_pad_none", kind="target", msg=M50, target=0, **R20),
    dict(name="hits_generic_pad", kind="hits", msg=M50, target=T_FEW, cap=4096, **R20),
    dict(name="search_two_word_inner", kind="search", msg=M46, lo=10**9, hi=10**9 + 2**28 - 1),
    dict(name="search_nbv2", kind="search", msg=M59, lo=10**9, hi=10**9 + 2**27 - 1),
    dict(name="split3_search", kind="search", msg=M50, **R20, **SPLIT3),
    dict(name="split3_target_found", kind="target", msg=M50, target=T_SOME, **R20, **SPLIT3),
    dict(name="split3_target_none", kind="target", msg=M50, target=0, **R20, **SPLIT3),
    dict(name="split3_hits", kind="hits", msg=M50, target=T_FEW, cap=4096, **R20, **SPLIT3),
    dict(name="header_one_device", kind="header", lo=0, hi=2**20 - 1, target=0),
    dict(name="header_three_found", kind="header", target=H_SOME, **HDR3),
    dict(name="header_three_none", kind="header", target=0, **HDR3),
    dict(name="header_one_nonce_two_empty", kind="header", devices=[0, 0, 0], lo=8603, hi=8603, target=0),
    dict(name="header_hits_one_device", kind="header_hits", lo=0, hi=2**20 - 1, target=H_SOME, cap=4096),
    dict(name="header_hits_three", kind="header_hits", target=H_SOME, cap=4096, **HDR3),
    dict(name="header_hits_three_overflow", kind="header_hits", target=H_SOME, cap=1, **HDR3),
    dict(name="header_hits_one_nonce_two_empty", kind="header_hits", target=H_SOME, cap=4096, **ONE_NONCE3),
    dict(name="header_versions_one_device_none", kind="header_versions", versions=VERSIONS7, target=0, **R18),
    dict(name="header_versions_three_none", kind="header_versions", versions=VERSIONS7, target=0, **HDR3),
    dict(name="header_versions_three_found", kind="header_versions", versions=VERSIONS7, target=H_SOME, **HDR3),
    dict(name="header_versions_one_version", kind="header_versions", versions=VERSIONS7[:1], target=0, **R18),
    dict(name="header_versions_hits_one_device", kind="header_versions_hits", versions=VERSIONS7, target=H_SOME,
         cap=4096, **R18),
    dict(name="header_versions_hits_three", kind="header_versions_hits", versions=VERSIONS7, target=H_SOME, cap=4096,
         **HDR3),
    dict(name="header_versions_hits_three_overflow", kind="header_versions_hits", versions=VERSIONS7, target=H_SOME,
         cap=1, **HDR3),
    dict(name="header_versions_hits_one_nonce_two_empty", kind="header_versions_hits", versions=VERSIONS7,
         target=H_SOME, cap=4096, **ONE_NONCE3),
]
assert all(c["hi"] - c["lo"] < 2**28 for c in CASES)

SATURATING = "search_tail_split_bpc1"  # its biggest launch fills the device: grid = CU count


def genesis_header():
    with open(os.path.join(HERE, "header_vectors.json")) as f:
        return bytes.fromhex(next(g for g in json.load(f)["headers"] if g["name"] == "genesis")["header"])


def run_case(Context, case):
    """The case on a fresh context -> what the golden file records of it."""
    with Context(devices=case.get("devices", [0])) as ctx:
        for knob in ("blocks_per_cu", "task_digits", "split"):
            if knob in case:
                getattr(ctx, "set_" + knob)(case[knob])
        lo, hi = case["lo"], case["hi"]
        found = None
        if case["kind"] == "search":
            result = list(ctx.search(bytes.fromhex(case["msg"]), lo, hi))
        elif case["kind"] == "target":
            found, h, n = ctx.search_target(bytes.fromhex(case["msg"]), lo, hi, case["target"])
            result = [found, h, n]
        elif case["kind"] == "hits":
            count, hits, best = ctx.search_hits(bytes.fromhex(case["msg"]), lo, hi, case["target"], case["cap"])
            result = [count, [list(x) for x in hits], list(best)]
        elif case["kind"] == "header":
            found, h, n = ctx.search_header(genesis_header(), lo, hi, case["target"])
            result = [found, str(h), n]  # a 256-bit integer: as a decimal string
        elif case["kind"] == "header_hits":
            count, hits, (h, n) = ctx.search_header_hits(genesis_header(), lo, hi, case["target"], case["cap"])
            result = [count, None if hits is None else [[str(x), m] for x, m in hits], [str(h), n]]
        elif case["kind"] == "header_versions":
            found, h, n, i = ctx.search_header_versions(genesis_header(), case["versions"], lo, hi, case["target"])
            result = [found, str(h), n, i]
        else:
            count, hits, (h, n, i) = ctx.search_header_versions_hits(genesis_header(), case["versions"], lo, hi,
                                                                     case["target"], case["cap"])
            result = [count, None if hits is None else [[str(x), m, k] for x, m, k in hits], [str(h), n, i]]
        st = ctx.last_stats()
        rec = dict(result=result, launches=st.launches, nonces=st.nonces,
                   launch=[[L.device, L.p, L.nbv, L.pad_block, L.digits, L.inner_digits, L.nonces, L.grid,
                            L.tasks_per_thread] for L in st.launch[:st.recorded]])
        if found is False:  # a full scan: every task was handed out
            rec["nonces_dispatched"] = ctx.last_target_stats().nonces_dispatched
        return rec


def cpu_hit_count(case):
    """How many (nonce, version) pairs of a header enumeration's window meet its target, from hashlib."""
    import hashlib
    import struct
    header = genesis_header()
    heads = [struct.pack("<I", v) + header[4:76] for v in case.get("versions", [struct.unpack("<I", header[:4])[0]])]
    return sum(int.from_bytes(hashlib.sha256(hashlib.sha256(head + struct.pack("<I", n)).digest()).digest(),
                              "little") <= case["target"]
               for n in range(case["lo"], case["hi"] + 1) for head in heads)


def check_windows():
    """Before recording: an H_SOME enumeration does contain hits (an overflow
    case more than its cap), unless its window is the single nonce."""
    counts = {}
    for case in CASES:
        if case["kind"] in ("header_hits", "header_versions_hits") and case["hi"] > case["lo"]:
            counts[case["name"]] = n = cpu_hit_count(case)
            assert n > (case["cap"] if case["cap"] < 4096 else 0), (case["name"], n)
            assert case["cap"] < 4096 or n <= case["cap"], (case["name"], n)
    return counts


def device_cus(Context):
    case = next(c for c in CASES if c["name"] == SATURATING)
    return max(row[7] for row in run_case(Context, case)["launch"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "launch_shape.json"))
    ap.add_argument("--made-from", required=True, help="the commit whose build is loaded (BTCMINER_LIB)")
    args = ap.parse_args()
    from distributed_bitcoin_minter_amd import Context, _lib
    counts = check_windows()
    doc = dict(made_from=args.made_from, library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" +
               os.path.basename(_lib.LIB_PATH), cus=device_cus(Context), columns=[
                   "device", "p", "nbv", "pad_block", "digits", "inner_digits", "nonces", "grid", "tasks_per_thread"],
               cases=[dict(case, expect=run_case(Context, case)) for case in CASES])
    for case in doc["cases"]:  # the enumerations' counts against hashlib's
        assert case["name"] not in counts or case["expect"]["result"][0] == counts[case["name"]], case["name"]
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {len(CASES)} cases, {doc['cus']} CUs")


if __name__ == "__main__":
    main()

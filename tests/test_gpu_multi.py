"""GPU tests of the multi-GPU paths, the reductions' tie rule and the
failure path, all through the C ABI (libbtcminer.so):

  * the N-device split of one context, rehearsed on one GPU (the same device
    listed N times, host combine), against the oracle at the split points,
    10^k digit boundaries, 2^64-1 and ranges shorter than N;
  * a context that is one rank of an RCCL group (world 1 on this box: RCCL
    cannot put two ranks on one GPU);
  * the long-range goldens: [0, N*2^32-1] for N = 1..8 (bench.py's weak
    scaling answers) and 64 random 2^24-nonce windows of C4's [0, 2^40-1];
  * bm_reduce_gpu with injected equal hashes (the tie rule, miner.go:61);
  * a search that fails part-way (test fault) leaves the context usable;
  * bench.py's multi-GPU modes, rehearsed on one GPU.
"""
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, U64, load_golden
from distributed_bitcoin_minter_amd import BtcMinerError, Context, rccl_unique_id
from distributed_bitcoin_minter_amd._lib import BM_COMBINE_RCCL, BM_EINTERNAL, BM_EINVAL
from distributed_bitcoin_minter_amd.dist import split_range

pytestmark = pytest.mark.gpu

C2 = next(c for c in load_golden("full_range.json")["cases"] if c["config"] == "C2")
M120 = (b"The quick brown fox jumps over the lazy dog. " * 3)[:120]


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_device_split_on_one_gpu(oracle, n):
    """Context(devices=[0]*n): n device slots, split_range pieces, per-slot
    plans and launches, host combine; equal to the oracle everywhere the
    split can go wrong."""
    msg = b"bradfitz"
    with Context(devices=[0] * n) as c:
        assert c.num_devices() == n
        cases = [(0, 9999), (999_999_000, 1_000_001_000), (10 ** 19 - 3000, 10 ** 19 + 3000),
                 (U64 - 5000, U64), (U64, U64), (7, 7), (5, 5 + n - 2), (10, 9)]
        # windows whose pieces meet exactly at a digit boundary
        for lo in (10 ** 9 - 1500, 10 ** 12 - 777):
            cases.append((lo, lo + 2999))
        for lo, hi in cases:
            want = oracle.search(msg, lo, hi, threads=8) if lo <= hi else (U64, U64)
            assert c.search(msg, lo, hi) == want, (n, lo, hi)
            if lo <= hi:
                st = c.last_stats()
                assert {st.launch[i].device for i in range(st.recorded)} <= set(range(n))
        # the answer sits in the second of two pieces / at a piece's first nonce
        h, nn = C2["hash"], C2["nonce"]
        for lo, hi in ((nn - 1000, nn + 1000), (nn, nn + 2 * n - 1)):
            want = oracle.search(msg, lo, hi, threads=8)
            assert c.search(msg, lo, hi) == want == (h, nn)
        # C2's whole range over n slots
        assert c.search(msg, C2["lower"], C2["upper"]) == (h, nn)


def test_device_split_rejects_rccl_on_one_gpu():
    with Context(devices=[0, 0]) as c:
        c.set_combine(BM_COMBINE_RCCL)
        with pytest.raises(BtcMinerError) as ei:
            c.search(b"bradfitz", 0, 9999)
        assert ei.value.status == BM_EINVAL
        c.set_combine(0)
        assert c.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)


def test_rank_context_world1(oracle):
    """bm_ctx_create_rank at world 1 (ncclCommInitRank + the in-library
    allgather over the process group) on the box's GPU."""
    with Context(devices=[0], rank=0, world=1, unique_id=rccl_unique_id()) as c:
        assert c.rank() == (0, 1)
        assert c.search(b"msg", 0, 2) == (4754799531757243342, 1)
        assert c.search(b"bradfitz", 999_000_000, 1_000_999_999) == \
            oracle.search(b"bradfitz", 999_000_000, 1_000_999_999, threads=8)
        assert c.search(b"bradfitz", 10, 9) == (U64, U64)
        assert c.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])


def _scale():
    path = os.path.join(ROOT, "tests", "golden", "scale_ranges.json")
    if not os.path.exists(path):
        pytest.skip("scale_ranges.json not generated")
    return json.load(open(path))


@pytest.mark.parametrize("n", [2, 4, 8])
def test_weak_scaling_goldens(gpu_ctx, n):
    """[0, N*2^32-1] (bench.py's C2 workload at N GPUs) on one GPU equals the
    committed answer (tests/golden/make_chunk_golden.py)."""
    d = _scale()
    r = next((r for r in d["ranges"] if r["name"] == f"weak{n}"), None)
    if r is None:
        pytest.skip(f"weak{n} golden not generated")
    assert gpu_ctx.search(bytes.fromhex(d["msg_hex"]), r["lower"], r["upper"]) == (r["hash"], r["nonce"])


def test_chunk_goldens_sample(gpu_ctx):
    """A sample of the 2^32-nonce chunks of [0, 2^40-1] (the C4 range), each
    against its committed answer: 11- to 13-digit nonces."""
    path = os.path.join(ROOT, "tests", "golden", "c4_chunks.json")
    if not os.path.exists(path):
        pytest.skip("c4_chunks.json not generated")
    d = json.load(open(path))
    ks = sorted(int(k) for k in d["chunks"])
    rng = random.Random(0x5EED)
    pick = sorted(set([ks[-1]] + rng.sample(ks, min(6, len(ks)))))
    for k in pick:
        h, n = d["chunks"][str(k)]
        assert gpu_ctx.search(d["msg"].encode(), k * d["chunk"], (k + 1) * d["chunk"] - 1) == (h, n), k


def test_c4_random_windows(gpu_ctx):
    """64 random 2^24-nonce windows of [0, 2^40-1] (seed
    0x5EED), answers from the oracle's byte-string loop."""
    path = os.path.join(ROOT, "tests", "golden", "c4_windows.json")
    if not os.path.exists(path):
        pytest.skip("c4_windows.json not generated")
    d = json.load(open(path))
    assert len(d["windows"]) == 64
    for w in d["windows"]:
        assert gpu_ctx.search(d["msg"].encode(), w["lower"], w["upper"]) == (w["hash"], w["nonce"]), w


@pytest.mark.parametrize("cfg", ["C4"])
def test_c4_whole_range(cfg):
    """C4 itself, [0, 2^40-1], through every visible device of one context
    (one GPU here: ~20 s), against the golden from 256 oracle chunks."""
    d = _scale()
    r = next((r for r in d["ranges"] if r["name"] == "C4"), None)
    if r is None:
        pytest.skip("C4 golden not generated")
    from distributed_bitcoin_minter_amd import device_count
    with Context(num_gpus=device_count()) as c:
        assert c.search(bytes.fromhex(d["msg_hex"]), r["lower"], r["upper"]) == (r["hash"], r["nonce"])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 100_003])
def test_reduce_tie_rule(gpu_ctx, n):
    """Equal hashes with shuffled nonces: the GPU reductions (wave ds_swizzle
    butterflies + readlane, LDS across waves, second pass) return the
    smallest nonce, i.e. the lexicographic (hash, nonce) min."""
    rng = random.Random(n)
    for trial in range(4):
        hmin = rng.randrange(1 << 64) if trial else 0
        pairs = [(rng.randrange(hmin, 1 << 64), rng.randrange(1 << 64)) for _ in range(n)]
        k = rng.randint(1, min(n, 40))
        ties = rng.sample(range(n), k)
        for i in ties:  # k entries share the minimum hash, nonces random
            pairs[i] = (hmin, rng.randrange(1 << 64))
        rng.shuffle(pairs)
        assert gpu_ctx.reduce(pairs) == min(pairs), (n, trial)
    # every lane tied, nonces descending across lanes, waves and workgroups
    pairs = [(5, U64 - i) for i in range(n)]
    assert gpu_ctx.reduce(pairs) == (5, U64 - (n - 1))
    # the empty partial (2^64-1, 2^64-1) never beats a real one
    assert gpu_ctx.reduce([(U64, U64)] * n) == (U64, U64)
    assert gpu_ctx.reduce([(U64, U64)] * (n - 1) + [(U64, 3)]) == (U64, 3)


def test_reduce_empty(gpu_ctx):
    assert gpu_ctx.reduce([]) == (U64, U64)


@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("fault", [0, 1, 3, 9])
def test_failure_midway_leaves_context_usable(fault, slots):
    """A search that fails after `fault` launches (some already running on the
    aux stream) returns BM_EINTERNAL, drains, and the same context then
    answers C2 and a small window correctly.  With 4 slots (round 6) the
    devices' work is submitted by the context's persistent submission threads
    at once, so the failing launch may be any slot's: the call still fails as
    a whole, every slot's streams are drained, and the threads serve the next
    calls."""
    with Context(devices=[0] * slots) as c:
        c.set_test_fault(fault)
        with pytest.raises(BtcMinerError) as ei:
            c.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"])
        assert ei.value.status == BM_EINTERNAL
        c.set_test_fault(-1)
        assert c.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        assert c.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)


def test_stats_span_vs_sum(gpu_ctx):
    """kernel_ms sums launch times, which overlap over two streams; span_ms is
    the first launch's start to the last one's end."""
    gpu_ctx.set_timing(True)
    try:
        gpu_ctx.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"])
        st = gpu_ctx.last_stats()
        assert st.launches >= 10 and st.span_ms > 0
        assert st.span_ms <= st.wall_ms
        assert max(st.launch[i].ms for i in range(st.recorded)) <= st.span_ms + 1e-3
        # the live clock probe (BM_CLOCK_PROBE builds only): a plausible shader clock
        dom = max((st.launch[i] for i in range(st.recorded)), key=lambda L: L.nonces)
        assert dom.clock_ghz == 0.0 or 1.0 < dom.clock_ghz < 3.0, dom.clock_ghz
    finally:
        gpu_ctx.set_timing(False)


def _bench(args, env=None, torchrun=0):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    if torchrun:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={torchrun}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py")] + args
    # its own process group: on a hang, torchrun's workers die with it
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                         start_new_session=True)
    try:
        out, err = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        import signal
        os.killpg(p.pid, signal.SIGKILL)
        out, err = p.communicate()
        pytest.fail(f"bench {args} did not finish in 300 s: {err[-2000:]}")
    return subprocess.CompletedProcess(cmd, p.returncode, out, err)


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_plain_run_dumps_outputs(tmp_path):
    """bench.py without --full: the timed steps and the line only (--steps is
    the number of timed steps, ms_per_step one step's time; no C4 step, no CPU
    baseline, no clock measurement), and --dump-outputs writes the last
    step's (hash, nonce) as result.npy, equal to the line's result and C2's
    golden."""
    import numpy as np
    out = _line(_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")]))
    assert out["result_ok"] is True and out["steps"] == 2 and out["warmup"] == 1
    assert out["unit"] == "GH/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert 10 < out["ms_per_step"] < 1000, out["ms_per_step"]  # 2^32 nonces: about 80 ms
    assert abs(out["value"] - 2 ** 32 / out["ms_per_step"] / 1e6) < 0.01 * out["value"]
    for k in ("c4", "c4_one_process", "cpu_baseline"):
        assert k not in out, k
    assert "clock_ghz_box" not in out["roofline"] and "clock_ghz_box_live" not in out["roofline"]
    a = np.load(tmp_path / "dump" / "result.npy")
    assert a.dtype == np.float64 and a.shape == (4,)
    got = [(int(a[0]) << 32) | int(a[1]), (int(a[2]) << 32) | int(a[3])]
    assert got == out["result"] == [C2["hash"], C2["nonce"]]


def test_bench_one_process_rehearsal():
    """bench.py --gpus 2 without a launcher on a one-GPU box: loud failure,
    unless --rehearse-one-gpu (2-way split on GPU 0); the answer matches the
    weak2 golden."""
    from distributed_bitcoin_minter_amd import device_count
    if device_count() < 2:
        r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"])
        assert r.returncode == 2 and "HIP device" in r.stderr
    out = _line(_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline",
                        "--rehearse-one-gpu"]))
    assert out["n_gpus"] == 2 and out["config"]["global_nonces"] == 2 ** 33
    assert out["result_ok"] in (True, None) and "rehearsal" in out
    assert out["scaling_valid"] is False and "rehearsal" in out["scaling_invalid"][0]
    # every line carries north_star's 2^40 target, one warm C4 step
    # split over the N slots, checked against the 2^40 golden
    c4 = out["c4"]
    assert (c4["lower"], c4["upper"], c4["nonces"], c4["scaling"]) == (0, 2 ** 40 - 1, 2 ** 40, "strong"), c4
    assert c4["result_ok"] is True and c4["result"] == c4["golden"] == [16555811, 890536971553], c4
    assert len(c4["devices"]) == 2 and sum(d["nonces"] for d in c4["devices"]) == 2 ** 40, c4
    assert c4["combine"] == "host" and c4["GHs"] > 10 and c4["seconds"] > 1, c4
    # every N > 1 line carries c4_one_process; without a launcher
    # the line is the one-process mode itself, so the block points at its c4
    one = out["c4_one_process"]
    assert one["same_as"] == "c4" and one["GHs"] == c4["GHs"] and one["result_ok"] is True, one
    # the one-process line reports the start of each device's work (a host
    # thread per device) and, with no RCCL combine, why there is no RCCL block
    assert out["start_threads"] == 2 and out["start_skew_ms"] >= 0, out
    assert out["rccl"] is None and "no RCCL collective ran" in out["rccl_absent"], out


def test_bench_torchrun_rehearsal():
    """bench.py under torchrun with 2 ranks on GPU 0 (file rendezvous,
    gather of the partials); the GPU processes map one HIP runtime."""
    out = _line(_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--rehearse-one-gpu", "--no-c4"], torchrun=2))
    assert out["n_gpus"] == 2 and out["result_ok"] in (True, None)
    assert out["start_skew_ms"] >= 0 and all("start_offset_ms" in r for r in out["config"]["ranks"]), out
    assert len(out["hip_runtime"]) == 1, out["hip_runtime"]
    assert out["scaling_valid"] is False and "rehearsal" in out["scaling_invalid"][0]


def test_bench_torchrun_rehearsal_c4_one_process():
    """a torchrun line at N > 1 also measures C4 through ONE
    process over the N devices (the Go shim's and BASELINE configs[3]'s
    design): rank 0 runs it in a child while the ranks idle.  Rehearsed on
    one GPU: 2 slots on GPU 0, host combine, the 2^40 golden, and no scaling
    claim."""
    out = _line(_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full", "--rehearse-one-gpu"], torchrun=2))
    assert out["result_ok"] is True and out["c4"]["result_ok"] is True, out.get("c4")
    one = out["c4_one_process"]
    assert "skipped" not in one, one
    assert one["result_ok"] is True and one["result"] == [16555811, 890536971553] and one["nonces"] == 2 ** 40, one
    assert one["combine"] == "host" and one["scaling_valid"] is False and one["GHs"] > 10, one
    assert len(one["devices"]) == 2 and sum(d["nonces"] for d in one["devices"]) == 2 ** 40, one
    assert all("start_ms" in d and "allgather_ms" in d for d in one["devices"]) and one["start_threads"] == 2
    assert "bm_ctx_create(2)" in one["design"] and one["child_cmd"].startswith("bench.py --gpus 2 --config C4")
    assert "--rehearse-one-gpu" in one["child_cmd"]


def test_bench_torchrun_rccl_world1():
    """bench.py under torchrun at world 1 is the plain path; the RCCL rank
    context at world 1 runs through the rendezvous with --combine rccl when
    WORLD_SIZE is forced to 1 by the launcher: covered by
    test_rank_context_world1.  Here: the N = 1 line is well formed and maps
    one HIP runtime."""
    out = _line(_bench(["--gpus", "1", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline", "--no-c4"]))
    assert out["result_ok"] is True and out["n_gpus"] == 1 and "c4" not in out
    assert len(out["hip_runtime"]) == 1 and "/opt/rocm" in out["hip_runtime"][0]
    assert out["roofline"]["frac"] > 0.5
    # the PMC figures are the committed pass's, marked as imported
    roof = out["roofline"]
    pm = roof["pmc"]
    assert pm["imported"] is True and pm["src"].startswith("profiles/") and pm["box_clock_ghz"] > 1.0, pm
    assert pm["valu_per_nonce"] > 1000 and 0.3 < pm["valu_dual_issued_frac"] < 0.6, pm  # C2: 0.477
    assert roof["traffic"] == pm["hbm_bytes_per_launch"] and roof["traffic_imported"] is True
    # the imported pass is tied to the kernel this run loaded (the
    # sha256 of its instructions in the library's gfx950 code object)
    assert pm["src"].startswith("profiles/r06/") and pm["same_kernel"] is True, pm
    assert pm["code_sha"] == pm["loaded_code_sha"] and len(pm["code_sha"]) == 64
    for k in ("valu_per_nonce_pmc", "valu_dual_issued_frac_pmc", "clock_ghz_pmc"):
        assert k not in roof, k
    assert "imported" in roof["executed"]["src"], roof["executed"]
    ex = out["roofline"]["executed"]  # executed VALU lane-ops, always below the peak
    assert ex and 0.5 < ex["frac"] < 1.0 and ex["valu_per_nonce"] > 1000, ex
    assert "ceiling" in out["roofline"]["issue_bound"]["role"]
    call = out["roofline"]["call"]
    assert "issue_frac" not in call or 0.8 < call["issue_frac"] < 1.05, call


def test_split_range_matches_library(gpu_ctx):
    """dist.split_range (Python) and bm::split_range (C++) cut alike: each
    device slot's launches stay inside its Python piece."""
    lo, hi = 123_456_789, 123_456_789 + 10_000_003
    with Context(devices=[0, 0, 0]) as c:
        c.search(b"bradfitz", lo, hi)
        st = c.last_stats()
        per = {}
        for i in range(st.recorded):
            per[st.launch[i].device] = per.get(st.launch[i].device, 0) + st.launch[i].nonces
    assert [per[i] for i in range(3)] == [b - a + 1 for a, b in split_range(lo, hi, 3)]


_RANK_BOOT = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
from distributed_bitcoin_minter_amd import _lib
_lib.load()
from distributed_bitcoin_minter_amd import BtcMinerError, Context, rccl_unique_id
from distributed_bitcoin_minter_amd.rendezvous import Rendezvous
with Rendezvous(timeout_s=120) as rz:
    uid = rz.broadcast_bytes(rccl_unique_id() if rz.rank == 0 else None)
    with Context(devices=[0], rank=rz.rank, world=rz.world) as c:
        try:
            c.join(uid, timeout_ms=60_000)  # bounded: a box where RCCL waits instead of refusing costs 60 s
            status = 0
        except BtcMinerError as e:
            status = e.status
    seen = rz.all_gather(status)
print(json.dumps({"rank": rz.rank, "status": status, "seen": seen}))
"""


def test_rank_group_bootstrap_two_ranks_one_gpu():
    """Two rank contexts on the SAME GPU: the unique id made by rank 0 reaches
    rank 1 over the rendezvous, both join RCCL's bootstrap (bm_ctx_join_rank,
    bounded), and RCCL then refuses the duplicate GPU -- both ranks get
    BM_ERCCL promptly (no hang), which is what bench.py's fallback relies on.  (Two distinct GPUs would
    form the group: the driver's multi-GPU run.)"""
    import socket
    from distributed_bitcoin_minter_amd._lib import BM_ERCCL
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r),
                   WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, "-c", _RANK_BOOT, ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=180)
            assert p.returncode == 0, e[-3000:]
            outs.append(json.loads(o.strip().splitlines()[-1]))
    finally:
        for p in procs:  # never leave a rank holding the GPU
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(o["seen"] == [BM_ERCCL, BM_ERCCL] for o in outs), outs


_RANK_EPEER = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
from distributed_bitcoin_minter_amd import _lib
_lib.load()
from distributed_bitcoin_minter_amd import BtcMinerError, Context, rccl_unique_id
from distributed_bitcoin_minter_amd.rendezvous import Rendezvous
out = {}
with Rendezvous(timeout_s=120) as rz:
    uid = rz.broadcast_bytes(rccl_unique_id() if rz.rank == 0 else None)
    with Context(devices=[rz.rank], rank=rz.rank, world=rz.world) as c:
        c.join(uid, timeout_ms=60_000)
        c.set_peer_timeout(60_000)
        out["ok"] = list(c.search(b"bradfitz", 0, 9999))
        st = c.last_stats()
        out["nranks"], out["rrank"], out["rdev"] = st.rccl_nranks, st.rccl_rank, st.dev_rccl_device[0]
        if rz.rank == 1:
            c.set_test_fault(0)  # this rank fails before the combine
        try:
            c.search(b"bradfitz", 0, 9999)
            out["fault"] = 0
        except BtcMinerError as e:
            out["fault"] = e.status
        c.set_test_fault(-1)
        out["after"] = list(c.search(b"bradfitz", 0, 9999))  # the group survived
        rz.barrier()
print(json.dumps(dict(out, rank=rz.rank)))
"""


def test_rank_group_epeer_two_gpus():
    """on a box with two distinct GPUs, a 2-rank group whose rank 1
    fails a search before the combine: rank 1 returns its own status
    (BM_EINTERNAL), rank 0 BM_EPEER -- neither waits -- and the next search
    answers on both.  RCCL reports 2 ranks, one per device.  (RCCL refuses
    two ranks on one GPU, so on a one-GPU box this is skipped and the
    world > 1 status path is unpinned: DESIGN.md §6.)"""
    from distributed_bitcoin_minter_amd import device_count
    from distributed_bitcoin_minter_amd._lib import BM_EPEER
    if device_count() < 2:
        pytest.skip("needs two GPUs")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), LOCAL_RANK=str(r),
                   WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, "-c", _RANK_EPEER, ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=240)
            assert p.returncode == 0, e[-3000:]
            outs.append(json.loads(o.strip().splitlines()[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    outs.sort(key=lambda o: o["rank"])
    want = [1419516646206828, 9898]
    assert all(o["ok"] == want and o["after"] == want for o in outs), outs
    assert [o["fault"] for o in outs] == [BM_EPEER, BM_EINTERNAL], outs
    assert [(o["nranks"], o["rrank"], o["rdev"]) for o in outs] == [(2, 0, 0), (2, 1, 1)], outs


def test_weighted_device_split_on_one_gpu(oracle):
    """The range partitioner with explicit shares (bm_ctx_set_split): three
    device slots on GPU 0 with shares 1:2:5 scan exactly the pieces
    bm_split_range cuts, and every answer equals the oracle's."""
    from distributed_bitcoin_minter_amd import _lib
    msg, shares = b"bradfitz", [1, 2, 5]
    with Context(devices=[0, 0, 0]) as c:
        c.set_split(shares)
        assert c.get_split() == shares
        c.set_timing(True)
        for lo, hi in [(0, 9999), (999_999_000, 1_000_001_000), (U64 - 5000, U64), (7, 9), (10 ** 12 - 4000,
                                                                                           10 ** 12 + 4000)]:
            assert c.search(msg, lo, hi) == oracle.search(msg, lo, hi, threads=8), (lo, hi)
            st = c.last_stats()
            per = {}
            for i in range(st.recorded):
                per[st.launch[i].device] = per.get(st.launch[i].device, 0) + st.launch[i].nonces
            want = [0 if p is None else p[1] - p[0] + 1 for p in _lib.split_range(lo, hi, 3, shares)]
            assert [per.get(i, 0) for i in range(3)] == want, (lo, hi)
        assert c.search(msg, C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        for bad in ([1, 2], [1, 0, 1]):
            with pytest.raises(BtcMinerError) as ei:
                c.set_split(bad)
            assert ei.value.status == BM_EINVAL
        c.set_split(None)
        assert c.get_split() == []


def test_balance_on_one_gpu():
    """bm_ctx_set_balance: after a search with >= 2^30 nonces per device the
    context's shares follow each device's measured rate (two slots on one GPU:
    about equal), the next search splits by them, and both answer C2 right;
    a small search leaves the shares alone."""
    msg = bytes.fromhex(C2["msg_hex"])
    with Context(devices=[0, 0]) as c:
        c.set_balance(True)
        assert c.get_split() == []
        assert c.search(msg, C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        sh = c.get_split()
        assert len(sh) == 2 and max(sh) == 65536 and min(sh) > 0.7 * 65536, sh
        assert c.search(msg, C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        sh2 = c.get_split()
        assert c.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
        assert c.get_split() == sh2


def test_rank_context_split_world1():
    with Context(devices=[0], rank=0, world=1, unique_id=rccl_unique_id()) as c:
        c.set_split([3])
        assert c.search(b"msg", 0, 2) == (4754799531757243342, 1)
        with pytest.raises(BtcMinerError):
            c.set_split([1, 1])  # one share per rank


def test_bench_rehearsals_balance_after_warmup():
    """bench.py's range partitioner, rehearsed on one GPU: after one warmup
    step the one-process 2-way split balances itself (bm_ctx_set_balance),
    and 2 torchrun ranks exchange the rates of their second (warm) warmup step
    over the rendezvous and cut by the shares (dist.rank_piece); both
    answers equal the weak2 golden."""
    out = _line(_bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--rehearse-one-gpu",
                        "--no-c4"]))
    sp = out["config"]["split"]
    assert out["result_ok"] is True and sp["mode"].startswith("measured device rates") and len(sp["shares"]) == 2
    out = _line(_bench(["--gpus", "2", "--steps", "1", "--warmup", "2", "--rehearse-one-gpu", "--no-c4"],
                       torchrun=2))
    sp = out["config"]["split"]
    assert out["result_ok"] is True and sp["mode"].startswith("measured rank rates"), sp
    assert len(sp["shares"]) == 2 and max(sp["shares"]) == 65536


# ---- fail-safe combines (ABI 5) ---------------------------------------------

from distributed_bitcoin_minter_amd._lib import (BM_COMBINED_HOST, BM_COMBINED_LOCAL,  # noqa: E402
                                                 BM_COMBINED_RCCL, BM_EPEER, BM_ERCCL, BM_ETIMEDOUT)


@pytest.mark.parametrize("where", [1, 2])
def test_rccl_failure_falls_back_to_host_copies(oracle, where):
    """A one-process context whose RCCL combine fails (1: ncclCommInitAll,
    2: the grouped allgather; forced by the test hook) aborts its
    communicators and combines by host copies -- the same answer, reported
    as combine_used = host with rccl_status = BM_ERCCL, for that call and
    every later one."""
    msg, lo, hi = b"bradfitz", 999_000_000, 1_000_999_999
    want = oracle.search(msg, lo, hi, threads=8)
    with Context(devices=[0]) as c:
        c.set_combine(BM_COMBINE_RCCL)
        c.set_timing(True)
        assert c.search(msg, lo, hi) == want
        st = c.last_stats()
        assert (st.combine_used, st.rccl_status) == (BM_COMBINED_RCCL, 0)
        # ncclCommInitAll over the context's one device: RCCL reports 1 rank, on device 0
        assert (st.rccl_nranks, st.rccl_rank, st.dev_rccl_rank[0], st.dev_rccl_device[0]) == (1, 0, 0, 0)
        # VERDICT r4 (ABI 7): RCCL's version, the communicator's set-up time and
        # the allgather's event pair, so a multi-GPU line reads without a rerun
        assert st.rccl_version >= 20000 and st.rccl_init_ms > 0, (st.rccl_version, st.rccl_init_ms)
        assert 0 < st.rccl_allgather_ms == st.dev_allgather_ms[0] < 1000 and st.combine_ms > 0
        assert st.start_threads == 1 and st.dev_start_ms[0] == 0
    with Context(devices=[0]) as c:
        c.set_combine(BM_COMBINE_RCCL)
        c.set_test_rccl_fault(where)
        c.set_timing(True)
        for _ in range(2):
            assert c.search(msg, lo, hi) == want
            st = c.last_stats()
            assert (st.combine_used, st.rccl_status) == (BM_COMBINED_HOST, BM_ERCCL)
            assert (st.rccl_nranks, st.rccl_rank) == (0, -1)
            # no communicator left, no allgather: nothing of RCCL but its version
            assert (st.rccl_init_ms, st.rccl_allgather_ms) == (0, 0) and st.rccl_version >= 20000
        c.set_test_rccl_fault(0)
        assert c.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        assert c.last_stats().combine_used == BM_COMBINED_HOST  # stays on host copies


def test_rank_contexts_outside_a_group(oracle):
    """the rank path of the library at world > 1 without a
    communicator.  Three rank contexts (ranks 0-2 of 3) on GPU 0 each scan
    exactly their bm_split_range piece -- near-equal, with shares 1:2:5, and
    for a range shorter than the group -- return their own partial
    (combine_used = local), and the lexicographic min of the three equals
    the oracle and the C2 golden."""
    from distributed_bitcoin_minter_amd import _lib
    from distributed_bitcoin_minter_amd.dist import lex_min
    msg = b"bradfitz"
    ctxs = [Context(devices=[0], rank=r, world=3) for r in range(3)]
    try:
        assert all(not c.joined() and c.rank() == (r, 3) for r, c in enumerate(ctxs))
        for shares in (None, [1, 2, 5]):
            for c in ctxs:
                c.set_split(shares)
            for lo, hi in [(0, 9999), (999_999_000, 1_000_001_000), (U64 - 5000, U64), (7, 8), (5, 5),
                           (C2["lower"], C2["upper"])]:
                pieces = _lib.split_range(lo, hi, 3, shares)
                parts = []
                for r, c in enumerate(ctxs):
                    parts.append(c.search(msg, lo, hi))
                    st = c.last_stats()
                    assert st.nonces == (0 if pieces[r] is None else pieces[r][1] - pieces[r][0] + 1), (shares, lo, r)
                    assert st.combine_used == BM_COMBINED_LOCAL
                    want_r = oracle.search(msg, *pieces[r], threads=8) if pieces[r] and hi - lo < 10 ** 7 else None
                    if pieces[r] is None:
                        assert parts[-1] == (U64, U64)
                    elif want_r is not None:
                        assert parts[-1] == want_r, (shares, lo, r)
                got = lex_min(parts)
                if (lo, hi) == (C2["lower"], C2["upper"]):
                    assert got == (C2["hash"], C2["nonce"])
                else:
                    assert got == oracle.search(msg, lo, hi, threads=8), (shares, lo, hi)
    finally:
        for c in ctxs:
            c.close()


def test_rank_group_world1_status_and_leave(oracle):
    """A joined rank context (world 1 on this box) combines through the
    status-carrying allgather: a failure before the combine comes back as the
    rank's own status; a gathered slot carrying a peer's failure (test hook
    3) is BM_EPEER and leaves the group joined and usable; an allgather
    failure (test hook 2) aborts the
    communicator and every later search returns BM_ERCCL until leave(); after
    leave() the context answers with its own partial; a fresh join works."""
    msg, lo, hi = b"bradfitz", 999_000_000, 1_000_999_999
    want = oracle.search(msg, lo, hi, threads=8)
    with Context(devices=[0], rank=0, world=1) as c:
        c.join(rccl_unique_id(), timeout_ms=60_000)
        assert c.joined()
        c.set_peer_timeout(60_000)
        c.set_timing(True)
        assert c.search(msg, lo, hi) == want and c.last_stats().combine_used == BM_COMBINED_RCCL
        st = c.last_stats()  # what RCCL itself says about the group
        assert (st.rccl_nranks, st.rccl_rank, st.dev_rccl_rank[0], st.dev_rccl_device[0]) == (1, 0, 0, 0)
        # VERDICT r4 (ABI 7): the join's init time, RCCL's version, the allgather's event pair
        assert st.rccl_version >= 20000 and st.rccl_init_ms > 0, (st.rccl_version, st.rccl_init_ms)
        assert 0 < st.rccl_allgather_ms == st.dev_allgather_ms[0] < 1000 and st.combine_ms > 0, st.rccl_allgather_ms
        for fault in (0, 1):
            c.set_test_fault(fault)
            with pytest.raises(BtcMinerError) as ei:
                c.search(msg, lo, hi)
            assert ei.value.status == BM_EINTERNAL
        c.set_test_fault(-1)
        assert c.search(msg, lo, hi) == want                   # the group survived a rank-side failure
        c.set_test_rccl_fault(3)
        with pytest.raises(BtcMinerError) as ei:
            c.search(msg, lo, hi)
        assert ei.value.status == BM_EPEER and c.joined()
        c.set_test_rccl_fault(0)
        assert c.search(msg, lo, hi) == want                   # and a peer's reported failure
        assert c.last_stats().combine_used == BM_COMBINED_RCCL  # over the same communicator
        c.set_test_rccl_fault(2)
        for _ in range(2):
            with pytest.raises(BtcMinerError) as ei:
                c.search(msg, lo, hi)
            assert ei.value.status == BM_ERCCL
        c.set_test_rccl_fault(0)
        with pytest.raises(BtcMinerError) as ei:               # the communicator is gone
            c.search(msg, lo, hi)
        assert ei.value.status == BM_ERCCL
        c.leave()
        assert not c.joined()
        assert c.search(msg, lo, hi) == want and c.last_stats().combine_used == BM_COMBINED_LOCAL
        st = c.last_stats()
        assert (st.rccl_nranks, st.rccl_rank, st.dev_rccl_rank[0], st.dev_rccl_device[0]) == (0, -1, -1, -1)
        assert (st.rccl_init_ms, st.rccl_allgather_ms) == (0, 0)  # out of the group: no communicator
        c.join(rccl_unique_id())
        assert c.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        c.leave()
        c.set_test_rccl_fault(1)
        with pytest.raises(BtcMinerError) as ei:
            c.join(rccl_unique_id())
        assert ei.value.status == BM_ERCCL and not c.joined()


def test_join_without_peers_times_out():
    """Rank 0 of 2 joining a group whose other rank never comes: the caller
    waits timeout_ms for the non-blocking ncclCommInitRankConfig, then gets
    BM_ETIMEDOUT instead of a hang, and the context still searches its own
    piece.  ADVICE r3: the worker may stay blocked inside RCCL's bootstrap;
    it stays the context's pending join, so a second join starts no second
    worker (the thread count does not grow) and times out as well; closing
    the context and exiting the process still ends with status 0.  Run in a
    child process with a hard limit, so a hang fails the test instead of
    stalling the suite."""
    env = dict(os.environ, PROBE_TIMEOUT_MS="3000", BTCMINER_TRACE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probe_join_timeout.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    out = r.stdout
    assert "join 1 failed after" in out and "join 2 failed after" in out, out
    assert "search (4754799531757243342, 1)" in out and "closed after" in out, out
    for k in (1, 2):
        secs = float(out.split(f"join {k} failed after ")[1].split(" s")[0])
        assert secs < 30, out
        assert "did not answer" in out.split(f"join {k} failed after ")[1].splitlines()[0], out
    n1 = int(out.split("threads after join 1 ")[1].split()[0])
    n2 = int(out.split("threads after join 2 ")[1].split()[0])
    assert n2 <= n1, out  # no second worker inside RCCL
    if "still inside RCCL" not in r.stderr:  # the first worker ended in the meantime: the second join ran anew
        assert r.stderr.count("joining (timeout") == 2, r.stderr[-3000:]


def test_bench_torchrun_with_per_rank_visibility_mask():
    """a launcher that gives every rank a one-device visibility
    mask.  Two torchrun ranks with HIP_VISIBLE_DEVICES=0 (LOCAL_RANK 0 and 1)
    both drive their one visible device; RCCL refuses the shared GPU, so the
    ranks agree to gather their partials over the rendezvous instead.  The
    line names that combine, and each rank's nonces, which add up to the
    workload; the answer equals the weak2 golden."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    out = _line(_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-c4"], env=env, torchrun=2))
    assert out["result_ok"] is True and out["n_gpus"] == 2
    cfg = out["config"]
    assert "rendezvous gather" in cfg["parallelism"] and "RCCL group failed" in cfg["parallelism"], cfg
    ranks = sorted(cfg["ranks"], key=lambda r: r["rank"])
    assert [r["device"] for r in ranks] == [0, 0] and all(r["combine"] == "local" for r in ranks)
    assert sum(r["nonces"] for r in ranks) == cfg["global_nonces"]
    # --combine rccl fell back, on one GPU: the line says it is no scaling measurement, and why
    assert out["scaling_valid"] is False and out["rccl_nranks"] == [0], out
    why = " | ".join(out["scaling_invalid"])
    assert "instead of one RCCL allgather" in why and "1 distinct GPUs" in why, why
    assert len({r["pci_bus_id"] for r in ranks}) == 1 and all(r["rccl_nranks"] == 0 for r in ranks)
    # nothing of RCCL ran, so the line has no RCCL costs, and says why
    assert out["rccl"] is None and "combine local" in out["rccl_absent"], out
    assert all(r["allgather_ms"] == 0 and r["rccl_init_ms"] == 0 for r in ranks), ranks


def test_clock_probe_library():
    """libbtcminer_probe.so (the same kernels with BM_CLOCK_PROBE=1, which
    bench.py loads beside the product library to measure the clock under the
    dominant kernel) answers C2 like the product and reports a plausible live
    shader clock for its launches."""
    from distributed_bitcoin_minter_amd import _lib
    if not os.path.exists(_lib.PROBE_LIB_PATH):
        pytest.skip("libbtcminer_probe.so not built (make -C distributed_bitcoin_minter_amd/csrc probe)")
    with Context(devices=[0], lib_path=_lib.PROBE_LIB_PATH) as c:
        c.set_timing(True)
        assert c.search(bytes.fromhex(C2["msg_hex"]), C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        st = c.last_stats()
        dom = max((st.launch[i] for i in range(st.recorded)), key=lambda L: L.nonces)
        assert 1.0 < dom.clock_ghz < 3.0, dom.clock_ghz


# ---- start skew and balance from a common start (ABI 7) ----------


def test_start_skew_reported_on_eight_slots():
    """A one-process context of 8 device slots (all GPU 0: a rehearsal of the
    one-process 8-GPU design) submits each slot's work from a host thread of
    its own and reports each slot's start against the earliest one
    (bm_stats_t.dev_start_ms): 8 threads, the earliest at 0, all within a few
    ms; the answer is C2's."""
    msg = bytes.fromhex(C2["msg_hex"])
    with Context(devices=[0] * 8) as c:
        c.set_timing(True)
        assert c.search(msg, C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        st = c.last_stats()
        starts = [st.dev_start_ms[i] for i in range(8)]
        assert st.start_threads == 8 and min(starts) == 0 and max(starts) < 50, starts
        assert all(st.dev_nonces[i] > 0 for i in range(8))


@pytest.mark.parametrize("late", [0, 1])
def test_balance_reacts_to_start_delay(late):
    """bm_ctx_set_balance measures each device's rate from the call's common
    start: with one device's submission held back by 150 ms (test hook), that
    device's share drops well below the other's, its dev_start_ms shows the
    delay, and the answers stay C2's."""
    msg = bytes.fromhex(C2["msg_hex"])
    with Context(devices=[0, 0]) as c:
        c.set_balance(True)
        c.set_test_start_delay(late, 150_000)
        assert c.search(msg, C2["lower"], C2["upper"]) == (C2["hash"], C2["nonce"])
        st = c.last_stats()
        assert st.dev_start_ms[late] >= 140 and st.dev_start_ms[1 - late] == 0, list(st.dev_start_ms[:2])
        sh = c.get_split()
        assert sh[1 - late] == 65536 and sh[late] < 0.75 * 65536, sh
        with pytest.raises(BtcMinerError) as ei:
            c.set_test_start_delay(2, 10)
        assert ei.value.status == BM_EINVAL
        c.set_test_start_delay(late, 0)
        # the delay moves to the other slot: the shares follow it (the weak4
        # range, so even a small piece holds the >= 2^30 nonces a rate is
        # measured on).  (Round 5 checked that, with no delay at all, the late
        # slot's share grows back; two slots on ONE GPU race for its CUs --
        # each launch is a whole resident grid, and whichever slot's launch
        # lands first holds them -- so that direction is not determined here.)
        c.set_test_start_delay(1 - late, 150_000)
        w4 = next(r for r in _scale()["ranges"] if r["name"] == "weak4")
        assert c.search(msg, w4["lower"], w4["upper"]) == (w4["hash"], w4["nonce"])
        sh2 = c.get_split()
        assert sh2[late] == 65536 and sh2[1 - late] < 0.75 * 65536, (sh2, sh)
        c.set_test_start_delay(1 - late, 0)

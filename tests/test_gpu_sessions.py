"""bm_sessions_* on a device table (gfx950): sessions_set_kernel, sessions_tally_kernel
and sessions_retarget_kernel around the verifier's, the share set's and the ledger's
kernels, which read the table through the pointers they always took.  Every step runs
on the device table, on the pure-Python model of tests/sessions_ref.py and on a CPU
table, and everything -- verdicts, results, ledger rows, set counts, the table's
arrays, its states and the change lists -- is compared byte for byte.  The scenarios
are the CPU table's (tests/test_sessions_abi.py); the shapes are small and chosen for
the places the kernels can go wrong: capacity 300 (a partial last wave), slots on both
sides of the wave edges, closed slots in between.

The device is the only place the rule runs in the 64-bit words of bm_sessions_args.hpp
inside a table (the CPU table uses a 128-bit type), and the host rechecks only the
target of a change, never its new difficulty.  So two scenarios aim at it:
* wide_arithmetic pins the kernel's multiply, division, compare and clamps with
  operands of every bit length up to 64 and directed rows at their edges, 48 rounds of
  300 slots, each class of operand counted by the model beforehand;
* dense_changes pins the change list: the rank of lane 63 under a full ballot, the
  wave bases the returning atomic hands out over five waves, `at < cap` with the cap
  at zero, one short and at a wave edge, BM_EFULL leaving every byte alone, and both
  of the host's orderings (18 and 19 entries of 300)."""
import random

import pytest

from distributed_bitcoin_minter_amd import Ledger, SessionTable, ShareSet
import jobs_verify_ref as jref
import ledger_ref as lref
import sessions_ref as sref

pytestmark = pytest.mark.gpu


def device_table(ctx):
    return lambda capacity: SessionTable(ctx, capacity)


def device_ledger(ctx):
    return lambda rows: Ledger(ctx, rows)


def device_set(ctx):
    return lambda capacity: ShareSet(ctx, capacity)


@pytest.mark.parametrize("scenario", [sref.division, sref.division_by_retarget, sref.set_semantics, sref.edge_cases,
                                      sref.burst_and_clock, sref.wide_arithmetic, sref.dense_changes],
                         ids=lambda f: f.__name__)
def test_device_table(gpu_ctx, scenario):
    """The division through set and get and as a retarget's new difficulty, set's
    semantics, the retarget edge cases, BM_EFULL one entry short included, the rule at
    full 64-bit width and the dense change lists."""
    scenario(device_table(gpu_ctx), witness=SessionTable.cpu)


def test_sequence_with_a_cpu_table_as_witness(gpu_ctx):
    """set, verify x3, retarget (one entry short first), verify, retarget, with and
    without a ledger and a set; between the table's calls bm_ledger_verify_jobs on a
    device ledger of the same context still gives a CPU ledger's bytes."""
    rng = random.Random(51)
    jobs, sessions = jref.open_jobs()
    accounts, weights = [0, 1, 2, 1, 0], [rng.getrandbits(64) for _ in range(5)]

    def between():
        subs = [(rng.getrandbits(8), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.randrange(6), i % 3)
                for i in range(70)]
        with Ledger(gpu_ctx, 3) as a, Ledger.cpu(3) as b:
            rc, out, r = lref.raw(a, None, jobs, sessions, subs, accounts, weights)
            rc2, out2, r2 = lref.raw(b, None, jobs, sessions, subs, accounts, weights)
            assert rc == rc2 == 0 and bytes(out) == bytes(out2) and bytes(r) == bytes(r2)
            assert bytes(a.read()) == bytes(b.read()) and r.credited > 0

    sref.sequence(device_table(gpu_ctx), device_ledger(gpu_ctx), device_set(gpu_ctx), SessionTable.cpu, Ledger.cpu,
                  ShareSet.cpu, between)


def test_tally_contention(gpu_ctx):
    """130 copies of one accepted submission on one session, over three waves: with a
    set one tallies, without one all 130 do."""
    sref.contention(device_table(gpu_ctx), device_set(gpu_ctx), SessionTable.cpu, ShareSet.cpu)


def test_refusals_leave_a_device_table_alone(gpu_ctx):
    """BM_EFULL from the set, an account past the ledger's rows, a malformed job, CPU
    objects with a device table, bad policies and ranges: everything is as before."""
    sref.refusals(device_table(gpu_ctx), device_ledger(gpu_ctx), device_set(gpu_ctx), Ledger.cpu, ShareSet.cpu)
    # and device objects with a CPU table
    jobs = (sref.block_job(random.Random(52)),)
    with SessionTable.cpu(2) as table, Ledger(gpu_ctx, 2) as ledger, ShareSet(gpu_ctx, 8) as s:
        table.set([(b"12345678", 1, 0)], 0)
        for led, st in ((ledger, None), (None, s)):
            rc, out, r = sref.raw_verify(table, led, st, jobs, [(1, 2, 3, 4, 0, 0)])
            assert rc == -1 and bytes(out) == b"\xa5" * 80 and bytes(r) == b"\x5a" * 88
        assert s.count == 0 and lref.table(ledger) == [lref.EMPTY] * 2 and table.state()[0].accepted == 0

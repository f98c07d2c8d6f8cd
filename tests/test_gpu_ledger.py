"""bm_ledger_verify_jobs on a device ledger (gfx950): ledger_credit_kernel behind
jobs_verify_kernel and the share set's kernels, against hashlib, a Python set and a
dict of rows (tests/ledger_ref.py), never against the library itself, but where a
test says so: the CPU ledger as a second witness.  Every comparison is exact
equality of every verdict, of the result struct and of every row read back; the
scenarios are the CPU ledger's (tests/test_ledger_abi.py)."""
import random

import pytest

from distributed_bitcoin_minter_amd import Ledger, ShareSet
import jobs_verify_ref as jref
import ledger_ref as lref
import pool_verify_ref as ref

pytestmark = pytest.mark.gpu


def device_ledger(ctx):
    return lambda rows: Ledger(ctx, rows)


def device_set(ctx):
    return lambda capacity: ShareSet(ctx, capacity)


@pytest.mark.parametrize("n", jref.BATCH_SIZES)
def test_batch_sizes(gpu_ctx, n):
    """Around the 64-lane workgroup and beyond one: partial last waves in the ballots."""
    lref.batch_sizes(device_ledger(gpu_ctx), device_set(gpu_ctx), n)


@pytest.mark.parametrize("peel", lref.PEELS)
def test_wave_shapes(gpu_ctx, peel):
    """One row in all 64 lanes, two alternating, 64 distinct, exactly five, 60 lanes
    and four strays, one row over three workgroups: at 0, 1, 4 and 64 peel rounds."""
    lref.wave_shapes(device_ledger(gpu_ctx), device_set(gpu_ctx), peel)


@pytest.mark.parametrize("scenario", [lref.row_mapping, lref.every_class, lref.unknown_sessions, lref.best,
                                      lref.agreement], ids=lambda f: f.__name__)
def test_device_ledger(gpu_ctx, scenario):
    scenario(device_ledger(gpu_ctx), device_set(gpu_ctx))


def test_accumulation_with_a_cpu_ledger_as_witness(gpu_ctx):
    """Three calls of 5,000 submissions over 8 jobs, 500 sessions and 37 accounts,
    with a set and without one: the model's rows, and a CPU ledger's bytes."""
    lref.accumulation(device_ledger(gpu_ctx), device_set(gpu_ctx), witness=Ledger.cpu)


def test_drain_and_clear(gpu_ctx):
    """drain, clear, two ledgers on one context, and other calls on the context in
    between (they share its buffers and stream)."""
    rng = random.Random(41)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, 2)
    sessions = ref.synthetic_sessions(rng, 4)
    big = ref.random_subs(rng, 4, 3000, 7)

    def between():
        verdicts, _ = gpu_ctx.verify_pool_submits(job, ref.session_array(sessions), ref.sub_array(big))
        assert (verdicts[0].value, verdicts[0].status) == ref.verdict(job, sessions, big[0])

    lref.drain_and_clear(device_ledger(gpu_ctx), device_set(gpu_ctx), between)


def test_refusals_leave_a_device_ledger_alone(gpu_ctx):
    """BM_EFULL from a capacity-8 set, an account equal to rows, the identity with
    more sessions than rows, a malformed job, a CPU set with a device ledger, ranges
    past the end and 65 rounds: the ledger is byte-identical after each."""
    lref.refusals(device_ledger(gpu_ctx), device_set(gpu_ctx), foreign_set=ShareSet.cpu)
    # and a device set with a CPU ledger
    jobs, sessions = jref.open_jobs()
    with Ledger.cpu(5) as ledger, ShareSet(gpu_ctx, 8) as s:
        lref.refused(ledger, lref.Model(5), lambda: lref.raw(ledger, s, jobs, sessions, [(1, 2, 3, 4, 0, 0)]))
        assert s.count == 0

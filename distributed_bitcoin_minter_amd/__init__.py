"""MI355X-native nonce search for the 15-440 distributed bitcoin miner.

Hot path: the reference miner's min-scan over bitcoin.Hash
(/root/reference/project2/bitcoin/miner/miner.go:58-65, bitcoin/hash.go:11-15),
re-built as gfx950 HIP kernels behind the C ABI in include/btcminer.h
(libbtcminer.so, built in-tree from csrc/).

    from distributed_bitcoin_minter_amd import Miner, bitcoin
    with Miner() as m:
        print(m.search("bradfitz", 0, 9999))   # (1419516646206828, 9898)
"""
from . import bitcoin, dist
from ._lib import (BM_EFULL, BM_MAX_SHARE_SET, BM_SUBMIT_DUPLICATE, BtcMinerError, Context, HeaderHit, HeaderHitsResult,
                   HeaderVersionHit, HeaderVersionsHitsResult, HeaderVersionsResult, HitsResult, Job, JobShare,
                   JobSharesResult, JobSubmit, JobVerdict, JobVerifyResult, LIB_PATH, PoolSession, PoolSubmit,
                   PoolVerifyResult, ShareSet, ShareSetResult, bits_to_target, device_count, difficulty_to_target,
                   parse_pool_submit, parse_submit, plan_segments, rccl_unique_id, roll_versions, submit_params,
                   verify_pool_submits_cpu, verify_submits_cpu)
from ._lib import BM_MAX_POOL_JOBS, JobsSubmit, PoolJob, parse_jobs_submit, verify_jobs_submits_cpu
from ._lib import BM_MAX_LEDGER_ROWS, Ledger, LedgerResult, LedgerRow
from ._lib import (SessionState, SessionTable, VardiffChange, VardiffPolicy, VardiffResult,
                   difficulty_fx_to_target)
from .miner import Miner

__all__ = ["bitcoin", "dist", "Miner", "Context", "BtcMinerError", "HeaderHit", "HeaderHitsResult",
           "HeaderVersionHit", "HeaderVersionsHitsResult", "HeaderVersionsResult", "HitsResult", "Job", "JobShare",
           "JobSharesResult", "JobSubmit", "JobVerdict", "JobVerifyResult", "LIB_PATH", "bits_to_target", "device_count",
           "difficulty_to_target", "parse_submit", "plan_segments", "rccl_unique_id", "roll_versions", "submit_params",
           "verify_submits_cpu", "PoolSession", "PoolSubmit", "PoolVerifyResult", "parse_pool_submit",
           "verify_pool_submits_cpu", "ShareSet", "ShareSetResult", "BM_SUBMIT_DUPLICATE", "BM_EFULL",
           "BM_MAX_SHARE_SET", "PoolJob", "JobsSubmit", "parse_jobs_submit", "verify_jobs_submits_cpu",
           "BM_MAX_POOL_JOBS", "Ledger", "LedgerRow", "LedgerResult", "BM_MAX_LEDGER_ROWS",
           "SessionTable", "SessionState", "VardiffPolicy", "VardiffChange", "VardiffResult", "difficulty_fx_to_target"]

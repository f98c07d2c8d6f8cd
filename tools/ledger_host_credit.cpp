// ledger_host_credit.cpp -- measurement only (tools/bench_ledger.py builds it into a
// shared object of its own): the library's CPU crediting loop
// (csrc/bm_ledger_host.hpp, host::ledger_credit_row -- what bm_ledger_verify_jobs runs
// on a CPU ledger after verification) over verdicts that bm_share_set_verify_jobs
// returned, on the calling thread.  This is what a caller without a device ledger
// does after every call.
#include "bm_ledger_host.hpp"

extern "C" void bench_ledger_credit(const bm_jobs_submit_t* submits, const bm_job_verdict_t* verdicts, size_t n,
                                    size_t nsessions, const uint32_t* accounts, const uint64_t* weights,
                                    bm_ledger_row_t* rows) {
    for (size_t i = 0; i < n; ++i) {
        const uint32_t s = submits[i].session;
        if (s >= nsessions) continue;
        bm::host::ledger_credit_row(rows[accounts[s]], verdicts[i], weights[s]);
    }
}

// bm_ledger_args.hpp -- what the ledger's kernels (bm_ledger.hpp), their launcher
// (bm_aux.hip) and the CPU ledger (bm_ledger.cpp) agree on: the classes of a
// submission, the words of a row, the control words of a call and the kernels'
// argument block.  Plain C++: no HIP in here.
#pragma once
#include <cstdint>

#include "bm_sha256.hpp"  // BM_HD
#include "btcminer.h"

namespace bm {

constexpr int kLedgerThreads = 64;  // one wave: the credit kernel's ballots cover the workgroup
constexpr int kLedgerFillThreads = 256;
constexpr uint32_t kLedgerMaxPeel = 64;
constexpr uint32_t kLedgerDefaultPeel = 64;  // measured: DESIGN.md section 4, "Share accounting"

// The words of a row (bm_ledger_row_t) and, the first seven, the control words of a
// call (zeroed by the host's copy up): this call's totals over all rows.
constexpr int kLedgerAccepted = 0;
constexpr int kLedgerBlocks = 1;
constexpr int kLedgerAbove = 2;
constexpr int kLedgerNtime = 3;
constexpr int kLedgerDuplicates = 4;
constexpr int kLedgerInvalid = 5;
constexpr int kLedgerWork = 6;
constexpr int kLedgerBest = 7;
constexpr int kLedgerRowWords = 8;
constexpr int kLedgerCtlWords = 7;
constexpr int kLedgerCtlUnits = 8;  // staged: the seven and one word of padding
constexpr uint64_t kLedgerNoBest = ~0ull;
static_assert(sizeof(bm_ledger_row_t) == 8 * kLedgerRowWords, "row layout");

// The class of a submission of a known session, by its final status: the first rule
// that applies decides.  The result is the row word that grows by one.
BM_HD inline int ledger_class(uint32_t status) {
    if (status & BM_SUBMIT_INVALID) return kLedgerInvalid;
    if (status & BM_SUBMIT_NTIME) return kLedgerNtime;
    if (status & BM_SUBMIT_DUPLICATE) return kLedgerDuplicates;
    if (status & (BM_SUBMIT_SHARE | BM_SUBMIT_BLOCK)) return kLedgerAccepted;
    return kLedgerAbove;
}

// Kernel argument of ledger_credit_kernel, by value (SGPRs).
struct LedgerArgs {
    uint32_t n;          // staged records
    uint32_t nsessions;  // entries of accounts[] and weights[]
    uint32_t rows;       // rows of the ledger
    uint32_t rounds;     // peel rounds, 0..64
};

}  // namespace bm

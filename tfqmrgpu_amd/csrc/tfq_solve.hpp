// What tfq_api.hip (the C-ABI) and tfq_solve.cpp (the host side of the solver) share: the entry points of the solve that the ABI
// calls, and the status check of runtime calls that both use.
#pragma once
#include "tfq_device.hpp"

namespace tfq {

// ---- RCCL, loaded on first use so that single-GPU callers carry no dependency -------------------
struct UidByValue { char internal[128]; };   // ncclUniqueId
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, UidByValue, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllReduce)(void const*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    bool load();
};

#pragma GCC visibility push(hidden)   // what follows is shared by two files of the library and no part of its symbol list

static inline tfqmrgpuStatus_t hipCheck(hipError_t e, int code, int line) {
    return (hipSuccess == e) ? TFQMRGPU_STATUS_SUCCESS : err(code, line % 10000);
}
#define TFQ_HIP(call, code) { auto const st_ = ::tfq::hipCheck((call), (code), __LINE__); if (st_) return st_; }

// one solve of the plan: tfQMR in the plan's precision, or the refinement around float solves for 'm'
tfqmrgpuStatus_t run_solve(Handle& h, Plan& p, double tol, int maxIt);

// small systems: the column operations and the decisions run in the producers' tails (tfq_colops.hpp).  One rank, built-in operator:
// a reduction over ranks or a foreign multiply sits between the producer and the decision otherwise
inline bool several_ranks(Handle const& h) { return h.comm != nullptr || h.reduceFn != nullptr; }
inline bool folds(Plan const& p, bool severalRanks) { return p.foldOk && !severalRanks && !p.opFn; }

// ---- block-Jacobi right preconditioner: the library-owned memory of a plan, and what a solve needs before its first iteration
struct PrecondMem { char* minv; uint32_t* diag; uint32_t* colA; uint32_t* counter; uint32_t* identity; size_t minvBytes, bytes; };
PrecondMem precond_mem(Plan const& p);
tfqmrgpuStatus_t precond_prepare(Handle& h, Plan& p);

// ---- the kept copy of the caller's A (tfqmrgpu_ext.h section 9): Plan::aKept holds the A window of the buffer, for 'm' the double A
// (`a`) followed by the float A (`aFloat`)
struct KeptA { char* a; char* aFloat; size_t aBytes, aFloatBytes, bytes; };
KeptA kept_a(Plan const& p);
inline bool kept_is_callers_a(Plan const& p) { return p.keepA && p.aKept && TFQMRGPU_PRECOND_NONE != p.precondInA; }
void forget_dirty(Plan& p);            // a whole new A, or the set-up has caught up
void release_kept(Plan& p);            // the copy goes (bufferSize, setBuffer, keepOperator(0), destroyPlan)

extern Rccl g_rccl;

// the device buffer of the collective in front of every solve: allocated with the communicator / the reduce callback, because a rank
// that failed to allocate it in the solve would leave before the collective and its peers would wait for ever (run_tfqmr)
tfqmrgpuStatus_t ensure_vote_buffer(Handle& h);

#pragma GCC visibility pop
} // namespace tfq

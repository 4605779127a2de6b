// What tfq_api.hip (the C-ABI), tfq_solve.cpp (the host side of the solver) and tfq_precond_host.cpp (that of the preconditioner) share:
// the entry points of the solve that the ABI calls, and the status check of runtime calls that all three use.
#pragma once
#include "tfq_device.hpp"
#include "tfq_vec.hpp"

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

#pragma GCC visibility push(hidden)   // what follows is shared by files of the library and no part of its symbol list

static inline tfqmrgpuStatus_t hipCheck(hipError_t e, int code, int line) {
    return (hipSuccess == e) ? TFQMRGPU_STATUS_SUCCESS : err(code, line % 10000);
}
#define TFQ_HIP(call, code) { auto const st_ = ::tfq::hipCheck((call), (code), __LINE__); if (st_) return st_; }

// one solve of the plan: tfQMR in the plan's precision, or the refinement around float solves for 'm'
tfqmrgpuStatus_t run_solve(Handle& h, Plan& p, double tol, int maxIt);

// the same from the X in the plan (tfqmrgpu_ext.h section 14): R = B - A X0 with the caller's A (`callersA`: tfq_grade_host.cpp, callers_a), the
// tfQMR driver on A D = R, X = X0 + D.  `early`: a refusal the ABI's checks have found already; several ranks are refused here -- either
// travels through the ranks' vote like every refusal of a solve
tfqmrgpuStatus_t run_solve_from(Handle& h, Plan& p, double tol, int maxIt, void const* callersA, tfqmrgpuStatus_t early);

// the same on an 'm' plan (tfqmrgpu_ext.h section 16): R in double from the caller's double A, the refinement of the mixed solve on A D = R,
// X = X0 + D in double.  Several ranks are refused through the mixed solve's own first collective (three doubles, the third one set)
tfqmrgpuStatus_t run_refine_from(Handle& h, Plan& p, double tol, int maxIt, void const* callersA, tfqmrgpuStatus_t early);

// small systems: the column operations and the decisions run in the producers' tails (tfq_colops.hpp).  One rank, built-in operator:
// a reduction over ranks or a foreign multiply sits between the producer and the decision otherwise
inline bool several_ranks(Handle const& h) { return h.comm != nullptr || h.reduceFn != nullptr; }
inline bool folds(Plan const& p, bool severalRanks) { return p.foldOk && !severalRanks && !p.opFn; }
// the "late v5" form of the iteration slot (DevPlan::lateV5): k_v5_nrm stores nothing and the second fused multiply applies its half step.  Built-in
// operator (the epilogue of a foreign product is k_spmm_direct's), no fold (a folded k_v5_nrm hands its sum to the column operation in its own tail,
// and the slot of a small system is launch latency, not bytes), fused multiplies on k_spmm_ilv16 (d: the plan as resolved, d.fold as the solve
// sets it).  One rank or several: a plan that does not fold on one rank takes the same slot on several.  Nothing reads v5 between the two kernels -- decT and k_x_v6_v7 do not, a reduction over ranks moves control records only, the
// probe, the warm start, the start projection and the refinement's set-up run in front of a solve or behind the second multiply -- and the two gate off
// together: the control block's state changes only in the decisions behind the second multiply
inline bool late_v5(Plan const& p, DevPlan const& d) { return !p.opFn && !d.fold && spmm_late_v5(d); }

extern Rccl g_rccl;

// the device buffer of the collective in front of every solve: allocated with the communicator / the reduce callback, because a rank
// that failed to allocate it in the solve would leave before the collective and its peers would wait for ever (run_tfqmr)
tfqmrgpuStatus_t ensure_vote_buffer(Handle& h);

#pragma GCC visibility pop
} // namespace tfq

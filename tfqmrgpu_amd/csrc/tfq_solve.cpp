// Host side of the solver: the tfQMR driver (run_tfqmr), the mixed-precision refinement around it (run_mixed), the RCCL and roctx loaders
// and the flop model.  No kernel lives here; tfq_api.hip is the C-ABI in front, tfq_precond_host.cpp the preconditioner's set-up.
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <new>
#include <vector>
#include <dlfcn.h>

#include "tfq_solve.hpp"
#include "tfq_vec.hpp"
#include "tfq_switch.hpp"
#include "tfq_precond.hpp"

namespace tfq {

Rccl g_rccl;
bool Rccl::load() {
    if (lib) return true;
    for (char const* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    if (!lib) return false;
    GetUniqueId  = (decltype(GetUniqueId)) dlsym(lib, "ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
    CommDestroy  = (decltype(CommDestroy)) dlsym(lib, "ncclCommDestroy");
    AllReduce    = (decltype(AllReduce))   dlsym(lib, "ncclAllReduce");
    return GetUniqueId && CommInitRank && CommDestroy && AllReduce;
}
enum { kNcclDouble = 8, kNcclMax = 2 };

// max-reduce n doubles of device memory over all ranks (in place, on the solver's stream)
static tfqmrgpuStatus_t reduce_over_ranks(Handle& h, double* red, int n, hipStream_t s) {
    if (h.comm) {
        int const rc = g_rccl.AllReduce(red, red, size_t(n), kNcclDouble, kNcclMax, h.comm, s);
        return rc ? TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED) : TFQMRGPU_STATUS_SUCCESS;
    }
    if (h.reduceFn) {
        double v[4];
        TFQ_HIP(hipMemcpyAsync(v, red, n * sizeof(double), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        h.reduceFn(h.reduceCtx, v, n);
        TFQ_HIP(hipMemcpyAsync(red, v, n * sizeof(double), hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    }
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t ensure_vote_buffer(Handle& h) {
    return h.voteBuf.reserve(4 * sizeof(double));
}

// the mark "this rank has failed" in a record that is about to be max-reduced: a pageable source the device may read at any later time
static double const kOne = 1.;

// HIP events that are destroyed on every path out of a solve
struct EventList {
    std::vector<hipEvent_t> v;
    bool create(size_t n) {
        v.reserve(n);
        for (size_t i = 0; i < n; ++i) { hipEvent_t e; if (hipSuccess != hipEventCreate(&e)) return false; v.push_back(e); }
        return true;
    }
    ~EventList() { for (auto e : v) (void)hipEventDestroy(e); }
    hipEvent_t operator[](size_t i) const { return v[i]; }
};

// ---- the tfQMR driver -----------------------------------------------------------------------------
// Optional roctx ranges around the two phases of a solve, named like the reference's NVTX ranges (tfqmrgpu_core.hxx:29,
// 176-177,332; there compiled in with -DUSE_NVTX, here switched on with TFQMRGPU_ROCTX=1: libroctx64 is loaded on demand so
// that the library carries no dependency on the tracing runtime).  rocprofv3 --marker-trace shows them.
struct Roctx {
    int (*push)(char const*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        auto const v = std::getenv("TFQMRGPU_ROCTX");
        if (!v || 0 == std::atoi(v)) return;
        // the rocprofiler-sdk flavour: it is the one rocprofv3 listens to (a run that loaded the legacy libroctx64 under
        // rocprofv3 recorded no ranges and did not exit)
        for (char const* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1"}) {
            if (void* lib = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
                push = (decltype(push))dlsym(lib, "roctxRangePushA");
                pop = (decltype(pop))dlsym(lib, "roctxRangePop");
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
struct RoctxRange {
    Roctx const& r;
    RoctxRange(Roctx const& r_, char const* name) : r(r_) { if (r.push) (void)r.push(name); }
    ~RoctxRange() { if (r.pop) (void)r.pop(); }
};
static Roctx const& roctx() { static Roctx const r; return r; }

// Algorithm = reference tfqmrgpu::solve (tfqmrgpu_core.hxx:179-306), restructured:
//   dec35 | v6 | SpMM+v4+dot | dec34 | v5,nrm | decT | x,v7,v6,v7 | SpMM+v5+nrm+dot | decT | decide
//   [ | x | SpMM residual | column records | decide ]   <- only does work when the bound asks for a probe
// The host never waits for the iteration it has just enqueued: it keeps DEPTH iterations in flight
// and reads the control block of iteration `it` (copied to pinned memory behind it) before it
// enqueues iteration it+DEPTH.  Iterations enqueued after the solve has stopped cost a few empty
// launches.  Every rank enqueues the same number of iterations, so collectives always match.
namespace {   // the driver: nothing of it is seen outside this file but run_tfqmr
struct SolveOutcome { Ctl last; double userFlops = 0; };
constexpr int DEPTH = Plan::kDepth;
constexpr int NK = TFQMRGPU_PROFILE_CLASSES;

// One collective in front of every solve of several ranks: {deepest queue any rank wants, some rank cannot start}.  Every rank must
// enqueue the same number of slots (the collectives have to match), and a rank that returned here on its own would
// leave its peers waiting in their first all-reduce for ever -- so the refusal travels through the same reduction.
// (the buffer of the vote is allocated with the communicator / callback, tfqmrgpuExt_commInit: a rank that failed to
//  allocate it HERE would leave before the collective and its peers would wait for ever)
// `early`: a refusal the caller has found already; returns it, or a peer's, or 0 with the queue depth every rank uses in `ahead`.
tfqmrgpuStatus_t vote(Handle& h, hipStream_t s, tfqmrgpuStatus_t early, int& ahead) {
    if (!several_ranks(h)) return early;
    if (!h.voteBuf) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    double ballot[2] = { double(ahead), early ? 1. : 0. };
    double* const buf = h.voteBuf.as<double>();
    TFQ_HIP(hipMemcpyAsync(buf, ballot, sizeof ballot, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (auto const st = reduce_over_ranks(h, buf, 2, s)) return st;
    TFQ_HIP(hipMemcpyAsync(ballot, buf, sizeof ballot, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    ahead = std::min(DEPTH, std::max(1, int(ballot[0])));
    if (!early && ballot[1] > 0.) early = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);   // a peer cannot start: nobody does
    return early;
}

// user-defined operator (tfqmrgpu_ext.h section 5): the plan's scratch [xu | yu | i2u | colindx in the caller's block order]
struct OpScratch { char* xu; char* yu; uint32_t* i2u; uint16_t* colU; };
size_t op_vector_bytes(Plan const& p) { return align256(size_t(p.nnzbX) * 2 * p.LM * p.LN * ('z' == p.precision ? 8 : 4)); }
size_t op_scratch_bytes(Plan const& p) { return 2 * op_vector_bytes(p) + align256(size_t(p.nnzbX) * 4) + align256(size_t(p.nnzbX) * 2); }
OpScratch op_scratch(Plan const& p) {       // the pieces of Plan::layout.opScratch (allocated)
    char* const b = p.layout.opScratch.as<char>();
    size_t const v = op_vector_bytes(p);
    return { b, b + v, (uint32_t*)(b + 2 * v), (uint16_t*)(b + 2 * v + align256(size_t(p.nnzbX) * 4)) };
}
tfqmrgpuStatus_t ensure_op_scratch(Plan& p, hipStream_t s) {
    if (p.layout.opScratch) return TFQMRGPU_STATUS_SUCCESS;
    if (auto const st = p.layout.opScratch.reserve(std::max<size_t>(op_scratch_bytes(p), 256))) return st;
    auto const o = op_scratch(p);
    std::vector<uint16_t> cu(p.nnzbX);      // compressed block column per block, caller's order
    for (uint32_t u = 0; u < p.nnzbX; ++u) cu[u] = p.colindx[u];
    TFQ_HIP(hipMemcpyAsync(o.i2u, p.i2u.data(), size_t(p.nnzbX) * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipMemcpyAsync(o.colU, cu.data(), size_t(p.nnzbX) * 2, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)   // cu goes out of scope
    return TFQMRGPU_STATUS_SUCCESS;
}

// what the launches of an iteration slot found: work, the work of the first iteration, the solve already stopped
enum class Found { Work, FirstWork, Stopped };

// The slots of one solve: what is enqueued per iteration, how its control block comes back, what the profile makes of it.
struct Slots {
    Handle& h; Plan& p; hipStream_t const s;
    bool const multi;                    // several ranks: a reduction sits in front of every decision
    bool const fold;
    DevPlan d, dFirst;                   // the plan's device pointers (d.R set: the right-hand side is the X-shaped vector R and the per-RHS scalars
                                         // have been set up by the refinement, tfq_vec.hip); dFirst: with the first-iteration flag
    OpScratch op{};
    double const histScale;              // every bound of the history is multiplied by it (a refinement cycle's bounds are relative to ITS right-hand side)
    int const prof;
    EventList pev;                       // profiling: NK+1 timing events per in-flight iteration, event k sits in front of kernel class k
    tfqmrgpuStatus_t fail = TFQMRGPU_STATUS_SUCCESS;   // the first failure of this rank
    double userFlops = 0;
    Ctl last{};                          // the latest control block the host has read
    int enq = 0, seen = 0;               // slots enqueued / read back
    int probesAccounted = 0;             // last.nprobes at the previous account()

    Slots(Handle& h_, Plan& p_, int maxIt, double histScale_)
        : h(h_), p(p_), s((hipStream_t)h_.stream), multi(several_ranks(h_)), fold(folds(p_, multi)), d(resolve(p_)),
          histScale(histScale_), prof(p_.profiling)
    {
        d.fold = fold ? 1 : 0;
        d.lateV5 = late_v5(p, d) ? 1 : 0;   // (in front of the copies: dFirst and, folded, the device-resident one of refresh_self see the flag)
        dFirst = d; dFirst.first = 1;
        if (p.opFn) op = op_scratch(p);
        last.state = (maxIt > 0) ? 0 : 3; last.residual2_reached = 1e300; last.iterations_needed = maxIt;
    }
    Ctl* ring() const { return (Ctl*)p.ring.ptr; }
    hipEvent_t ringEvent(int slot) const { return p.ring.event[slot]; }

    // the device-resident copy that the folded column operations read: taken again whenever a plan flag has changed since the last
    // one (hashV3, m3: setShadowVector / setShadowMode / setThreeProductMultiply; the copy of setBuffer predates the shadow vector),
    // so that device code never sees a flag that the host's DevPlan does not have
    tfqmrgpuStatus_t refresh_self() {
        if (!fold || !p.selfStale) return TFQMRGPU_STATUS_SUCCESS;
        TFQ_HIP(hipMemcpyAsync((void*)d.self, &d, sizeof d, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        p.selfStale = false;
        return TFQMRGPU_STATUS_SUCCESS;
    }

    // level 2: only the fused multiplies are bracketed (class k needs events k and k + 1)
    bool timed(int k) const { return 1 == prof || (2 == prof && (TFQMRGPU_PROF_SPMM_V4_DOT == k || TFQMRGPU_PROF_SPMM_V5_NRM_DOT == k)); }
    void mark(int slot, int k) {
        if (!(k < NK && timed(k)) && !(k > 0 && timed(k - 1))) return;
        if (hipSuccess != hipEventRecord(pev[slot * (NK + 1) + k], s) && !fail) fail = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
    }

    // Y = A*X with a fused epilogue.  User-defined operator: gather the operand into the caller's block order,
    // let the callback enqueue Y = A*X, apply the fused epilogue to the product
    void multiply(int epi, DevPlan const& dS) {     // dS: the plan with the first-iteration flag of the slot
        if (!p.opFn) { spmm_launch(epi, dS, s); return; }
        launch_convert(1, dS.dbl, dS.dbl, (EPI_RESIDUAL == epi) ? dS.x : dS.v6, op.xu, dS.u2i, 0, p.nnzbX, p.LM, p.LN,
                       TFQMRGPU_LAYOUT_RRRRIIII, false, false, p.ilv, s);
        double fl = 0;
        auto const st = ((tfqmrgpuOperator_t)p.opFn)(p.opCtx, op.yu, op.xu, op.colU, p.nnzbX, p.nCols, p.LM, p.LN, p.precision, (tfqmrgpuStream_t)s, &fl);
        if (st && !fail) fail = st;   // the slot is completed all the same: its reduction tells the other ranks
        userFlops += fl;
        epilogue_launch(epi, dS, op.yu, op.i2u, s);
    }

    // the max-reduction of a slot; a rank that has failed marks the record, so that every rank stops at THAT slot (the failing rank
    // goes on completing slots until then, see run_ahead(); a rank whose device is lost cannot, its peers then wait in RCCL)
    void reduce(int what) {
        if (fail && hipSuccess != hipMemcpyAsync(&d.ctl->red[3 * what + 2], &kOne, sizeof kOne, hipMemcpyHostToDevice, s)) return;
        auto const st = reduce_over_ranks(h, &d.ctl->red[3 * what], 3, s);
        if (st && !fail) fail = st;
    }

    // the kernels of one iteration (most of them gate themselves off when the solve has stopped)
    void iteration_part(int slot, bool first) {
        DevPlan const& dS = first ? dFirst : d;
        mark(slot, TFQMRGPU_PROF_DEC35);            (void)vec_launch(VEC_DEC35, d, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_XPAY_V6);          (void)vec_launch(VEC_XPAY_V6, dS, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_SPMM_V4_DOT);      multiply(EPI_XPAY_DOT, dS);
        // (fold: dec34, decT, decT + decide and the probe's column records + decision run in the tails of the kernels in front of them)
        mark(slot, TFQMRGPU_PROF_DEC34);            if (!fold) (void)vec_launch(VEC_DEC34, d, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_V5_NRM);           (void)vec_launch(VEC_V5_NRM, dS, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_DECT_C67);         if (!fold) (void)vec_launch(VEC_DECT_C67, d, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_X_V6_V7);          (void)vec_launch(VEC_X_V6_V7, dS, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_SPMM_V5_NRM_DOT);  multiply(EPI_AXPY_NRM_DOT, dS);
        mark(slot, TFQMRGPU_PROF_DECT_FINAL);       if (!fold) (void)vec_launch(VEC_DECT_FIN, d, 0, 0, s);
        mark(slot, TFQMRGPU_PROF_DECIDE);
        if (multi) {
            launch_decide(d, 1, s);
            reduce(0);
            launch_decide(d, 2, s);
        } else if (!fold) launch_decide(d, 0, s);
        mark(slot, TFQMRGPU_PROF_PROBE);
    }
    // the true residual: only does work when the decision in front of it has asked for a probe
    void probe_part(bool first) {
        (void)vec_launch(VEC_X_FLUSH, d, 0, 0, s);
        multiply(EPI_RESIDUAL, first ? dFirst : d);
        if (!fold) (void)vec_launch(VEC_PROBE_COL, d, 0, 0, s);
        if (multi) {
            launch_probe_decide(d, 1, s);
            reduce(1);
            launch_probe_decide(d, 2, s);
        } else if (!fold) launch_probe_decide(d, 0, s);
    }
    // behind the part(s) of a slot: the control block travels to the slot's place in the pinned ring
    void close(int slot) {
        mark(slot, NK);
        // a copy that did not start would be read as a stale "still running": both calls are checked
        if ((hipSuccess != hipMemcpyAsync(&ring()[slot], d.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s) ||
             hipSuccess != hipEventRecord(ringEvent(slot), s)) && !fail) fail = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
    }
    void enqueue(int slot, bool first) { iteration_part(slot, first); probe_part(first); close(slot); }

    // wait for a slot and read its control block; `iteration`: an iteration part ran in it, its bound joins the history.
    // false: the device is gone
    bool harvest(int slot, bool iteration = true) {
        if (hipSuccess != hipEventSynchronize(ringEvent(slot))) { if (!fail) fail = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED); return false; }
        last = ring()[slot];
        if (iteration) p.last.boundHistory.push_back(last.max_bound2 * histScale);
        return true;
    }

    // the profile of a slot that has been harvested (Found::Stopped: that has completed).  Launches that returned at once are counted
    // apart: all of a slot that found the solve stopped, and the probe's when the iteration in front of it asked for none
    void account(int slot, Found found) {
        if (!prof) return;
        bool const probed = (last.nprobes != probesAccounted);
        probesAccounted = last.nprobes;
        for (int k = 0; k < NK; ++k) {
            float ms = 0;
            if (!timed(k) || hipSuccess != hipEventElapsedTime(&ms, pev[slot * (NK + 1) + k], pev[slot * (NK + 1) + k + 1])) continue;
            if (Found::Stopped == found || (TFQMRGPU_PROF_PROBE == k && !probed)) { p.last.gated.ms[k] += ms; p.last.gated.launches[k] += 1; continue; }
            p.last.all.ms[k] += ms; p.last.all.launches[k] += 1;
            if (Found::FirstWork == found) { p.last.first.ms[k] += ms; p.last.first.launches[k] += 1; }
        }
    }

    // built-in operator: the host runs `ahead` slots in front of the decisions it reads
    void run_ahead(int ahead, int maxIt) {
        for (; enq < std::min(ahead, maxIt); ++enq) enqueue(enq % DEPTH, 0 == enq);   // slot n runs iteration n (or nothing)
        // A rank that has failed on the way (fail != 0) does not leave on its own when there are peers: they have slots with
        // collectives enqueued ahead, which it must match.  It keeps completing slots -- reduce() marks every one of its records -- until
        // the control block shows state 4 (every rank stops at the slot whose reduction carried the mark) or the iterations run out.
        while (seen < enq && (!fail || multi)) {
            int const slot = seen % DEPTH;
            if (!harvest(slot)) break;   // nothing left to match
            ++seen;
            account(slot, (1 == seen) ? Found::FirstWork : Found::Work);
            if (last.state != 0) break;
            if (enq < maxIt) { enqueue(enq % DEPTH, false); ++enq; }
        }
    }
    // user-defined operator: the callback's kernels cannot look at the control block, so nothing is enqueued ahead of a decision:
    // one host round trip per iteration (and one per probe), like the reference (tfqmrgpu_core.hxx:235-304)
    void round_trips(int maxIt) {
        for (int it = 0; it < maxIt && !fail && 0 == last.state; ++it) {
            bool const first = (0 == it);
            iteration_part(0, first); close(0);      // (a failing operator still completes its slot: see reduce())
            if (harvest(0) && !fail && 0 == last.state && last.probe) { probe_part(first); close(0); (void)harvest(0, false); }
            account(0, first ? Found::FirstWork : Found::Work);
        }
    }

    tfqmrgpuStatus_t verdict(SolveOutcome& out) {
        (void)hipStreamSynchronize(s);
        // iterations that were enqueued ahead and found the solve finished: their launches return at once
        for (; seen < enq; ++seen) account(seen % DEPTH, Found::Stopped);
        if (hipSuccess != hipGetLastError() && !fail) fail = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
        if (fail) return fail;
        if (4 == last.state) return TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);   // another rank reported a failure; all ranks stopped at the same slot
        out.last = last; out.userFlops = userFlops;
        return TFQMRGPU_STATUS_SUCCESS;
    }
};
} // namespace

// One tfQMR solve on the plan's buffer.  `early`: a refusal the caller has found already (it still has to travel through the ranks' vote;
// the plan is not looked at before the vote has passed, so a plan without a buffer can take part in it).
static tfqmrgpuStatus_t run_tfqmr(Handle& h, Plan& p, double tol, int maxIt, tfqmrgpuStatus_t early, double histScale, SolveOutcome& out) {
    hipStream_t const s = (hipStream_t)h.stream;
    // How far the host runs ahead: 2 slots.  Every slot that is still queued when the solve stops costs ~14 empty
    // launches, and enqueuing a slot (~50 us) is never slower than executing one (>= 60 us even for tiny systems), so a
    // deeper queue only adds to the tail (measured: 4 -> 2 gains 8 % on the 2-iteration solves of config 3, 5 % on
    // 1000-block systems, 0.8 % on P2; 1 loses on small systems).  TFQMRGPU_DEPTH = 1..4 overrides.
    static int const depthEnv = lab_switch("TFQMRGPU_DEPTH", 0);
    int ahead = (depthEnv >= 1 && depthEnv <= DEPTH) ? depthEnv : 2;
    if (auto const st = vote(h, s, early, ahead)) return st;

    if (auto const st = p.ring.ensure(sizeof(Ctl))) return st;
    if (p.opFn) if (auto const st = ensure_op_scratch(p, s)) return st;
    Slots run(h, p, maxIt, histScale);
    if (auto const st = run.refresh_self()) return st;
    if (run.prof && !run.pev.create(size_t(DEPTH) * (NK + 1))) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);

    { RoctxRange const range(roctx(), "tfQMR preparation"); TFQ_HIP(vec_launch(VEC_SETUP, run.d, tol, maxIt, s), TFQMRGPU_STATUS_LAUNCH_FAILED) }
    RoctxRange const range(roctx(), "tfQMR iterations");

    if (p.opFn) run.round_trips(maxIt); else run.run_ahead(ahead, maxIt);
    return run.verdict(out);
}

// flop model of the reference: tfqmrgpu_linalg.hxx:587,625,684,703 and tfqmrgpu_blocksparse.hxx:198
struct FlopModel {
    double fMult, fDot, fNrm, fAxp;
    explicit FlopModel(Plan const& p) {
        double const blk = double(p.LM) * p.LN, nX = p.nnzbX;
        fMult = double(p.nPairs()) * 8. * p.LM * blk; fDot = nX * 8. * blk; fNrm = nX * 4. * blk; fAxp = nX * 8. * blk;
    }
    double solve(Ctl const& c) const { return fNrm + c.iteration * (2 * fMult + 2 * fDot + 2 * fNrm + 10 * fAxp) + c.nprobes * (fMult + fNrm); }
};

// What a refinement cycle asks of its float solve (host arithmetic only; every rank computes the same values from the same reduced residual).
// tol: the refinement's threshold, res2: the double residual^2 in front of this cycle, bestGain / lastGain: the factor the best / the last
// cycle delivered (1: none yet), lastIts: the float iterations of the last cycle, itsLeft: what maxIterations leaves, mixedFloor: Plan::mixedFloor
struct CycleAsk { double innerTol; int innerIts; bool predicted; };
static CycleAsk next_cycle(double tol, double res2, int cycle, double bestGain, double lastGain, int lastIts, int itsLeft, double mixedFloor) {
    // what a float solve is asked for per cycle: a quarter of what is missing, but not more digits than float iterations deliver; a solve
    // that reaches its floor earlier ends itself (Ctl::stallStop) and the next cycle continues from the double residual
    double const kInnerFloor = 3e-5;
    // What this cycle is asked for.  The first cycle: a quarter of what is missing -- the floor of a float solve is not known beforehand (2.4e-4 on
    // P2, 2.4e-7 on a 32 x 32 stencil); a solve that reaches it ends itself (Ctl::stallStop) at the price of 2-3 iterations.  Later cycles know
    // what a cycle has delivered (bestGain): if what is missing is more than that, it is split evenly over the cycles it will take anyway, so
    // that none of them runs into its floor (P2: 9 + 9 + 5 -> 9 + 6 + 5 float iterations); systems whose first cycle delivers nearly everything keep
    // their two cycles.  Lab builds: TFQMRGPU_MIXED_SPLIT=0 a quarter of what is missing in every cycle, =2 an even split into cycles of at
    // most 3 digits from the first cycle on (P2: 7 + 7 + 5, but fast-converging systems then take three cycles: profiles/r03_mixed_policy.txt).
    static int const splitEnv = lab_switch("TFQMRGPU_MIXED_SPLIT", 1);
    double const need = tol / std::sqrt(res2);                                   // the factor still to gain, < 1
    double ask = 0.25 * need;
    if (2 == splitEnv) {
        int const n = std::max(1, int(std::ceil(-std::log10(need) / 3.0)));
        if (n > 1) ask = std::pow(need, 1. / n); else ask = 0.5 * need;
    } else if (1 == splitEnv && cycle > 0 && bestGain < 1.) {
        double const cap = std::min(0.5, 2. * bestGain);                         // what a cycle delivers without searching for its floor
        int const n = std::max(1, int(std::ceil(std::log(need) / std::log(cap))));
        if (n > 1) ask = std::pow(need, 1. / n);
    }
    static int const floorEnv = lab_switch("TFQMRGPU_MIXED_FLOOR", 1), predictEnv = lab_switch("TFQMRGPU_MIXED_PREDICT", 1);
    if (0 == cycle && floorEnv && mixedFloor > 0.) ask = std::max(ask, 2. * mixedFloor);   // (twice the floor: the last iterations in front of a floor are its slowest)
    // (r04) a LAST cycle that has less than two digits to gain does not search: the previous cycle's rate per iteration says how many iterations
    // that takes (+ 1), the float solve runs them without a probe of its own -- the refinement's residual in double decides anyway -- and stops
    // (P2's third cycle: 5 iterations and three float probes for a factor 4 -> 3 iterations and the one probe at the end)
    CycleAsk a{ 0., itsLeft, false };
    if (predictEnv && cycle > 0 && need >= 0.01 && lastIts > 0 && lastGain < 0.5) {
        double const rate = std::pow(lastGain, 1. / lastIts);
        int const want = int(std::ceil(std::log(0.5 * need) / std::log(rate))) + 1;
        a.innerIts = std::min(a.innerIts, std::max(2, std::min(want, lastIts)));
        ask = 0.5 * need;
        a.predicted = true;
    }
    a.innerTol = std::min(0.5, std::max(kInnerFloor, ask));
    return a;
}

// Mixed precision 'm' (reference: dormant, tfqmrgpu.cu:42 "load float, multiply-accumulate double, store float"; documented as
// "start with float and converge double", tfqmrgpu.h:72).  Iterative refinement: x, B, A in double; per cycle r = b - A x in double,
// A d = r solved by the complex<float> tfQMR (its kernels unchanged; the right-hand side is the X-shaped R), x += d in double.  The
// float iteration moves half the bytes of the double one; a cycle gains the digits a float solve delivers, the refinement's own
// stopping test is max_rhs |b - A x| / |b| <= threshold in double.  maxIterations bounds the SUM of the inner iterations.
// ONE failure protocol for several ranks: the first collective of a mixed-precision solve is the refinement's
// max-reduction of {max |r|^2/|b|^2, a value is not finite, a rank failed} (3 doubles) -- not the vote of run_tfqmr (2 doubles).  A
// rank that cannot start (no buffer; a user-defined operator, which 'm' plans refuse) therefore takes part in THAT reduction with
// the third value set: its peers read it in their cycle 0 and every rank leaves at the same collective, the refusing one with
// its own status, the others with "a peer failed".  A rank that fails later, between two collectives, hands its failure to the
// next one it would have entered: the vote of the inner solve (`early`), or the next refinement reduction (`mine`).
static tfqmrgpuStatus_t leave_marked(Handle& h, tfqmrgpuStatus_t st) {
    hipStream_t const s = (hipStream_t)h.stream;
    if (!several_ranks(h)) return st;
    if (!h.voteBuf) return st;                           // (allocated with the communicator / callback; without it no collective can be entered)
    double const mark[3] = { 0., 0., 1. };
    if (hipSuccess != hipMemcpyAsync(h.voteBuf.ptr, mark, sizeof mark, hipMemcpyHostToDevice, s)) return st;
    if (hipSuccess != hipStreamSynchronize(s)) return st;
    (void)reduce_over_ranks(h, h.voteBuf.as<double>(), 3, s);
    (void)hipStreamSynchronize(s);
    return st;
}

// The warm form of the refinement (tfqmrgpuExt_refineFrom; run_refine_from below has formed R, saved X0, preset |b|^2 in wBn2z and run
// precond_prepare): it runs on the correction system A D = R.  x holds X0 until the first update writes D over it -- cycle 0's update does not
// read x --, so a refinement that leaves before any update leaves X0 where it is and skips the back transform.  Plan::mixedFloor is read, not written.
struct MixedWarm {
    double const* R;          // the X-shaped right-hand side, double, element order ilvZ
    bool updated = false;     // an update has run: x holds D (in Y space on a preconditioned plan until precond_back)
    bool finished = false;    // the refinement has come to its own end (any status): x is X0 or a D that can be added to it
};

static tfqmrgpuStatus_t run_mixed(Handle& h, Plan& p, double tol, int maxIt, MixedWarm* const warm = nullptr) {
    hipStream_t const s = (hipStream_t)h.stream;
    SolveOutcome o;
    bool const multi = several_ranks(h);
    if (!warm) {
        if (!p.buffer)  return leave_marked(h, TFQ_ERR(TFQMRGPU_POINTER_INVALID));
        if (p.opFn)     return leave_marked(h, TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION));  // user-defined operators: 'z' and 'c' only
        if (auto const st = precond_prepare(h, p)) return leave_marked(h, st);
    }
    DevPlan const d = resolve(p), dz = resolveZ(p);
    FlopModel const fm(p);
    RefineArgs a{};
    a.d = d; a.xz = (double*)dz.x; a.Bz = warm ? warm->R : (double const*)dz.B; a.Yz = (double const*)d.v4;   // A x lives in v4 ... v7, free between two inner solves
    a.bn2z = (double*)(p.buffer + p.wBn2z.offset); a.refine = (double*)(p.buffer + p.wRefine.offset); a.ilvZ = p.ilvZ;
    if (maxIt <= 0 && !warm) TFQ_HIP(hipMemsetAsync(a.xz, 0, p.wXz.bytes, s), TFQMRGPU_STATUS_LAUNCH_FAILED)   // no iteration at all: x = 0 is the answer
    int used = 0, strikes = 0, lastIts = 0;
    bool brokeDown = false, firstStalled = false;
    double res2 = 1e300, prev2 = 1e300, bestGain = 1.;
    tfqmrgpuStatus_t result = TFQMRGPU_STATUS_MAX_ITERATIONS;
    tfqmrgpuStatus_t mine = TFQMRGPU_STATUS_SUCCESS;     // this rank's own failure between two collectives: rides the next refinement reduction
    // what a cycle copies into the control block of its float solve: pageable sources, alive until run_tfqmr has synchronised the stream
    double t2[2]; int32_t lim;
    for (int cycle = 0; ; ++cycle) {
        if (cycle > 0) { spmm_apply(dz, dz.x, (void*)a.Yz, s); p.last.flops_performed += fm.fMult; }
        a.cycle = cycle; a.innerTol = 1e-4; a.innerMaxIt = std::max(0, maxIt - used);
        launch_refine_residual(a, s, nullptr != warm);
        p.last.flops_performed += fm.fNrm;
        if (!mine && hipSuccess != hipGetLastError()) mine = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
        // (k_refine_max has written {.., .., 0}: this rank's mark behind it, on the same stream)
        if (mine && multi) (void)hipMemcpyAsync(a.refine + 2, &kOne, sizeof kOne, hipMemcpyHostToDevice, s);
        if (auto const st = reduce_over_ranks(h, a.refine, 3, s)) return mine ? mine : st;
        if (mine) return mine;                                              // every rank leaves behind this reduction
        double v[3];
        TFQ_HIP(hipMemcpyAsync(v, a.refine, sizeof v, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        if (v[2] > 0.) return TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);      // a rank failed: every rank reads the same value and leaves here
        res2 = v[0];
        p.last.cycleResidual.push_back(std::sqrt(res2));
        p.last.refinementCycles = cycle;
        if (v[1] > 0.) { result = TFQMRGPU_STATUS_BREAKDOWN; break; }      // the residual is not finite
        if (res2 <= tol * tol) { result = TFQMRGPU_STATUS_SUCCESS; break; }
        if (used >= maxIt) break;
        double lastGain = 1.;
        if (cycle > 0 && prev2 > 0. && prev2 < 1e299) { lastGain = std::sqrt(res2 / prev2); bestGain = std::min(bestGain, lastGain); }   // what the last cycle delivered
        // (r04) the float floor of THIS plan: where its first float solve gave up by itself (Ctl::stallStop).  The next solve of the plan -- same A, new B, the
        // use the reference's README names (:97-104) -- asks its first cycle for twice that instead of searching for it again (P2: 9 -> 7 iterations)
        if (1 == cycle && firstStalled && lastGain < 1. && !warm) p.mixedFloor = lastGain;   // (the floor belongs to cold solves: a later solve must not depend on a refineFrom in between)
        if (cycle > 0) {   // two cycles in a row gained less than a factor 2: give up (a breakdown of the last float solve is reported as one)
            strikes = (res2 > 0.25 * prev2) ? strikes + 1 : 0;
            if (strikes >= 2) { if (brokeDown) result = TFQMRGPU_STATUS_BREAKDOWN; break; }
        }
        prev2 = res2;
        auto const ask = next_cycle(tol, res2, cycle, bestGain, lastGain, lastIts, maxIt - used, p.mixedFloor);
        // Ctl::tol2, Ctl::target_bound2 (every rank the same values; 0: no probe before the last iteration)
        t2[0] = ask.innerTol * ask.innerTol; t2[1] = ask.predicted ? 0. : ask.innerTol * ask.innerTol * 1e4;
        // (a failure here travels through the vote in front of the inner solve: the peers are about to enter THAT collective)
        tfqmrgpuStatus_t early = (hipSuccess == hipMemcpyAsync(&d.ctl->tol2, t2, sizeof t2, hipMemcpyHostToDevice, s))
                                 ? TFQMRGPU_STATUS_SUCCESS : TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
        if (ask.predicted) {   // the inner solve's own iteration limit (k_refine_init_col has written maxIt - used)
            lim = ask.innerIts;
            if (!early && hipSuccess != hipMemcpyAsync(&d.ctl->maxIterations, &lim, sizeof lim, hipMemcpyHostToDevice, s)) early = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
        }
        // run_tfqmr's own protocol makes every rank come back at the same point: a refusal through its vote, a failure inside through the
        // third value of its slot records (state 4) -- so a status from it ends the refinement on every rank alike
        if (auto const st = run_tfqmr(h, p, ask.innerTol, ask.innerIts, early, res2, o)) return st;
        used += o.last.iteration;
        lastIts = o.last.iteration;
        if (0 == cycle) firstStalled = (3 == o.last.state && o.last.iteration < ask.innerIts);   // ended by itself at its floor, not at a limit
        p.last.cycleIterations.push_back(o.last.iteration);
        brokeDown = (2 == o.last.state);                                    // every right-hand side of this float solve broke down
        p.last.flops_performed += fm.solve(o.last) - fm.fNrm;                    // (|r|^2 of the set-up is the refinement's, counted above)
        launch_refine_update(a, s);
        if (warm) warm->updated = true;
        p.last.flops_performed += 2. * p.nnzbX * p.LM * p.LN;
    }
    if (!warm || warm->updated)                          // (warm and no update: x still holds X0, in X space)
    if (auto const st = precond_back(h, p)) return st;   // (every rank gets here: errors that one rank alone could see have left above, behind a collective)
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    p.flops_performed_all += p.last.flops_performed;
    p.residuum_reached = std::sqrt(std::max(res2, 1.4e-76 * 1.4e-76));
    p.last.iterations_needed = (TFQMRGPU_STATUS_SUCCESS == result) ? used : maxIt;
    if (warm) warm->finished = true;
    return result;
}

// what a solve leaves for getInfo, getBoundHistory and the profile, as it is before the solve starts (residuum_reached: see Plan)
static void reset_results(Plan& p, int maxIt) {
    p.last = Plan::Last{};
    p.last.iterations_needed = maxIt; p.last.flops_performed = 0;
}

// the tail of a tfQMR solve that came to its end (the back transform has run, flops_performed is complete): getInfo's values and the status
static tfqmrgpuStatus_t finish_tfqmr(Plan& p, Ctl const& last, int maxIt) {
    p.flops_performed_all += p.last.flops_performed;
    p.residuum_reached = std::sqrt(last.residual2_reached);
    p.last.iterations_needed = (1 == last.state) ? last.iterations_needed : maxIt;
    switch (last.state) {
        case 1: return TFQMRGPU_STATUS_SUCCESS;
        case 2: return TFQMRGPU_STATUS_BREAKDOWN;
        default: return TFQMRGPU_STATUS_MAX_ITERATIONS;
    }
}

// a warm solve that was given no iteration at all: X0 is the answer, untouched; status and getInfo of a cold solve that was given none
static tfqmrgpuStatus_t finish_warm_unstarted(Plan& p) {
    p.flops_performed_all += p.last.flops_performed;
    p.residuum_reached = std::sqrt(1e300);
    return TFQMRGPU_STATUS_MAX_ITERATIONS;
}

// Warm start (tfqmrgpu_ext.h section 14): the driver above, untouched, wrapped in a correction solve the way run_mixed wraps it.
//   Y = A X0 (the caller's A, one spmm_apply into v9) | X0 := x, R := B - Y, tau = |r|^2, 1 / |b|^2 (tfq_warm.hip) | [A := A M^-1] |
//   run_tfqmr on A D = R from zero, R its X-shaped right-hand side (DevPlan::R) | [D := M^-1 D] | x := X0 + D
// v9 holds Y: before its first iteration the driver reads neither x nor v4 ... v9 -- the kernels of that iteration take x, v4, v6, v7, v8 as
// zero and v5 as the right-hand side (DevPlan::first), and v9 is written by the first multiply before k_v5_nrm reads it -- and the
// residual pass has consumed Y by then.  X0 cannot live there: the first iteration writes every work vector, and x itself.
tfqmrgpuStatus_t run_solve_from(Handle& h, Plan& p, double tol, int maxIt, void const* callersA, tfqmrgpuStatus_t early) {
    SolveOutcome o;
    // several ranks: refused (the residual pass has no reduction over ranks yet).  Through the vote, so that every rank leaves together
    if (several_ranks(h)) return run_tfqmr(h, p, tol, maxIt, early ? early : TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION), 1., o);
    if (early) return early;
    if ('z' != p.precision && 'c' != p.precision) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    reset_results(p, maxIt);
    if (maxIt <= 0) return finish_warm_unstarted(p);
    hipStream_t const s = (hipStream_t)h.stream;
    size_t const S = align256(p.S);
    if (auto const st = p.held.warm.reserve(std::max<size_t>(2 * S, 256))) return st;
    char* const X0 = p.held.warm.as<char>();
    char* const R = X0 + S;
    DevPlan const d = resolve(p);
    {   // R from the caller's A, before precond_prepare scales the A in the buffer (or brings it up to date with pending patches: the kept copy has them)
        DevPlan dA = d; dA.A = const_cast<void*>(callersA);
        spmm_apply(dA, d.x, d.v9, s);
        if (!warm_residual_launch(d, d.v9, X0, R, tol, maxIt, s)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
        TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    }
    if (auto const st = precond_prepare(h, p)) return st;           // (x has not been written yet)
    p.warmR = R;                                                    // resolve(): DevPlan::R for this solve
    auto const st = run_tfqmr(h, p, tol, maxIt, TFQMRGPU_STATUS_SUCCESS, 1., o);
    p.warmR = nullptr;
    if (st) {   // the driver failed on the way: x is a partial correction at best.  X0 goes back, as far as the device still takes a copy
        (void)hipMemcpyAsync(d.x, X0, p.S, hipMemcpyDeviceToDevice, s);
        return st;
    }
    Ctl const& last = o.last;
    FlopModel const fm(p);
    // the correction solve (its set-up norm is |r|^2 of the residual pass) + the product A X0 + |b|^2 + the subtraction and the update
    p.last.flops_performed = fm.solve(last) + fm.fMult + fm.fNrm + 4. * p.nnzbX * p.LM * p.LN;
    if (auto const st2 = precond_back(h, p)) return st2;            // D := M^-1 Y, also after max iterations or a breakdown
    if (!warm_update_launch(d, X0, s)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    return finish_tfqmr(p, last, maxIt);
}

// The same for an 'm' plan (tfqmrgpu_ext.h section 16): the refinement of run_mixed, its float driver untouched, on the correction system.
//   Y = A X0 (the caller's double A, one spmm_apply into v4 ... v7) | X0 := x, R := B - Y, |b|^2 -> wBn2z (tfq_warm.hip, all in double) | [A := A M^-1] |
//   run_mixed on A D = R from D = 0: per cycle r = R - A D in double (cycle 0: r = R), A d = r in float, D += d in double | [D := M^-1 D] | x := X0 + D
// D lives in the plan's double x: cycle 0's update writes it without reading what is there, which is X0 -- saved by then.  A refinement that ends
// before any update (X0 meets the threshold) leaves x alone: no back transform, no update.
tfqmrgpuStatus_t run_refine_from(Handle& h, Plan& p, double tol, int maxIt, void const* callersA, tfqmrgpuStatus_t early) {
    // several ranks: refused (the residual pass has no reduction over ranks).  Through the mixed solve's own first collective, so that every rank leaves together
    if (several_ranks(h)) return leave_marked(h, early ? early : TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION));
    if (early) return early;
    if ('m' != p.precision) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    reset_results(p, maxIt);
    if (maxIt <= 0) return finish_warm_unstarted(p);
    hipStream_t const s = (hipStream_t)h.stream;
    size_t const Z = align256(p.wXz.bytes);
    if (auto const st = p.held.warm.reserve(std::max<size_t>(2 * Z, 256))) return st;
    char* const X0 = p.held.warm.as<char>();
    char* const R = X0 + Z;
    DevPlan const dz = resolveZ(p);
    FlopModel const fm(p);
    double const nReal = 2. * p.nnzbX * p.LM * p.LN;
    {   // R from the caller's A, before precond_prepare scales the A in the buffer (or brings it up to date with pending patches: the kept copy has them)
        DevPlan dA = dz; dA.A = const_cast<void*>(callersA);
        spmm_apply(dA, dz.x, dz.v4, s);
        if (!warm_refine_residual_launch(dz, dz.v4, X0, R, (double*)(p.buffer + p.wBn2z.offset), s)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
        TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
        p.last.flops_performed += fm.fMult + fm.fNrm + nReal;            // the product A X0, |b|^2 and the subtraction (|r|^2: cycle 0 of the refinement counts it)
    }
    if (auto const st = precond_prepare(h, p)) return st;           // (x has not been written yet)
    MixedWarm w{ (double const*)R };
    auto const st = run_mixed(h, p, tol, maxIt, &w);
    if (!w.finished) {   // it failed on the way: x is a partial correction at best.  X0 goes back, as far as the device still takes a copy
        (void)hipMemcpyAsync(dz.x, X0, p.wXz.bytes, hipMemcpyDeviceToDevice, s);
        return st;
    }
    if (w.updated) {     // x holds D, back-transformed: x := X0 + D
        if (!warm_update_launch(dz, X0, s)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
        TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
        p.last.flops_performed += nReal; p.flops_performed_all += nReal;
    }
    return st;
}

tfqmrgpuStatus_t run_solve(Handle& h, Plan& p, double tol, int maxIt) {
    reset_results(p, maxIt);
    if ('m' == p.precision) return run_mixed(h, p, tol, maxIt);
    // what this rank can tell before it touches the device
    tfqmrgpuStatus_t early = TFQMRGPU_STATUS_SUCCESS;
    if (!p.buffer) early = TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    else if ('z' != p.precision && 'c' != p.precision) early = err(TFQMRGPU_PRECISION_MISSMATCH, __LINE__ % 10000, p.precision);
    // a user-defined operator on a padded plan (tfqmrgpu_ext.h section 18): the callback contract names ONE block shape
    if (!early && p.opFn && p.padded()) early = TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    if (!early) early = precond_prepare(h, p);   // (off: returns at once; a refusal travels through the ranks' vote like the others)
    SolveOutcome o;
    if (auto const st = run_tfqmr(h, p, tol, maxIt, early, 1., o)) return st;
    Ctl const& last = o.last;
    FlopModel const fm(p);
    p.last.flops_performed = fm.solve(last);
    if (p.opFn) p.last.flops_performed += o.userFlops - (2. * last.iteration + last.nprobes) * fm.fMult;  // the operator's own count
    if (auto const st = precond_back(h, p)) return st;   // X := M^-1 Y, also when the solve ended at maxIterations or in a breakdown
    return finish_tfqmr(p, last, maxIt);
}

} // namespace tfq

// bench_tfqmrgpu: compiled counterpart of the reference's benchmark driver (real-space/tfQMRgpu
// tfQMRgpu/source/bench_tfqmrgpu.cu:442-590): same positional arguments, same result lines, a plain C++ caller of
// libtfQMRgpu.so through include/tfqmrgpu.h (+ tfqmrgpuExt_multiply for the `multi` mode).
//
//   bench_tfqmrgpu multi <planfile> [precision=f] [nrep=1] [nsamp=1] [lm=16] [ln=lm]
//       plan file `#nnzb_for_Y_A_X= nY nA nX` + lines `iY iA iX beta` (bench_tfqmrgpu.cu:456-498), cos/sin fill
//       (:274-287), host re-computation check maxdev <= 1e-4 (:349-420).  A `.gz` file is read with zlib.  precision f | c, d | z, or m
//       (float data summed in double, the reference's gemmNxNf<float, ..., double>: float arrays, `f` result lines, the f64 matrix peak).
//   bench_tfqmrgpu tfQMR <problem.xml> [precision=z] [nrep=1] [MaxIter=2000]
//       solves the <LinearProblem> (schema of tfqmrgpu_example_xml_reader.hxx:125-292) through createPlan ->
//       bufferSize -> setBuffer -> setMatrix -> solve -> getInfo -> getMatrix and compares with the stored X if any
//       (:178-205).  Blocks of the XML are row-major; transposition flag 'n' (see DESIGN.md on the reference's 't').
//       Extensions of this build, printed behind the reference's own result lines:
//         multi:  the host re-computation is timed (threads over the Y blocks) = the CPU number beside the GPU one, and the
//                 multiply is priced against the MI355X roofs (compulsory bytes of SURVEY 8d / HBM 8 TB/s, flops / matrix peak);
//         tfQMR:  iterations per second, the fused multiply kernel of the iteration against the HBM roof (per-kernel times from
//                 tfqmrgpuExt_getProfile), and `--gpus N` anywhere on the command line: N processes, one per GPU, the block
//                 columns of X/B sharded with tfqmrgpuExt_shardColumns, the stopping test all-reduced by the library over RCCL.
//   bench_tfqmrgpu read <problem.xml>
//       parses the file with the reader below and prints what it found (no GPU call; used by tests/test_fd_generator.py).
// The XML reader below handles exactly that schema (elements with attributes and whitespace-separated numbers);
// it is this program's own, the reference uses RapidXML.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdint>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include <sys/wait.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>
#include <zlib.h>

#include "tfqmrgpu.h"
#include "tfqmrgpu_ext.h"

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define CHECK_HIP(call) do { hipError_t const e_ = (call); if (e_ != hipSuccess) { \
    std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); std::exit(3); } } while (0)
#define CHECK_TFQ(call) do { tfqmrgpuStatus_t const s_ = (call); if (s_ != TFQMRGPU_STATUS_SUCCESS) { \
    tfqmrgpuPrintError(s_); std::fprintf(stderr, "%s:%d %s failed with status %d\n", __FILE__, __LINE__, #call, int(s_)); std::exit(2); } } while (0)

std::string slurp(std::string const& path) {
    // gzopen reads plain files as well as gzip streams (no shell, no sub-process)
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open '%s'\n", path.c_str()); std::exit(1); }
    std::string s; char buf[1 << 16]; int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) s.append(buf, size_t(n));
    if (n < 0) { std::fprintf(stderr, "error while reading '%s'\n", path.c_str()); std::exit(1); }
    gzclose(f);
    return s;
}

// ---------------------------------------------------------------------------------------------------
// multi mode
int bench_multi(int argc, char** argv) {
    std::string const path = (argc > 2) ? argv[2] : "plan";
    char const fF = (argc > 3) ? char(argv[3][0] | 32) : 'f';
    int const nrep = (argc > 4) ? std::atoi(argv[4]) : 1;
    int const nsamp = (argc > 5) ? std::atoi(argv[5]) : 1;
    int const lm = (argc > 6) ? std::atoi(argv[6]) : 16;
    int const ln = (argc > 7) ? std::atoi(argv[7]) : lm;
    bool const dbl = ('d' == fF || 'z' == fF);
    // m: float data summed in double (the reference's gemmNxNf<float, ..., double>, bench_tfqmrgpu.cu:520-547): float arrays, the f64 matrix pipe
    bool const mixed = ('m' == fF);
    char const prec = dbl ? 'z' : mixed ? 'm' : 'c';

    std::string const text = slurp(path);
    std::istringstream in(text);
    std::string tag; long nY = 0, nA = 0, nX = 0;
    in >> tag >> nY >> nA >> nX;
    if (tag.empty() || tag[0] != '#' || nY < 1) { std::fprintf(stderr, "'%s' is not a plan file\n", path.c_str()); return 1; }
    std::vector<uint32_t> starts, pairs;
    long iY, iA, iX, beta, last = -1;
    while (in >> iY >> iA >> iX >> beta) {
        // the lists go to the device as they are: refuse what would index outside of A or X there (Y blocks are numbered by
        // group, a group = run of equal iY, as in the reference: the reordered plan file's iY values do not ascend)
        if (iA < 0 || iA >= nA || iX < 0 || iX >= nX) {
            std::fprintf(stderr, "'%s': line `%ld %ld %ld %ld` is out of range (nA %ld nX %ld)\n", path.c_str(), iY, iA, iX, beta, nA, nX);
            return 1;
        }
        if (iY != last) { starts.push_back(uint32_t(pairs.size() / 2)); last = iY; }
        pairs.push_back(uint32_t(iA)); pairs.push_back(uint32_t(iX));
    }
    starts.push_back(uint32_t(pairs.size() / 2));
    if (long(starts.size()) != nY + 1) { std::fprintf(stderr, "plan file lists %zu Y blocks, header says %ld\n", starts.size() - 1, nY); return 1; }
    size_t const nPairs = pairs.size() / 2;
    std::printf("\n# bench_multi<%d,%d> on GPU !!!!\n", lm, ln);
    std::printf("# Execute %d repetitions, sample %d times.\n", nrep, nsamp);

    size_t const rb = dbl ? 8 : 4;
    auto fill = [&](size_t n, int rows, int cols) {   // Re = cos(arg), Im = sin(arg), arg = running element index
        std::vector<char> v(n * 2 * rows * cols * rb);
        for (size_t b = 0; b < n; ++b)
            for (int e = 0; e < rows * cols; ++e) {
                double const arg = double(b * rows * cols + e);
                size_t const re = (b * 2 + 0) * rows * cols + e, im = (b * 2 + 1) * rows * cols + e;
                if (dbl) { ((double*)v.data())[re] = std::cos(arg); ((double*)v.data())[im] = std::sin(arg); }
                else     { ((float*) v.data())[re] = float(std::cos(arg)); ((float*)v.data())[im] = float(std::sin(arg)); }
            }
        return v;
    };
    auto const A = fill(nA, lm, lm), X = fill(nX, lm, ln);
    size_t const yBytes = size_t(nY) * 2 * lm * ln * rb;
    void *dA, *dX, *dY; uint32_t *dS, *dP;
    CHECK_HIP(hipMalloc(&dA, A.size())); CHECK_HIP(hipMalloc(&dX, X.size())); CHECK_HIP(hipMalloc(&dY, yBytes));
    CHECK_HIP(hipMalloc((void**)&dS, starts.size() * 4)); CHECK_HIP(hipMalloc((void**)&dP, pairs.size() * 4));
    CHECK_HIP(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dX, X.data(), X.size(), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dY, 0, yBytes));
    CHECK_HIP(hipMemcpy(dS, starts.data(), starts.size() * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dP, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));

    tfqmrgpuHandle_t handle = nullptr;
    CHECK_TFQ(tfqmrgpuCreateHandle(&handle));
    CHECK_TFQ(tfqmrgpuExt_multiply(handle, prec, lm, ln, uint32_t(nY), dS, dP, dA, dX, dY));   // warm-up (module load)
    CHECK_HIP(hipDeviceSynchronize());
    // the launch order is prepared ONCE, in front of the timed loop -- as the reference prepares its launch there (bench_tfqmrgpu.cu:442-556 reads,
    // sorts and uploads the lists; :289-440 times the multiplications).  Mode 4: the library chooses how the XCDs split the listing; the results are
    // those of the caller's order bit for bit.  BENCH_ORDER=0 in the environment of THIS driver: the caller's order.
    void* order = nullptr;
    {
        char const* env = std::getenv("BENCH_ORDER");
        int const mode = env ? std::atoi(env) : 4;
        CHECK_TFQ(tfqmrgpuExt_multiplyPrepare(handle, prec, lm, ln, uint32_t(nY), dS, dP, mode, &order));
        std::printf("# launch order: %s\n", order ? "prepared by the library (tfqmrgpuExt_multiplyPrepare)" : "the listing's own");
    }
    std::vector<double> times;
    double nflop = 0;
    for (int s = 0; s < nsamp; ++s) {
        double const t0 = now();
        for (int r = 0; r < nrep; ++r) CHECK_TFQ(tfqmrgpuExt_multiplyOrdered(handle, prec, lm, ln, uint32_t(nY), dS, dP, dA, dX, dY, order));
        CHECK_HIP(hipDeviceSynchronize());
        times.push_back(now() - t0);
        nflop += double(nrep) * double(nPairs) * 8.0 * lm * lm * ln;
    }
    double tsum = 0, t2 = 0;
    for (double t : times) { tsum += t; t2 += t * t; }
    double const tavg = tsum / nsamp, tdev = std::sqrt(std::max(0.0, t2 / nsamp - tavg * tavg));
    std::printf("# GPU needed %.3f seconds, %.6f +/- %.6f sec per sample\n", tsum, tavg, tdev);

    // host re-computation in double: Y[iY] = sum_p A^T-stored[iA] * X[iX]
    std::vector<char> Yg(yBytes);
    CHECK_HIP(hipMemcpy(Yg.data(), dY, yBytes, hipMemcpyDeviceToHost));
    auto get = [&](std::vector<char> const& v, size_t idx) { return dbl ? ((double const*)v.data())[idx] : double(((float const*)v.data())[idx]); };
    size_t const PA = size_t(lm) * lm, PX = size_t(lm) * ln;
    unsigned const nthreads = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
    std::vector<double> devs(nthreads, 0.0);
    double const tc0 = now();
    {   // the reference checks with an OpenMP loop over the Y blocks (bench_tfqmrgpu.cu:358-365); here plain threads
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nthreads; ++t) pool.emplace_back([&, t] {
            std::vector<double> yr(PX), yi(PX);
            double md = 0;
            for (long y = t; y < nY; y += nthreads) {
                std::fill(yr.begin(), yr.end(), 0.0); std::fill(yi.begin(), yi.end(), 0.0);
                for (uint32_t q = starts[y]; q < starts[y + 1]; ++q) {
                    size_t const a0 = size_t(pairs[2 * q]) * 2 * PA, x0 = size_t(pairs[2 * q + 1]) * 2 * PX;
                    for (int k = 0; k < lm; ++k)
                        for (int i = 0; i < lm; ++i) {
                            double const ar = get(A, a0 + k * lm + i), ai = get(A, a0 + PA + k * lm + i);   // A[k][i]: stored transposed
                            for (int j = 0; j < ln; ++j) {
                                double const xr = get(X, x0 + k * ln + j), xi = get(X, x0 + PX + k * ln + j);
                                yr[i * ln + j] += ar * xr - ai * xi; yi[i * ln + j] += ar * xi + ai * xr;
                            }
                        }
                }
                for (size_t e = 0; e < PX; ++e) {
                    md = std::max(md, std::abs(get(Yg, size_t(y) * 2 * PX + e) - yr[e]));
                    md = std::max(md, std::abs(get(Yg, size_t(y) * 2 * PX + PX + e) - yi[e]));
                }
            }
            devs[t] = md;
        });
        for (auto& th : pool) th.join();
    }
    double const tcpu = now() - tc0;
    double maxdev = 0;
    for (double d : devs) maxdev = std::max(maxdev, d);
    std::printf("# GPU maxdev %g\n", maxdev);
    int rc = 0;
    if (maxdev > 1e-4) { std::printf("# Warning! GPU result has large deviations (%g) for blockDim=%d x %d\n", maxdev, lm, ln); rc = 1; }
    else {
        char const ch = dbl ? 'F' : 'f';
        std::printf("# GPU performed %.3f T%clop in %.3f seconds\n", nflop * 1e-12, ch, tsum);
        std::printf("# GPU performance (lm,ln,tune)=(%3d,%3d,%d) is  %.1f G%clop/sec\n", lm, ln, 0, nflop * 1e-9 / tsum, ch);
        // ---- not in the reference: the CPU beside it and the MI355X roofs (compulsory bytes = the A blocks that
        // occur + X read once + Y written once + index lists; HBM3E 8 TB/s, matrix peaks 78.6 / 157.3 TFLOP/s)
        double const flop1 = double(nPairs) * 8.0 * lm * lm * ln;
        std::printf("# CPU performance (host re-computation in double, %u threads) is  %.2f GFlop/sec (%.3f seconds)\n", nthreads, flop1 * 1e-9 / tcpu, tcpu);
        std::vector<char> usedA(size_t(nA), 0); size_t nAref = 0;
        for (size_t q = 0; q < nPairs; ++q) if (!usedA[pairs[2 * q]]) { usedA[pairs[2 * q]] = 1; ++nAref; }
        double const bytes = double(nAref) * 2 * PA * rb + double(nX + nY) * 2 * PX * rb + 4.0 * (nY + 1) + 8.0 * nPairs;
        double const t1 = tsum / (double(nsamp) * nrep), peak = (dbl || mixed) ? 78.6e12 : 157.3e12;
        bool const hbm = bytes / 8.0e12 >= flop1 / peak;
        std::printf("# MI355X roofline: %.1f GB/s of compulsory bytes (%.3f of 8 TB/s HBM), %.2f T%clop/s (%.3f of the %.1f T%clop/s matrix peak): %s-bound, fraction %.3f\n",
                    bytes * 1e-9 / t1, bytes / t1 / 8.0e12, flop1 * 1e-12 / t1, ch, flop1 / t1 / peak, peak * 1e-12, ch,
                    hbm ? "HBM" : "matrix-pipe", hbm ? bytes / t1 / 8.0e12 : flop1 / t1 / peak);
    }
    CHECK_TFQ(tfqmrgpuExt_multiplyRelease(order));
    CHECK_TFQ(tfqmrgpuDestroyHandle(handle));
    for (void* p : {dA, dX, dY, (void*)dS, (void*)dP}) (void)hipFree(p);
    return rc;
}

// ---------------------------------------------------------------------------------------------------
// minimal reader for the <LinearProblem> files
struct Element {
    std::string name;
    std::map<std::string, std::string> attr;
    std::string text;
    std::vector<Element> kids;
    Element const* child(char const* n) const { for (auto const& k : kids) if (k.name == n) return &k; return nullptr; }
    std::string get(char const* a, char const* dflt) const { auto it = attr.find(a); return it == attr.end() ? dflt : it->second; }
};

size_t parse_element(std::string const& s, size_t pos, Element& e) {   // pos at '<' of the start tag
    size_t p = pos + 1;
    while (p < s.size() && !std::isspace((unsigned char)s[p]) && s[p] != '>' && s[p] != '/') ++p;
    e.name = s.substr(pos + 1, p - pos - 1);
    for (;;) {                                                             // attributes
        while (p < s.size() && std::isspace((unsigned char)s[p])) ++p;
        if (p >= s.size()) return p;
        if (s[p] == '/') return s.find('>', p) + 1;                        // <tag ... />
        if (s[p] == '>') { ++p; break; }
        size_t const eq = s.find('=', p);
        std::string key = s.substr(p, eq - p);
        while (!key.empty() && std::isspace((unsigned char)key.back())) key.pop_back();
        size_t q0 = eq + 1;
        while (std::isspace((unsigned char)s[q0])) ++q0;
        char const quote = s[q0];
        size_t const q1 = s.find(quote, q0 + 1);
        e.attr[key] = s.substr(q0 + 1, q1 - q0 - 1);
        p = q1 + 1;
    }
    for (;;) {                                                             // content
        size_t const lt = s.find('<', p);
        if (lt == std::string::npos) return s.size();
        e.text.append(s, p, lt - p);
        if (s.compare(lt, 4, "<!--") == 0) { p = s.find("-->", lt) + 3; continue; }
        if (s[lt + 1] == '/') return s.find('>', lt) + 1;                  // end tag
        Element k; p = parse_element(s, lt, k); e.kids.push_back(std::move(k));
    }
}

template <typename T> std::vector<T> numbers(std::string const& text) {
    std::vector<T> v; char const* p = text.c_str(); char* end;
    for (;;) {
        double const d = std::strtod(p, &end);
        if (end == p) break;
        v.push_back(T(d)); p = end;
    }
    return v;
}

struct Operator { std::vector<int32_t> rowPtr, colInd; std::vector<std::complex<double>> val; int rows = 0, cols = 0; bool hasData = false; };

Operator read_operator(Element const& bsm) {
    Operator o;
    auto const* sm = bsm.child("SparseMatrix");
    auto const* csr = sm ? sm->child("CompressedSparseRow") : nullptr;
    if (!csr) { std::fprintf(stderr, "BlockSparseMatrix without CompressedSparseRow\n"); std::exit(1); }
    if (auto const* n = csr->child("NonzerosPerRow")) {
        auto const per = numbers<int64_t>(n->text);
        o.rowPtr.assign(1, 0);
        for (auto c : per) o.rowPtr.push_back(o.rowPtr.back() + int32_t(c));
    } else if (auto const* r = csr->child("RowStart")) o.rowPtr = numbers<int32_t>(r->text);
    if (auto const* c = csr->child("ColumnIndex")) o.colInd = numbers<int32_t>(c->text);
    size_t const nnzb = o.colInd.size();
    std::vector<int64_t> ind;
    if (auto const* i = sm->child("Indirection")) ind = numbers<int64_t>(i->text);
    if (auto const* dt = bsm.child("DataTensor")) {
        double const scale = std::atof(dt->get("scale", "1").c_str());
        bool const cplx = ((dt->get("type", "complex")[0] | 32) == 'c');
        auto const dims = numbers<int64_t>(dt->get("dimensions", "0 0 0"));
        o.rows = int(dims.size() > 1 ? dims[1] : 0); o.cols = int(dims.size() > 2 ? dims[2] : 0);
        size_t const blk = size_t(o.rows) * o.cols;
        o.val.assign(nnzb * blk, 0.0);
        if (!dims.empty() && dims[0] > 0) {
            auto const data = numbers<double>(dt->text);
            for (size_t b = 0; b < nnzb; ++b) {
                size_t const src = ind.empty() ? b : size_t(ind[b]);
                for (size_t e = 0; e < blk; ++e)
                    o.val[b * blk + e] = scale * (cplx ? std::complex<double>(data[(src * blk + e) * 2], data[(src * blk + e) * 2 + 1])
                                                       : std::complex<double>(data[src * blk + e], 0.0));
            }
            o.hasData = true;
        }
    }
    return o;
}

struct ProblemFile { double tol = 0; Operator A, B, X; };

bool read_problem(std::string const& path, ProblemFile& pf) {
    std::string const text = slurp(path);
    size_t const pos = text.find("<LinearProblem");
    if (pos == std::string::npos) { std::fprintf(stderr, "%s: no <LinearProblem> root\n", path.c_str()); return false; }
    Element root; parse_element(text, pos, root);
    pf.tol = std::atof(root.get("tolerance", "0").c_str());
    std::printf("# found tolerance= %g\n", pf.tol);
    for (auto const& k : root.kids) if (k.name == "BlockSparseMatrix") {
        char const id = k.get("id", "?")[0];
        (id == 'A' ? pf.A : id == 'B' ? pf.B : pf.X) = read_operator(k);
    }
    return true;
}

// what the reader found, one line per operator; the checksum weighs every value with its position (1-based, flat over
// [block][row][col]) so that a transposed block or a wrong indirection shows
int bench_read(int argc, char** argv) {
    ProblemFile pf;
    if (argc < 3 || !read_problem(argv[2], pf)) return 1;
    for (auto const* o : {&pf.A, &pf.B, &pf.X}) {
        std::complex<double> sum = 0;
        for (size_t e = 0; e < o->val.size(); ++e) sum += o->val[e] * double(e + 1);
        std::printf("# operator %c rows %d nnzb %zu block %d x %d rowPtr [", o == &pf.A ? 'A' : o == &pf.B ? 'B' : 'X',
                    int(o->rowPtr.size()) - 1, o->colInd.size(), o->rows, o->cols);
        for (auto v : o->rowPtr) std::printf(" %d", v);
        std::printf(" ] colInd [");
        for (auto v : o->colInd) std::printf(" %d", v);
        std::printf(" ] checksum %.17g %.17g\n", sum.real(), sum.imag());
    }
    return 0;
}

// one rank of the tfQMR mode: the whole problem (nranks == 1) or the block columns tfqmrgpuExt_shardColumns gives this rank
int tfqmr_rank(std::string const& path, char prec, int maxiter, int rank, int nranks, std::string const& tmp) {
    bool const root = (0 == rank);
    if (root) std::printf("\n# read file '%s' as input.\n", path.c_str());
    ProblemFile pf;
    if (!read_problem(path, pf)) return 1;
    double const tol = pf.tol;
    Operator const &A = pf.A; Operator B = pf.B, X = pf.X;
    int const mb = int(A.rowPtr.size()) - 1, LM = A.rows, LN = B.cols;
    if (nranks > 1) {   // this rank's block columns: sub-patterns of X and B, the values of its B blocks
        tfqmrgpuShard_t sh;
        CHECK_TFQ(tfqmrgpuExt_shardColumns(mb, X.rowPtr.data(), int(X.colInd.size()), X.colInd.data(), B.rowPtr.data(), int(B.colInd.size()),
                                           B.colInd.data(), 0, nranks, rank, &sh));
        Operator Bs, Xs;
        Xs.rowPtr.assign(sh.rowPtrX, sh.rowPtrX + mb + 1); Xs.colInd.assign(sh.colIndX, sh.colIndX + sh.nnzbX); Xs.rows = X.rows; Xs.cols = X.cols;
        Bs.rowPtr.assign(sh.rowPtrB, sh.rowPtrB + mb + 1); Bs.colInd.assign(sh.colIndB, sh.colIndB + sh.nnzbB); Bs.rows = B.rows; Bs.cols = B.cols;
        size_t const blk = size_t(B.rows) * B.cols;
        Bs.val.resize(size_t(sh.nnzbB) * blk);
        for (int b = 0; b < sh.nnzbB; ++b) std::copy(B.val.begin() + size_t(sh.bBlocks[b]) * blk, B.val.begin() + size_t(sh.bBlocks[b] + 1) * blk, Bs.val.begin() + size_t(b) * blk);
        std::printf("# [rank %d of %d] block columns %d .. %d: %d X blocks, %d B blocks\n", rank, nranks, sh.firstCol, sh.firstCol + sh.nCols - 1, sh.nnzbX, sh.nnzbB);
        tfqmrgpuExt_freeShard(&sh);
        B = std::move(Bs); X = std::move(Xs);
        CHECK_HIP(hipSetDevice(rank));
    }
    if (root) {
        std::printf("# requested precision= '%c' for LM= %d, LN= %d\n", prec, LM, LN);
        std::printf("\n# nnzb for A=%zu, X=%zu, B=%zu\n", A.colInd.size(), X.colInd.size(), B.colInd.size());
    }
    tfqmrgpuHandle_t handle = nullptr; tfqmrgpuBsrsvPlan_t plan = nullptr;
    CHECK_TFQ(tfqmrgpuCreateHandle(&handle));
    if (nranks > 1 || !tmp.empty()) {   // RCCL communicator of the stopping test: rank 0 makes the id, the others read it from a file
        char id[128];
        std::string const idfile = tmp + "/rccl_id";
        if (root) {
            CHECK_TFQ(tfqmrgpuExt_commUniqueId(id));
            std::ofstream(idfile + ".part", std::ios::binary).write(id, 128);
            std::rename((idfile + ".part").c_str(), idfile.c_str());
        } else {
            for (int tries = 0; ; ++tries) {
                std::ifstream f(idfile, std::ios::binary);
                if (f && f.read(id, 128)) break;
                if (tries > 6000) { std::fprintf(stderr, "[rank %d] no RCCL id after 60 s\n", rank); return 4; }
                usleep(10000);
            }
        }
        CHECK_TFQ(tfqmrgpuExt_commInit(handle, nranks, rank, id));
    }
    CHECK_TFQ(tfqmrgpu_bsrsv_createPlan(handle, &plan, mb, A.rowPtr.data(), int(A.colInd.size()), A.colInd.data(),
        X.rowPtr.data(), int(X.colInd.size()), X.colInd.data(), B.rowPtr.data(), int(B.colInd.size()), B.colInd.data(), 0, 0));
    size_t nbytes = 0;
    CHECK_TFQ(tfqmrgpu_bsrsv_bufferSize(handle, plan, LM, LM, LN, LN, prec, &nbytes));
    if (root) std::printf("# use %.6f GByte GPU memory\n", nbytes * 1e-9);
    // not in the reference: BENCH_PRECOND=1 switches the block-Jacobi right preconditioner on (tfqmrgpu_ext.h section 7); without it
    // the output of this driver is what it always was
    char const* const pcEnv = std::getenv("BENCH_PRECOND");
    int const precond = (pcEnv && std::atoi(pcEnv) > 0) ? TFQMRGPU_PRECOND_BLOCK_JACOBI : TFQMRGPU_PRECOND_NONE;
    if (precond) {
        CHECK_TFQ(tfqmrgpuExt_setPreconditioner(plan, precond));
        if (root) std::printf("# block-Jacobi right preconditioner: on (set-up at the first solve, inside the timed region)\n");
    }
    void* buffer = nullptr;
    CHECK_TFQ(tfqmrgpuCreateWorkspace(&buffer, nbytes, 'd'));
    CHECK_TFQ(tfqmrgpu_bsrsv_setBuffer(handle, plan, buffer));
    auto convert = [&](std::vector<std::complex<double>> const& v) {   // interleaved Re/Im in the plan's precision
        std::vector<char> out(v.size() * 2 * (prec == 'z' ? 8 : 4));
        for (size_t e = 0; e < v.size(); ++e) {
            if (prec == 'z') { ((double*)out.data())[2 * e] = v[e].real(); ((double*)out.data())[2 * e + 1] = v[e].imag(); }
            else             { ((float*) out.data())[2 * e] = float(v[e].real()); ((float*)out.data())[2 * e + 1] = float(v[e].imag()); }
        }
        return out;
    };
    auto const Ah = convert(A.val), Bh = convert(B.val);
    CHECK_TFQ(tfqmrgpu_bsrsv_setMatrix(handle, plan, 'A', Ah.data(), prec, LM, LM, 'n', TFQMRGPU_LAYOUT_RIRIRIRI));
    CHECK_TFQ(tfqmrgpu_bsrsv_setMatrix(handle, plan, 'B', Bh.data(), prec, LN, LM, 'n', TFQMRGPU_LAYOUT_RIRIRIRI));
    CHECK_TFQ(tfqmrgpuExt_setProfiling(plan, 1));
    CHECK_HIP(hipDeviceSynchronize());
    double const t0 = now();
    tfqmrgpuStatus_t const st = tfqmrgpu_bsrsv_solve(handle, plan, tol, maxiter);
    CHECK_HIP(hipDeviceSynchronize());
    double const dt = now() - t0;
    if (root) tfqmrgpuPrintError(st);
    std::vector<char> Xh(X.colInd.size() * size_t(LM) * LN * 2 * (prec == 'z' ? 8 : 4));
    CHECK_TFQ(tfqmrgpu_bsrsv_getMatrix(handle, plan, 'X', Xh.data(), prec, LN, LM, 'n', TFQMRGPU_LAYOUT_RIRIRIRI));
    double residual = 0, flops = 0, flops_all = 0; int32_t iterations = 0;
    CHECK_TFQ(tfqmrgpu_bsrsv_getInfo(handle, plan, &residual, &iterations, &flops, &flops_all));
    int rc = int(st);
    if (X.hasData && 1 == nranks) {
        double maxdev = 0, sum = 0, maxref = 0;
        for (size_t e = 0; e < X.val.size(); ++e) {
            double const xr = prec == 'z' ? ((double*)Xh.data())[2 * e] : ((float*)Xh.data())[2 * e];
            double const xi = prec == 'z' ? ((double*)Xh.data())[2 * e + 1] : ((float*)Xh.data())[2 * e + 1];
            double const d = std::abs(std::complex<double>(xr, xi) - X.val[e]);
            maxdev = std::max(maxdev, d); sum += d; maxref = std::max(maxref, std::abs(X.val[e]));
        }
        if (maxref > 0) {
            std::printf("# GPU maxdev %g avgdev %g\n", maxdev, sum / double(X.val.size()));
            if (maxdev >= 1e-5) rc = 1;
        }
    }
    char const ch = (prec == 'z') ? 'F' : 'f';
    if (root) {
        std::printf("# GPU converged to %.1e in %d iterations\n", residual, int(iterations));
        std::printf("# GPU performed %.3f T%clop in %.3f seconds = %.3f T%clop/s\n", flops * 1e-12, ch, dt, flops * 1e-12 / std::max(dt, 1e-6), ch);
        // ---- not in the reference: iterations per second and the fused multiply of the iteration against the HBM roof ----
        std::printf("# GPU iterations per second: %.1f (%d block columns x %d right-hand sides each on this rank)\n", iterations / std::max(dt, 1e-9),
                    int(std::set<int32_t>(X.colInd.begin(), X.colInd.end()).size()), LN);
        int64_t launches[TFQMRGPU_PROFILE_CLASSES]; double ms[TFQMRGPU_PROFILE_CLASSES];
        CHECK_TFQ(tfqmrgpuExt_getProfile(plan, launches, ms));
        {   // the launches of the first iteration read fewer vectors (tfqmrgpu_ext.h): the roofline line is about the steady ones
            int64_t l1[TFQMRGPU_PROFILE_CLASSES]; double m1[TFQMRGPU_PROFILE_CLASSES];
            CHECK_TFQ(tfqmrgpuExt_getProfileFirst(plan, l1, m1));
            for (int c = 0; c < TFQMRGPU_PROFILE_CLASSES; ++c) if (launches[c] > l1[c]) { launches[c] -= l1[c]; ms[c] -= m1[c]; }
        }
        tfqmrgpuPlanView_t v;
        CHECK_TFQ(tfqmrgpuExt_planView(plan, &v));
        int const k = (ms[TFQMRGPU_PROF_SPMM_V4_DOT] >= ms[TFQMRGPU_PROF_SPMM_V5_NRM_DOT]) ? TFQMRGPU_PROF_SPMM_V4_DOT : TFQMRGPU_PROF_SPMM_V5_NRM_DOT;
        if (launches[k] > 0) {
            double const rb = (prec == 'z') ? 8 : 4, S = double(v.nnzbX) * 2 * LM * LN * rb, S3 = double(v.nnzbX) * 2 * LM * LN * 4;
            std::vector<char> usedA(v.nnzbA, 0); double nAref = 0;
            for (uint64_t q = 0; q < v.nPairs; ++q) if (!usedA[v.pairs[2 * q]]) { usedA[v.pairs[2 * q]] = 1; nAref += 1; }
            double const bytes = ((TFQMRGPU_PROF_SPMM_V4_DOT == k) ? 5 : 4) * S + S3 + nAref * 2 * LM * LM * rb + 4.0 * (v.nnzbX + 1) + 8.0 * double(v.nPairs);
            double const t1 = ms[k] * 1e-3 / double(launches[k]);
            std::printf("# MI355X roofline: fused multiply %s, %lld launches of %.4f ms: %.1f GB/s of algorithmic bytes = %.3f of 8 TB/s HBM (%.2f T%clop/s)\n",
                        (TFQMRGPU_PROF_SPMM_V4_DOT == k) ? "spmm_v4_dot" : "spmm_v5_nrm_dot", (long long)launches[k], t1 * 1e3, bytes * 1e-9 / t1,
                        bytes / t1 / 8.0e12, double(v.nPairs) * 8.0 * LM * LM * LN * 1e-12 / t1, ch);
        }
    }
    if (!tmp.empty()) {   // for the parent's aggregate line
        std::ofstream f(tmp + "/rank" + std::to_string(rank));
        f << flops << " " << dt << " " << iterations << " " << int(st) << "\n";
    }
    if (nranks > 1 || !tmp.empty()) CHECK_TFQ(tfqmrgpuExt_commDestroy(handle));
    CHECK_TFQ(tfqmrgpu_bsrsv_destroyPlan(handle, plan));
    CHECK_TFQ(tfqmrgpuDestroyWorkspace(buffer));
    CHECK_TFQ(tfqmrgpuDestroyHandle(handle));
    return rc;
}

int bench_tfqmr(int argc, char** argv) {
    // `--gpus N` may stand anywhere; the positional arguments are the reference's
    int gpus = 0;
    std::vector<char*> pos;
    for (int i = 0; i < argc; ++i) {
        if (0 == std::strcmp(argv[i], "--gpus") && i + 1 < argc) { gpus = std::atoi(argv[++i]); continue; }
        pos.push_back(argv[i]);
    }
    int const n = int(pos.size());
    std::string const path = (n > 2) ? pos[2] : "problem";
    char p0 = (n > 3) ? char(pos[3][0] | 32) : 'z';
    // z: double, c: float, m: mixed -- float arrays in and out like the reference's driver (bench_tfqmrgpu.cu:140-151,573), solved by
    // complex<float> iterations inside a refinement in double (the reference's library answers 16 to solve)
    char const prec = ('d' == p0 || 'z' == p0) ? 'z' : ('m' == p0) ? 'm' : 'c';
    int const maxiter = (n > 5) ? std::atoi(pos[5]) : 2000;
    if (gpus < 1) return tfqmr_rank(path, prec, maxiter, 0, 1, "");
    // one child process per GPU, started before this process has made any HIP call
    char tmpl[] = "/tmp/bench_tfqmrgpu.XXXXXX";
    char const* dir = mkdtemp(tmpl);
    if (!dir) { std::perror("mkdtemp"); return 1; }
    std::string const tmp = dir;
    std::vector<pid_t> kids;
    for (int r = 0; r < gpus; ++r) {
        std::fflush(nullptr);
        pid_t const pid = fork();
        if (pid < 0) { std::perror("fork"); return 1; }
        if (0 == pid) { int const rc = tfqmr_rank(path, prec, maxiter, r, gpus, tmp); std::fflush(nullptr); _exit(rc); }
        kids.push_back(pid);
    }
    // the first rank that ends with an error takes the others with it: they would wait for ever in a collective it never joins
    int worst = 0;
    for (size_t left = kids.size(); left > 0; --left) {
        int status = 0;
        pid_t const pid = waitpid(-1, &status, 0);
        if (pid < 0) break;
        int const rc = WIFEXITED(status) ? WEXITSTATUS(status) : 128;
        if (rc != 0 && 0 == worst) for (auto k : kids) if (k != pid) kill(k, SIGTERM);
        worst = std::max(worst, rc);
    }
    double flops = 0, tmax = 0; int its = 0;
    for (int r = 0; r < gpus; ++r) {
        std::ifstream f(tmp + "/rank" + std::to_string(r));
        double fl = 0, dt = 0; int it = 0, st = 0;
        if (f >> fl >> dt >> it >> st) { flops += fl; tmax = std::max(tmax, dt); its = it; }
        std::remove((tmp + "/rank" + std::to_string(r)).c_str());
    }
    std::remove((tmp + "/rccl_id").c_str()); rmdir(tmp.c_str());
    char const ch = (prec == 'z') ? 'F' : 'f';
    std::printf("# %d GPUs: %.3f T%clop in %.3f seconds (slowest rank) = %.3f T%clop/s aggregate, %d iterations, %.1f iterations per second\n",
                gpus, flops * 1e-12, ch, tmax, flops * 1e-12 / std::max(tmax, 1e-9), ch, its, its / std::max(tmax, 1e-9));
    return worst;
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("Usage:  %s  [tfQMR/multiply]  [file]  [float/double]  [#repetitions]  [#iterations]  [#blocksize]\n", argv[0]);
        return 1;
    }
    if ('r' == argv[1][0]) return bench_read(argc, argv);
    return ('m' == argv[1][0]) ? bench_multi(argc, argv) : bench_tfqmr(argc, argv);
}

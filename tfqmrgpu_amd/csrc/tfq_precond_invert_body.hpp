// The body of k_precond_invert and k_precond_invert_listed (tfq_precond.hip), included once in each: ONE arithmetic, and the whole
// set-up's kernel compiles to the instructions it had before the listed form existed (a shared __device__ function, force-inlined,
// changed the register allocation of all its instances).  Expects: LM, TA, TW, A, diagOfRow, Minv, ilv of the kernel, `row` (the block
// row of this work group) and the statement TFQ_INVERT_REPORT_IDENTITY that thread 0 runs when the row gets the unit matrix.
    constexpr int CPT = invert_cpt(LM), NG = LM / CPT, NT = LM * NG, P = LM * LM;
    __shared__ double2 colv[LM], rowK[LM], rowP[LM];
    __shared__ int piv[LM];
    __shared__ int notFinite;
    uint32_t const ia = diagOfRow[row];
    int const t = threadIdx.x;
    TW* const out = Minv + size_t(row) * 2 * P;
    if (~0u == ia) {                                       // no diagonal block in the pattern: M_ii = 1
        store_identity(out, LM, t, int(blockDim.x));
        if (0 == t) { TFQ_INVERT_REPORT_IDENTITY; }
        return;
    }
    bool const active = (t < NT);
    int const r = t % LM, g = (t / LM) % NG;
    TA const* const blk = A + size_t(ia) * 2 * P;
    double ar[CPT], ai[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {                        // M[r][c] sits at (k = c, i = r) of the transposed block
        int const off = plane_offset(ilv, g * CPT + j, r, LM);
        ar[j] = double(blk[off]); ai[j] = double(blk[P + off]);
    }
    bool singular = false;
    if (0 == t) notFinite = 0;                          // (visible behind the first barrier of the loop below)
    for (int k = 0; k < LM; ++k) {
        int const gk = k / CPT, jk = k % CPT;
        if (active && g == gk) {
            double vr = 0, vi = 0;
#pragma unroll
            for (int j = 0; j < CPT; ++j) if (j == jk) { vr = ar[j]; vi = ai[j]; }
            colv[r] = make_double2(vr, vi);
        }
        __syncthreads();
        // the pivot: the first row of the largest magnitude among k ... LM - 1 -- every thread finds the same one
        int p = k; double best = -1.; bool finite = true;
        for (int q = k; q < LM; ++q) {
            double2 const v = colv[q];
            double const m = fmax(fabs(v.x), fabs(v.y));
            if (!(m <= 1.7e308)) finite = false;           // inf or NaN
            if (m > best) { best = m; p = q; }
        }
        if (!finite || !(best > 0.)) { singular = true; break; }   // (uniform: no thread waits at a barrier below)
        if (active && r == k) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) rowK[g * CPT + j] = make_double2(ar[j], ai[j]);
        }
        if (active && r == p) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) rowP[g * CPT + j] = make_double2(ar[j], ai[j]);
        }
        if (0 == t) piv[k] = p;
        __syncthreads();
        double2 const pv = colv[p];
        double2 inv;                                        // 1 / pivot without squaring it (Smith)
        if (fabs(pv.x) >= fabs(pv.y)) { double const q = pv.y / pv.x, d = pv.x + pv.y * q; inv = make_double2(1. / d, -q / d); }
        else                          { double const q = pv.x / pv.y, d = pv.x * q + pv.y; inv = make_double2(q / d, -1. / d); }
        // after the exchange row k is the pivot row and row p is what row k was
        double2 const f = (r == p) ? colv[k] : colv[r];     // this row's multiplier (row k itself: not used)
        if (r == p && p != k) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) { double2 const v = rowK[g * CPT + j]; ar[j] = v.x; ai[j] = v.y; }
        }
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            int const c = g * CPT + j;
            double2 pr = rowP[c];
            if (c == k) pr = make_double2(1., 0.);          // in place: column k becomes column k of the inverse
            double const sr = pr.x * inv.x - pr.y * inv.y, si = pr.x * inv.y + pr.y * inv.x;
            if (r == k) { ar[j] = sr; ai[j] = si; }
            else {
                double const br = (c == k) ? 0. : ar[j], bi = (c == k) ? 0. : ai[j];
                ar[j] = br - (f.x * sr - f.y * si); ai[j] = bi - (f.x * si + f.y * sr);
            }
        }
        __syncthreads();                                    // the next step rewrites colv, rowK, rowP
    }
    if (!singular) {                                        // an overflow on the way, or a NaN that never reached a pivot column: nothing but finite numbers is stored
        constexpr double kMax = (sizeof(TW) == 4) ? 3.4e38 : 1.7e308;   // finite in the precision it is stored in
        bool bad = false;
#pragma unroll
        for (int j = 0; j < CPT; ++j) bad = bad || !(fabs(ar[j]) <= kMax) || !(fabs(ai[j]) <= kMax);
        if (active && bad) notFinite = 1;
        __syncthreads();
        singular = (0 != notFinite);
    }
    if (singular) {                                         // a pivot that is zero or not finite, or a result that is not finite: M_ii = 1
        store_identity(out, LM, t, int(blockDim.x));
        if (0 == t) { TFQ_INVERT_REPORT_IDENTITY; }
        return;
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {                        // inverse of the row-exchanged block -> of the block: its columns exchanged back, last exchange first
        int c = g * CPT + j;
        for (int k = LM - 1; k >= 0; --k) { int const pk = piv[k]; if (c == k) c = pk; else if (c == pk) c = k; }
        out[r * LM + c] = TW(ar[j]); out[P + r * LM + c] = TW(ai[j]);
    }

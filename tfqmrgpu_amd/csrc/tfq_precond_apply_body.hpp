// The body of k_precond_apply and k_precond_apply_listed (tfq_precond.hip), included once in each, for the reason given in
// tfq_precond_invert_body.hpp.  Expects: T, TW, TRANSW, LM, nC, ilv of the kernel, MAXE, P, tpb, lt, `live` (this thread has a block),
// `src` and `dst` (the block that is read, the block that is written: the same one in place) and W (its M^-1).
    double accr[MAXE], acci[MAXE];
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
        accr[m] = 0.; acci[m] = 0.;
        int const e = lt + m * tpb;
        if (live && e < P) {
            int const r = e / nC, s = e % nC;
            for (int l = 0; l < LM; ++l) {
                int const wo = TRANSW ? l * LM + r : r * LM + l;
                double const wr = double(W[wo]), wi = double(W[LM * LM + wo]);
                int const io = plane_offset(ilv, l, s, nC);
                double const xr = double(src[io]), xi = double(src[P + io]);
                accr[m] += wr * xr - wi * xi; acci[m] += wr * xi + wi * xr;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
        int const e = lt + m * tpb;
        if (live && e < P) {
            int const o = plane_offset(ilv, e / nC, e % nC, nC);
            dst[o] = T(accr[m]); dst[P + o] = T(acci[m]);
        }
    }

// Device helpers shared by the two checks that sum in double whatever the plan's precision: tfq_residual.hip (tfqmrgpu_ext.h section 10) and
// tfq_leak.hip (section 11).
#pragma once
#include "tfq_spmm.hpp"

namespace tfq {

// plane_offset with the group size as a constant in each branch (the order is uniform over the launch: a scalar branch, no division)
__device__ __forceinline__ int res_offset(int ilv, int r, int s, int nC) {
    switch (ilv) {
        case 2:  return plane_offset(2, r, s, nC);
        case 4:  return plane_offset(4, r, s, nC);
        default: return plane_offset(0, r, s, nC);
    }
}

// One fixed pattern of fused multiply-adds (the rule of tfq_device.hpp: fma_): y += a x (complex)
__device__ __forceinline__ void res_cmac(double& yr, double& yi, double ar, double ai, double xr, double xi) {
    yr = fma_(-ai, xi, fma_(ar, xr, yr)); yi = fma_(ai, xr, fma_(ar, xi, yi));
}

} // namespace tfq

// Carry an operand from one plan to another on the device (tfqmrgpu_ext.h section 15): the launch interface of tfq_carry.hip
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace tfq {

// One operand window on either side: nBlocks blocks of nR x nC complex elements (planes Re | Im) at `data`, stored as double (dbl) or
// float in element order ilv (tfq_device.hpp: ilv_offset)
struct CarrySide { void* data; bool dbl; int ilv; };

// stored block n of `dst` := stored block list[n] of `src`, converted to dst's storage type and element order; kCarryZero (tfq_plan.hpp):
// zeros; list == nullptr: block n.  Asynchronous on `s`.  false: no launch was made (more work groups than a grid holds)
bool carry_launch(CarrySide const& dst, CarrySide const& src, uint32_t const* list, uint32_t nBlocks, int nR, int nC, hipStream_t s);

} // namespace tfq

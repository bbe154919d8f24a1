// The -DMVS_STAMPS diagnostic build's cycle stamps (build_lib.py --stamps;
// tools/stamps.py): a unit that stamps owns its g_stamps array and exports a
// reader with MVS_STAMPS_READER(name); nothing in the product build.
#pragma once
#include "mvs_internal.h"

#ifdef MVS_STAMPS
namespace {
// diagnostic build only: per-workgroup cycle sums of the scorer's phases
// (slot 0 items, 1 staging + barrier, 2 moments, 3 candidates, 4 wave 0's own
// candidate time, 5 wave 0's M-blocks), read by the unit's reader; k_bin's
// workgroups use rows 2048 + (slot 0 workgroups, 1 projection + LDS ranks,
// 2 global tile bases, 3 bucket writes)
__device__ unsigned long long g_stamps[4096 * 16];
}  // namespace
#define STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define STAMP_ADD(slot, val) \
    do { if (threadIdx.x == 0) atomicAdd(&g_stamps[(blockIdx.x & 4095) * 16 + (slot)], (unsigned long long)(val)); } while (0)
#define STAMP_ADD_W0(slot, val) \
    do { if ((threadIdx.x & 1023) == 0) atomicAdd(&g_stamps[(blockIdx.x & 4095) * 16 + (slot)], (unsigned long long)(val)); } while (0)
// any lane / one lane per wave
#define STAMP_ADD_ANY(slot, val) atomicAdd(&g_stamps[(blockIdx.x & 4095) * 16 + (slot)], (unsigned long long)(val))
#define STAMP_ADD_LANE0(slot, val) \
    do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_stamps[(blockIdx.x & 4095) * 16 + (slot)], (unsigned long long)(val)); } while (0)
#define STAMP_ADD_ROW(row, slot, val) \
    do { if (threadIdx.x == 0) atomicAdd(&g_stamps[((row) & 4095) * 16 + (slot)], (unsigned long long)(val)); } while (0)
#define MVS_STAMPS_READER(name)                                                                           \
    extern "C" int name(unsigned long long* out) {                                                         \
        return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(g_stamps)) == hipSuccess ? 0 : -1; \
    }
#else
#define STAMP_ADD_ROW(row, slot, val)
#define STAMP(var)
#define STAMP_ADD(slot, val)
#define STAMP_ADD_W0(slot, val)
#define STAMP_ADD_ANY(slot, val)
#define STAMP_ADD_LANE0(slot, val)
#define MVS_STAMPS_READER(name)
#endif

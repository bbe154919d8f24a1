// The stage's device sort, alone in its unit: hipCUB's radix sort brings a
// few hundred rocprim kernels, parsed and compiled here and nowhere else.
#include <hipcub/hipcub.hpp>

#include "mvs_internal.h"

// Stable sort of (key, value) pairs on the device (hipCUB LSD radix sort over
// the low `bits` key bits); tmp / tmp_bytes as hipcub: call with tmp == NULL
// to size the scratch.
extern "C" int mvs_sort_pairs(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                              const int32_t* vals_in, int32_t* vals_out, int64_t n, int bits, hipStream_t s) {
    if (hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, bits,
                                           s) != hipSuccess)
        return -1;
    return 0;
}

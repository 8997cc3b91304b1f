// The stable radix sort of tfrt_order.hip (sort_keys: two passes of 13-bit digits) for the other
// files of the library: keys of up to 26 bits, perm = argsort(keys, stable).  Thin wrappers; the
// kernels and what tfrt_ray_order does with them stay where they are.
#pragma once
#include "tfrt_common.h"

namespace tfrt {

// Bytes of `ws` for n keys (n <= 0 sizes like one key).
size_t sort_keys26_workspace_bytes(int64_t n);

// perm[r] = index of the key of rank r, 0 <= n < 2^31.  `keys` is read only; eight launches on
// `st` (a tile histogram, then scan, scan, scatter per digit, and a histogram in between).
// Returns 0 or TFRT_E_UNSUPPORTED.
int sort_keys26(void* ws, int n, unsigned* keys, int32_t* perm, hipStream_t st);

}  // namespace tfrt

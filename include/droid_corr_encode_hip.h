/*
 * droid_corr_encode_hip.h -- the prototypes of the fused correlation lookup + encoder convolution.  The contract is
 * stated in full in droid_update_hip.h, which includes this file; include that header, not this one.  Binding table:
 * droid_backends/_lib.py ABI_CORR_ENCODE (tests/test_corr_encode_abi.py holds it against the prototypes here).
 */
#ifndef DROID_CORR_ENCODE_HIP_H
#define DROID_CORR_ENCODE_HIP_H

#include "droid_update_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t droid_corr_encode_packed_bytes(void);
int droid_corr_encode(const void* const* volumes, const int64_t* slots, const float* coords, const void* packed, void* out,
                      int B, int64_t cap, int H1, int W1, int radius, int levels, int out_channels, int dtype,
                      int coords_layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_CORR_ENCODE_HIP_H */

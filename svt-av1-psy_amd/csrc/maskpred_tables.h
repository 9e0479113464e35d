// maskpred_tables.h -- the layout of the device's wedge table, shared by maskpred.hip (which fills and reads it) and interpred.hip (whose masked compound reads it):
// the ONE definition of block_size_wide / high, of the nine BlockSize values with wedge bits and of where each one's 32 masks start.
#pragma once
#include <stdint.h>

namespace svt_maskpred {
// BlockSize (definitions.h:1010-1036): block_size_wide / block_size_high
__device__ constexpr uint8_t kBw[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64};
__device__ constexpr uint8_t kBh[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};
// the nine sizes with wedge bits (wedge_params_lookup, inter_prediction.c:1912-1935), in BlockSize order: slot, first byte of the slot's 32 masks (index, then sign,
// each bw x bh bytes); kSlotOff[9] is the size of the table
__device__ constexpr uint8_t  kSlotBsize[9] = {3, 4, 5, 6, 7, 8, 9, 18, 19};
__device__ constexpr uint32_t kSlotOff[10]  = {0, 2048, 6144, 10240, 18432, 34816, 51200, 83968, 92160, 100352};
__device__ __forceinline__ int wedge_slot(const int bsize) {
    int s = -1;
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (kSlotBsize[k] == bsize) s = k;
    return s;
}
} // namespace svt_maskpred

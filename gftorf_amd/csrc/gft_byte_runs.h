// gft_byte_runs.h -- byte-granular images and file rows written as whole dwords (k_present.hip's 3-byte and 1-byte pixels,
// k_pcd.hip's 27..38-byte rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A run of `nbytes` staged bytes to dst, by a workgroup of THREADS.  The bytes lie in `lds` from byte (dst & 3) on, so a dword
// of the destination is a dword of the staging: whole dwords leave as such, the first and last dword of the run byte by byte
// where the run does not cover them (a neighbouring run, or the next image's padding, owns the rest).
template <int THREADS>
__device__ __forceinline__ void gft_put_run(uint8_t* dst, int nbytes, const uint32_t* lds)
{
    const int mis = (int)((uintptr_t)dst & 3u), total = mis + nbytes;
    uint8_t* base = dst - mis;
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lds);
    for (int w = threadIdx.x; w * 4 < total; w += THREADS) {
        const int first = w * 4;
        if (first >= mis && first + 4 <= total) {
            reinterpret_cast<uint32_t*>(base)[w] = lds[w];
        } else {
            for (int b = first; b < first + 4; b++)
                if (b >= mis && b < total) base[b] = lb[b];
        }
    }
}

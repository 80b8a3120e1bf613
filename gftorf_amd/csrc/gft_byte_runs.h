// gft_byte_runs.h -- byte-granular images and file rows written as whole dwords (k_present.hip's 3-byte and 1-byte pixels,
// k_pcd.hip's 27..38-byte rows) or as whole 16-byte words (k_debugviz.hip).
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

// gft_put_run with 16-byte words: the bytes lie in `lds` (16-byte aligned) from byte (dst & 15) on, so a 16-byte word of the
// destination is one of the staging.  Whole words leave as one 16-byte store each, the first and last word of the run byte
// by byte where the run does not cover them; nothing outside [dst, dst + nbytes) is written.  A team of TEAM threads writes
// the run, `member` = 0 .. TEAM - 1 the caller's place in it (a wave of the workgroup, or all of it).
template <int TEAM>
__device__ __forceinline__ void gft_put_run16(uint8_t* dst, int nbytes, const uint4* lds, int member)
{
    const int mis = (int)((uintptr_t)dst & 15u), total = mis + nbytes;
    uint8_t* base = dst - mis;
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lds);
    for (int w = member; w * 16 < total; w += TEAM) {
        const int first = w * 16;
        if (first >= mis && first + 16 <= total) {
            reinterpret_cast<uint4*>(base)[w] = lds[w];
        } else {
            for (int b = first; b < first + 16; b++)
                if (b >= mis && b < total) base[b] = lb[b];
        }
    }
}

// k_schedule.hip -- the run's schedule on the device (include/gftorf_schedule.h; train.py:120-129, 146-147).
//   k_schedule_tick   "make iteration `it` current", `it` read from a device counter that the launch itself advances.
//                     Workgroup 0 writes the iteration word and scatters row it - first_iter of a table of doubles to its
//                     destinations (learning-rate slots as doubles, anything else rounded once to float32).  The other
//                     workgroups, SC_MAX_BLOCKS at most, fill the background, 256 x 4 elements per step of a grid-stride loop:
//                     a thread computes the one Philox4x32-10 block that torch's own fill of the tensor, seeded with `it`,
//                     would compute in thread idx at its j-th draw, and stores its four elements, so lanes store consecutive
//                     floats.  Then the last workgroup to finish -- by a ticket word, the scheme of k_views_draw -- leaves
//                     it + 1 behind.  (Returning atomics on one address are served one after the other, ~12 ns each: with a
//                     workgroup per 1024 elements the 2049 tickets of a 7 x 240 x 320 background took 24 of the launch's 29 us.)
// No memset and no atomic but the ticket's; no LDS but two words, no scratch.
#include "gft_internal.h"
#include "gftorf_schedule.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_BLOCKS = 256;          // workgroups that fill the background
constexpr int64_t SC_MAX_N = 1ll << 40;

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct TickArgs {
    int64_t* state;
    const double* __restrict__ table;
    const gft_schedule_dest* __restrict__ dests;
    float* __restrict__ bg;
    int64_t N, first_iter, n, T;
    int64_t draws;                  // draws of four a thread of torch's fill makes: pairs (idx, j), j < draws, idx < min(T, n - 4 j T)
    int32_t C, D;
};

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key moved on by the Weyl constants in front of every round but the first
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(SC_THREADS) void k_schedule_tick(TickArgs a)
{
    __shared__ int64_t s_it;
    const int tid = threadIdx.x;
    // One thread reads the counter for its workgroup: its read has returned before the barrier, hence before this workgroup's
    // ticket, hence before the last workgroup's write of the counter.
    if (tid == 0) s_it = *(volatile const int64_t*)(a.state + GFT_SCHEDULE_COUNTER);
    __syncthreads();
    const int64_t it = s_it;
    if (blockIdx.x == 0) {
        int64_t row = it - a.first_iter;
        const bool outside = row < 0 || row >= a.N;
        row = row < 0 ? 0 : (row >= a.N ? a.N - 1 : row);
        if (tid == 0) {
            a.state[GFT_SCHEDULE_ITERATION] = it;
            if (outside) {
                // (ticks of one schedule follow one another on one stream: a plain read and write)
                a.state[GFT_SCHEDULE_OVERRUN] = 1;
                a.state[GFT_SCHEDULE_OVERRUNS] = a.state[GFT_SCHEDULE_OVERRUNS] + 1;
            }
        }
        const double* line = a.table + row * a.C;
        for (int d = tid; d < a.D; d += SC_THREADS) {
            const u4 raw = reinterpret_cast<const u4*>(a.dests)[d];             // {address lo, hi, column, kind}
            void* address = reinterpret_cast<void*>(((uint64_t)raw.y << 32) | raw.x);
            const int32_t column = (int32_t)raw.z;
            if (column < 0 || column >= a.C || !address) continue;
            const double v = line[column];
            if ((int32_t)raw.w == GFT_SCHEDULE_F64) *static_cast<double*>(address) = v;
            else *static_cast<float*>(address) = (float)v;
        }
    } else {
        const int64_t stride = (int64_t)(gridDim.x - 1) * SC_THREADS, first = (int64_t)(blockIdx.x - 1) * SC_THREADS + tid;
        for (int64_t j = 0; j < a.draws; j++) {
            const int64_t base = 4 * j * a.T, left = a.n - base;
            const int64_t owners = left < a.T ? left : a.T;                     // threads of the fill whose j-th draw has an element
            for (int64_t idx = first; idx < owners; idx += stride) {
                uint32_t c[4] = {(uint32_t)j, (uint32_t)((uint64_t)j >> 32), (uint32_t)idx, (uint32_t)((uint64_t)idx >> 32)};
                philox4x32_10(c, (uint32_t)it, (uint32_t)((uint64_t)it >> 32));
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int64_t e = base + idx + k * a.T;
                    // 2^-32 + v 2^-32 in (0, 1] (the product is exact, so one rounding whether or not it is fused); 1 becomes
                    // 0 (torch's uniform_ reverses the bounds); 2 u is exact, so 2 u - 1 rounds once either way
                    float u = 2.3283064e-10f + (float)c[k] * 2.3283064e-10f;
                    u = u == 1.0f ? 0.0f : u;
                    if (e < a.n) a.bg[e] = u * 2.0f - 1.0f;
                }
            }
        }
    }
    __syncthreads();
    // (relaxed: the ticket orders nothing but this workgroup's read of the counter above, which has returned; what the launch
    // writes reaches the next launch at the kernel's end)
    int32_t* ticket = reinterpret_cast<int32_t*>(a.state + GFT_SCHEDULE_TICKET);
    if (tid == 0 && __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int32_t)gridDim.x - 1) {
        a.state[GFT_SCHEDULE_COUNTER] = it + 1;
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" int gft_schedule_tick(void* hip_stream, const gft_schedule* sc)
{
    if (!sc) return gft_fail("gft_schedule_tick: NULL argument");
    if (!sc->state || !sc->table) return gft_fail("gft_schedule_tick: NULL state or table");
    if (reinterpret_cast<uintptr_t>(sc->state) & 7u) return gft_fail("gft_schedule_tick: the state block is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(sc->table) & 7u) return gft_fail("gft_schedule_tick: the table is not 8-byte aligned");
    if (sc->N < 1 || sc->C < 1 || sc->N > SC_MAX_N / sc->C)
        return gft_fail("gft_schedule_tick: a table of N=%lld rows and C=%d columns", (long long)sc->N, (int)sc->C);
    if (sc->D < 0 || sc->D > GFT_SCHEDULE_MAX_DESTS)
        return gft_fail("gft_schedule_tick: D=%d destinations; a tick takes 0..%d", (int)sc->D, GFT_SCHEDULE_MAX_DESTS);
    if (sc->D > 0 && !sc->dests) return gft_fail("gft_schedule_tick: D=%d destinations and a NULL array", (int)sc->D);
    if (reinterpret_cast<uintptr_t>(sc->dests) & 15u) return gft_fail("gft_schedule_tick: the destinations are not 16-byte aligned");
    TickArgs a = {};
    a.state = sc->state; a.table = sc->table; a.dests = sc->dests; a.N = sc->N; a.first_iter = sc->first_iter; a.C = sc->C; a.D = sc->D;
    int64_t blocks = 1;
    if (sc->bg) {
        if (sc->n < 1 || sc->n > SC_MAX_N) return gft_fail("gft_schedule_tick: a background of n=%lld elements", (long long)sc->n);
        if (sc->T < 1 || sc->T > 0x7fffffffll) return gft_fail("gft_schedule_tick: T=%lld threads of the fill", (long long)sc->T);
        if (reinterpret_cast<uintptr_t>(sc->bg) & 3u) return gft_fail("gft_schedule_tick: the background is not 4-byte aligned");
        a.bg = sc->bg; a.n = sc->n; a.T = sc->T;
        a.draws = (sc->n - 1) / (4 * sc->T) + 1;
        const int64_t owners = sc->n < sc->T ? sc->n : sc->T;              // threads of the fill whose first draw has an element
        const int64_t fill = (owners + SC_THREADS - 1) / SC_THREADS;
        blocks += fill < SC_MAX_BLOCKS ? fill : SC_MAX_BLOCKS;
    }
    hipLaunchKernelGGL(k_schedule_tick, dim3((unsigned)blocks), dim3(SC_THREADS), 0, (hipStream_t)hip_stream, a);
    return gft_launched("gft_schedule_tick");
}

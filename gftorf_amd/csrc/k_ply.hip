// k_ply.hip -- the rows of the Gaussian model's PLY files (include/gftorf_ply.h; scene/gaussian_model.py:315-367, 378-454).
// Both kernels move float32 bit patterns and compute nothing; both are bound by their HBM bytes.
// k_ply_pack: a workgroup takes PLY_ROWS consecutive Gaussians.  What it needs of a source tensor is one contiguous run of
// rows x w floats, which it reads as whole dwords, coalesced (the sources are 4-byte aligned, no more: a view one row into a
// [P + 1, 3] buffer starts 12 bytes off), eight loads in flight per lane and across the sources, since most runs are shorter
// than one load per lane and a wait per source would leave the kernel bound by latency.  Every float goes to its column of an
// LDS tile of rows x K floats (a table in LDS holds the column of every source float: the feature tensors' ch * n + j
// permutation and the zeros of the normals cost nothing extra).  The tile is the workgroup's block of the full sheet as it
// lies in memory: it leaves as 16-byte stores; the sibr sheet's block, the first K_sibr columns of every row, leaves the same
// way from the same tile.
// k_ply_unpack: the reverse.  A workgroup's rows x K_file floats of the chunk are contiguous and 16-byte aligned: 16-byte loads
// into the tile, then every destination tensor's run of rows x w floats is written as coalesced dwords, each float from the
// file column the table names.
#include "gft_internal.h"
#include "gftorf_ply.h"

namespace {

constexpr int PLY_THREADS = 256;
constexpr int PLY_ROWS = GFT_PLY_ROWS;
constexpr int PLY_BATCH = 8;                     // loads in flight per lane
constexpr int64_t PLY_MAX_ROWS = 1ll << 40;

// the column blocks of a row (pack) or the destination tensors (unpack): a kernel argument, passed by value
struct PlyBlocks {
    float* ptr[GFT_PLY_MAX_SOURCES];             // pack: the source, nullptr = zeros; unpack: the destination
    int32_t width[GFT_PLY_MAX_SOURCES];          // floats per row
    int32_t first[GFT_PLY_MAX_SOURCES];          // the block's first entry of `map`
    uint32_t magic[GFT_PLY_MAX_SOURCES];         // ceil(2^32 / width): e / width = umulhi(e, magic) while e * width < 2^32
    uint16_t map[GFT_PLY_MAX_COLUMNS];           // pack: the sheet column of every source float; unpack: the file column of every destination float
    int32_t count, total;                        // blocks; entries of `map`
};

inline uint32_t ply_magic(int32_t w) { return w > 1 ? (uint32_t)((0x100000000ull + (uint64_t)w - 1) / (uint64_t)w) : 0u; }

// e / w for 0 <= e < PLY_ROWS * GFT_PLY_MAX_COLUMNS
__device__ __forceinline__ int ply_div(int e, int w, uint32_t magic) { return w > 1 ? (int)__umulhi((uint32_t)e, magic) : e; }

__global__ __launch_bounds__(PLY_THREADS) void k_ply_pack(int64_t P, PlyBlocks b, int K, int Ks, uint32_t magic_ks,
                                                          float* __restrict__ out_full, float* __restrict__ out_sibr)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tile = reinterpret_cast<float*>(smem);                                   // [rows][K]
    uint16_t* map = reinterpret_cast<uint16_t*>(smem + (size_t)PLY_ROWS * K * 4);   // [b.total]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PLY_ROWS;                            // row0 < P: the grid is ceil(P / PLY_ROWS)
    const int rows = (int)(P - row0 < PLY_ROWS ? P - row0 : PLY_ROWS);
    for (int m = tid; m < b.total; m += PLY_THREADS) map[m] = b.map[m];
    __syncthreads();

    // the runs cut into pieces of PLY_THREADS floats; (k, q) = the next piece, the same in every lane
    int k = 0, q = 0;
    while (k < b.count && rows * b.width[k] <= 0) k++;
    while (k < b.count) {
        float v[PLY_BATCH];
        int at[PLY_BATCH];                                                          // the float's place in the tile; -1: none
#pragma unroll
        for (int u = 0; u < PLY_BATCH; u++) {
            at[u] = -1;
            v[u] = 0.f;
            if (k < b.count) {
                const int w = b.width[k], len = rows * w, e = q * PLY_THREADS + tid;
                if (e < len) {
                    const int r = ply_div(e, w, b.magic[k]);
                    at[u] = r * K + map[b.first[k] + (e - r * w)];
                    const float* src = b.ptr[k];
                    if (src) v[u] = src[row0 * w + e];
                }
                q++;
                if (q * PLY_THREADS >= len) {
                    q = 0;
                    k++;
                    while (k < b.count && rows * b.width[k] <= 0) k++;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PLY_BATCH; u++)
            if (at[u] >= 0) tile[at[u]] = v[u];
    }
    __syncthreads();

    if (out_full) {
        float* dst = out_full + row0 * K;                                           // 256-byte aligned: row0 is a multiple of 64
        const int n = rows * K, nv = n >> 2;
        for (int i = tid; i < nv; i += PLY_THREADS) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(tile)[i];
        for (int e = 4 * nv + tid; e < n; e += PLY_THREADS) dst[e] = tile[e];
    }
    if (out_sibr) {
        float* dst = out_sibr + row0 * Ks;
        const int n = rows * Ks, nv = n >> 2;
        auto at = [&](int e) { const int r = ply_div(e, Ks, magic_ks); return r * K + (e - r * Ks); };
        for (int i = tid; i < nv; i += PLY_THREADS)
            reinterpret_cast<float4*>(dst)[i] = make_float4(tile[at(4 * i)], tile[at(4 * i + 1)], tile[at(4 * i + 2)], tile[at(4 * i + 3)]);
        for (int e = 4 * nv + tid; e < n; e += PLY_THREADS) dst[e] = tile[at(e)];
    }
}

__global__ __launch_bounds__(PLY_THREADS) void k_ply_unpack(int64_t rows_total, int64_t row_first, int K, const float* __restrict__ chunk,
                                                            PlyBlocks b)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tile = reinterpret_cast<float*>(smem);                                   // [rows][K]
    uint16_t* map = reinterpret_cast<uint16_t*>(smem + (size_t)PLY_ROWS * K * 4);   // [b.total]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PLY_ROWS;                            // row0 < rows_total
    const int rows = (int)(rows_total - row0 < PLY_ROWS ? rows_total - row0 : PLY_ROWS);
    for (int m = tid; m < b.total; m += PLY_THREADS) map[m] = b.map[m];

    const float* src = chunk + row0 * K;                                            // 256-byte aligned
    const int n = rows * K, nv = n >> 2;
    constexpr int UNROLL = 4;
    for (int base = 0; base < nv; base += UNROLL * PLY_THREADS) {
        float4 x[UNROLL];                                                           // (loaded under `i < nv` they live in scratch)
#pragma unroll
        for (int u = 0; u < UNROLL; u++) x[u] = reinterpret_cast<const float4*>(src)[min(base + u * PLY_THREADS + tid, nv - 1)];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int i = base + u * PLY_THREADS + tid;
            if (i < nv) reinterpret_cast<float4*>(tile)[i] = x[u];
        }
    }
    for (int e = 4 * nv + tid; e < n; e += PLY_THREADS) tile[e] = src[e];
    __syncthreads();

    for (int k = 0; k < b.count; k++) {
        const int w = b.width[k], len = rows * w, first = b.first[k];
        const uint32_t magic = b.magic[k];
        float* dst = b.ptr[k] + (row_first + row0) * w;                             // not touched when len == 0
        for (int e = tid; e < len; e += PLY_THREADS) {
            const int r = ply_div(e, w, magic);
            dst[e] = tile[r * K + map[first + (e - r * w)]];
        }
    }
}

size_t ply_lds_bytes(int K, int total) { return (size_t)PLY_ROWS * K * 4 + (((size_t)total * 2 + 15) & ~(size_t)15); }

}  // namespace

extern "C" int gft_ply_pack(void* hip_stream, int64_t P, int32_t count, const float* const* sources, const int32_t* widths,
                            const int32_t* channels, int32_t K_full, int32_t K_sibr, float* out_full, float* out_sibr)
{
    if (P < 0 || P > PLY_MAX_ROWS) return gft_fail("gft_ply_pack: bad row count P=%lld", (long long)P);
    if (count < 1 || count > GFT_PLY_MAX_SOURCES)
        return gft_fail("gft_ply_pack: %d column blocks, must be 1..%d", count, GFT_PLY_MAX_SOURCES);
    if (K_full < 1 || K_full > GFT_PLY_MAX_COLUMNS)
        return gft_fail("gft_ply_pack: K_full=%d, a row holds 1..%d columns", K_full, GFT_PLY_MAX_COLUMNS);
    if (!sources || !widths || !channels) return gft_fail("gft_ply_pack: NULL argument");
    if (!out_full && !out_sibr) return gft_fail("gft_ply_pack: both outputs are NULL");
    if (out_sibr && (K_sibr < 1 || K_sibr > K_full))
        return gft_fail("gft_ply_pack: K_sibr=%d, the sibr row is the first 1..%d columns of the full row", K_sibr, K_full);
    if (((uintptr_t)out_full & 15u) || ((uintptr_t)out_sibr & 15u)) return gft_fail("gft_ply_pack: an output is not 16-byte aligned");
    PlyBlocks b = {};
    int64_t sum = 0;
    for (int k = 0; k < count; k++) {
        const int32_t w = widths[k], c = channels[k];
        if (w < 0 || c < 0 || (c > 0 && w % c != 0))
            return gft_fail("gft_ply_pack: block %d has width %d and %d channels", k, w, c);
        sum += w;
        if (sum > K_full) break;
    }
    if (sum != K_full)
        return gft_fail("gft_ply_pack: the widths add up to %s%lld columns, K_full=%d", sum > K_full ? "more than " : "", (long long)sum, K_full);
    int32_t col = 0;
    for (int k = 0; k < count; k++) {
        const int32_t w = widths[k], c = channels[k];
        if (w > 0 && c > 0 && P > 0 && !sources[k]) return gft_fail("gft_ply_pack: source %d is NULL", k);
        b.ptr[k] = w > 0 && c > 0 ? const_cast<float*>(sources[k]) : nullptr;
        b.width[k] = w;
        b.first[k] = col;
        b.magic[k] = ply_magic(w);
        const int32_t n = c > 0 ? w / c : w;
        for (int32_t j = 0; j < w; j++) b.map[col + j] = (uint16_t)(col + (c > 1 ? (j % c) * n + j / c : j));
        col += w;
    }
    b.count = count;
    b.total = col;
    if (P == 0) return 0;
    const int64_t blocks = (P + PLY_ROWS - 1) / PLY_ROWS;
    if (blocks > 0x7fffffffll) return gft_fail("gft_ply_pack: too many rows");
    const int32_t Ks = out_sibr ? K_sibr : K_full;
    hipLaunchKernelGGL(k_ply_pack, dim3((unsigned)blocks), dim3(PLY_THREADS), ply_lds_bytes(K_full, b.total), (hipStream_t)hip_stream, P, b,
                       (int)K_full, (int)Ks, ply_magic(Ks), out_full, out_sibr);
    return gft_launched("gft_ply_pack");
}

extern "C" int gft_ply_unpack(void* hip_stream, int64_t rows, int64_t row0, int32_t K_file, const float* chunk, int32_t count,
                              float* const* dests, const int32_t* widths, const int32_t* table)
{
    if (rows < 0 || rows > PLY_MAX_ROWS || row0 < 0 || row0 > PLY_MAX_ROWS)
        return gft_fail("gft_ply_unpack: bad rows=%lld row0=%lld", (long long)rows, (long long)row0);
    if (K_file < 1 || K_file > GFT_PLY_MAX_COLUMNS)
        return gft_fail("gft_ply_unpack: K_file=%d, a file row holds 1..%d columns", K_file, GFT_PLY_MAX_COLUMNS);
    if (count < 1 || count > GFT_PLY_MAX_SOURCES)
        return gft_fail("gft_ply_unpack: %d destination tensors, must be 1..%d", count, GFT_PLY_MAX_SOURCES);
    if (!dests || !widths || !table) return gft_fail("gft_ply_unpack: NULL argument");
    if ((uintptr_t)chunk & 15u) return gft_fail("gft_ply_unpack: chunk is not 16-byte aligned");
    PlyBlocks b = {};
    int32_t at = 0;
    for (int k = 0; k < count; k++) {
        const int32_t w = widths[k];
        if (w < 0 || w > GFT_PLY_MAX_COLUMNS - at)
            return gft_fail("gft_ply_unpack: tensor %d has width %d; the tensors hold at most %d floats per row", k, w, GFT_PLY_MAX_COLUMNS);
        if (w > 0 && rows > 0 && !dests[k]) return gft_fail("gft_ply_unpack: destination %d is NULL", k);
        b.ptr[k] = w > 0 ? dests[k] : nullptr;
        b.width[k] = w;
        b.first[k] = at;
        b.magic[k] = ply_magic(w);
        for (int32_t j = 0; j < w; j++) {
            const int32_t c = table[at + j];
            if (c < 0 || c >= K_file)
                return gft_fail("gft_ply_unpack: table entry %d names file column %d, the file has K_file=%d", at + j, c, K_file);
            b.map[at + j] = (uint16_t)c;
        }
        at += w;
    }
    b.count = count;
    b.total = at;
    if (rows == 0) return 0;
    if (!chunk) return gft_fail("gft_ply_unpack: chunk is NULL");
    const int64_t blocks = (rows + PLY_ROWS - 1) / PLY_ROWS;
    if (blocks > 0x7fffffffll) return gft_fail("gft_ply_unpack: too many rows");
    hipLaunchKernelGGL(k_ply_unpack, dim3((unsigned)blocks), dim3(PLY_THREADS), ply_lds_bytes(K_file, b.total), (hipStream_t)hip_stream, rows,
                       row0, (int)K_file, chunk, b);
    return gft_launched("gft_ply_unpack");
}

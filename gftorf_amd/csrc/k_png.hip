// k_png.hip -- PNG files formed on the device (include/gftorf_png.h states the file and the encoder's rules).
// k_png_filter:   one wave per scanline of the batch: the three filter costs, the least one's type into the scratch.
// k_png_segment:  one workgroup per 32 KiB segment of a filtered stream, the steps of gft_png_coder.h with barriers between:
//                 filtered bytes into LDS, the best of five candidate distances and one hash candidate per byte, the greedy parse (every thread's
//                 128 bytes first as an exit table, then one thread hops from thread to thread), token bits by a prefix sum,
//                 the codes ORed into LDS words, the chunk's CRC from per-thread pieces.  The chunk leaves as whole dwords into
//                 the segment's scratch slot; its size and the segment's Adler sums go into the segment's row of the table.
//                 152 KiB of LDS: one workgroup per CU.  The serial steps are latency bound (one dependent LDS round trip per
//                 byte of a thread); a batch is tens to hundreds of segments, so the device is filled by width, not by depth.
// k_png_assemble: a workgroup per segment copies the chunk behind the chunks before it (it adds up their sizes itself) and a
//                 workgroup per image writes signature, IHDR, the closing IDAT chunk with the Adler-32 folded over the
//                 segments in order, IEND and the file's size.
#include "gft_internal.h"
#include "gft_png_coder.h"
#include "gftorf_png.h"

namespace {

constexpr int PNG_META_WORDS = 4;                // per segment in the scratch: chunk bytes, Adler sum of bytes, weighted sum, segment bytes

struct PngImage {
    const uint8_t* src;
    int64_t stride;
    int64_t out_offset;
    int32_t H, L, C;                             // L = 1 + W * C
    uint32_t total;                              // H * L
    int32_t seg0, row0;                          // the image's first segment and first row in the batch
    uint32_t ldist_code, ldist_bits;
};

struct PngBatch {
    PngImage im[GFT_PNG_MAX_IMAGES];
    int32_t count, level, nseg, nrows;
    uint32_t x2n_piece, x2n_group;
};

// scratch: filter types [nrows rounded up to 16] | table [nseg][PNG_META_WORDS] | slots [nseg][GFT_PNG_CHUNK_SLOT]
__host__ __device__ inline int64_t png_types_bytes(int64_t nrows) { return (nrows + 15) & ~(int64_t)15; }
__host__ __device__ inline int64_t png_table_at(int64_t nrows) { return png_types_bytes(nrows); }
__host__ __device__ inline int64_t png_slots_at(int64_t nrows, int64_t nseg) { return png_table_at(nrows) + nseg * PNG_META_WORDS * 4; }

__global__ __launch_bounds__(PNG_THREADS) void k_png_filter(PngBatch b, uint8_t* __restrict__ scratch)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (PNG_THREADS / 64) + (threadIdx.x >> 6);          // of the batch
    if (row >= b.nrows) return;
    int i = 0;
    while (i + 1 < b.count && b.im[i + 1].row0 <= row) i++;
    const int y = row - b.im[i].row0, C = b.im[i].C, n = b.im[i].L - 1;
    const uint8_t* r = b.im[i].src + (int64_t)y * b.im[i].stride;
    const uint8_t* up = r - b.im[i].stride;
    uint32_t c0 = 0, c1 = 0, c2 = 0;
    for (int x = lane; x < n; x += 64) {
        const uint32_t v = r[x];
        const uint32_t s = (v - (x >= C ? (uint32_t)r[x - C] : 0u)) & 255u;
        const uint32_t u = (v - (y > 0 ? (uint32_t)up[x] : 0u)) & 255u;
        c0 += v < 128 ? v : 256 - v;
        c1 += s < 128 ? s : 256 - s;
        c2 += u < 128 ? u : 256 - u;
    }
    for (int k = 32; k > 0; k >>= 1) {
        c0 += __shfl_xor(c0, k, 64);
        c1 += __shfl_xor(c1, k, 64);
        c2 += __shfl_xor(c2, k, 64);
    }
    if (lane == 0) {
        uint32_t t = 0, best = c0;
        if (c1 < best) { best = c1; t = 1; }
        if (c2 < best) t = 2;
        scratch[row] = (uint8_t)t;
    }
}

__device__ __forceinline__ PngSeg png_segment_of(const PngBatch& b, const uint8_t* scratch, int g, int* image)
{
    int i = 0;
    while (i + 1 < b.count && b.im[i + 1].seg0 <= g) i++;
    const PngImage& im = b.im[i];
    PngSeg s;
    s.src = im.src;
    s.ftype = b.level >= 1 ? scratch + im.row0 : nullptr;
    s.stride = im.stride;
    s.H = im.H;
    s.L = im.L;
    s.C = im.C;
    s.p0 = (uint32_t)(g - im.seg0) * (uint32_t)PNG_SEG;
    const uint32_t rest = im.total - s.p0;
    s.n = (int32_t)(rest < (uint32_t)PNG_SEG ? rest : (uint32_t)PNG_SEG);
    s.first = g == im.seg0;
    s.level = b.level;
    s.ldist_code = im.ldist_code;
    s.ldist_bits = im.ldist_bits;
    s.x2n_piece = b.x2n_piece;
    s.x2n_group = b.x2n_group;
    *image = i;
    return s;
}

__global__ __launch_bounds__(PNG_THREADS) void k_png_segment(PngBatch b, uint8_t* __restrict__ scratch)
{
    __shared__ PngLds l;
    const int tid = threadIdx.x, g = blockIdx.x;                                   // g < b.nseg: the grid is b.nseg
    int image;
    const PngSeg s = png_segment_of(b, scratch, g, &image);
    png_step_load(l, s, tid);
    __syncthreads();
    if (b.level >= 1) {
        png_step_lead(l, s, tid);
        __syncthreads();
        png_step_match(l, s, tid);
        __syncthreads();
        png_step_exit(l, s, tid);
        __syncthreads();
    }
    png_step_chain(l, s, tid);
    __syncthreads();
    if (b.level >= 1) png_step_count(l, s, tid);
    else l.red[tid] = 0;
    __syncthreads();
    png_step_scan(l, s, tid);
    __syncthreads();
    png_step_emit(l, s, tid);
    __syncthreads();
    png_step_crc(l, s, tid);
    __syncthreads();
    png_step_fold(l, s, tid);
    __syncthreads();
    png_step_close(l, s, tid);
    __syncthreads();
    const PngForm f = png_form(s, l.total_bits);
    uint32_t* slot = reinterpret_cast<uint32_t*>(scratch + png_slots_at(b.nrows, b.nseg) + (int64_t)g * GFT_PNG_CHUNK_SLOT);
    const int words = (f.chunk_bytes + 3) >> 2;                                    // <= GFT_PNG_CHUNK_SLOT / 4
    for (int w = tid; w < words; w += PNG_THREADS) slot[w] = l.b[w];
    if (tid == 0) {
        uint32_t* row = reinterpret_cast<uint32_t*>(scratch + png_table_at(b.nrows)) + (int64_t)g * PNG_META_WORDS;
        row[0] = (uint32_t)f.chunk_bytes;
        row[1] = l.adler_a;
        row[2] = l.adler_b;
        row[3] = (uint32_t)s.n;
    }
}

__device__ __forceinline__ uint32_t png_crc_bytes(uint32_t c, const uint8_t* p, int n)
{
    for (int k = 0; k < n; k++) c = png_crc_byte(c, p[k]);
    return c;
}

__device__ __forceinline__ void png_be32(uint8_t* p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

constexpr int PNG_HEAD = 33;                     // signature and IHDR
constexpr int PNG_TAIL = 21 + 12;                // the closing IDAT chunk and IEND

__global__ __launch_bounds__(PNG_THREADS) void k_png_assemble(PngBatch b, const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
                                                              int64_t* __restrict__ sizes)
{
    __shared__ uint32_t part[PNG_THREADS];
    __shared__ uint32_t sum;
    const int tid = threadIdx.x, g = blockIdx.x;                                   // the grid is b.nseg + b.count
    const uint32_t* table = reinterpret_cast<const uint32_t*>(scratch + png_table_at(b.nrows));
    if (g < b.nseg) {
        int i = 0;
        while (i + 1 < b.count && b.im[i + 1].seg0 <= g) i++;
        uint32_t before = 0;
        for (int k = b.im[i].seg0 + tid; k < g; k += PNG_THREADS) before += table[(int64_t)k * PNG_META_WORDS];
        part[tid] = before;
        __syncthreads();
        if (tid == 0) {
            uint32_t t = 0;
            for (int k = 0; k < PNG_THREADS; k++) t += part[k];
            sum = t;
        }
        __syncthreads();
        const int nbytes = (int)table[(int64_t)g * PNG_META_WORDS];
        uint8_t* dst = out + b.im[i].out_offset + PNG_HEAD + (int64_t)sum;
        const uint8_t* srcb = scratch + png_slots_at(b.nrows, b.nseg) + (int64_t)g * GFT_PNG_CHUNK_SLOT;   // 16-byte aligned
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(srcb);
        // dst + head is dword aligned; the dwords from there on are funnelled out of two dwords of the slot (reading one
        // dword past the chunk's last stays inside the slot: the longest chunk is 13 bytes short of it)
        const int head = (int)((4u - ((uintptr_t)dst & 3u)) & 3u);                 // a chunk is 13 bytes at least
        const int whole = (nbytes - head) >> 2;
        if (tid < head) dst[tid] = srcb[tid];
        uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
        const int sh = 8 * head;                                                   // head is the slot's byte of dw[0]
        for (int w = tid; w < whole; w += PNG_THREADS)
            dw[w] = sh ? (srcw[w] >> sh) | (srcw[w + 1] << (32 - sh)) : srcw[w];
        const int done = head + 4 * whole;
        if (tid < nbytes - done) dst[done + tid] = srcb[done + tid];
        return;
    }
    if (tid != 0) return;
    const PngImage& im = b.im[g - b.nseg];
    uint8_t* file = out + im.out_offset;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int k = 0; k < 8; k++) file[k] = sig[k];
    uint8_t* h = file + 8;
    png_be32(h, 13);
    h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
    png_be32(h + 8, (uint32_t)((im.L - 1) / im.C));
    png_be32(h + 12, (uint32_t)im.H);
    h[16] = 8;
    h[17] = im.C == 1 ? 0 : (im.C == 3 ? 2 : 6);
    h[18] = 0; h[19] = 0; h[20] = 0;
    png_be32(h + 21, ~png_crc_bytes(0xffffffffu, h + 4, 17));
    uint32_t a = 1, bsum = 0;
    int64_t bytes = 0;
    const int nseg = (int)((im.total + (uint32_t)PNG_SEG - 1u) / (uint32_t)PNG_SEG);
    for (int k = im.seg0; k < im.seg0 + nseg; k++) {
        const uint32_t* row = table + (int64_t)k * PNG_META_WORDS;
        bytes += row[0];
        bsum = (uint32_t)(((uint64_t)bsum + (uint64_t)row[3] * a + row[2]) % PNG_ADLER);
        a = (a + row[1]) % PNG_ADLER;
    }
    uint8_t* t = file + PNG_HEAD + bytes;
    png_be32(t, 9);
    t[4] = 'I'; t[5] = 'D'; t[6] = 'A'; t[7] = 'T';
    t[8] = 1; t[9] = 0; t[10] = 0; t[11] = 0xff; t[12] = 0xff;
    png_be32(t + 13, (bsum << 16) | a);
    png_be32(t + 17, ~png_crc_bytes(0xffffffffu, t + 4, 13));
    png_be32(t + 21, 0);
    t[25] = 'I'; t[26] = 'E'; t[27] = 'N'; t[28] = 'D';
    png_be32(t + 29, ~png_crc_bytes(0xffffffffu, t + 25, 4));
    sizes[g - b.nseg] = PNG_HEAD + bytes + PNG_TAIL;
}

int64_t png_stream_bytes(int32_t H, int32_t W, int32_t C)
{
    if (H < 1 || W < 1 || (C != 1 && C != 3 && C != 4)) return -1;
    const int64_t L = 1 + (int64_t)W * C;
    if (L > GFT_PNG_MAX_STREAM || (int64_t)H * L > GFT_PNG_MAX_STREAM) return -1;
    return (int64_t)H * L;
}

}  // namespace

extern "C" int64_t gft_png_bound(int32_t H, int32_t W, int32_t channels)
{
    const int64_t total = png_stream_bytes(H, W, channels);
    if (total < 0) return -1;
    const int64_t nseg = (total + PNG_SEG - 1) / PNG_SEG;
    return PNG_HEAD + 2 + nseg * (12 + 5) + total + PNG_TAIL;
}

extern "C" int64_t gft_png_scratch_bytes(int32_t count, const gft_png_image* images)
{
    if (count < 1 || count > GFT_PNG_MAX_IMAGES || !images) return -1;
    int64_t nrows = 0, nseg = 0;
    for (int i = 0; i < count; i++) {
        const int64_t total = png_stream_bytes(images[i].H, images[i].W, images[i].channels);
        if (total < 0) return -1;
        nrows += images[i].H;
        nseg += (total + PNG_SEG - 1) / PNG_SEG;
    }
    return png_slots_at(nrows, nseg) + nseg * GFT_PNG_CHUNK_SLOT;
}

extern "C" int gft_png_encode(void* hip_stream, int32_t count, const gft_png_image* images, int32_t level, void* out, int64_t out_bytes,
                              int64_t* sizes, void* scratch, int64_t scratch_bytes)
{
    if (count < 1 || count > GFT_PNG_MAX_IMAGES)
        return gft_fail("gft_png_encode: %d images, a call takes 1..%d", count, GFT_PNG_MAX_IMAGES);
    if (!images || !out || !sizes || !scratch) return gft_fail("gft_png_encode: NULL argument");
    if (level != 0 && level != 1) return gft_fail("gft_png_encode: level=%d, must be 0 or 1", level);
    if ((uintptr_t)scratch & 15u) return gft_fail("gft_png_encode: scratch is not 16-byte aligned");
    static const PngBatch zero = {};
    PngBatch b = zero;
    int64_t nrows = 0, nseg = 0;
    for (int i = 0; i < count; i++) {
        const gft_png_image& g = images[i];
        const int64_t total = png_stream_bytes(g.H, g.W, g.channels);
        if (total < 0) return gft_fail("gft_png_encode: image %d is H=%d W=%d channels=%d", i, g.H, g.W, g.channels);
        if (!g.src) return gft_fail("gft_png_encode: image %d has no source", i);
        const int64_t L = 1 + (int64_t)g.W * g.channels, bound = gft_png_bound(g.H, g.W, g.channels);
        if (g.row_stride < L - 1 && g.H > 1) return gft_fail("gft_png_encode: image %d has row stride %lld, a row is %lld bytes", i, (long long)g.row_stride, (long long)(L - 1));
        if (g.out_offset < 0 || g.out_offset > out_bytes - bound)
            return gft_fail("gft_png_encode: image %d needs %lld bytes at offset %lld, out holds %lld", i, (long long)bound, (long long)g.out_offset, (long long)out_bytes);
        for (int k = 0; k < i; k++) {
            const int64_t other = gft_png_bound(images[k].H, images[k].W, images[k].channels);
            if (g.out_offset < images[k].out_offset + other && images[k].out_offset < g.out_offset + bound)
                return gft_fail("gft_png_encode: the slots of images %d and %d overlap", k, i);
        }
        PngImage& im = b.im[i];
        im.src = static_cast<const uint8_t*>(g.src);
        im.stride = g.row_stride;
        im.out_offset = g.out_offset;
        im.H = g.H;
        im.C = g.channels;
        im.L = (int32_t)L;
        im.total = (uint32_t)total;
        im.seg0 = (int32_t)nseg;
        im.row0 = (int32_t)nrows;
        im.ldist_code = png_distance_bits((uint32_t)(L < 32768 ? L : 32768), &im.ldist_bits);      // L >= 32768 never matches
        nrows += g.H;
        nseg += (total + PNG_SEG - 1) / PNG_SEG;
        if (nrows > 0x7fffffffll - 4 || nseg > 0x7fffffffll - GFT_PNG_MAX_IMAGES) return gft_fail("gft_png_encode: the batch is too large");
    }
    if (scratch_bytes < png_slots_at(nrows, nseg) + nseg * GFT_PNG_CHUNK_SLOT)
        return gft_fail("gft_png_encode: scratch holds %lld bytes, the batch needs %lld", (long long)scratch_bytes,
                        (long long)(png_slots_at(nrows, nseg) + nseg * GFT_PNG_CHUNK_SLOT));
    b.count = count;
    b.level = level;
    b.nseg = (int32_t)nseg;
    b.nrows = (int32_t)nrows;
    uint32_t x = 0x40000000u;                                                       // x^1; squared k times: x^(2^k)
    for (int k = 1; k <= 15; k++) {
        x = png_mulmod(x, x);
        if (k == 11) b.x2n_piece = x;                                               // 8 * PNG_PIECE = 2^11 bits
        if (k == 15) b.x2n_group = x;                                               // 8 * PNG_PIECE * PNG_GROUP = 2^15
    }
    static_assert(sizeof(PngBatch) <= 3840 && PNG_PIECE == 256 && PNG_GROUP == 16, "the two CRC shifts above");
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t* sc = static_cast<uint8_t*>(scratch);
    if (level >= 1)
        hipLaunchKernelGGL(k_png_filter, dim3((unsigned)((nrows + PNG_THREADS / 64 - 1) / (PNG_THREADS / 64))), dim3(PNG_THREADS), 0, stream, b, sc);
    hipLaunchKernelGGL(k_png_segment, dim3((unsigned)nseg), dim3(PNG_THREADS), 0, stream, b, sc);
    hipLaunchKernelGGL(k_png_assemble, dim3((unsigned)(nseg + count)), dim3(PNG_THREADS), 0, stream, b, (const uint8_t*)sc, static_cast<uint8_t*>(out), sizes);
    return gft_launched("gft_png_encode");
}

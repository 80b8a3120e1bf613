// k_views.hip -- the training views on the device (include/gftorf_views.h; train.py:155-163, 184-187, 219-220).
//   k_views_draw           view v's slab of the arena into the current buffer.  The grid is cut into segments, one per image
//                          group and one for the record; a workgroup moves VW_CHUNKS 16-byte chunks of a float32 segment
//                          (four 16-byte loads in flight per thread, lanes on consecutive chunks) or VW_CHUNKS pixels of a uint8
//                          segment (its interleaved bytes through LDS as whole 16-byte chunks, then one planar 16-byte store
//                          per thread and channel).  Every segment starts on a 16-byte boundary and is padded to one, so
//                          there is no byte path.  v comes by value or from order[cursor % N]; then the last workgroup to
//                          finish -- by a ticket word -- leaves cursor + 1 behind.
//   k_views_select_plane   out = x[p] / g_x = (plane p: g_out, every other plane: zeros), p read on the device
// No memset and no atomic but the ticket's; the kernels have no scratch and k_views_draw 4 KB of LDS.
#include "gft_internal.h"
#include "gftorf_views.h"

namespace {

constexpr int VW_THREADS = 256, VW_CHUNKS = GFT_VIEWS_CHUNKS, VW_PER_THREAD = VW_CHUNKS / VW_THREADS;
constexpr int VW_SEGMENTS = GFT_VIEWS_MAX_GROUPS + 1;
constexpr int64_t VW_MAX_SLAB = 1ll << 40;
static_assert(VW_PER_THREAD == 4, "a thread of k_views_draw moves four chunks, or the four pixels of one planar store");

// a 16-byte access that needs its element's alignment only: the planes of a [C, H, W] image start at multiples of 4 H W bytes
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
// a 16-byte chunk (the compiler's own vector type: an array of HIP's uint4 struct is copied through scratch)
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

int64_t align_up(int64_t v) { return (v + GFT_VIEWS_ALIGN - 1) / GFT_VIEWS_ALIGN * GFT_VIEWS_ALIGN; }

struct Plan {
    int64_t slab_bytes, current_bytes;
    int64_t slab_off[VW_SEGMENTS], current_off[VW_SEGMENTS];       // the groups, then the record
    int64_t slab_len[VW_SEGMENTS], current_len[VW_SEGMENTS];       // padded bytes
};

// The one statement of the layout: the record first in a slab (behind the header in the current buffer), then the groups in
// their order, each padded to GFT_VIEWS_ALIGN.
bool make_plan(int32_t F, int32_t J, int32_t count, const int32_t* kinds, const int32_t* C, const int32_t* H, const int32_t* W, Plan& p)
{
    if (count < 0 || count > GFT_VIEWS_MAX_GROUPS || F < 0 || J < 0) return false;
    if (count == 0 && F == 0 && J == 0) return false;
    if (count > 0 && (!kinds || !C || !H || !W)) return false;
    const int64_t record = align_up(((int64_t)F + J) * 4);
    int64_t s = record, c = GFT_VIEWS_HEADER_BYTES + record;
    p.slab_off[count] = 0; p.current_off[count] = GFT_VIEWS_HEADER_BYTES;
    p.slab_len[count] = p.current_len[count] = record;
    for (int g = 0; g < count; g++) {
        if (C[g] < 1 || H[g] < 1 || W[g] < 1) return false;
        if (kinds[g] != GFT_VIEWS_F32 && kinds[g] != GFT_VIEWS_U8) return false;
        if (kinds[g] == GFT_VIEWS_U8 && C[g] > 4) return false;
        const int64_t hw = (int64_t)H[g] * W[g];
        if (hw > VW_MAX_SLAB / 4 / C[g]) return false;
        const int64_t n = hw * C[g];
        p.slab_off[g] = s; p.current_off[g] = c;
        p.slab_len[g] = align_up(kinds[g] == GFT_VIEWS_U8 ? n : 4 * n);
        p.current_len[g] = align_up(4 * n);
        s += p.slab_len[g]; c += p.current_len[g];
        if (s > VW_MAX_SLAB || c > VW_MAX_SLAB) return false;
    }
    p.slab_bytes = s; p.current_bytes = c;
    return true;
}

struct Segment {
    int64_t src, dst;               // byte offsets in the slab and in the current buffer
    int64_t units;                  // 16-byte chunks, or the pixels of a uint8 group
    int64_t hw;                     // pixels of a plane (uint8 group)
    uint32_t first_block;
    int32_t channels;               // 0: a copy; 1..4: a uint8 group of that many channels
};

struct DrawArgs {
    const uint8_t* __restrict__ arena;
    uint8_t* __restrict__ current;
    int64_t V, slab_bytes, index;
    const int32_t* __restrict__ order;
    int32_t* cursor;
    int32_t* ticket;
    uint32_t N;
    int32_t segments;
    Segment seg[VW_SEGMENTS];
};

__global__ __launch_bounds__(VW_THREADS) void k_views_draw(DrawArgs a)
{
    __shared__ u4 s_bytes[VW_THREADS];           // a uint8 tile: VW_CHUNKS pixels of up to 4 bytes
    __shared__ int64_t s_view;
    __shared__ int32_t s_cursor;
    const int tid = threadIdx.x;
    // One thread reads the schedule for its workgroup: its read has returned before the barrier, hence before this workgroup's
    // ticket, hence before the last workgroup's write of the cursor.
    if (tid == 0) {
        int64_t v = a.index;
        int32_t c = -1;
        if (a.order) {
            c = *(volatile const int32_t*)a.cursor;
            v = a.order[(uint32_t)c % a.N];
        }
        s_view = v < 0 ? 0 : (v >= a.V ? a.V - 1 : v);
        s_cursor = c;
    }
    __syncthreads();
    const int64_t view = s_view;
    if (blockIdx.x == 0 && tid == 0) {
        int32_t* head = reinterpret_cast<int32_t*>(a.current);
        head[GFT_VIEWS_INDEX_WORD] = (int32_t)view;
        head[GFT_VIEWS_CURSOR_WORD] = s_cursor;
    }
    // (selects over constant indices: an index computed here would move the argument block to scratch)
    Segment sg = a.seg[0];
#pragma unroll
    for (int k = 1; k < VW_SEGMENTS; k++)
        if (k < a.segments && blockIdx.x >= a.seg[k].first_block) sg = a.seg[k];
    const int64_t unit0 = (int64_t)(blockIdx.x - sg.first_block) * VW_CHUNKS;
    const uint8_t* src = a.arena + view * a.slab_bytes + sg.src;
    uint8_t* dst = a.current + sg.dst;
    if (sg.channels == 0) {
        const u4* in = reinterpret_cast<const u4*>(src);
        u4* out = reinterpret_cast<u4*>(dst);
        u4 v[VW_PER_THREAD];
#pragma unroll
        for (int j = 0; j < VW_PER_THREAD; j++) {
            const int64_t i = unit0 + j * VW_THREADS + tid;
            if (i < sg.units) v[j] = in[i];
        }
#pragma unroll
        for (int j = 0; j < VW_PER_THREAD; j++) {
            const int64_t i = unit0 + j * VW_THREADS + tid;
            if (i < sg.units) out[i] = v[j];
        }
    } else {
        // pixels unit0 .. unit0 + n - 1 of the group: their n C bytes start at a multiple of 16 (VW_CHUNKS C is one) and end
        // inside the group's padding
        const int C = sg.channels;
        const int64_t left = sg.units - unit0;
        const int n = (int)(left < VW_CHUNKS ? left : VW_CHUNKS);
        const int chunks = (n * C + 15) >> 4;
        if (tid < chunks) s_bytes[tid] = reinterpret_cast<const u4*>(src + unit0 * C)[tid];
        __syncthreads();
        const int mine = n - VW_PER_THREAD * tid;                      // pixels of this thread: 4 tid .. 4 tid + 3 of the tile
        if (mine > 0) {
            const uint32_t* words = reinterpret_cast<const uint32_t*>(s_bytes) + tid * C;     // their 4 C bytes
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = k < C ? words[k] : 0u;
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (c < C) {
                    float f[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int b = i * C + c;                        // byte of the thread's 4 C
                        uint32_t word = w[0];
#pragma unroll
                        for (int k = 1; k < 4; k++) word = (b >> 2) == k ? w[k] : word;
                        f[i] = (float)((word >> (8 * (b & 3))) & 0xffu) / 255.0f;       // IEEE division, as torch's `/ 255.0`
                    }
                    float* plane = reinterpret_cast<float*>(dst) + c * sg.hw + unit0 + VW_PER_THREAD * tid;
                    if (mine >= 4) {
                        f4u q = {f[0], f[1], f[2], f[3]};
                        *reinterpret_cast<f4u*>(plane) = q;
                    } else {
#pragma unroll
                        for (int i = 0; i < 3; i++)
                            if (i < mine) plane[i] = f[i];
                    }
                }
        }
    }
    if (a.order) {
        __syncthreads();
        // (relaxed: the ticket orders nothing but this workgroup's read of the cursor above, which has returned; what the
        // launch writes reaches the next launch at the kernel's end)
        if (tid == 0 && __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int32_t)gridDim.x - 1) {
            *a.cursor = (int32_t)((uint32_t)s_cursor + 1u);
            __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

struct PlaneArgs {
    const float* __restrict__ in;       // x, or g_out
    float* __restrict__ out;            // out, or g_x
    int64_t plane, index;
    const int32_t* __restrict__ index_dev;
    const int32_t* __restrict__ table;
    int32_t C, modulo, T;
};

__device__ __forceinline__ int64_t chosen_plane(const PlaneArgs& a)
{
    int64_t i = a.index_dev ? (int64_t)*a.index_dev : a.index;
    if (a.modulo > 0) i = ((i % a.modulo) + a.modulo) % a.modulo;
    int64_t p = i;
    if (a.table) p = a.table[i < 0 ? 0 : (i >= a.T ? a.T - 1 : i)];
    return p < 0 ? 0 : (p >= a.C ? a.C - 1 : p);
}

__global__ __launch_bounds__(VW_THREADS) void k_views_select_plane(PlaneArgs a)
{
    const float* src = a.in + chosen_plane(a) * a.plane;
    const int64_t quads = (a.plane + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * VW_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * VW_THREADS) {
        const int64_t e = 4 * q;
        if (e + 4 <= a.plane) {
            *reinterpret_cast<f4u*>(a.out + e) = *reinterpret_cast<const f4u*>(src + e);
        } else {
            for (int64_t i = e; i < a.plane; i++) a.out[i] = src[i];
        }
    }
}

__global__ __launch_bounds__(VW_THREADS) void k_views_select_plane_backward(PlaneArgs a)
{
    const int64_t lo = chosen_plane(a) * a.plane, total = (int64_t)a.C * a.plane;
    const int64_t quads = (total + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * VW_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * VW_THREADS) {
        const int64_t e = 4 * q;
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int64_t r = e + i - lo;
            f[i] = (r >= 0 && r < a.plane && e + i < total) ? a.in[r] : 0.f;
        }
        if (e + 4 <= total) {
            f4u v = {f[0], f[1], f[2], f[3]};
            *reinterpret_cast<f4u*>(a.out + e) = v;
        } else {
            for (int i = 0; e + i < total; i++) a.out[e + i] = f[i];
        }
    }
}

int plane_launch(hipStream_t s, bool backward, int32_t C, int64_t plane, const float* in, int64_t index, const int32_t* index_dev,
                 int32_t modulo, const int32_t* table, int32_t T, float* out, const char* who)
{
    if (C < 1 || plane < 1 || plane > (1ll << 40) / C) return gft_fail("%s: bad shape C=%d, H W=%lld", who, (int)C, (long long)plane);
    if (!in || !out) return gft_fail("%s: NULL argument", who);
    if (modulo < 0) return gft_fail("%s: modulo=%d is negative", who, (int)modulo);
    if (table && T < 1) return gft_fail("%s: a table of %d entries", who, (int)T);
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) return gft_fail("%s: a pointer is not 4-byte aligned", who);
    PlaneArgs a = {};
    a.in = in; a.out = out; a.plane = plane; a.index = index; a.index_dev = index_dev; a.table = table; a.C = C; a.modulo = modulo;
    a.T = T;
    const int64_t quads = ((backward ? C * plane : plane) + 3) / 4;
    int64_t blocks = (quads + VW_THREADS - 1) / VW_THREADS;
    if (blocks > 4096) blocks = 4096;
    if (backward)
        hipLaunchKernelGGL(k_views_select_plane_backward, dim3((unsigned)blocks), dim3(VW_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(k_views_select_plane, dim3((unsigned)blocks), dim3(VW_THREADS), 0, s, a);
    return gft_launched(who);
}

}  // namespace

extern "C" int64_t gft_views_layout(int32_t F, int32_t J, int32_t count, const int32_t* kinds, const int32_t* C, const int32_t* H,
                                    const int32_t* W, int64_t* current_bytes, int64_t* slab_offsets, int64_t* current_offsets)
{
    Plan p;
    if (!make_plan(F, J, count, kinds, C, H, W, p)) return 0;
    if (current_bytes) *current_bytes = p.current_bytes;
    for (int g = 0; g <= count; g++) {
        if (slab_offsets) slab_offsets[g] = p.slab_off[g];
        if (current_offsets) current_offsets[g] = p.current_off[g];
    }
    return p.slab_bytes;
}

extern "C" int gft_views_draw(void* hip_stream, int32_t F, int32_t J, int32_t count, const int32_t* kinds, const int32_t* C,
                              const int32_t* H, const int32_t* W, const void* arena, void* current, int64_t V, int64_t index,
                              const int32_t* order, int32_t* cursor, int64_t N, int32_t* ticket)
{
    Plan p;
    if (!make_plan(F, J, count, kinds, C, H, W, p)) return gft_fail("gft_views_draw: the views cannot be laid out (gft_views_layout returns 0)");
    if (!arena || !current) return gft_fail("gft_views_draw: NULL argument");
    if ((reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(current)) & (GFT_VIEWS_ALIGN - 1))
        return gft_fail("gft_views_draw: the arena and the current buffer must be %d-byte aligned", GFT_VIEWS_ALIGN);
    if (V < 1 || V > 0x7fffffffll) return gft_fail("gft_views_draw: V=%lld views", (long long)V);
    if (order) {
        if (!cursor || !ticket) return gft_fail("gft_views_draw: a schedule needs its cursor and its ticket word");
        if (N < 1 || N > 0x7fffffffll) return gft_fail("gft_views_draw: a schedule of N=%lld entries", (long long)N);
    } else if (index < 0 || index >= V) {
        return gft_fail("gft_views_draw: index=%lld is not in [0, %lld)", (long long)index, (long long)V);
    }
    DrawArgs a = {};
    a.arena = static_cast<const uint8_t*>(arena); a.current = static_cast<uint8_t*>(current);
    a.V = V; a.slab_bytes = p.slab_bytes; a.index = index; a.order = order; a.cursor = cursor; a.ticket = ticket;
    a.N = order ? (uint32_t)N : 1u;
    int64_t blocks = 0;
    // the record first: its workgroup is one of the first to run, and the iteration's first kernels read the cameras
    for (int k = 0; k <= count; k++) {
        const int g = k == 0 ? count : k - 1;
        if (p.slab_len[g] == 0) continue;
        Segment& sg = a.seg[a.segments++];
        sg.src = p.slab_off[g]; sg.dst = p.current_off[g];
        sg.first_block = (uint32_t)blocks;
        if (g < count && kinds[g] == GFT_VIEWS_U8) {
            sg.channels = C[g];
            sg.hw = (int64_t)H[g] * W[g];
            sg.units = sg.hw;
        } else {
            sg.units = p.slab_len[g] / GFT_VIEWS_ALIGN;
        }
        blocks += (sg.units + VW_CHUNKS - 1) / VW_CHUNKS;
        if (blocks > 0x7fffffffll) return gft_fail("gft_views_draw: a view of %lld bytes is too large for one launch", (long long)p.slab_bytes);
    }
    hipLaunchKernelGGL(k_views_draw, dim3((unsigned)blocks), dim3(VW_THREADS), 0, (hipStream_t)hip_stream, a);
    return gft_launched("gft_views_draw");
}

extern "C" int gft_views_select_plane(void* hip_stream, int32_t C, int64_t plane, const float* x, int64_t index, const int32_t* index_dev,
                                      int32_t modulo, const int32_t* table, int32_t T, float* out)
{
    return plane_launch((hipStream_t)hip_stream, false, C, plane, x, index, index_dev, modulo, table, T, out, "gft_views_select_plane");
}

extern "C" int gft_views_select_plane_backward(void* hip_stream, int32_t C, int64_t plane, const float* g_out, int64_t index,
                                               const int32_t* index_dev, int32_t modulo, const int32_t* table, int32_t T, float* g_x)
{
    return plane_launch((hipStream_t)hip_stream, true, C, plane, g_out, index, index_dev, modulo, table, T, g_x,
                        "gft_views_select_plane_backward");
}

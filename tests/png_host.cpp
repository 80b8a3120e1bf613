// The segment coder of csrc/gft_png_coder.h run on the host, thread by thread and step by step, in the order k_png_segment
// calls the steps (tests/test_png_host.py builds this with the address and undefined-behaviour sanitizers and compares what
// it writes with the numpy model).  Arguments: pairs of an input and an output file.  Input file: int32 H, W, C, level; H filter
// types; H * W * C image bytes.  Output file, per segment: uint32 chunk bytes, Adler byte sum, Adler weighted sum; then the
// chunk's bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gft_png_coder.h"

template <class Step>
static void all_threads(Step step)
{
    for (int tid = 0; tid < PNG_THREADS; tid++) step(tid);
}

static int run(const char* in_path, const char* out_path)
{
    FILE* in = fopen(in_path, "rb");
    if (!in) return 3;
    int32_t head[4];
    if (fread(head, 4, 4, in) != 4) return 4;
    const int32_t H = head[0], W = head[1], C = head[2], level = head[3];
    std::vector<uint8_t> types(H), image((size_t)H * W * C);        // exact sizes: a read past either is reported
    if (fread(types.data(), 1, types.size(), in) != types.size()) return 5;
    if (fread(image.data(), 1, image.size(), in) != image.size()) return 6;
    fclose(in);
    FILE* out = fopen(out_path, "wb");
    if (!out) return 7;
    const int64_t L = 1 + (int64_t)W * C, total = H * L;
    std::unique_ptr<PngLds> lds(new PngLds);
    uint32_t x = 0x40000000u, x2n_piece = 0, x2n_group = 0;
    for (int k = 1; k <= 15; k++) {
        x = png_mulmod(x, x);
        if (k == 11) x2n_piece = x;
        if (k == 15) x2n_group = x;
    }
    for (int64_t p0 = 0; p0 < total; p0 += PNG_SEG) {
        memset(lds.get(), 0xa5, sizeof(PngLds));                      // LDS holds anything when a workgroup starts
        PngLds& l = *lds;
        PngSeg s;
        s.src = image.data();
        s.ftype = level >= 1 ? types.data() : nullptr;
        s.stride = (int64_t)W * C;
        s.H = H;
        s.L = (int32_t)L;
        s.C = C;
        s.p0 = (uint32_t)p0;
        s.n = (int32_t)(total - p0 < PNG_SEG ? total - p0 : PNG_SEG);
        s.first = p0 == 0;
        s.level = level;
        s.ldist_code = png_distance_bits((uint32_t)(L < 32768 ? L : 32768), &s.ldist_bits);      // as gft_png_encode does
        s.x2n_piece = x2n_piece;
        s.x2n_group = x2n_group;
        all_threads([&](int tid) { png_step_load(l, s, tid); });
        if (level >= 1) {
            all_threads([&](int tid) { png_step_lead(l, s, tid); });
            all_threads([&](int tid) { png_step_match(l, s, tid); });
            all_threads([&](int tid) { png_step_exit(l, s, tid); });
        }
        all_threads([&](int tid) { png_step_chain(l, s, tid); });
        all_threads([&](int tid) { if (level >= 1) png_step_count(l, s, tid); else l.red[tid] = 0; });
        all_threads([&](int tid) { png_step_scan(l, s, tid); });
        all_threads([&](int tid) { png_step_emit(l, s, tid); });
        all_threads([&](int tid) { png_step_crc(l, s, tid); });
        all_threads([&](int tid) { png_step_fold(l, s, tid); });
        all_threads([&](int tid) { png_step_close(l, s, tid); });
        const PngForm f = png_form(s, l.total_bits);
        if (f.chunk_bytes > GFT_PNG_CHUNK_SLOT) return 8;
        const uint32_t row[3] = {(uint32_t)f.chunk_bytes, l.adler_a, l.adler_b};
        fwrite(row, 4, 3, out);
        fwrite(l.b, 1, (size_t)f.chunk_bytes, out);
    }
    fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3 || !(argc & 1)) return 2;
    for (int k = 1; k + 1 < argc; k += 2) {
        const int rc = run(argv[k], argv[k + 1]);
        if (rc) return rc;
    }
    return 0;
}

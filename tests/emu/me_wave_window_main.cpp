// Stand-alone check that the wave kernel of the full-pel search reads nothing outside its operands: links the CPU interpreter build of the kernel sources, all of it
// compiled with -fsanitize=address,undefined (tests/emu/Makefile: `make -C tests/emu asan-run`).  Every operand is a heap block of its exact size: the reference
// window begins at the block's first byte and ends at its last one ((rows - 1) * stride + width bytes), the 64x64 source block likewise, so a read of one byte in
// front of, behind or below the window is a report with a stack.  Widths and heights are those at which stage_window_wave takes another path, and those that put the
// last step of a column on every position of the ring (tests/test_me_wave_start.py runs the same areas against the checker).  Exit status 0 = no report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/svtav1_hip.h"

static int run(int W, int H, int sub_sad, uint32_t stride_pad) {
    const int      width = 64 + W - 1, rows = 64 + H - 1;
    const uint32_t rstride = (uint32_t)width + stride_pad, sstride = 64;
    const size_t   rbytes = (size_t)(rows - 1) * rstride + (size_t)width, sbytes = 64 * 64;
    uint8_t*       ref = (uint8_t*)malloc(rbytes);
    uint8_t*       src = (uint8_t*)malloc(sbytes);
    SvtHipMeSearchDesc* d  = (SvtHipMeSearchDesc*)malloc(sizeof(SvtHipMeSearchDesc));
    uint32_t*      bs = (uint32_t*)malloc(SVT_HIP_ME_NUM_BLOCKS * 4);
    uint32_t*      bm = (uint32_t*)malloc(SVT_HIP_ME_NUM_BLOCKS * 4);
    uint32_t       x  = 12345u + (uint32_t)(W * 131 + H * 7 + sub_sad);
    for (size_t i = 0; i < rbytes; i++) { x = x * 1664525u + 1013904223u; ref[i] = (uint8_t)(x >> 24); }
    for (size_t i = 0; i < sbytes; i++) { x = x * 1664525u + 1013904223u; src[i] = (uint8_t)(x >> 24); }
    memset(d, 0, sizeof(*d));
    d->src_stride = sstride;
    d->ref_stride = rstride;
    d->x_search_area_origin = (int16_t)-(W >> 1);
    d->y_search_area_origin = (int16_t)-(H >> 1);
    d->search_area_width    = (uint16_t)W;
    d->search_area_height   = (uint16_t)H;
    memset(bs, 0xff, SVT_HIP_ME_NUM_BLOCKS * 4);
    svt_hip_me_fullpel_search_batch(src, ref, d, 1, (uint32_t)W, (uint32_t)H, sub_sad, bs, bm, nullptr, nullptr);
    int bad = 0;
    for (int k = 0; k < SVT_HIP_ME_NUM_BLOCKS; k++) bad |= bs[k] == 0xffffffffu; // every block found a position
    free(bm); free(bs); free(d); free(src); free(ref);
    return bad;
}

int main() {
    if (svt_hip_init(0) != 0) { fprintf(stderr, "svt_hip_init failed\n"); return 2; }
    static const int widths[]  = {1, 2, 8, 9, 16, 17, 18, 24};
    static const int heights[] = {1, 2, 9, 13, 16};
    static const int ring[][2] = {{4, 1}, {4, 2}, {4, 7}, {4, 8}, {4, 9}, {8, 15}, {8, 16}, {24, 16}};
    int n = 0, bad = 0;
    for (int sub = 0; sub < 2; sub++) {
        for (int W : widths)
            for (int H : heights) { bad |= run(W, H, sub, 37); bad |= run(W, H, sub, 0); n += 2; } // (stride == width: the next row starts where this one ends)
        for (auto& a : ring) { bad |= run(a[0], a[1], sub, 5); n++; }
    }
    printf("me_wave_window: %d launches, %s\n", n, bad ? "a block without a result" : "no report");
    return bad;
}

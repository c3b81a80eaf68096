// What the two-pass exact distance transforms share (seg_loss.hip: s2e_seg_dist_maps; mask_clean.hip: the nearest-class
// fill): a column pass keeps the vertical distance of every pixel to the nearest pixel of a set in its column as uint16,
// a row pass squares them and takes min over x' of (x - x')^2 + g(x')^2.  The limits and sentinels of that scheme live here.
#pragma once
#include "common.h"

namespace {

constexpr int DIST_MAX_SIDE = 1024;                          // H and W at most: uint16 distances, and rint(sqrtf(m)^2) == m up to 2 * 1023^2
constexpr int DIST_COL_THREADS = 64;                         // one wave per column-pass workgroup: N ncls ceil(W / 64) workgroups
constexpr int DIST_COL_DEPTH = 32;                           // rows of a lane whose loads are in flight together: the walk is a chain of load latencies
constexpr uint32_t DIST_NONE16 = 0xFFFFu;                    // a column without a pixel of the set
constexpr uint32_t DIST_NONE = 0x40000000u;                  // a squared distance no pixel has; (x - x')^2 added to it does not wrap

// the square of a column distance, the sentinel kept
__device__ __forceinline__ uint32_t dist_sq16(uint32_t g) { return g == DIST_NONE16 ? DIST_NONE : g * g; }
// the column distance from row y to the last row seen of the set (-1: none yet), walking either way
__device__ __forceinline__ uint32_t dist_to_last(int y, int last) { return last < 0 ? DIST_NONE16 : (uint32_t)(y > last ? y - last : last - y); }
// threads of a row-pass workgroup: W rounded up to whole waves, at most `cap` (a 40-pixel row takes one wave, not four)
static inline int dist_row_threads(int W, int cap) { return W >= cap ? cap : ceil_div(W, 64) * 64; }

}  // namespace

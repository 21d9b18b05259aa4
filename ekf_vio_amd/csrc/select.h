// ekf_vio_amd/csrc/select.h — the integer pieces of the replenishment's selection (include/ekfvio.h, ekfvio_replenish and
// ekfvio_set_replenish_grid): the lines of its specification, shared by replenish_select_kernel (fast.hip) and the host function
// ekfvio_replenish_select: one set of inline functions, compiled for the host and for the device.  Everything is integer work, so both
// give the pixels of a pure-Python restatement (tests/_replenish_grid.py).  The per-cell maximum comes from LDS atomics on the device and
// from a loop on the host; the order of the cells from a count of smaller keys there and from the same count here.
#pragma once
#include <stdint.h>

#define SELECT_MAX_CELLS 256  // cells_x * cells_y of ekfvio_set_replenish_grid: one cell per lane of the selection's workgroup
#define SELECT_MAX_RADIUS 63  // min_new_feature_dist: two passes of 64 circle rows (fast.hip, OCC_PASSES)

// drawing.cpp Circle(), filled: half-width of the span in row cy + dyrow (-1: the row is outside the circle)
__host__ __device__ inline int circle_half_width(int radius, int dyrow) {
    // The midpoint walk emits, for each step (dx, dy): rows +-dy get half-width dx, rows +-dx get half-width dy.
    // A row |r| is reached as a "dy row" while dx >= dy, and as a "dx row" each time dx takes the value |r|
    // (then with the LAST dy written before dx decrements being the widest).  Re-walk it: the circle is small.
    const int ar = dyrow < 0 ? -dyrow : dyrow;
    int best = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        if (dy == ar) best = best > dx ? best : dx;
        if (dx == ar) best = best > dy ? best : dy;
        dy++;
        err += plus;
        plus += 2;
        const int m = (err <= 0) - 1;
        err -= minus & m;
        dx += m;
        minus -= m & 2;
    }
    return best;
}

// Frame::isPixelInBox: the kill-box test of a keypoint at (x, y) of a w x h level 0
__host__ __device__ inline bool select_in_box(int x, int y, int w, int h, int kill_pad) {
    return !(x < kill_pad || y < kill_pad || w - x < kill_pad || h - y < kill_pad);
}

// the grid: cw = ceil(W / cells_x), ch = ceil(H / cells_y); cell(x, y) = (y / ch) * cells_x + x / cw
__host__ __device__ inline int select_cell_size(int extent, int cells) { return (extent + cells - 1) / cells; }
__host__ __device__ inline int select_cell(int x, int y, int cw, int ch, int cells_x) { return (y / ch) * cells_x + x / cw; }

// what a cell keeps of its candidates: the largest score s, ties to the smallest keypoint index k, as the maximum of one 64-bit key
// (s >= 0 and k < 2^32 - 1: no key is 0, which stands for "no candidate")
__host__ __device__ inline unsigned long long select_key(int s, int k) {
    return ((unsigned long long)(unsigned)s << 32) | (unsigned long long)(0xffffffffu - (unsigned)k);
}
__host__ __device__ inline int select_key_index(unsigned long long key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }

// the order of the cells' winners: cnt ascending, then s descending, then k ascending -- the last two are the key, descending.  No two
// winners compare equal (their k differ).
__host__ __device__ inline bool select_before(int cnt_a, unsigned long long key_a, int cnt_b, unsigned long long key_b) {
    return cnt_a < cnt_b || (cnt_a == cnt_b && key_a > key_b);
}

// what ekfvio_set_replenish_grid accepts: (0, 0) = off, else both >= 1 and at most SELECT_MAX_CELLS cells
inline bool select_grid_off(int cells_x, int cells_y) { return cells_x == 0 && cells_y == 0; }
inline bool select_grid_valid(int cells_x, int cells_y) {
    return select_grid_off(cells_x, cells_y) || (cells_x >= 1 && cells_y >= 1 && (long long)cells_x * cells_y <= SELECT_MAX_CELLS);
}

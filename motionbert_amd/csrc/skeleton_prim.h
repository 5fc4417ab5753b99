// The primitive of the two skeleton rasterisers (skeleton.hip: one skeleton per frame; scene.hip: any number of people per frame): the capsule
// dist(s, [a, a + d]) <= r in 1/RD_SUB samples, its set-up from two projected joints and its exact coverage test.  include/mbx.h has the
// definition and the no-wrap argument; both kernels take every comparison from here, so a sample is covered in one exactly when it is in the other.
#pragma once
#include "render_tile.h"

#define SK_GUARD (1 << 18)
#define SK_OUTSIDE (1 << 30)          // a joint that is not drawn: both components
#define SK_WHITE 0x00ffffffu

struct SkPrim {                       // the capsule dist(s, [a, a + d]) <= r; a marker is the capsule with d = 0
    int ax, ay, dx, dy;
    long long dd, r2, r2dd;
    int rin2;                         // a marker is white where |s - a|^2 <= rin2; -1: a capsule
    unsigned col;
    int hit;                          // the primitive is drawn and its box meets this tile
    int id;                           // scene.hip: rank 3 Nb + primitive index
};

// both ends inside the guard (the sentinel is outside)
__device__ __forceinline__ bool sk_drawn(int ax, int ay, int bx, int by) {
    return min(min(ax, ay), min(bx, by)) >= -SK_GUARD && max(max(ax, ay), max(bx, by)) <= SK_GUARD;
}

// part 0: the capsule a -> b of radius r_line; 1 / 2: the marker at a / b.  (cx0, cy0): the centre of the tile's first sample; `hit` is
// whether the primitive's box meets the sample centres [c0, c0 + RD_SUB (RD_TILE - 1)] of the tile on both axes.
__device__ __forceinline__ void sk_setup(SkPrim& r, int part, int ax, int ay, int bx, int by, int r_line, int r_out, int r_in, unsigned col, int cx0,
                                         int cy0) {
    const int rad = part == 0 ? r_line : r_out;
    r.ax = part == 2 ? bx : ax; r.ay = part == 2 ? by : ay;
    r.dx = part == 0 ? bx - ax : 0; r.dy = part == 0 ? by - ay : 0;
    r.dd = (long long)r.dx * r.dx + (long long)r.dy * r.dy;
    r.r2 = (long long)rad * rad;
    r.r2dd = r.r2 * r.dd;
    r.rin2 = part == 0 ? -1 : r_in * r_in;
    r.col = col;
    const int span = RD_SUB * (RD_TILE - 1);
    r.hit = min(r.ax, r.ax + r.dx) - rad <= cx0 + span && max(r.ax, r.ax + r.dx) + rad >= cx0 &&
            min(r.ay, r.ay + r.dy) - rad <= cy0 + span && max(r.ay, r.ay + r.dy) + rad >= cy0;
}

// (px, py) = s - a.  Returns whether the sample is covered; pp = |s - a|^2 (against rin2: the marker's white centre).
__device__ __forceinline__ bool sk_covers(const SkPrim& r, int px, int py, long long& pp) {
    pp = (long long)px * px + (long long)py * py;
    const long long td = (long long)px * r.dx + (long long)py * r.dy;
    if (td <= 0) return pp <= r.r2;
    if (td >= r.dd) {
        const int ex = px - r.dx, ey = py - r.dy;
        return (long long)ex * ex + (long long)ey * ey <= r.r2;
    }
    const long long c = (long long)px * r.dy - (long long)py * r.dx;
    return c > -(1ll << 31) && c < (1ll << 31) && c * c <= r.r2dd;
}

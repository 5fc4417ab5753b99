// Skeleton video frames as compute (the view of lib/utils/vismo.py:246-285, motion2video_3d): the 3D-skeleton branch of render_and_save, an
// exact fixed-point tile rasteriser of capsules and ringed discs.  include/mbx.h has the definition.
//   mbx_skeleton_project : x [F,J,3] f32 -> jq [F,J,2] i32 in 1/RD_SUB samples through the constant 4 x 4 matrix of the reference's 3D axes.
//                          x + 1 in fp32 as numpy takes it, everything after that in float64 with every operation rounded on its own
//                          (contraction is off for the whole file), so numpy float64 in the same order gives the same integers.
//   mbx_skeleton_raster  : one launch, no atomics: one workgroup per tile of RD_TILE x RD_TILE samples of one frame.  The first 3 Nb lanes set
//                          up the frame's primitives (per bone: the capsule and the two markers) in LDS, each with the answer whether its box
//                          meets the tile; a tile that none meets writes background and leaves.  Every lane owns a 2 x 2 quad of samples and
//                          reads the records as broadcasts; the winner of a sample is the covering primitive of highest priority, a maximum
//                          over a set.  The tile leaves through render_tile.h, as the mesh rasteriser's tiles do.  The primitive, its set-up
//                          and its coverage test are in skeleton_prim.h, which scene.hip (any number of people per frame) shares.
// Exactness.  Ends inside the guard |q| <= SK_GUARD = 2^18 and sample centres in [8, 16 (4096 + 31) + 8] give |s - a|, |b - a| < 2^19 + 2^10 per
// component, so |p|^2, t, dd < 2^40 and the cross product is below 2^40 in magnitude: all int64.  r <= 2^11: r^2 dd < 2^62.  A cross product
// of magnitude >= 2^31 has a square >= 2^62 > r^2 dd and is rejected before squaring; below that the square is < 2^62.  No product overflows.
#include "skeleton_prim.h"
#include <math.h>

#pragma clang fp contract(off)

#define SK_MAX_PRIMS (3 * MBX_SKELETON_MAX_BONES)

struct SkView {
    double m[12];                     // rows 0, 1 and 3 of the projection matrix
    double u_lo, v_hi, inv_w;
};

// ---------------------------------------------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_THREADS) void skeleton_project_kernel(const float* __restrict__ x, SkView vw, int n, double scale,
                                                                       int* __restrict__ jq) {
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= n) return;
    const float fx = x[(size_t)3 * i], fy = x[(size_t)3 * i + 1], fz = x[(size_t)3 * i + 2];
    const float ax = fx + 1.0f, ay = fy + 1.0f;                                          // pixel2world_vis_motion on the float32 motion
    const double px = -256.0 * (double)ax, py = -256.0 * (double)fz, pz = -256.0 * (double)ay;      // exact: the plotted (-X, -Z, -Y)
    const double U = ((vw.m[0] * px + vw.m[1] * py) + vw.m[2] * pz) + vw.m[3];          // plain operators under contract(off)
    const double V = ((vw.m[4] * px + vw.m[5] * py) + vw.m[6] * pz) + vw.m[7];
    const double W = ((vw.m[8] * px + vw.m[9] * py) + vw.m[10] * pz) + vw.m[11];
    const double u = U / W, v = V / W;
    const double qx = floor(((u - vw.u_lo) * vw.inv_w) * scale), qy = floor(((vw.v_hi - v) * vw.inv_w) * scale);
    const bool ok = isfinite(fx) && isfinite(fy) && isfinite(fz) && W > 0.0 && fabs(qx) <= (double)SK_GUARD && fabs(qy) <= (double)SK_GUARD;      // NaN compares false
    jq[(size_t)2 * i] = ok ? (int)qx : SK_OUTSIDE;
    jq[(size_t)2 * i + 1] = ok ? (int)qy : SK_OUTSIDE;
}

extern "C" int mbx_skeleton_project(const float* x, const double* view15, int F, int J, int size, int ss, int* jq, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 24) && J >= 1 && J <= MBX_SKELETON_MAX_JOINTS, "skeleton_project: bad sizes F=%d J=%d (F <= 2^24, 1 <= J <= %d)",
                  F, J, MBX_SKELETON_MAX_JOINTS);
    MBX_CHECK_ARG(size >= 1 && size <= MBX_RENDER_MAX_SIZE && (ss == 1 || ss == 2), "skeleton_project: size %d / ss %d (1 <= size <= %d, ss 1 or 2)",
                  size, ss, MBX_RENDER_MAX_SIZE);
    if (F == 0) return 0;
    MBX_CHECK_ARG(x && view15 && jq, "skeleton_project: null pointer");
    MBX_CHECK_ARG((((uintptr_t)x | (uintptr_t)jq) & 3) == 0, "skeleton_project: pointers must be 4-byte aligned");
    SkView vw;
    for (int k = 0; k < 12; ++k) vw.m[k] = view15[k];
    vw.u_lo = view15[12]; vw.v_hi = view15[13]; vw.inv_w = view15[14];
    for (int k = 0; k < 15; ++k) MBX_CHECK_ARG(isfinite(view15[k]), "skeleton_project: view[%d] is not finite", k);
    const int n = F * J;
    hipLaunchKernelGGL(skeleton_project_kernel, dim3((n + RD_THREADS - 1) / RD_THREADS), dim3(RD_THREADS), 0, (hipStream_t)stream, x, vw, n,
                       (double)(size * ss * RD_SUB), jq);
    MBX_LAUNCH_CHECK("skeleton_project");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_THREADS) void skeleton_tile_kernel(const int* __restrict__ jq, const int* __restrict__ bones,
                                                                    const unsigned char* __restrict__ colors, int J, int Nb, int r_line, int r_out,
                                                                    int r_in, int S, int size, int ss, int tiles, unsigned char* __restrict__ rgb,
                                                                    int* __restrict__ prim_id) {
    __shared__ SkPrim prims[SK_MAX_PRIMS];
    __shared__ unsigned stage[RD_STAGE_WORDS];
    __shared__ int any_hit;
    const int tid = threadIdx.x;
    const int per_frame = tiles * tiles;
    const int f = blockIdx.x / per_frame, t = blockIdx.x % per_frame, ty = t / tiles, tx = t % tiles;
    const int qx = tid & 15, qy = tid >> 4;
    const int sx = tx * RD_TILE + 2 * qx, sy = ty * RD_TILE + 2 * qy;                    // the quad's first sample
    const int np = 3 * Nb;
    int best[4] = {-1, -1, -1, -1};                                                      // 2 priority + (inside the marker's white centre)

    if (tid == 0) any_hit = 0;
    __syncthreads();
    if (tid < np) {
        const int k = tid / 3, part = tid - 3 * k;
        const int ia = bones[2 * k], ib = bones[2 * k + 1];
        SkPrim r = {};
        if ((unsigned)ia < (unsigned)J && (unsigned)ib < (unsigned)J) {
            const int* fj = jq + (size_t)f * 2 * J;
            const int ax = fj[2 * ia], ay = fj[2 * ia + 1], bx = fj[2 * ib], by = fj[2 * ib + 1];
            if (sk_drawn(ax, ay, bx, by))
                sk_setup(r, part, ax, ay, bx, by, r_line, r_out, r_in,
                         (unsigned)colors[3 * k] | (unsigned)colors[3 * k + 1] << 8 | (unsigned)colors[3 * k + 2] << 16, tx * RD_TILE * RD_SUB + RD_SUB / 2,
                         ty * RD_TILE * RD_SUB + RD_SUB / 2);
        }
        prims[tid] = r;
        if (r.hit) any_hit = 1;
    }
    __syncthreads();

    if (any_hit) {
        for (int k = 0; k < np; ++k) {
            const SkPrim& r = prims[k];                                                  // the same address on every lane: a broadcast
            if (!r.hit) continue;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int px = (sx + (s & 1)) * RD_SUB + RD_SUB / 2 - r.ax, py = (sy + (s >> 1)) * RD_SUB + RD_SUB / 2 - r.ay;
                long long pp;
                const bool cov = sk_covers(r, px, py, pp);
                const int key = 2 * k + (pp <= (long long)r.rin2 ? 1 : 0);
                best[s] = cov ? max(best[s], key) : best[s];
            }
        }
    }

    unsigned col[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int x = sx + (s & 1), y = sy + (s >> 1);
        col[s] = (best[s] < 0 || (best[s] & 1)) ? SK_WHITE : prims[max(best[s] >> 1, 0)].col;
        if (prim_id && x < S && y < S) prim_id[((size_t)f * S + y) * S + x] = best[s] >> 1;          // -1 where empty
    }
    rd_store_tile(col, stage, tid, qx, qy, tx, ty, f, size, ss, rgb);
}

extern "C" int mbx_skeleton_raster(const int* jq, const int* bones, const unsigned char* colors, int F, int J, int Nb, int r_line, int r_out,
                                   int r_in, int size, int ss, unsigned char* rgb, int* prim_id, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 24) && J >= 1 && J <= MBX_SKELETON_MAX_JOINTS && Nb >= 1 && Nb <= MBX_SKELETON_MAX_BONES,
                  "skeleton_raster: bad sizes F=%d J=%d Nb=%d (F <= 2^24, 1 <= J <= %d, 1 <= Nb <= %d)", F, J, Nb, MBX_SKELETON_MAX_JOINTS,
                  MBX_SKELETON_MAX_BONES);
    MBX_CHECK_ARG(size >= 1 && size <= MBX_RENDER_MAX_SIZE && (ss == 1 || ss == 2), "skeleton_raster: size %d / ss %d (1 <= size <= %d, ss 1 or 2)",
                  size, ss, MBX_RENDER_MAX_SIZE);
    MBX_CHECK_ARG(r_line >= 0 && r_line <= MBX_SKELETON_MAX_RADIUS && r_in >= 0 && r_in <= r_out && r_out <= MBX_SKELETON_MAX_RADIUS,
                  "skeleton_raster: radius r_line %d / r_out %d / r_in %d (0 <= r_line <= %d, 0 <= r_in <= r_out <= %d)", r_line, r_out, r_in,
                  MBX_SKELETON_MAX_RADIUS, MBX_SKELETON_MAX_RADIUS);
    if (F == 0) return 0;
    MBX_CHECK_ARG(jq && bones && colors && rgb, "skeleton_raster: null pointer");
    MBX_CHECK_ARG((((uintptr_t)jq | (uintptr_t)bones | (uintptr_t)prim_id) & 3) == 0, "skeleton_raster: jq, bones and prim_id must be 4-byte aligned");
    const int S = size * ss, tiles = (S + RD_TILE - 1) / RD_TILE;
    MBX_CHECK_ARG((long long)F * tiles * tiles <= 0x7fffffffll, "skeleton_raster: %d frames of %d x %d tiles are too many for one launch", F, tiles, tiles);
    hipLaunchKernelGGL(skeleton_tile_kernel, dim3(F * tiles * tiles), dim3(RD_THREADS), 0, (hipStream_t)stream, jq, bones, colors, J, Nb, r_line,
                       r_out, r_in, S, size, ss, tiles, rgb, prim_id);
    MBX_LAUNCH_CHECK("skeleton_raster");
    return 0;
}

// Crowd video frames as compute: every tracked person of a video frame drawn into one W x H image, over a colour or over the video's own
// frames.  The primitives, their coverage test and the winner rule inside one skeleton are those of skeleton.hip (skeleton_prim.h); a person
// later in the frame's list covers an earlier one.  include/mbx.h has the definition.
//   mbx_scene_project : x [R,J,C] f32 in video pixels -> jq [R,J,2] i32 in 1/RD_SUB samples, float64: floor(double(x) (16 ss) + 0.5).
//   mbx_scene_raster  : one launch, no atomics, no workspace: one workgroup per tile of RD_TILE x RD_TILE samples of one video frame.  A frame
//                       whose list is empty writes background and leaves.  Otherwise the list is walked SC_CHUNK persons at a time:
//                         1. the first SC_CHUNK lanes take one person each and test the box of its joints, grown by the largest radius,
//                            against the tile; the survivors are compacted in list order with a ballot (no LDS crossbar);
//                         2. the survivors' primitives are set up in LDS, RD_THREADS records at a time (one per lane), and every lane tests
//                            its 2 x 2 quad of samples against the records that meet the tile, read as broadcasts.
//                       A sample keeps the largest id = rank 3 Nb + primitive among the covering primitives and that primitive's colour: a
//                       maximum over a set, so neither the chunking nor the batching shows.  Nothing caps the list.
// Exactness: the bound of skeleton.hip holds as it stands: W, H <= 2048 and ss <= 2 keep sample centres in [8, 16 (4096 + 31) + 8].
#include "skeleton_prim.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

#define SC_CHUNK MBX_SCENE_CHUNK
#define SC_MAX_RANK (1 << 23)         // rank 3 Nb + primitive stays below 2^31 for Nb <= 64

static_assert(SC_CHUNK == 64, "the cull compacts with one wave's ballot");
static_assert(3 * MBX_SKELETON_MAX_BONES <= RD_THREADS, "one person's primitives fit one batch of records");

// ---------------------------------------------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_THREADS) void scene_project_kernel(const float* __restrict__ x, int n, int C, double scale, int* __restrict__ jq) {
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= n) return;
    const float fx = x[(size_t)C * i], fy = x[(size_t)C * i + 1];
    const double qx = floor((double)fx * scale + 0.5), qy = floor((double)fy * scale + 0.5);      // the product is exact; one rounding in the sum
    const bool ok = isfinite(fx) && isfinite(fy) && fabs(qx) <= (double)SK_GUARD && fabs(qy) <= (double)SK_GUARD;
    jq[(size_t)2 * i] = ok ? (int)qx : SK_OUTSIDE;
    jq[(size_t)2 * i + 1] = ok ? (int)qy : SK_OUTSIDE;
}

extern "C" int mbx_scene_project(const float* x, int R, int J, int C, int ss, int* jq, void* stream) {
    MBX_CHECK_ARG(R >= 0 && R <= (1 << 24) && J >= 1 && J <= MBX_SKELETON_MAX_JOINTS && (C == 2 || C == 3),
                  "scene_project: bad sizes R=%d J=%d C=%d (R <= 2^24, 1 <= J <= %d, C 2 or 3)", R, J, C, MBX_SKELETON_MAX_JOINTS);
    MBX_CHECK_ARG(ss == 1 || ss == 2, "scene_project: ss %d (1 or 2)", ss);
    if (R == 0) return 0;
    MBX_CHECK_ARG(x && jq, "scene_project: null pointer");
    MBX_CHECK_ARG((((uintptr_t)x | (uintptr_t)jq) & 3) == 0, "scene_project: pointers must be 4-byte aligned");
    const int n = R * J;
    hipLaunchKernelGGL(scene_project_kernel, dim3((n + RD_THREADS - 1) / RD_THREADS), dim3(RD_THREADS), 0, (hipStream_t)stream, x, n, C,
                       (double)(ss * RD_SUB), jq);
    MBX_LAUNCH_CHECK("scene_project");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------------------------------------------
struct ScArgs {
    const int *jq, *frame_ptr, *rows, *person, *bones;
    const unsigned char *palette, *bg_frames;
    unsigned char* rgb;
    int* prim_id;
    int n_entries, R, J, Nb, P, r_line, r_out, r_in, W, H, ss, tiles_x, tiles_y, bg_n;
    unsigned bg_rgb;
};

__global__ __launch_bounds__(RD_THREADS) void scene_tile_kernel(ScArgs a) {
    __shared__ SkPrim prims[RD_THREADS];
    __shared__ unsigned stage[RD_STAGE_WORDS];
    __shared__ int surv[SC_CHUNK];                                                       // the chunk's survivors: their table entries, in list order
    __shared__ int n_surv;
    const int tid = threadIdx.x;
    const int per_frame = a.tiles_x * a.tiles_y;
    const int f = blockIdx.x / per_frame, t = blockIdx.x % per_frame, ty = t / a.tiles_x, tx = t % a.tiles_x;
    const int qx = tid & 15, qy = tid >> 4;
    const int sx = tx * RD_TILE + 2 * qx, sy = ty * RD_TILE + 2 * qy;                    // the quad's first sample
    const int SW = a.W * a.ss, SH = a.H * a.ss;
    const int np = 3 * a.Nb, per_batch = RD_THREADS / np;                                // persons per batch of records: >= 1
    const int cx0 = tx * RD_TILE * RD_SUB + RD_SUB / 2, cy0 = ty * RD_TILE * RD_SUB + RD_SUB / 2, span = RD_SUB * (RD_TILE - 1);
    const int rmax = max(a.r_line, a.r_out);
    // the frame's list; a table that does not describe [0, n_entries) is cut to it, and ranks end where the id would pass 2^31
    const int lo = min(max(a.frame_ptr[f], 0), a.n_entries);
    const int hi = min(min(max(a.frame_ptr[f + 1], lo), a.n_entries), lo + SC_MAX_RANK);
    int best[4] = {-1, -1, -1, -1};                                                      // the winner's id
    unsigned bcol[4] = {0u, 0u, 0u, 0u};                                                 // and its colour at the sample

    for (int c0 = lo; c0 < hi; c0 += SC_CHUNK) {                                         // the same trips on every lane
        __syncthreads();                                                                 // n_surv and surv of the chunk before have been read
        if (tid < SC_CHUNK) {                                                            // the first wave, whole
            const int k = c0 + tid;
            bool keep = false;
            if (k < hi) {
                const int row = a.rows[k], per = a.person[k];
                if ((unsigned)row < (unsigned)a.R && (a.P == 1 || (unsigned)per < (unsigned)a.P)) {
                    const int* fj = a.jq + (size_t)row * 2 * a.J;
                    int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
                    for (int j = 0; j < a.J; ++j) {
                        const int x = fj[2 * j], y = fj[2 * j + 1];
                        if (sk_drawn(x, y, x, y)) {
                            x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
                        }
                    }
                    keep = x0 <= x1 && x0 - rmax <= cx0 + span && x1 + rmax >= cx0 && y0 - rmax <= cy0 + span && y1 + rmax >= cy0;
                }
            }
            const unsigned long long m = __ballot(keep);
            if (keep) surv[__popcll(m & ((1ull << tid) - 1ull))] = k;
            if (tid == 0) n_surv = __popcll(m);
        }
        __syncthreads();
        const int ns = n_surv;
        for (int b0 = 0; b0 < ns; b0 += per_batch) {
            const int n_rec = min(per_batch, ns - b0) * np;
            if (tid < n_rec) {
                const int slot = tid / np, pr = tid - slot * np, kb = pr / 3, part = pr - 3 * kb;
                const int k = surv[b0 + slot];
                const int row = a.rows[k], per = a.P == 1 ? 0 : a.person[k];              // both checked by the cull
                const int ia = a.bones[2 * kb], ib = a.bones[2 * kb + 1];
                SkPrim r = {};
                if ((unsigned)ia < (unsigned)a.J && (unsigned)ib < (unsigned)a.J) {
                    const int* fj = a.jq + (size_t)row * 2 * a.J;
                    const int ax = fj[2 * ia], ay = fj[2 * ia + 1], bx = fj[2 * ib], by = fj[2 * ib + 1];
                    if (sk_drawn(ax, ay, bx, by)) {
                        const unsigned char* pc = a.palette + ((size_t)per * a.Nb + kb) * 3;
                        sk_setup(r, part, ax, ay, bx, by, a.r_line, a.r_out, a.r_in, (unsigned)pc[0] | (unsigned)pc[1] << 8 | (unsigned)pc[2] << 16, cx0,
                                 cy0);
                    }
                }
                r.id = (k - lo) * np + pr;
                prims[tid] = r;
            }
            __syncthreads();
            for (int k = 0; k < n_rec; ++k) {
                const SkPrim& r = prims[k];                                              // the same address on every lane: a broadcast
                if (!r.hit) continue;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int px = (sx + (s & 1)) * RD_SUB + RD_SUB / 2 - r.ax, py = (sy + (s >> 1)) * RD_SUB + RD_SUB / 2 - r.ay;
                    long long pp;
                    const bool win = sk_covers(r, px, py, pp) && r.id > best[s];
                    best[s] = win ? r.id : best[s];
                    bcol[s] = win ? (pp <= (long long)r.rin2 ? SK_WHITE : r.col) : bcol[s];
                }
            }
            __syncthreads();                                                             // the records have been read
        }
    }

    unsigned col[4];
    const int sh = a.ss - 1;                                                             // samples to pixels
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int x = sx + (s & 1), y = sy + (s >> 1);
        const bool inside = x < SW && y < SH;
        unsigned bg = a.bg_rgb;
        if (a.bg_frames && inside) {
            const unsigned char* p = a.bg_frames + (((size_t)(a.bg_n == 1 ? 0 : f) * a.H + (y >> sh)) * a.W + (x >> sh)) * 3;
            bg = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
        }
        col[s] = best[s] < 0 ? bg : bcol[s];
        if (a.prim_id && inside) a.prim_id[((size_t)f * SH + y) * SW + x] = best[s];     // -1 where empty
    }
    rd_store_tile_rect(col, stage, tid, qx, qy, tx, ty, f, a.W, a.H, a.ss, a.rgb);
}

extern "C" int mbx_scene_raster(const int* jq, const int* frame_ptr, const int* rows, const int* person, int n_entries, const int* bones,
                                const unsigned char* palette, int Fv, int R, int J, int Nb, int P, int r_line, int r_out, int r_in, int W, int H,
                                int ss, const unsigned char* bg_frames, int bg_n, int bg_rgb, unsigned char* rgb, int* prim_id, void* stream) {
    MBX_CHECK_ARG(Fv >= 0 && Fv <= (1 << 24) && R >= 0 && R <= (1 << 24) && n_entries >= 0 && n_entries <= (1 << 30) && J >= 1 && J <= MBX_SKELETON_MAX_JOINTS && Nb >= 1 &&
                  Nb <= MBX_SKELETON_MAX_BONES && P >= 1,
                  "scene_raster: bad sizes Fv=%d R=%d entries=%d J=%d Nb=%d P=%d (Fv, R <= 2^24, entries <= 2^30, 1 <= J <= %d, 1 <= Nb <= %d, P >= 1)", Fv, R, n_entries, J,
                  Nb, P, MBX_SKELETON_MAX_JOINTS, MBX_SKELETON_MAX_BONES);
    MBX_CHECK_ARG(W >= 1 && W <= MBX_RENDER_MAX_SIZE && H >= 1 && H <= MBX_RENDER_MAX_SIZE && (ss == 1 || ss == 2),
                  "scene_raster: frames of W=%d x H=%d / ss %d (1 <= W, H <= %d, ss 1 or 2)", W, H, ss, MBX_RENDER_MAX_SIZE);
    MBX_CHECK_ARG(r_line >= 0 && r_line <= MBX_SKELETON_MAX_RADIUS && r_in >= 0 && r_in <= r_out && r_out <= MBX_SKELETON_MAX_RADIUS,
                  "scene_raster: radius r_line %d / r_out %d / r_in %d (0 <= r_line <= %d, 0 <= r_in <= r_out <= %d)", r_line, r_out, r_in,
                  MBX_SKELETON_MAX_RADIUS, MBX_SKELETON_MAX_RADIUS);
    MBX_CHECK_ARG(bg_frames ? (bg_n == 1 || bg_n == Fv) : (bg_rgb >= 0 && bg_rgb <= 0xffffff),
                  "scene_raster: background: %d frames for %d video frames (1 or all), or a colour r | g << 8 | b << 16, got %#x", bg_n, Fv, bg_rgb);
    if (Fv == 0) return 0;
    MBX_CHECK_ARG(frame_ptr && bones && palette && rgb && (jq || R == 0) && ((rows && person) || n_entries == 0), "scene_raster: null pointer");
    MBX_CHECK_ARG((((uintptr_t)jq | (uintptr_t)frame_ptr | (uintptr_t)rows | (uintptr_t)person | (uintptr_t)bones | (uintptr_t)prim_id) & 3) == 0,
                  "scene_raster: jq, the table, bones and prim_id must be 4-byte aligned");
    ScArgs a;
    a.jq = jq; a.frame_ptr = frame_ptr; a.rows = rows; a.person = person; a.bones = bones; a.palette = palette; a.bg_frames = bg_frames;
    a.rgb = rgb; a.prim_id = prim_id; a.n_entries = n_entries; a.R = R; a.J = J; a.Nb = Nb; a.P = P; a.r_line = r_line; a.r_out = r_out;
    a.r_in = r_in; a.W = W; a.H = H; a.ss = ss; a.bg_n = bg_n; a.bg_rgb = bg_frames ? 0u : (unsigned)bg_rgb;
    a.tiles_x = (W * ss + RD_TILE - 1) / RD_TILE; a.tiles_y = (H * ss + RD_TILE - 1) / RD_TILE;
    MBX_CHECK_ARG((long long)Fv * a.tiles_x * a.tiles_y <= 0x7fffffffll, "scene_raster: %d frames of %d x %d tiles are too many for one launch", Fv,
                  a.tiles_x, a.tiles_y);
    hipLaunchKernelGGL(scene_tile_kernel, dim3(Fv * a.tiles_x * a.tiles_y), dim3(RD_THREADS), 0, (hipStream_t)stream, a);
    MBX_LAUNCH_CHECK("scene_raster");
    return 0;
}

// Mesh video frames as compute (the view of lib/utils/vismo.py:297-334, motion2video_mesh): an exact fixed-point tile rasteriser.
//   mbx_render_project : verts [F,V,3] f32 -> [F,V,3] i32 in the bounding cube of the frame's track: x, y in 1/RD_SUB samples, z in 1/2^20 of
//                        the cube.  Every fp32 operation is rounded on its own (contraction is off for the whole file), so numpy float32 in the
//                        same order gives the same integers.
//   mbx_render_raster  : three launches, no atomics on global memory:
//                          1. frame box   one workgroup per frame: the tile box of the frame's vertices inside the guard;
//                          2. face setup  one thread per (frame, face): the dropped-face rules, the face's tile box and its flat colour (from the
//                             fp32 vertices), 8 bytes per (frame, face) in the workspace;
//                          3. tiles       one workgroup per tile of RD_TILE x RD_TILE samples of one frame.  A tile outside the frame box writes
//                             background and leaves.  Otherwise the workgroup scans the frame's face boxes RD_THREADS at a time; a lane whose
//                             face meets the tile sets up its three edge functions at the tile's first sample and appends them to a list in
//                             LDS; whenever the list could not take another scan block it is consumed and emptied, so a tile met by any number
//                             of faces is complete.  Every lane owns a 2 x 2 quad of samples and keeps their four minimum keys
//                             (depth << 32 | face) in registers: the winner is a minimum over a set, independent of any order.  The 64-bit
//                             divide of the depth runs for covered samples only, as a reciprocal estimate with an exact integer correction.
//                             The tile's colours go through LDS and leave as whole dwords where the image rows allow it (render_tile.h).
#include "render_tile.h"
#include <math.h>

#pragma clang fp contract(off)

#define RD_ZQ MBX_RENDER_ZQ
#define RD_GUARD (1 << 17)
#define RD_OUTSIDE (1 << 30)          // what a non-finite or far-away coordinate projects to: outside the guard in x, y and z
#define RD_LIST 512                   // face records in LDS; consumed as soon as fewer than RD_THREADS slots are left
#define RD_EMPTY_BOX 0x000000ffu      // tx0 = 255 > tx1 = 0: meets no tile
#define RD_EMPTY_KEY 0x7fffffffffffffffull
#define RD_PROJ_CHUNK 1024

// ---------------------------------------------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rd_snap(float v, float c, float inv, float scale) {
    const float p = ((v - c) * inv + 0.5f) * scale;          // plain operators under contract(off): four instructions, four roundings
    return fabsf(p) < 1073741824.0f ? (int)floorf(p) : RD_OUTSIDE;          // NaN compares false
}

__global__ __launch_bounds__(RD_THREADS) void render_project_kernel(const float* __restrict__ verts, const float* __restrict__ cube,
                                                                     const int* __restrict__ seq_ptr, int n_tracks, int V, float xy_scale,
                                                                     int* __restrict__ out) {
    const int f = blockIdx.x;
    int lo = 0, hi = n_tracks;                                               // the last track with seq_ptr[s] <= f
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seq_ptr[mid] <= f) lo = mid; else hi = mid;
    }
    const bool in_track = seq_ptr[lo] <= f && f < seq_ptr[lo + 1];
    const float cx = cube[lo * 4], cy = cube[lo * 4 + 1], cz = cube[lo * 4 + 2], inv = cube[lo * 4 + 3];
    const float* src = verts + (size_t)f * 3 * V;
    int* dst = out + (size_t)f * 3 * V;
    const int v0 = blockIdx.y * RD_PROJ_CHUNK, v1 = min(v0 + RD_PROJ_CHUNK, V);
    for (int e = 3 * v0 + threadIdx.x; e < 3 * v1; e += RD_THREADS) {
        const int c = e % 3;
        dst[e] = !in_track ? RD_OUTSIDE : rd_snap(src[e], c == 0 ? cx : (c == 1 ? cy : cz), inv, c == 2 ? (float)RD_ZQ : xy_scale);
    }
}

extern "C" int mbx_render_project(const float* verts, const float* cube, const int* seq_ptr, int n_tracks, int F, int V, int size, int ss,
                                  int* out, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 24) && V >= 1 && V <= (1 << 24) && n_tracks >= 1 && n_tracks <= (1 << 20),
                  "render_project: bad sizes F=%d V=%d n_tracks=%d (F <= 2^24, 1 <= V <= 2^24, 1 <= n_tracks <= 2^20)", F, V, n_tracks);
    MBX_CHECK_ARG(size >= 1 && size <= MBX_RENDER_MAX_SIZE && (ss == 1 || ss == 2), "render_project: size %d / ss %d (1 <= size <= %d, ss 1 or 2)",
                  size, ss, MBX_RENDER_MAX_SIZE);
    if (F == 0) return 0;
    MBX_CHECK_ARG(verts && cube && seq_ptr && out, "render_project: null pointer");
    MBX_CHECK_ARG((((uintptr_t)verts | (uintptr_t)cube | (uintptr_t)seq_ptr | (uintptr_t)out) & 3) == 0, "render_project: pointers must be 4-byte aligned");
    const int chunks = (V + RD_PROJ_CHUNK - 1) / RD_PROJ_CHUNK;
    MBX_CHECK_ARG(chunks <= 65535, "render_project: V=%d needs more than 65535 vertex chunks", V);
    hipLaunchKernelGGL(render_project_kernel, dim3(F, chunks), dim3(RD_THREADS), 0, (hipStream_t)stream, verts, cube, seq_ptr, n_tracks, V,
                       (float)(size * ss * RD_SUB), out);
    MBX_LAUNCH_CHECK("render_project");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// boxes.  The sample j sits at RD_SUB j + RD_SUB / 2, so the samples inside [lo, hi] are ceil((lo - 8) / 16) .. floor((hi - 8) / 16); >> on a
// negative int is the floor.  A box is four tile indices in one word (at most 128 tiles per side), RD_EMPTY_BOX when it holds no sample.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned rd_pack_box(int xlo, int xhi, int ylo, int yhi, int S) {
    int j0 = (xlo + RD_SUB / 2 - 1) >> 4, j1 = (xhi - RD_SUB / 2) >> 4;
    int i0 = (ylo + RD_SUB / 2 - 1) >> 4, i1 = (yhi - RD_SUB / 2) >> 4;
    j0 = max(j0, 0); i0 = max(i0, 0); j1 = min(j1, S - 1); i1 = min(i1, S - 1);
    if (j0 > j1 || i0 > i1) return RD_EMPTY_BOX;
    return (unsigned)(j0 / RD_TILE) | (unsigned)(i0 / RD_TILE) << 8 | (unsigned)(j1 / RD_TILE) << 16 | (unsigned)(i1 / RD_TILE) << 24;
}
__device__ __forceinline__ bool rd_box_hits(unsigned box, int tx, int ty) {
    return (int)(box & 255u) <= tx && tx <= (int)(box >> 16 & 255u) && (int)(box >> 8 & 255u) <= ty && ty <= (int)(box >> 24);
}

__global__ __launch_bounds__(RD_THREADS) void render_frame_box_kernel(const int* __restrict__ vq, int V, int S, unsigned* __restrict__ frame_box) {
    __shared__ int red[4][RD_THREADS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int* p = vq + (size_t)f * 3 * V;
    int xlo = INT_MAX, xhi = INT_MIN, ylo = INT_MAX, yhi = INT_MIN;
    for (int v = tid; v < V; v += RD_THREADS) {
        const int x = p[3 * v], y = p[3 * v + 1];
        if (x >= -RD_GUARD && x <= RD_GUARD && y >= -RD_GUARD && y <= RD_GUARD) {          // a vertex outside the guard only has dropped faces
            xlo = min(xlo, x); xhi = max(xhi, x); ylo = min(ylo, y); yhi = max(yhi, y);
        }
    }
    red[0][tid] = xlo; red[1][tid] = xhi; red[2][tid] = ylo; red[3][tid] = yhi;
    __syncthreads();
    for (int s = RD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = min(red[0][tid], red[0][tid + s]);
            red[1][tid] = max(red[1][tid], red[1][tid + s]);
            red[2][tid] = min(red[2][tid], red[2][tid + s]);
            red[3][tid] = max(red[3][tid], red[3][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) frame_box[f] = red[0][0] > red[1][0] ? RD_EMPTY_BOX : rd_pack_box(red[0][0], red[1][0], red[2][0], red[3][0], S);
}

// the three snapped vertices of a face, oriented so that the doubled area is positive; false: the face is dropped
struct RdTri {
    int x0, y0, z0, x1, y1, z1, x2, y2, z2;
    long long a2;
};
__device__ __forceinline__ bool rd_load_tri(const int* __restrict__ vq, const int* __restrict__ face, int V, RdTri& t) {
    const int i0 = face[0], i1 = face[1], i2 = face[2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
    t.x0 = vq[3 * i0]; t.y0 = vq[3 * i0 + 1]; t.z0 = vq[3 * i0 + 2];
    t.x1 = vq[3 * i1]; t.y1 = vq[3 * i1 + 1]; t.z1 = vq[3 * i1 + 2];
    t.x2 = vq[3 * i2]; t.y2 = vq[3 * i2 + 1]; t.z2 = vq[3 * i2 + 2];
    const int xlo = min(t.x0, min(t.x1, t.x2)), xhi = max(t.x0, max(t.x1, t.x2));
    const int ylo = min(t.y0, min(t.y1, t.y2)), yhi = max(t.y0, max(t.y1, t.y2));
    const int zlo = min(t.z0, min(t.z1, t.z2)), zhi = max(t.z0, max(t.z1, t.z2));
    if (xlo < -RD_GUARD || xhi > RD_GUARD || ylo < -RD_GUARD || yhi > RD_GUARD || zlo < 0 || zhi > RD_ZQ) return false;
    t.a2 = (long long)(t.x1 - t.x0) * (t.y2 - t.y0) - (long long)(t.y1 - t.y0) * (t.x2 - t.x0);
    if (t.a2 == 0) return false;
    if (t.a2 < 0) {
        int s;
        s = t.x1; t.x1 = t.x2; t.x2 = s;
        s = t.y1; t.y1 = t.y2; t.y2 = s;
        s = t.z1; t.z1 = t.z2; t.z2 = s;
        t.a2 = -t.a2;
    }
    return true;
}

// flat colour of a face from the fp32 vertices, taken in ascending index order so that it does not depend on how the face lists them
__device__ __forceinline__ unsigned rd_face_colour(const float* __restrict__ v, const int* __restrict__ face, float kr, float kg, float kb,
                                                   float kw) {
    int a = face[0], b = face[1], c = face[2], s;
    if (a > b) { s = a; a = b; b = s; }
    if (b > c) { s = b; b = c; c = s; }
    if (a > b) { s = a; a = b; b = s; }
    const float ax = v[3 * b] - v[3 * a], ay = v[3 * b + 1] - v[3 * a + 1], az = v[3 * b + 2] - v[3 * a + 2];
    const float bx = v[3 * c] - v[3 * a], by = v[3 * c + 1] - v[3 * a + 1], bz = v[3 * c + 2] - v[3 * a + 2];
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float l2 = nx * nx + ny * ny + nz * nz;
    const float cosz = (l2 > 0.f && l2 < INFINITY) ? fabsf(nz) / sqrtf(l2) : 0.f;          // no usable normal: taken as edge-on
    const float I = 0.35f + 0.65f * cosz;
    const int r = min(255, max(0, (int)floorf(kr * I + kw + 0.5f)));
    const int g = min(255, max(0, (int)floorf(kg * I + kw + 0.5f)));
    const int bl = min(255, max(0, (int)floorf(kb * I + kw + 0.5f)));
    return (unsigned)r | (unsigned)g << 8 | (unsigned)bl << 16;
}

__global__ __launch_bounds__(RD_THREADS) void render_face_setup_kernel(const int* __restrict__ vq, const float* __restrict__ verts,
                                                                        const int* __restrict__ faces, int Nf, int V, int S, float kr, float kg,
                                                                        float kb, float kw, uint2* __restrict__ face_rec) {
    const int f = blockIdx.y, n = blockIdx.x * RD_THREADS + threadIdx.x;
    if (n >= Nf) return;
    RdTri t;
    uint2 rec = make_uint2(RD_EMPTY_BOX, 0u);
    if (rd_load_tri(vq + (size_t)f * 3 * V, faces + (size_t)3 * n, V, t)) {
        rec.x = rd_pack_box(min(t.x0, min(t.x1, t.x2)), max(t.x0, max(t.x1, t.x2)), min(t.y0, min(t.y1, t.y2)), max(t.y0, max(t.y1, t.y2)), S);
        if (rec.x != RD_EMPTY_BOX) rec.y = rd_face_colour(verts + (size_t)f * 3 * V, faces + (size_t)3 * n, kr, kg, kb, kw);
    }
    face_rec[(size_t)f * Nf + n] = rec;
}

// ---------------------------------------------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------------------------------------------
// edge function of a -> b at s, positive inside a face of positive doubled area
__device__ __forceinline__ long long rd_edge(int ax, int ay, int bx, int by, int sx, int sy) {
    return (long long)(bx - ax) * (sy - ay) - (long long)(by - ay) * (sx - ax);
}
// a sample exactly on the edge a -> b belongs to the face iff this holds; the reversed edge of the neighbour answers the opposite
__device__ __forceinline__ bool rd_owns_edge(int ax, int ay, int bx, int by) { return by - ay > 0 || (by == ay && bx - ax > 0); }

struct RdRec {              // the edge functions of one face at the tile's first sample: w_i(dx, dy) = w[i] + a[i] dx + b[i] dy per sample step
    long long w[3];
    int a[3], b[3], z[3];
    float rcp;              // 1 / doubled area, an estimate
    int id;                 // face | (bit 28 + i: edge i does not own its own line)
};

__global__ __launch_bounds__(RD_THREADS) void render_tile_kernel(const int* __restrict__ vq, const int* __restrict__ faces,
                                                                  const unsigned* __restrict__ frame_box, const uint2* __restrict__ face_rec,
                                                                  int Nf, int V, int S, int size, int ss, int tiles, unsigned char* __restrict__ rgb,
                                                                  int* __restrict__ face_id, int* __restrict__ depth) {
    __shared__ RdRec list[RD_LIST];
    __shared__ unsigned stage[RD_STAGE_WORDS];
    __shared__ int wave_count[RD_THREADS / MBX_WAVE];
    __shared__ int list_count;
    const int tid = threadIdx.x, lane = tid & (MBX_WAVE - 1), wave = tid / MBX_WAVE;
    const int per_frame = tiles * tiles;
    const int f = blockIdx.x / per_frame, t = blockIdx.x % per_frame, ty = t / tiles, tx = t % tiles;
    const int qx = tid & 15, qy = tid >> 4;
    const int sx = tx * RD_TILE + 2 * qx, sy = ty * RD_TILE + 2 * qy;                    // the quad's first sample
    unsigned long long best[4] = {RD_EMPTY_KEY, RD_EMPTY_KEY, RD_EMPTY_KEY, RD_EMPTY_KEY};

    if (rd_box_hits(frame_box[f], tx, ty)) {
        const int* fv = vq + (size_t)f * 3 * V;
        const uint2* frec = face_rec + (size_t)f * Nf;
        const int ox = tx * RD_TILE * RD_SUB + RD_SUB / 2, oy = ty * RD_TILE * RD_SUB + RD_SUB / 2;
        if (tid == 0) list_count = 0;
        __syncthreads();
        for (int base = 0; base < Nf; base += RD_THREADS) {
            const int n = base + tid;
            const bool hit = n < Nf && rd_box_hits(frec[n].x, tx, ty);
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wave_count[wave] = __popcll(m);
            __syncthreads();
            int slot = list_count + __popcll(m & ((1ull << lane) - 1));
            int total = 0;
#pragma unroll
            for (int w = 0; w < RD_THREADS / MBX_WAVE; ++w) {
                if (w < wave) slot += wave_count[w];
                total += wave_count[w];
            }
            RdTri tr;
            if (hit && !rd_load_tri(fv, faces + (size_t)3 * n, V, tr)) {     // a face with a box passed the same rules in the setup; if it ever
                RdRec r = {};                                                // did not, its slot holds a face that covers nothing
                r.w[0] = r.w[1] = r.w[2] = -1;
                list[slot] = r;
            } else if (hit) {
                RdRec r;
                r.w[0] = rd_edge(tr.x1, tr.y1, tr.x2, tr.y2, ox, oy);
                r.w[1] = rd_edge(tr.x2, tr.y2, tr.x0, tr.y0, ox, oy);
                r.w[2] = rd_edge(tr.x0, tr.y0, tr.x1, tr.y1, ox, oy);
                r.a[0] = -(tr.y2 - tr.y1) * RD_SUB; r.b[0] = (tr.x2 - tr.x1) * RD_SUB;
                r.a[1] = -(tr.y0 - tr.y2) * RD_SUB; r.b[1] = (tr.x0 - tr.x2) * RD_SUB;
                r.a[2] = -(tr.y1 - tr.y0) * RD_SUB; r.b[2] = (tr.x1 - tr.x0) * RD_SUB;
                r.z[0] = tr.z0; r.z[1] = tr.z1; r.z[2] = tr.z2;
                r.rcp = 1.0f / (float)tr.a2;
                r.id = n | (rd_owns_edge(tr.x1, tr.y1, tr.x2, tr.y2) ? 0 : 1 << 28) | (rd_owns_edge(tr.x2, tr.y2, tr.x0, tr.y0) ? 0 : 1 << 29) |
                       (rd_owns_edge(tr.x0, tr.y0, tr.x1, tr.y1) ? 0 : 1 << 30);
                list[slot] = r;
            }
            __syncthreads();                                                 // the records are written, wave_count has been read
            const int count = list_count + total;
            const bool consume = count > RD_LIST - RD_THREADS || base + RD_THREADS >= Nf;
            if (consume) {
                for (int k = 0; k < count; ++k) {
                    const RdRec& r = list[k];                                // the same address on every lane: a broadcast
                    const int id = r.id;
                    const long long a2 = r.w[0] + r.w[1] + r.w[2];
                    long long e[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) e[i] = r.w[i] + (long long)r.a[i] * (2 * qx) + (long long)r.b[i] * (2 * qy);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const long long w0 = e[0] + ((s & 1) ? r.a[0] : 0) + ((s & 2) ? r.b[0] : 0);
                        const long long w1 = e[1] + ((s & 1) ? r.a[1] : 0) + ((s & 2) ? r.b[1] : 0);
                        const long long w2 = e[2] + ((s & 1) ? r.a[2] : 0) + ((s & 2) ? r.b[2] : 0);
                        // w_i >= 0 on an owned edge, w_i > 0 otherwise: the sign of w_i - (0 or 1)
                        if (((w0 - (id >> 28 & 1)) | (w1 - (id >> 29 & 1)) | (w2 - (id >> 30 & 1))) >= 0) {
                            const long long num = w0 * r.z[0] + w1 * r.z[1] + w2 * r.z[2];      // 0 <= num <= a2 2^20 < 2^58
                            long long q = (long long)((float)num * r.rcp);                      // within 1 of the quotient
                            long long rem = num - q * a2;
                            if (rem < 0) { q -= 1; rem += a2; }
                            if (rem < 0) { q -= 1; rem += a2; }
                            if (rem >= a2) { q += 1; rem -= a2; }
                            if (rem >= a2) q += 1;
                            const unsigned long long key = (unsigned long long)q << 32 | (unsigned)(id & 0x0fffffff);
                            best[s] = key < best[s] ? key : best[s];
                        }
                    }
                }
            }
            __syncthreads();                                                 // the list has been read
            if (tid == 0) list_count = consume ? 0 : count;
            // the next round's first barrier orders this store before the reads of list_count
        }
    }

    // resolve: colours into the staging tile, the optional sample buffers straight out
    unsigned col[4];
    const uint2* frec = face_rec + (size_t)f * Nf;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int x = sx + (s & 1), y = sy + (s >> 1);
        const int id = (int)(unsigned)best[s];                               // -1 where empty
        col[s] = best[s] == RD_EMPTY_KEY ? 0x00ffffffu : frec[id].y;
        if (x < S && y < S) {
            const size_t o = ((size_t)f * S + y) * S + x;
            if (face_id) face_id[o] = id;
            if (depth) depth[o] = (int)(best[s] >> 32);
        }
    }
    rd_store_tile(col, stage, tid, qx, qy, tx, ty, f, size, ss, rgb);
}

extern "C" size_t mbx_render_raster_ws(int F, int Nf) {
    if (F < 0 || Nf < 0) return 0;
    return (((size_t)F * 4 + 15) & ~(size_t)15) + (size_t)F * Nf * 8 + 16;
}

extern "C" int mbx_render_raster(const int* vq, const float* verts, const int* faces, int F, int V, int Nf, int size, int ss, float red,
                                 float green, float blue, float alpha, unsigned char* rgb, int* face_id, int* depth, void* ws, size_t ws_bytes,
                                 void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 24) && V >= 1 && V <= (1 << 24) && Nf >= 1 && Nf < (1 << 28),
                  "render_raster: bad sizes F=%d V=%d Nf=%d (F <= 2^24, 1 <= V <= 2^24, 1 <= Nf < 2^28)", F, V, Nf);
    MBX_CHECK_ARG(size >= 1 && size <= MBX_RENDER_MAX_SIZE && (ss == 1 || ss == 2), "render_raster: size %d / ss %d (1 <= size <= %d, ss 1 or 2)",
                  size, ss, MBX_RENDER_MAX_SIZE);
    MBX_CHECK_ARG(red >= 0.f && red <= 255.f && green >= 0.f && green <= 255.f && blue >= 0.f && blue <= 255.f && alpha >= 0.f && alpha <= 1.f,
                  "render_raster: colour (%g, %g, %g) outside [0, 255] or alpha %g outside [0, 1]", red, green, blue, alpha);
    if (F == 0) return 0;
    MBX_CHECK_ARG(vq && verts && faces && rgb && ws, "render_raster: null pointer");
    MBX_CHECK_ARG((((uintptr_t)vq | (uintptr_t)verts | (uintptr_t)faces | (uintptr_t)face_id | (uintptr_t)depth) & 3) == 0 && ((uintptr_t)ws & 7) == 0,
                  "render_raster: vq, verts, faces, face_id and depth must be 4-byte aligned, ws 8-byte aligned");
    MBX_CHECK_ARG(ws_bytes >= mbx_render_raster_ws(F, Nf), "render_raster: workspace of %zu bytes, %zu needed", ws_bytes, mbx_render_raster_ws(F, Nf));
    const int S = size * ss, tiles = (S + RD_TILE - 1) / RD_TILE;
    MBX_CHECK_ARG((long long)F * tiles * tiles <= 0x7fffffffll, "render_raster: %d frames of %d x %d tiles are too many for one launch", F, tiles, tiles);
    const int face_blocks = (Nf + RD_THREADS - 1) / RD_THREADS;
    MBX_CHECK_ARG(F <= 65535, "render_raster: at most 65535 frames per call, got %d", F);
    unsigned* frame_box = (unsigned*)ws;
    uint2* face_rec = (uint2*)((char*)ws + (((size_t)F * 4 + 15) & ~(size_t)15));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(render_frame_box_kernel, dim3(F), dim3(RD_THREADS), 0, s, vq, V, S, frame_box);
    MBX_LAUNCH_CHECK("render_raster (frame box)");
    hipLaunchKernelGGL(render_face_setup_kernel, dim3(face_blocks, F), dim3(RD_THREADS), 0, s, vq, verts, faces, Nf, V, S, alpha * red,
                       alpha * green, alpha * blue, 255.f * (1.f - alpha), face_rec);
    MBX_LAUNCH_CHECK("render_raster (face setup)");
    hipLaunchKernelGGL(render_tile_kernel, dim3(F * tiles * tiles), dim3(RD_THREADS), 0, s, vq, faces, frame_box, face_rec, Nf, V, S, size, ss, tiles,
                       rgb, face_id, depth);
    MBX_LAUNCH_CHECK("render_raster (tiles)");
    return 0;
}

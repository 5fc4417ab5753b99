// In-the-wild inference around the backbone (infer_wild.py:56-97; lib/data/dataset_wild.py:15-86; lib/utils/utils_data.py:7-29).
//   mbx_wild_input  : halpe2h36m + the normalisation of read_input for F frames of S tracks (Halpe-26 detections, float64 as json.load and
//                     np.array leave them) -> [F,17,channels] float32.  ALL arithmetic is float64 in the reference's operation order with
//                     floating-point contraction off for the whole file; the one rounding to float32 is the store (`.astype(np.float32)`).
//                     IEEE float64 +, -, *, / are correctly rounded on both sides, so the result is the reference's BIT FOR BIT.
//                     Three launches, no atomics:
//                       1. one workgroup per chunk of at most MBX_WILD_CHUNK frames of one track: box (min / max of x and y) and count of
//                          the joints whose mapped confidence is != 0, DPP reductions inside a wave, LDS across the four waves;
//                       2. one wave per track: lanes 0..4 each fold one of the five quantities over the track's chunks in index order;
//                       3. the transform, one workgroup per chunk again.
//                     The mapped and pixel-normalised coordinates are never stored: launch 3 recomputes them with the same operations
//                     (hence the same bits) that launch 1 took the box of.
//   mbx_wild_output : infer_wild.py:81-96 for a batch of clips, written straight to each clip's rows of the stitched [F,17,3] result.
//   mbx_wild_output_ragged : the same for one packed batch of clips of different lengths (rows dst0 .. dst0 + Fb - 1).
//   mbx_scale_fit   : solve_scale of infer_wild_mesh.py:42-56 for S tracks, one workgroup per track, the whole IRLS solve in the kernel.
//   mbx_wild_mesh_place : infer_wild_mesh.py:153-154 in place, in numpy 2's arithmetic.
#include "mbx_common.h"
#include <math.h>

#pragma clang fp contract(off)

#define WI_THREADS 256
#define WI_WAVES (WI_THREADS / MBX_WAVE)
#define WI_J 17
#define WI_V 26
#define WI_GRID_CAP (256 * 16)

static inline int wi_clamp_grid(size_t want, int cap) { return (int)(want < (size_t)cap ? (want ? want : 1) : (size_t)cap); }

// lib/data/dataset_wild.py:48-64: H36M joint j takes Halpe joint WI_MAP[j]; joint 7 is the mean of Halpe 18 and 19 (all three channels)
__constant__ int WI_MAP[WI_J] = {19, 12, 14, 16, 11, 13, 15, -1, 18, 0, 17, 5, 7, 9, 6, 8, 10};

__device__ __forceinline__ void wi_joint(const double* __restrict__ frame, int j, double& x, double& y, double& c) {
    if (j == 7) {
        const double* a = frame + 18 * 3;
        const double* b = frame + 19 * 3;
        x = (a[0] + b[0]) * 0.5;
        y = (a[1] + b[1]) * 0.5;
        c = (a[2] + b[2]) * 0.5;
    } else {
        const double* a = frame + WI_MAP[j] * 3;
        x = a[0]; y = a[1]; c = a[2];
    }
}
// dataset_wild.py:81-82: (xy - (w, h) / 2) / (min(w, h) / 2): a subtraction and a DIVISION
__device__ __forceinline__ void wi_pixel(double& x, double& y, double half_w, double half_h, double pix_scale) {
    x = (x - half_w) / pix_scale;
    y = (y - half_h) / pix_scale;
}

// wave_reduce of mbx_common.h for float64: the two halves of the value travel through the same DPP controls
template <int CTRL, int ROW_MASK = 0xf> __device__ __forceinline__ double dpp_mov_d(double old, double v) {
    const uint64_t ob = __builtin_bit_cast(uint64_t, old), vb = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)ob, (int)(uint32_t)vb, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(ob >> 32), (int)(uint32_t)(vb >> 32), CTRL, ROW_MASK, 0xf, false);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
struct WaveMinD { static __device__ __forceinline__ double op(double a, double b) { return fmin(a, b); } };
struct WaveMaxD { static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); } };
// min and max only (the identity of the masked steps is the lane's own value).  Every lane of the wave must be active.
template <typename Op> __device__ __forceinline__ double wave_reduce_d(double v) {
    v = Op::op(v, dpp_mov_d<0xB1>(v, v));
    v = Op::op(v, dpp_mov_d<0x4E>(v, v));
    v = Op::op(v, dpp_mov_d<0x141>(v, v));
    v = Op::op(v, dpp_mov_d<0x140>(v, v));
    v = Op::op(v, dpp_mov_d<0x142, 0xa>(v, v));
    v = Op::op(v, dpp_mov_d<0x143, 0xc>(v, v));
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), 63);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// a chunk-table row that cannot be trusted is skipped by all three launches (the table is device memory: the host cannot check it here)
__device__ __forceinline__ bool wi_chunk(const int* __restrict__ chunk_tab, int ch, int S, int F, int& trk, int& f0, int& nf) {
    trk = chunk_tab[ch * 3]; f0 = chunk_tab[ch * 3 + 1]; nf = chunk_tab[ch * 3 + 2];
    return trk >= 0 && trk < S && f0 >= 0 && nf >= 1 && nf <= MBX_WILD_CHUNK && f0 <= F - nf;
}

// launch 1: part[ch] = {xmin, xmax, ymin, ymax, count} of chunk ch
__global__ __launch_bounds__(WI_THREADS) void wild_box_partial_kernel(const double* __restrict__ kp, const int* __restrict__ chunk_tab, int n_chunks,
                                                                       int S, int F, double half_w, double half_h, double pix_scale, int pixel,
                                                                       double* __restrict__ part) {
    __shared__ double red[WI_WAVES][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        int trk, f0, nf;
        const bool ok = wi_chunk(chunk_tab, ch, S, F, trk, f0, nf);          // uniform over the workgroup
        double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        float cnt = 0.f;                                                      // at most 64 * 17 per chunk: exact
        if (ok)
            for (int r = tid; r < nf * WI_J; r += WI_THREADS) {
                double x, y, c;
                wi_joint(kp + (size_t)(f0 + r / WI_J) * (WI_V * 3), r % WI_J, x, y, c);
                if (c != 0.0) {
                    if (pixel) wi_pixel(x, y, half_w, half_h, pix_scale);
                    xmin = fmin(xmin, x); xmax = fmax(xmax, x);
                    ymin = fmin(ymin, y); ymax = fmax(ymax, y);
                    cnt += 1.f;
                }
            }
        xmin = wave_reduce_d<WaveMinD>(xmin); xmax = wave_reduce_d<WaveMaxD>(xmax);
        ymin = wave_reduce_d<WaveMinD>(ymin); ymax = wave_reduce_d<WaveMaxD>(ymax);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            double* r = red[wave];
            r[0] = xmin; r[1] = xmax; r[2] = ymin; r[3] = ymax; r[4] = (double)cnt;
        }
        __syncthreads();
        if (tid == 0) {
            double q[5] = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4]};
#pragma unroll
            for (int w = 1; w < WI_WAVES; ++w) {
                q[0] = fmin(q[0], red[w][0]); q[1] = fmax(q[1], red[w][1]);
                q[2] = fmin(q[2], red[w][2]); q[3] = fmax(q[3], red[w][3]);
                q[4] += red[w][4];
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) part[(size_t)ch * 5 + k] = q[k];
        }
        __syncthreads();                                                      // red is written again in the next trip
    }
}

// launch 2: box[s] = {xs, ys, scale, n_valid} (utils_data.py:14-25); a track that crop_scale answers with zeros has scale = xs = ys = 0
__global__ __launch_bounds__(MBX_WAVE) void wild_box_fold_kernel(const double* __restrict__ part, const int* __restrict__ seq_chunk_ptr, int S,
                                                                  int n_chunks, double ratio, double* __restrict__ box) {
    __shared__ double q[5];
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        int c0 = seq_chunk_ptr[s], c1 = seq_chunk_ptr[s + 1];
        if (c0 < 0 || c1 > n_chunks || c0 > c1) c0 = c1 = 0;
        if (lane < 5) {
            double v = lane == 4 ? 0.0 : (lane & 1) ? -INFINITY : INFINITY;
            for (int ch = c0; ch < c1; ++ch) {                                 // index order
                const double p = part[(size_t)ch * 5 + lane];
                v = lane == 4 ? v + p : (lane & 1) ? fmax(v, p) : fmin(v, p);
            }
            q[lane] = v;
        }
        __syncthreads();
        if (lane == 0) {
            const double xmin = q[0], xmax = q[1], ymin = q[2], ymax = q[3], n = q[4];
            double xs = 0.0, ys = 0.0, scale = 0.0;
            if (n >= 4.0) {
                scale = fmax(xmax - xmin, ymax - ymin) * ratio;
                if (scale != 0.0) {
                    xs = (xmin + xmax - scale) / 2;
                    ys = (ymin + ymax - scale) / 2;
                } else {
                    scale = 0.0;                                               // (-0.0 too)
                }
            }
            double* b = box + (size_t)s * 4;
            b[0] = xs; b[1] = ys; b[2] = scale; b[3] = n;
        }
        __syncthreads();
    }
}

// launch 3: the transform.  flags bit 0: pixel mode, bit 1: crop mode (after the pixel mode where both are set, dataset_wild.py:78-85)
__global__ __launch_bounds__(WI_THREADS) void wild_transform_kernel(const double* __restrict__ kp, const int* __restrict__ chunk_tab, int n_chunks,
                                                                     int S, int F, double half_w, double half_h, double pix_scale, int flags,
                                                                     int channels, const double* __restrict__ box, float* __restrict__ y) {
    const bool pixel = flags & 1, crop = flags & 2;
    for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        int trk, f0, nf;
        if (!wi_chunk(chunk_tab, ch, S, F, trk, f0, nf)) continue;
        double xs = 0.0, ys = 0.0, scale = 1.0;
        if (crop) {
            const double* b = box + (size_t)trk * 4;
            xs = b[0]; ys = b[1]; scale = b[2];
        }
        const bool zero = crop && scale == 0.0;                               // np.zeros(motion.shape): all three channels
        for (int r = threadIdx.x; r < nf * WI_J; r += WI_THREADS) {
            const int f = f0 + r / WI_J, j = r % WI_J;
            double x, yy, c;
            wi_joint(kp + (size_t)f * (WI_V * 3), j, x, yy, c);
            if (pixel) wi_pixel(x, yy, half_w, half_h, pix_scale);
            if (zero) {
                x = yy = c = 0.0;
            } else if (crop) {
                x = (x - xs) / scale;                                          // utils_data.py:26
                yy = (yy - ys) / scale;
                x = (x - 0.5) * 2;                                             // :27
                yy = (yy - 0.5) * 2;
                x = fmin(fmax(x, -1.0), 1.0);                                  // :28, the confidence too
                yy = fmin(fmax(yy, -1.0), 1.0);
                c = fmin(fmax(c, -1.0), 1.0);
            }
            float* o = y + ((size_t)f * WI_J + j) * channels;
            o[0] = (float)x;
            o[1] = (float)yy;
            if (channels == 3) o[2] = (float)c;
        }
    }
}

extern "C" size_t mbx_wild_input_ws(int F, int S) {
    if (F < 0 || S < 0) return 0;
    const size_t chunks = (size_t)F / MBX_WILD_CHUNK + (size_t)S + 1;         // every track ends with at most one partial chunk
    return (chunks * 5 + (size_t)S * 4) * sizeof(double) + 64;
}

extern "C" int mbx_wild_input(const double* kp, const int* chunk_tab, int n_chunks, const int* seq_chunk_ptr, int S, int F, double half_w,
                              double half_h, double pix_scale, double ratio, int flags, int channels, float* y, double* box, void* ws,
                              size_t ws_bytes, void* stream) {
    MBX_CHECK_ARG(F >= 0, "wild_input: bad frame count F=%d", F);
    if (F == 0) return 0;
    MBX_CHECK_ARG(kp && chunk_tab && seq_chunk_ptr && y && ws, "wild_input: null pointer");
    MBX_CHECK_ARG(S >= 1 && n_chunks >= 1, "wild_input: bad sizes S=%d n_chunks=%d (both >= 1)", S, n_chunks);
    MBX_CHECK_ARG((long long)n_chunks <= (long long)F / MBX_WILD_CHUNK + S + 1 && (long long)n_chunks <= (long long)F,
                  "wild_input: %d chunks for %d frames of %d tracks (chunks of at most %d frames that never span tracks)", n_chunks, F, S,
                  MBX_WILD_CHUNK);
    MBX_CHECK_ARG(flags >= 1 && flags <= 3, "wild_input: bad flags %d (bit 0 pixel mode, bit 1 crop mode; at least one)", flags);
    MBX_CHECK_ARG(channels == 2 || channels == 3, "wild_input: bad channels %d (2 or 3)", channels);
    if (flags & 1)
        MBX_CHECK_ARG(isfinite(half_w) && isfinite(half_h) && isfinite(pix_scale) && pix_scale > 0.0,
                      "wild_input: bad pixel mode half_w=%g half_h=%g pix_scale=%g (finite, pix_scale > 0)", half_w, half_h, pix_scale);
    if (flags & 2) MBX_CHECK_ARG(isfinite(ratio), "wild_input: bad crop ratio %g", ratio);
    MBX_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)kp & 7) == 0 && (!box || ((uintptr_t)box & 7) == 0), "wild_input: kp, box and ws must be 8-byte aligned");
    const size_t need = ((size_t)n_chunks * 5 + (size_t)S * 4) * sizeof(double);
    MBX_CHECK_ARG(ws_bytes >= need, "wild_input: workspace of %zu bytes, %zu needed (mbx_wild_input_ws)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    double* bx = box ? box : part + (size_t)n_chunks * 5;
    const int grid = wi_clamp_grid((size_t)n_chunks, WI_GRID_CAP);
    if ((flags & 2) || box) {
        hipLaunchKernelGGL(wild_box_partial_kernel, dim3(grid), dim3(WI_THREADS), 0, s, kp, chunk_tab, n_chunks, S, F, half_w, half_h, pix_scale,
                           flags & 1, part);
        MBX_LAUNCH_CHECK("wild_box_partial");
        hipLaunchKernelGGL(wild_box_fold_kernel, dim3(wi_clamp_grid((size_t)S, WI_GRID_CAP)), dim3(MBX_WAVE), 0, s, (const double*)part,
                           seq_chunk_ptr, S, n_chunks, (flags & 2) ? ratio : 1.0, bx);
        MBX_LAUNCH_CHECK("wild_box_fold");
    }
    hipLaunchKernelGGL(wild_transform_kernel, dim3(grid), dim3(WI_THREADS), 0, s, kp, chunk_tab, n_chunks, S, F, half_w, half_h, pix_scale, flags,
                       channels, (const double*)bx, y);
    MBX_LAUNCH_CHECK("wild_transform");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the output stage.  One thread per joint of the batch.  flags bit 0: rootrel (infer_wild.py:81-82: joint 0 of every frame = 0), otherwise
// only [clip, frame 0, joint 0, z] = 0 (:84); bit 1: gt_2d (:86-87: xy from the network input, AFTER the zeroing); bit 2: pixel mode
// (:93-96) in numpy's arithmetic: the float32 product p * float32(min(w, h) / 2), and for xy that product widened to float64, (w, h) / 2
// added, the sum rounded to float32.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WI_THREADS) void wild_output_kernel(const float* __restrict__ pred, const float* __restrict__ x, int xc,
                                                                  const int* __restrict__ dst_frames, size_t total, int T, int flags,
                                                                  float pix_scale, double half_w, double half_h, float* __restrict__ out) {
    const bool rootrel = flags & 1, gt2d = flags & 2, pixel = flags & 4;
    const size_t per_clip = (size_t)T * WI_J;
    for (size_t idx = (size_t)blockIdx.x * WI_THREADS + threadIdx.x; idx < total; idx += (size_t)gridDim.x * WI_THREADS) {
        const int i = (int)(idx / per_clip);
        const int rem = (int)(idx % per_clip), t = rem / WI_J, j = rem % WI_J;
        const int d = dst_frames[i];
        if (d < 0) continue;
        const float* p = pred + idx * 3;
        float px = p[0], py = p[1], pz = p[2];
        if (rootrel) {
            if (j == 0) px = py = pz = 0.f;
        } else if (t == 0 && j == 0) {
            pz = 0.f;
        }
        if (gt2d) {
            const float* xi = x + idx * xc;
            px = xi[0]; py = xi[1];
        }
        if (pixel) {
            px = px * pix_scale; py = py * pix_scale; pz = pz * pix_scale;
            px = (float)((double)px + half_w);
            py = (float)((double)py + half_h);
        }
        float* o = out + ((size_t)d + t) * (WI_J * 3) + j * 3;
        o[0] = px; o[1] = py; o[2] = pz;
    }
}

extern "C" int mbx_wild_output(const float* pred, const float* x, int x_channels, const int* dst_frames, int n, int T, int flags,
                               float pix_scale, double half_w, double half_h, float* out, void* stream) {
    MBX_CHECK_ARG(n >= 0 && T >= 1, "wild_output: bad shape n=%d T=%d (n >= 0, T >= 1)", n, T);
    if (n == 0) return 0;
    MBX_CHECK_ARG(pred && dst_frames && out, "wild_output: null pointer");
    MBX_CHECK_ARG((flags & ~7) == 0, "wild_output: unknown flags %d (bit 0 rootrel, bit 1 gt_2d, bit 2 pixel mode)", flags);
    if (flags & 2) MBX_CHECK_ARG(x && (x_channels == 2 || x_channels == 3), "wild_output: gt_2d needs the network input x with 2 or 3 channels (got %d)", x_channels);
    if (flags & 4)
        MBX_CHECK_ARG(isfinite(pix_scale) && isfinite(half_w) && isfinite(half_h), "wild_output: bad pixel mode pix_scale=%g half_w=%g half_h=%g",
                      (double)pix_scale, half_w, half_h);
    MBX_CHECK_ARG((long long)n * T <= (1ll << 26), "wild_output: a batch of %lld frames is too large", (long long)n * T);
    const size_t total = (size_t)n * T * WI_J;
    hipLaunchKernelGGL(wild_output_kernel, dim3(wi_clamp_grid((total + WI_THREADS - 1) / WI_THREADS, WI_GRID_CAP)), dim3(WI_THREADS), 0,
                       (hipStream_t)stream, pred, x, x_channels, dst_frames, total, T, flags, pix_scale, half_w, half_h, out);
    MBX_LAUNCH_CHECK("wild_output");
    return 0;
}

// The output stage of one RAGGED batch: pred [Fb,17,3] holds whole clips of different lengths one after another and goes to rows
// dst0 .. dst0 + Fb - 1 of out; frame_t [Fb] = the index of each frame inside its clip.  The reference zeroes z of joint 0 of frame 0 of
// every clip (infer_wild.py:84): here that is every frame with frame_t == 0.  Everything else is wild_output_kernel's arithmetic.
__global__ __launch_bounds__(WI_THREADS) void wild_output_ragged_kernel(const float* __restrict__ pred, const float* __restrict__ x, int xc,
                                                                         const int* __restrict__ frame_t, size_t total, int flags,
                                                                         float pix_scale, double half_w, double half_h, float* __restrict__ out) {
    const bool rootrel = flags & 1, gt2d = flags & 2, pixel = flags & 4;
    for (size_t idx = (size_t)blockIdx.x * WI_THREADS + threadIdx.x; idx < total; idx += (size_t)gridDim.x * WI_THREADS) {
        const int f = (int)(idx / WI_J), j = (int)(idx % WI_J);
        const float* p = pred + idx * 3;
        float px = p[0], py = p[1], pz = p[2];
        if (rootrel) {
            if (j == 0) px = py = pz = 0.f;
        } else if (j == 0 && frame_t[f] == 0) {
            pz = 0.f;
        }
        if (gt2d) {
            const float* xi = x + idx * xc;
            px = xi[0]; py = xi[1];
        }
        if (pixel) {
            px = px * pix_scale; py = py * pix_scale; pz = pz * pix_scale;
            px = (float)((double)px + half_w);
            py = (float)((double)py + half_h);
        }
        float* o = out + idx * 3;
        o[0] = px; o[1] = py; o[2] = pz;
    }
}

extern "C" int mbx_wild_output_ragged(const float* pred, const float* x, int x_channels, const int* frame_t, int Fb, int dst0, int F, int flags,
                                      float pix_scale, double half_w, double half_h, float* out, void* stream) {
    MBX_CHECK_ARG(Fb >= 0 && F >= 0 && dst0 >= 0 && (long long)dst0 + Fb <= (long long)F,
                  "wild_output_ragged: a batch of %d frames at row %d does not fit out [%d,17,3]", Fb, dst0, F);
    if (Fb == 0) return 0;
    MBX_CHECK_ARG(pred && frame_t && out, "wild_output_ragged: null pointer");
    MBX_CHECK_ARG((flags & ~7) == 0, "wild_output_ragged: unknown flags %d (bit 0 rootrel, bit 1 gt_2d, bit 2 pixel mode)", flags);
    if (flags & 2) MBX_CHECK_ARG(x && (x_channels == 2 || x_channels == 3), "wild_output_ragged: gt_2d needs the network input x with 2 or 3 channels (got %d)", x_channels);
    if (flags & 4)
        MBX_CHECK_ARG(isfinite(pix_scale) && isfinite(half_w) && isfinite(half_h), "wild_output_ragged: bad pixel mode pix_scale=%g half_w=%g half_h=%g",
                      (double)pix_scale, half_w, half_h);
    MBX_CHECK_ARG(Fb <= (1 << 26), "wild_output_ragged: a batch of %d frames is too large", Fb);
    const size_t total = (size_t)Fb * WI_J;
    hipLaunchKernelGGL(wild_output_ragged_kernel, dim3(wi_clamp_grid((total + WI_THREADS - 1) / WI_THREADS, WI_GRID_CAP)), dim3(WI_THREADS), 0,
                       (hipStream_t)stream, pred, x, x_channels, frame_t, total, flags, pix_scale, half_w, half_h, out + (size_t)dst0 * (WI_J * 3));
    MBX_LAUNCH_CHECK("wild_output_ragged");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// mbx_scale_fit: the camera-frame scale of infer_wild_mesh.py:42-56.  One workgroup per track runs the whole iteratively reweighted
// least-squares solve: a pass over the track's points leaves ten sums (thread partials in point order, DPP inside a wave, the waves added in
// wave order), every thread forms the same closed-form update from them and the same decision to stop.  Point p of a track is frame
// p / 17, joint p % 17, whatever else the call holds: pooled and single-track calls add the same values in the same order.
// ---------------------------------------------------------------------------------------------------------------
#define SF_THREADS 1024
#define SF_WAVES (SF_THREADS / MBX_WAVE)
#define SF_Q 10

// wave_sum of mbx_common.h for float64 (the masked rows of the two row_bcast steps receive 0).  Every lane of the wave must be active.
__device__ __forceinline__ double wave_sum_d(double v) {
    v = v + dpp_mov_d<0xB1>(v, v);
    v = v + dpp_mov_d<0x4E>(v, v);
    v = v + dpp_mov_d<0x141>(v, v);
    v = v + dpp_mov_d<0x140>(v, v);
    v = v + dpp_mov_d<0x142, 0xa>(0.0, v);
    v = v + dpp_mov_d<0x143, 0xc>(0.0, v);
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), 63);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// x = ref - ref[:, :1] in float64; y = kp - kp[:, :1] in float32 (numpy on the float32 reg3d_all), widened
__device__ __forceinline__ void sf_point(const double* __restrict__ ref, const float* __restrict__ kp, int f0, int p, double (&x)[3], double (&y)[3]) {
    const int f = f0 + p / WI_J, j = p % WI_J;
    const double* rf = ref + (size_t)f * (WI_J * 3);
    const float* kf = kp + (size_t)f * (WI_J * 3);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        x[c] = rf[j * 3 + c] - rf[c];
        y[c] = (double)(kf[j * 3 + c] - kf[c]);
    }
}

// the sums of q[0 .. nq) over the workgroup, the same bits in every thread
template <int NQ> __device__ __forceinline__ void sf_fold(double (&q)[NQ], double (*red)[SF_Q], int lane, int wave) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) q[k] = wave_sum_d(q[k]);
    __syncthreads();                                                          // the previous fold's readers are through
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) red[wave][k] = q[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        double s = red[0][k];
        for (int w = 1; w < SF_WAVES; ++w) s += red[w][k];
        q[k] = s;
    }
}

__global__ __launch_bounds__(SF_THREADS) void scale_fit_kernel(const double* __restrict__ ref, const float* __restrict__ kp,
                                                               const int* __restrict__ seq_ptr, int F, double* __restrict__ fit) {
    __shared__ double red[SF_WAVES][SF_Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int trk = blockIdx.x;
    const int f0 = seq_ptr[trk], f1 = seq_ptr[trk + 1];
    double* out = fit + (size_t)trk * 6;
    const double nan = __builtin_nan("");
    if (f0 < 0 || f1 > F || f0 >= f1) {                                       // uniform over the workgroup
        if (tid < 6) out[tid] = tid == 5 ? -1.0 : nan;
        return;
    }
    const int N = (f1 - f0) * WI_J;
    // max |y|: the magnitude delta and the stopping rule hang on
    double ymax = 0.0;
    for (int p = tid; p < N; p += SF_THREADS) {
        double x[3], y[3];
        sf_point(ref, kp, f0, p, x, y);
        ymax = fmax(ymax, fmax(fabs(y[0]), fmax(fabs(y[1]), fabs(y[2]))));
    }
    ymax = wave_reduce_d<WaveMaxD>(ymax);
    if (lane == 0) red[wave][0] = ymax;
    __syncthreads();
    ymax = red[0][0];
    for (int w = 1; w < SF_WAVES; ++w) ymax = fmax(ymax, red[w][0]);
    const double delta = MBX_SCALE_FIT_DELTA * ymax;
    double s = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
    int status = -3, it = 0;
    for (; it < MBX_SCALE_FIT_CAP; ++it) {
        double q[SF_Q];
#pragma unroll
        for (int k = 0; k < SF_Q; ++k) q[k] = 0.0;
        for (int p = tid; p < N; p += SF_THREADS) {
            double x[3], y[3];
            sf_point(ref, kp, f0, p, x, y);
            const double e0 = s * x[0] + t0 - y[0], e1 = s * x[1] + t1 - y[1], e2 = s * x[2] + t2 - y[2];
            const double r = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            const double w = it == 0 ? 1.0 : 1.0 / fmax(r, delta);
            q[0] += w;
            q[1] += w * x[0]; q[2] += w * x[1]; q[3] += w * x[2];
            q[4] += w * y[0]; q[5] += w * y[1]; q[6] += w * y[2];
            q[7] += w * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            q[8] += w * (x[0] * y[0] + x[1] * y[1] + x[2] * y[2]);
            q[9] += r;
        }
        sf_fold<SF_Q>(q, red, lane, wave);
        const double W = q[0];
        const double den = q[7] - (q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) / W;
        if (!(den > 1e-12 * q[7])) { status = -2; break; }
        const double sn = (q[8] - (q[1] * q[4] + q[2] * q[5] + q[3] * q[6]) / W) / den;
        const double n0 = (q[4] - sn * q[1]) / W, n1 = (q[5] - sn * q[2]) / W, n2 = (q[6] - sn * q[3]) / W;
        const double ds = fabs(sn - s), dt = fmax(fabs(n0 - t0), fmax(fabs(n1 - t1), fabs(n2 - t2)));
        s = sn; t0 = n0; t1 = n1; t2 = n2;
        if (it > 0 && ds <= MBX_SCALE_FIT_TOL * fmax(fabs(sn), 1e-300) && dt <= MBX_SCALE_FIT_TOL * ymax) { status = 0; ++it; break; }
    }
    if (status < 0) {
        if (tid < 6) out[tid] = tid == 5 ? (double)status : nan;
        return;
    }
    double o[1] = {0.0};
    for (int p = tid; p < N; p += SF_THREADS) {
        double x[3], y[3];
        sf_point(ref, kp, f0, p, x, y);
        const double e0 = s * x[0] + t0 - y[0], e1 = s * x[1] + t1 - y[1], e2 = s * x[2] + t2 - y[2];
        o[0] += sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    }
    sf_fold<1>(o, red, lane, wave);
    if (tid == 0) {
        out[0] = s; out[1] = t0; out[2] = t1; out[3] = t2; out[4] = o[0] / (double)N; out[5] = (double)it;
    }
}

extern "C" int mbx_scale_fit(const double* ref, const float* kp, const int* seq_ptr, int S, int F, double* fit, void* stream) {
    MBX_CHECK_ARG(S >= 0 && F >= 0 && (long long)F * WI_J <= (1ll << 30), "scale_fit: bad sizes S=%d F=%d (S, F >= 0, 17 F <= 2^30)", S, F);
    if (S == 0) return 0;
    MBX_CHECK_ARG(seq_ptr && fit && (F == 0 || (ref && kp)), "scale_fit: null pointer");
    MBX_CHECK_ARG(((uintptr_t)ref & 7) == 0 && ((uintptr_t)fit & 7) == 0 && ((uintptr_t)kp & 3) == 0 && ((uintptr_t)seq_ptr & 3) == 0,
                  "scale_fit: ref and fit must be 8-byte aligned, kp and seq_ptr 4-byte aligned");
    MBX_CHECK_ARG(S <= (1 << 20), "scale_fit: %d tracks are too many (at most 2^20)", S);
    hipLaunchKernelGGL(scale_fit_kernel, dim3(S), dim3(SF_THREADS), 0, (hipStream_t)stream, ref, kp, seq_ptr, F, fit);
    MBX_LAUNCH_CHECK("scale_fit");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// mbx_wild_mesh_place: infer_wild_mesh.py:153-154.  Workgroup = one frame x PL_CHUNK values; the frame's track is found by bisection in
// seq_ptr (uniform over the workgroup).
// ---------------------------------------------------------------------------------------------------------------
#define PL_CHUNK 4096

__global__ __launch_bounds__(WI_THREADS) void wild_mesh_place_kernel(float* verts, const float* __restrict__ kp, int K,
                                                                      const double* __restrict__ ref, const int* __restrict__ seq_ptr, int S,
                                                                      const double* __restrict__ fit, int F, int V) {
    const int f = blockIdx.x;
    int lo = 0, hi = S;                                                       // the last s with seq_ptr[s] <= f
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seq_ptr[mid] <= f) lo = mid; else hi = mid;
    }
    if (!(seq_ptr[lo] <= f && f < seq_ptr[lo + 1])) return;
    const double sc = fit[(size_t)lo * 6];
    const float* k0 = kp + (size_t)f * K * 3;
    const double* r0 = ref + (size_t)f * (WI_J * 3);
    const float kx = k0[0], ky = k0[1], kz = k0[2];
    const double cx = r0[0] * sc, cy = r0[1] * sc, cz = r0[2] * sc;           // root_cam = ref_pose[:, :1] * scale
    float* row = verts + (size_t)f * 3 * V;
    const int e0 = blockIdx.y * PL_CHUNK, e1 = min(e0 + PL_CHUNK, 3 * V);
    for (int e = e0 + threadIdx.x; e < e1; e += WI_THREADS) {
        const int c = e % 3;
        const float d = row[e] - (c == 0 ? kx : (c == 1 ? ky : kz));
        row[e] = (float)((double)d + (c == 0 ? cx : (c == 1 ? cy : cz)));
    }
}

extern "C" int mbx_wild_mesh_place(float* verts, const float* kp, int K, const double* ref, const int* seq_ptr, int S, const double* fit, int F,
                                   int V, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= (1 << 24) && V >= 1 && V <= (1 << 20) && K >= 1 && K <= 32 && S >= 0 && S <= (1 << 20),
                  "wild_mesh_place: bad sizes F=%d V=%d K=%d S=%d (V >= 1, 1 <= K <= 32)", F, V, K, S);
    if (F == 0 || S == 0) return 0;
    MBX_CHECK_ARG(verts && kp && ref && seq_ptr && fit, "wild_mesh_place: null pointer");
    MBX_CHECK_ARG(((uintptr_t)ref & 7) == 0 && ((uintptr_t)fit & 7) == 0 && (((uintptr_t)verts | (uintptr_t)kp | (uintptr_t)seq_ptr) & 3) == 0,
                  "wild_mesh_place: ref and fit must be 8-byte aligned, verts, kp and seq_ptr 4-byte aligned");
    const int chunks = (3 * V + PL_CHUNK - 1) / PL_CHUNK;
    hipLaunchKernelGGL(wild_mesh_place_kernel, dim3(F, chunks), dim3(WI_THREADS), 0, (hipStream_t)stream, verts, kp, K, ref, seq_ptr, S, fit, F, V);
    MBX_LAUNCH_CHECK("wild_mesh_place");
    return 0;
}

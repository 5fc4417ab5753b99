// The way a tile of samples leaves the two tile rasterisers (render.hip, skeleton.hip): RD_TILE x RD_TILE samples per workgroup of RD_THREADS
// lanes, a lane owns the 2 x 2 quad (qx, qy); the tile's colours go through LDS and leave as whole dwords where the image rows allow it.
#pragma once
#include "mbx_common.h"

#define RD_SUB MBX_RENDER_SUB
#define RD_TILE 32                    // samples per tile edge; a lane owns a 2 x 2 quad: 16 x 16 quads = RD_THREADS
#define RD_THREADS 256
#define RD_STAGE_WORDS (RD_TILE * RD_TILE * 3 / 4)

// col[s]: the colour of the quad's sample (s & 1, s >> 1) as r | g << 8 | b << 16.  ss = 2: pixel = (a + b + c + d + 2) >> 2 per channel.
// Every lane of the workgroup calls this (it holds a barrier); stage: RD_STAGE_WORDS words of LDS.
__device__ __forceinline__ void rd_store_tile(const unsigned (&col)[4], unsigned* stage, int tid, int qx, int qy, int tx, int ty, int f, int size,
                                              int ss, unsigned char* __restrict__ rgb) {
    const int PW = RD_TILE / ss;                                             // pixels per tile edge
    unsigned char* st = (unsigned char*)stage;
    if (ss == 2) {
        unsigned char* p = st + (qy * PW + qx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            p[c] = (unsigned char)(((col[0] >> 8 * c & 255u) + (col[1] >> 8 * c & 255u) + (col[2] >> 8 * c & 255u) + (col[3] >> 8 * c & 255u) + 2u) >> 2);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            unsigned char* p = st + ((2 * qy + (s >> 1)) * PW + 2 * qx + (s & 1)) * 3;
            p[0] = (unsigned char)(col[s] & 255u); p[1] = (unsigned char)(col[s] >> 8 & 255u); p[2] = (unsigned char)(col[s] >> 16 & 255u);
        }
    }
    __syncthreads();
    const int px0 = tx * PW, py0 = ty * PW;
    const int pw = min(PW, size - px0), ph = min(PW, size - py0);            // the part of the tile inside the image (>= 1: the grid covers S)
    unsigned char* out = rgb + ((size_t)f * size * size) * 3;
    if (pw == PW && (size & 3) == 0 && ((uintptr_t)rgb & 3) == 0) {          // whole rows of 3 PW bytes at a 4-byte aligned address: dword stores
        const int dpr = 3 * PW / 4;
        for (int e = tid; e < ph * dpr; e += RD_THREADS) {
            const int row = e / dpr, d = e % dpr;
            *(unsigned*)(out + ((size_t)(py0 + row) * size + px0) * 3 + 4 * d) = stage[row * dpr + d];
        }
    } else {
        for (int e = tid; e < ph * pw * 3; e += RD_THREADS) {
            const int row = e / (pw * 3), b = e % (pw * 3);
            out[((size_t)(py0 + row) * size + px0) * 3 + b] = st[row * PW * 3 + b];
        }
    }
}

// The same for an image of W x H pixels (scene.hip): rgb [F,H,W,3].  bg: the colour an uncovered sample takes, per sample (the caller fills col with
// it), so the mean of ss = 2 is that of the four samples as they are.  Dword stores where a row of the image is a whole number of dwords.
__device__ __forceinline__ void rd_store_tile_rect(const unsigned (&col)[4], unsigned* stage, int tid, int qx, int qy, int tx, int ty, int f, int W,
                                                   int H, int ss, unsigned char* __restrict__ rgb) {
    const int PW = RD_TILE / ss;
    unsigned char* st = (unsigned char*)stage;
    if (ss == 2) {
        unsigned char* p = st + (qy * PW + qx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            p[c] = (unsigned char)(((col[0] >> 8 * c & 255u) + (col[1] >> 8 * c & 255u) + (col[2] >> 8 * c & 255u) + (col[3] >> 8 * c & 255u) + 2u) >> 2);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            unsigned char* p = st + ((2 * qy + (s >> 1)) * PW + 2 * qx + (s & 1)) * 3;
            p[0] = (unsigned char)(col[s] & 255u); p[1] = (unsigned char)(col[s] >> 8 & 255u); p[2] = (unsigned char)(col[s] >> 16 & 255u);
        }
    }
    __syncthreads();
    const int px0 = tx * PW, py0 = ty * PW;
    const int pw = min(PW, W - px0), ph = min(PW, H - py0);                  // >= 1: the grid covers W ss x H ss samples
    unsigned char* out = rgb + ((size_t)f * H * W) * 3;
    if (pw == PW && (W & 3) == 0 && ((uintptr_t)rgb & 3) == 0) {
        const int dpr = 3 * PW / 4;
        for (int e = tid; e < ph * dpr; e += RD_THREADS) {
            const int row = e / dpr, d = e % dpr;
            *(unsigned*)(out + ((size_t)(py0 + row) * W + px0) * 3 + 4 * d) = stage[row * dpr + d];
        }
    } else {
        for (int e = tid; e < ph * pw * 3; e += RD_THREADS) {
            const int row = e / (pw * 3), b = e % (pw * 3);
            out[((size_t)(py0 + row) * W + px0) * 3 + b] = st[row * PW * 3 + b];
        }
    }
}

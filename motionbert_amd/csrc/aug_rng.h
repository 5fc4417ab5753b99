// Counter-based random numbers of the input-stage kernels (augment.hip, action.hip): u(stream, index) = hash(seed, stream, index) -- a
// value depends only on WHICH number it is, so the torch restatement in oracle/augment_oracle.py reproduces every draw.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

__device__ __forceinline__ uint32_t aug_hash(uint32_t slo, uint32_t shi, uint32_t stream, uint32_t idx) {
    uint32_t h = idx * 0x9E3779B1u ^ slo;
    h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
    h += stream * 0xC2B2AE3Du + shi;
    h ^= h >> 16; h *= 0x27D4EB2Fu; h ^= h >> 15;
    return h;
}
// uniform in [0, 1) with 24 random bits
__device__ __forceinline__ float aug_uniform(uint32_t slo, uint32_t shi, uint32_t stream, uint32_t idx) {
    return (float)(aug_hash(slo, shi, stream, idx) >> 8) * (1.0f / 16777216.0f);
}

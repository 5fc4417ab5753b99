// Diagnostic builds of libmbx.so: the ablation-bit defaults, and -- only when a diagnostic flag is set -- the in-kernel time stamps read by
// tools/*_trace.py.  The flags (tools/build_variants.py): MBX_DIAG (MBX_DBG switches and the ntp / pp256 kernel-argument stamps, the latter
// with MBX_TRACE), MBX_TN_TRACE, MBX_ROWS_TRACE, MBX_RN_TRACE, MBX_MLP_TRACE (=2: five more stamps), MBX_ATTN_TRACE.  The product build
// defines none of them and gets nothing from this header but four zeros.
#pragma once
#include "mbx_common.h"

// ---------------------------------------------------------------- ablation bits (timing only, results are wrong): -DMBX_x_DBG=bits
#ifndef MBX_ROWS_DBG
#define MBX_ROWS_DBG 0      // gemm_rows.hip: 1 no epilogue, 2 no LDS-DMA, 4 no fragment reads, 16 no MFMAs
#endif
#ifndef MBX_RN_DBG
#define MBX_RN_DBG 0        // gemm_rows_n.hip: 1 no epilogue, 2 no loop (prologue + epilogue only)
#endif
#ifndef MBX_MLP_DBG
#define MBX_MLP_DBG 0       // mlp_fused.hip: 1 no GELU micro-steps beside fc2, 2 no LDS-DMA in the loop, 4 no fragment reads, 8 no epilogue, 16 no MFMAs,
                            // 32 no barriers, 64 no stages at all (prologue + epilogue only), 128 GELU micro-steps spread over all four stages of a
                            // chunk (dummy source)
#endif
#ifndef MBX_ATTN_DBG
#define MBX_ATTN_DBG 0      // attention.hip: 1 no compute loops, 2 no copy-out stores, 4 no tile / statistics loads, 8 no exp2 (p = 1)
#endif

#if defined(MBX_TRACE) && !defined(MBX_DIAG)
#error "-DMBX_TRACE stamps the kernel of gemm_pipe.hip that takes its buffer as a -DMBX_DIAG argument: build with both"
#endif
#if defined(MBX_DIAG) || defined(MBX_TRACE) || defined(MBX_TN_TRACE) || defined(MBX_ROWS_TRACE) || defined(MBX_RN_TRACE) || \
    defined(MBX_MLP_TRACE) || defined(MBX_ATTN_TRACE)
#include <mutex>

// ---------------------------------------------------------------- host side: the one sized trace buffer of the process
// A tool hands over (buf, bytes) -- device memory it owns -- and withdraws it with (NULL, 0).  Every traced launcher computes the bytes its
// launch can write (grid x record length) and arms its kernel with the buffer only if they fit, with nullptr otherwise: the kernels skip
// their write-out on a null pointer, so an undersized or withdrawn buffer means "no trace", never a store outside the buffer.
struct MbxDiagState {
    std::mutex mu;
    long long* buf = nullptr;       // what an armed kernel is handed (read by the asynchronous copy to the kernel's symbol: static storage)
    long long* none = nullptr;      // what a refused one is handed
    size_t bytes = 0, last_need = 0;
};
inline MbxDiagState g_mbx_diag;     // (C++17 inline variable: one instance per library, whichever sources include this header)

extern "C" __attribute__((used, visibility("default"))) inline void mbx_diag_set_trace(void* buf, size_t bytes) {
    (void)hipDeviceSynchronize();   // no launch armed with the buffer that leaves is still running when its owner gets it back
    std::lock_guard<std::mutex> lk(g_mbx_diag.mu);
    g_mbx_diag.buf = bytes ? (long long*)buf : nullptr;
    g_mbx_diag.bytes = buf ? bytes : 0;
}
// the `need_bytes` of the last arming attempt: the tools assert it against their own record layout
extern "C" __attribute__((used, visibility("default"))) inline size_t mbx_diag_last_need(void) {
    std::lock_guard<std::mutex> lk(g_mbx_diag.mu);
    return g_mbx_diag.last_need;
}
// the address of the pointer to hand a launch that writes at most need_bytes
static inline long long* const* mbx_diag_slot(size_t need_bytes) {
    std::lock_guard<std::mutex> lk(g_mbx_diag.mu);
    g_mbx_diag.last_need = need_bytes;
    return g_mbx_diag.buf && need_bytes <= g_mbx_diag.bytes ? &g_mbx_diag.buf : &g_mbx_diag.none;
}
// kernels that take the buffer as an argument (MBX_DIAG: ntp_diag / pp256_diag)
static inline long long* mbx_diag_trace(size_t need_bytes) { return *mbx_diag_slot(need_bytes); }
// kernels that read a device global: mbx_diag_arm(HIP_SYMBOL(g_x_trace), need_bytes, stream) just before the launch
template <class Sym> static inline void mbx_diag_arm(const Sym& symbol, size_t need_bytes, hipStream_t s) {
    (void)hipMemcpyToSymbolAsync(symbol, mbx_diag_slot(need_bytes), sizeof(long long*), 0, hipMemcpyHostToDevice, s);
}

// ---------------------------------------------------------------- device side
// XCC_ID | HW_ID << 32 of the wave: which XCD / SE / CU / SIMD it runs on (tools/trace_common.py same_cu_gaps)
__device__ __forceinline__ long long mbx_hw_id() {
    return (long long)__builtin_amdgcn_s_getreg(63492) | ((long long)__builtin_amdgcn_s_getreg(63508) << 32);
}
// s_memrealtime (100 MHz, one clock for the whole chip) into dst if `on`; nothing is scheduled across a stamp either way
#define MBX_STAMP_IF(on_, dst_) do { if (on_) (dst_) = (long long)wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define MBX_STAMP(dst_) MBX_STAMP_IF(true, dst_)
// the shader-cycle counter of the wave's CU
__device__ __forceinline__ long long mbx_cycles() { return (long long)__builtin_readcyclecounter(); }
#endif

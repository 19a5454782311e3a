// Global -> LDS tiles: the coalesced copy of a contiguous run of floats (a tile of whole [C+12]-rows), and the buffer descriptors and
// LDS-DMA loads of every kernel that streams tiles into LDS without VGPR staging.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip_bf16.h"

namespace ssdhip {

// Copies src[0..total) to LDS with 16-byte vector loads where global memory is 16-byte aligned.
// `lds_base` must be 16-byte aligned and have room for total + 4 floats; returns the pointer p with
// p[i] <-> src[i] (LDS keeps the 16-byte phase of the global address).  Caller must __syncthreads().
//
// The plain loop below keeps ONE load in flight per thread (the compiler emits load / wait / ds_write per iteration).
// Measured on MI355X (profiles/r01l_loss_copy_variants.txt): batching 8 or 16 loads per thread ahead of the LDS stores
// made the loss kernels SLOWER (L1 27 -> 36 -> 41 us, backward 37 -> 46 -> 52 us); the latency is covered by the other
// workgroups of the CU instead, so the kernels that use this keep their LDS footprint small (>= 4 workgroups per CU).
__device__ __forceinline__ float* tile_copy_f32(float* lds_base, const float* __restrict__ src, int total, int tid, int nthreads) {
    const int phase = (int)(((uintptr_t)src & 15u) >> 2);
    float* tile = lds_base + phase;
    const int head = min(total, (4 - phase) & 3);
    if (tid < head) tile[tid] = src[tid];
    const int nvec = (total - head) >> 2;
    const float4* vsrc = reinterpret_cast<const float4*>(src + head);
    float4* vdst = reinterpret_cast<float4*>(tile + head);
    for (int i = tid; i < nvec; i += nthreads) vdst[i] = vsrc[i];
    const int done = head + (nvec << 2);
    if (tid < total - done) tile[done + tid] = src[done + tid];
    return tile;
}

// ---- buffer descriptors and LDS-DMA ---------------------------------------------------------------------------------------------
// The only place that builds a raw buffer descriptor or issues buffer_load ... lds.
// One wave-wide buffer_load ... lds: lane l writes 16 (or 4) bytes at lds_dst + 16 l (4 l) from base(rsrc) + soff + voff; an offset at
// or past num_records writes zeros.  No VGPR staging, so a wave keeps a whole tile (two or three dozen 1 KiB loads) in flight while it
// works on the previous one.  Issued from inline asm and counted by hand (wait_vmcnt, tile_wait_vmcnt): a __builtin load makes hipcc put
// s_waitcnt vmcnt(0) in front of every LDS read that might alias an in-flight DMA, and __syncthreads() waits vmcnt(0) as well.
// M0 holds the LDS destination; hipcc does not model M0 around an asm statement, so it is saved and restored INSIDE the statement (the
// s_nop 0 is the wait state between the write of M0 and the LDS-DMA instruction that reads it: nothing inside an asm string is padded).
//
// lds_dst and soff must be wave-uniform: they go into SGPRs.  An "s" constraint does not insert a v_readfirstlane by itself -- when
// hipcc has folded a common factor of a uniform expression into a vector register the statement does not compile, or compiles only
// by luck of the surrounding code.  So the callers whose destination depends on values hipcc keeps in VGPRs say wave_uniform(...)
// at the call: ssdhip_convh.hip forces both lds_dst and soff, ssdhip_convimg.hip and ssdhip_wgrad.hip force lds_dst.  The callers whose
// operands are uniform as written (ssdhip_conv.hip, ssdhip_conv64.hip, the loss, decode and head tiles) pass them straight through; a
// readfirstlane there would be one more instruction per request.  ssdhip_conv64.hip passes its constant soffset 0 through
// tile_dma16_soff, i.e. in an SGPR, where the other kernels use tile_dma16's immediate.  These differences are kept as each kernel
// was tuned and tested; a new kernel takes tile_dma16 / tile_dma16_soff and adds wave_uniform only where hipcc asks for it.
constexpr unsigned int TILE_OOB = 0x80000000u;

// base + offset_bytes .. + num_bytes as a raw buffer: stride 0, no swizzle, 32-bit raw data format (offset_bytes may be negative:
// ssdhip_conv.hip moves the base down by its largest negative tap displacement so that every soffset is non-negative)
__device__ __forceinline__ i32x4 tile_rsrc(const void* base, long offset_bytes, u32 num_bytes) {
    const unsigned long long a = (unsigned long long)(uintptr_t)base + (unsigned long long)offset_bytes;
    i32x4 r;
    r.x = (int)(u32)a;
    r.y = (int)((u32)(a >> 32) & 0xffffu);
    r.z = (int)num_bytes;
    r.w = 0x00020000;
    return r;
}
__device__ __forceinline__ i32x4 tile_rsrc(const void* base, u32 num_bytes) { return tile_rsrc(base, 0, num_bytes); }

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ u32 wave_uniform(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

#define SSDHIP_LDS_DMA(load, soff) "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" load " %1, %2, " soff " offen lds\n\ts_mov_b32 m0, %0"
__device__ __forceinline__ void tile_dma16(u32 voff, i32x4 rsrc, u32 lds_dst) {                  // 16 bytes per lane, soffset 0
    u32 keep;
    asm volatile(SSDHIP_LDS_DMA("buffer_load_dwordx4", "0") : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void tile_dma16_soff(u32 voff, i32x4 rsrc, u32 lds_dst, u32 soff) {   // ... soffset in an SGPR
    u32 keep;
    asm volatile(SSDHIP_LDS_DMA("buffer_load_dwordx4", "%4") : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_dst), "s"(soff) : "memory");
}
__device__ __forceinline__ void tile_dma4(u32 voff, i32x4 rsrc, u32 lds_dst) {                   // 4 bytes per lane, soffset 0
    u32 keep;
    asm volatile(SSDHIP_LDS_DMA("buffer_load_dword", "0") : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_dst) : "memory");
}
#undef SSDHIP_LDS_DMA
// s_waitcnt vmcnt(N) for a compile-time N
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
// s_waitcnt vmcnt(n) for a wave-uniform run-time n <= 63 (the immediate has to be a constant: a jump over 64 one-instruction cases)
__device__ __forceinline__ void tile_wait_vmcnt(int n) {
#define SSDHIP_W1(k) case k: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(k) : "memory"); break;
#define SSDHIP_W8(k) SSDHIP_W1(k) SSDHIP_W1(k + 1) SSDHIP_W1(k + 2) SSDHIP_W1(k + 3) SSDHIP_W1(k + 4) SSDHIP_W1(k + 5) SSDHIP_W1(k + 6) SSDHIP_W1(k + 7)
    switch (n) {
        SSDHIP_W8(0) SSDHIP_W8(8) SSDHIP_W8(16) SSDHIP_W8(24) SSDHIP_W8(32) SSDHIP_W8(40) SSDHIP_W8(48) SSDHIP_W8(56)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef SSDHIP_W8
#undef SSDHIP_W1
}
#else
__device__ inline u32 wave_uniform(u32 v) { return v; }
__device__ inline void tile_dma16(u32, i32x4, u32) {}
__device__ inline void tile_dma16_soff(u32, i32x4, u32, u32) {}
__device__ inline void tile_dma4(u32, i32x4, u32) {}
template <int N> __device__ inline void wait_vmcnt() {}
__device__ inline void tile_wait_vmcnt(int) {}
#endif

}  // namespace ssdhip

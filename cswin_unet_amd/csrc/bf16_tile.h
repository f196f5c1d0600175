// What the bf16 MFMA kernels of libcswin_hip share (gemm.hip: the tiled family's bf16 loop and epilogue; gemm16.hip; wgrad16.hip),
// gfx950 / CDNA4: the LDS-DMA primitive, the transposing LDS read, the accumulator patch, the bf16 widening and the debug stamps.
// Each exists once, here.  Ring depths, wait ladders, swizzles and tile sizes stay with the kernels.
#pragma once
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// widen one bf16 / 4 bf16 held as two raw dwords.  Raw bf16 bits travel in INTEGER vectors: hipcc 7.2 miscompiles bit casts of the
// elements of a 2-float vector (element 1 reads element 0).
__device__ __forceinline__ float widen_bf16(unsigned short raw) { return __builtin_bit_cast(float, (unsigned)raw << 16); }
__device__ __forceinline__ f32x4 widen_bf16x4(u32x2 raw) {
    return f32x4{__builtin_bit_cast(float, raw[0] << 16), __builtin_bit_cast(float, raw[0] & 0xffff0000u),
                 __builtin_bit_cast(float, raw[1] << 16), __builtin_bit_cast(float, raw[1] & 0xffff0000u)};
}

// ---- LDS-DMA: 64 lanes x 16 B from per-lane global addresses to lds_dst + 16 * lane, no VGPRs and no ds_write.
// Contract: lds_dst is wave-uniform (it travels in m0, saved and restored here); hipcc does not count these loads, so their
// completion is tracked by hand -- dma_wait<N>() returns when at most N of this wave's DMAs are outstanding, the caller counts how
// many it has issued since -- and nothing else in a main loop that uses them may touch vmcnt (loads the loop's epilogue needs are
// requested BEFORE the first DMA: older in the in-order queue, they leave the counts alone).  dma_barrier(): this wave's LDS
// accesses are done and every wave of the workgroup has arrived, i.e. a landed step is visible and the stage read before it is free.
__device__ __forceinline__ void lds_dma(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N> __device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void dma_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- transposing read (ds_read_b64_tr_b16) of a [row][column] bf16 image: lane (q, p) of its 16-lane group supplies row r + q,
// columns c0 + 4 p .. + 3 of a 4-row x 16-column block and receives column c0 + (lane & 15) of rows r .. r + 3.  Two reads, of
// rows r and r + 4, give the 8 row-contiguous values of this lane's column that v_mfma_f32_32x32x16_bf16 wants.  a0, a4: this
// lane's addresses in rows r and r + 4, the caller's swizzle applied (two addresses, not an address and a distance: where the
// two rows' swizzles differ the distance is one more value per lane, 6 VGPRs in wgrad16.hip).
__device__ __forceinline__ bf16x8 tr16_frag(const void* a0, const void* a4) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a4);
    const s16x8 f = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    return __builtin_bit_cast(bf16x8, f);
}

// ---- accumulator patch.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), i.e. a lane
// owns one COLUMN of the fragment.  Storing from that layout is 16 dword stores per fragment (store-issue bound, measured 20-26 %
// of a workgroup's life).  Each wave therefore transposes its fragment through a private [32][EP_LD] LDS patch so that a lane
// owns 4 consecutive columns of one row (row (lane >> 3) + 8 p, columns 4 (lane & 7) .. + 3): operands are read and results
// written with 16-B accesses, 8 full 128-B lines per wave instruction.
constexpr int EP_LD = 36;
constexpr int EP_WAVE_FLOATS = 32 * EP_LD;

// what a wave wrote to its own patch is visible to all its lanes, and what they read is read, before the patch is written again
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void patch_put(float* patch, const f32x16& acc, int lane) {
    float* at = patch + 4 * (lane >> 5) * EP_LD + (lane & 31);      // one base, constant offsets: the stores pair (ds_write2_b32)
#pragma unroll
    for (int g = 0; g < 16; ++g) at[((g & 3) + 8 * (g >> 2)) * EP_LD] = acc[g];
    wave_lds_fence();
}

// ---- debug stamps (cswin_debug_set_stamps; tools/gemm_stamps.py, tools/wgrad16_stamps.py): thread 0 of workgroup `row` writes
// its row of stamps[workgroups][8].  Slots 0 .. 3: s_memtime at the kernel's start, after the first k-step's data is in LDS, after
// the main loop and at the end; 4: the hardware id register; 5, 6: s_memrealtime beside slots 0 and 3; 7: not written.
constexpr int STAMP_HW_ID = 6164;      // s_getreg operand: register id 20 (the XCC id), offset 0, 4 bits  (20 | 0 << 6 | 3 << 11)
__device__ __forceinline__ void stamp_slot(long long* stamps, long row, int slot) {
    if (!stamps || threadIdx.x != 0) return;
    long long* s = stamps + 8L * row;
    s[slot] = __builtin_amdgcn_s_memtime();
    if (slot == 0) { s[4] = __builtin_amdgcn_s_getreg(STAMP_HW_ID); s[5] = __builtin_amdgcn_s_memrealtime(); }
    if (slot == 3) s[6] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace

// What the matrix-core kernel families share below their own tile structure (gfx950): operand vector types, the 16-bit MFMA
// wrappers and format traits, LDS-DMA issue, hand-counted waits and the XCD-aware tile order.  Every piece is a typedef or a
// __forceinline__ helper: a kernel that uses them compiles to the instructions it would have with the code written out.
#pragma once
#include "common.hpp"

namespace peclr {

typedef uint16_t h16_t;                  // storage of both 16-bit formats
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- v_mfma_f32_32x32x16_{bf16,f16}: a lane's 16-byte fragments (8 consecutive k of row / column lane & 31, k-half lane >> 5)
__device__ __forceinline__ f32x16 mma_bf16(const uint4& a, const uint4& b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mma_f16(const uint4& a, const uint4& b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

// ---- the six products of the exact bf16 triple (x == h + m + l: planes 0, 1, 2; m.l, l.m and l.l are dropped): product pr is
// plane X6_PA[pr] of the first operand times plane X6_QB[pr] of the second -- l.h, h.l, m.m, m.h, h.m, h.h, smallest first.  An
// accumulator receives them in THIS order: the order is part of the numerical contract (it fixes the rounding of every fp32
// result, and the kernels that exist in two forms are tested for bit equality).
constexpr int X6_PA[6] = {2, 0, 1, 1, 0, 0}, X6_QB[6] = {0, 2, 1, 0, 1, 0};

// ---- per-format pieces of the 16-bit kernels: MFMA, 16-bit -> fp32, fp32 pair -> packed word (round to nearest even)
struct BF16 {
    static constexpr int io = PECLR_DTYPE_BF16;
    static __device__ __forceinline__ f32x16 mma(const uint4& a, const uint4& b, f32x16 acc) { return mma_bf16(a, b, acc); }
    static __device__ __forceinline__ float up(unsigned lo16) { return __uint_as_float(lo16 << 16); }
    static __device__ __forceinline__ float lo(unsigned w) { return __uint_as_float(w << 16); }           // the two halves of a word,
    static __device__ __forceinline__ float hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }   // one instruction each
    static __device__ __forceinline__ unsigned pack2(float a, float b) { return pk_bf16(a, b); }
};
struct F16 {
    static constexpr int io = PECLR_DTYPE_F16;
    static __device__ __forceinline__ f32x16 mma(const uint4& a, const uint4& b, f32x16 acc) { return mma_f16(a, b, acc); }
    static __device__ __forceinline__ float up(unsigned lo16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)lo16); }
    static __device__ __forceinline__ float lo(unsigned w) { return f16_lo(w); }
    static __device__ __forceinline__ float hi(unsigned w) { return f16_hi(w); }
    static __device__ __forceinline__ unsigned pack2(float a, float b) { return pk_f16(a, b); }
};

// ---- LDS-DMA: 16 bytes per lane, global -> LDS at (wave-uniform, in an SGPR) lds_byte_offset + lane * 16; no VGPRs, no VALU, no
// ds_write.  Targets must lie below 64 KiB (M0 carries a 16-bit LDS address).  Issued through inline assembly on purpose: for the
// builtin, hipcc's wait-count pass makes EVERY later ds_read wait for the DMA (vmcnt(0) right behind the issue -- LDS accesses
// carry no alias information that would tell the buffer being filled from the one being read), which serialises the pipeline.
// Here the compiler does not know the instruction touches the vm counter: every wait on it is written by hand (wait_vmcnt
// below), and a kernel must know which other VMEM instructions are in flight while DMAs are.
__device__ __forceinline__ void lds_dma16(const void* src, unsigned lds_byte_offset) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                 :: "v"(src), "s"(lds_byte_offset) : "memory", "m0");
}
// ... with the non-temporal hint (rows that no other workgroup reads)
__device__ __forceinline__ void lds_dma16_nt(const void* src, unsigned lds_byte_offset) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off nt"
                 :: "v"(src), "s"(lds_byte_offset) : "memory", "m0");
}
// ... with a wave-uniform 64-bit base (scalar registers) + a 32-bit lane offset + an immediate: no vector arithmetic per
// request.  The instruction's immediate offset is added to the global address AND to the LDS address (M0 + offset +
// lane * 16): piece k of a contiguous run is (same base, same M0, offset k * 1024)
template <int IMM>
__device__ __forceinline__ void lds_dma16s(const void* sbase, unsigned lane_off, unsigned lds_byte_offset) {
    // (s_nop 4: the base may come straight from scalar arithmetic -- a vector memory instruction reading a scalar register the
    // scalar unit has just written needs five wait states, and the compiler does not see into this string)
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3"
                 :: "v"(lane_off), "s"(sbase), "s"(lds_byte_offset), "n"(IMM) : "memory", "m0");
}

// ---- hand-counted waits: at most N vector-memory requests of this wave still in flight (the counter retires in order) / every
// LDS operation of this wave done
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- XCD-aware tile order: the grid is 1-D (x), 8 * ceil(row blocks / 8) * column tiles (nct).  Workgroups go to the 8 XCDs
// round-robin, so hardware block b runs row block 8 * (j / nct) + b % 8, column tile j % nct with j = b / 8: every column tile
// of a row block lands on the SAME XCD, one after the other, and the operand tile they share is read from HBM once and from
// that XCD's L2 afterwards.  (Row blocks past the last one exist in the grid: the caller returns for them.)
struct XcdTile { int row_block, col_tile; };
__device__ __forceinline__ XcdTile xcd_tile(unsigned b, int nct) {
    const int j = b / 8;
    return {8 * (j / nct) + (int)(b % 8), j % nct};
}

}  // namespace peclr

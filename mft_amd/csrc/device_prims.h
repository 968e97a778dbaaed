// Device primitives shared by the MFMA kernels (conv_gemm.hip, tile_conv.hip, flow_branch.hip, volume_tile.hip and the two
// fused-lookup files): vector types, the LDS barrier, the fp16 MFMA, the split arithmetic, the GRU gate algebra, the pooling
// mean and the buffer-load helpers.  Every kernel must round these value for value like every other (the bitwise cross-unit
// tests rest on it), so each is defined here, once.  Device code only; include it from the kernel files, not from common.h.
#pragma once
#ifdef __HIPCC__

namespace mftx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The ONE s_barrier of the project (tests/test_host_logic.py holds csrc to that), with compiler fences on both sides: the
// intrinsic alone does not order LDS accesses.
__device__ __forceinline__ void lds_barrier() {
    // s_waitcnt lgkmcnt(0): gfx950 has back-off barriers, so the compiler inserts NO wait in front of s_barrier and the builtin is no
    // fence -- without this a wave's last ds_write may still sit in the LDS queue when another wave reads the slot behind the
    // barrier (found in round 5 with tools/race_kernels.py: harmless with the GPU to itself, wrong values under contention).
    // LDS only: global prefetches and LDS-DMA loads (vmcnt) stay in flight, their consumers count them themselves.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {   // counted wait: leaves N LDS-DMA loads in flight
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_waitcnt vmcnt(n) for a wave-uniform run-time n (the instruction takes an immediate).  Waiting for a smaller count than
// necessary is always safe, so n is rounded DOWN to a multiple of 8 (a gather of the fused lookup is 8, 16, 24 or 32
// operations: the exact counts are the ones that matter) -- nine cases instead of 64
#define MFTX_W(n) case n: asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory"); break;
__device__ __forceinline__ void wait_vmcnt_upto(int n) {
    switch (n < 63 ? (n & ~7) : 56) {
        MFTX_W(0) MFTX_W(8) MFTX_W(16) MFTX_W(24) MFTX_W(32) MFTX_W(40) MFTX_W(48)
        default: asm volatile("s_waitcnt vmcnt(56)" ::: "memory"); break;
    }
}
#undef MFTX_W

__device__ __forceinline__ f32x4 buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}

// LDS-DMA: 16 bytes (buf_load_lds) or one dword (buf_load_lds4) per lane straight into LDS: the wave's 64 lanes land
// lane-linear at `dst` (wave-uniform); an out-of-range offset stores zeros.
// soff: wave-uniform byte offset added to the address (not part of the range check, which is on voff alone)
__device__ __forceinline__ void buf_load_lds(__amdgpu_buffer_rsrc_t r, void *dst, unsigned voff, unsigned soff = 0) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void *)dst, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void buf_load_lds4(__amdgpu_buffer_rsrc_t r, void *dst, unsigned voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void *)dst, 4, voff, 0, 0, 0);
}

// v_mfma_f32_32x32x16_f16: fp16 operands, fp32 accumulation (each fp16 product is exact in fp32)
__device__ __forceinline__ f32x16 mfma_f16(const f16x8 &a, const f16x8 &b, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// ---- split arithmetic: x = hi + lo / 2048 with hi = fp16(x) and lo = fp16((x - hi) * 2048) (conv_gemm.hip: Arith) ----------
// hi / lo halves of 8 consecutive values, 2.5 instructions per value: v_cvt_pk_f16_f32 for two (round to nearest), the
// exact residual as one mixed-precision fma each (x - hi, hi read as fp16), and the scaled low half as
// v_fma_mixlo/mixhi_f16 (r * 2048 rounded to fp16 into one half of the destination).  Written as one assembly block: the
// compiler's own selection for this arithmetic takes 4 instructions per value, and does not know the mixed forms.
// (The block's text, once; TAIL = what follows the last instruction.  Expects u, v, k2048 and declares the results h0..3, l0..3.)
#define MFTX_SPLIT8_ASM(TAIL)                                                                                              \
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;                                                                               \
    float r0, r1, r2, r3, r4, r5, r6, r7;                                                                                  \
    asm("v_cvt_pk_f16_f32 %0, %16, %17\n\t"                                                                                \
        "v_cvt_pk_f16_f32 %1, %18, %19\n\t"                                                                                \
        "v_cvt_pk_f16_f32 %2, %20, %21\n\t"                                                                                \
        "v_cvt_pk_f16_f32 %3, %22, %23\n\t"                                                                                \
        "v_fma_mix_f32 %8, %0, -1.0, %16 op_sel_hi:[1,0,0]\n\t"                                                            \
        "v_fma_mix_f32 %9, %0, -1.0, %17 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"                                             \
        "v_fma_mix_f32 %10, %1, -1.0, %18 op_sel_hi:[1,0,0]\n\t"                                                           \
        "v_fma_mix_f32 %11, %1, -1.0, %19 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"                                            \
        "v_fma_mix_f32 %12, %2, -1.0, %20 op_sel_hi:[1,0,0]\n\t"                                                           \
        "v_fma_mix_f32 %13, %2, -1.0, %21 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"                                            \
        "v_fma_mix_f32 %14, %3, -1.0, %22 op_sel_hi:[1,0,0]\n\t"                                                           \
        "v_fma_mix_f32 %15, %3, -1.0, %23 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"                                            \
        "v_fma_mixlo_f16 %4, %8, %24, 0\n\t"                                                                               \
        "v_fma_mixlo_f16 %5, %10, %24, 0\n\t"                                                                              \
        "v_fma_mixlo_f16 %6, %12, %24, 0\n\t"                                                                              \
        "v_fma_mixlo_f16 %7, %14, %24, 0\n\t"                                                                              \
        "v_fma_mixhi_f16 %4, %9, %24, 0\n\t"                                                                               \
        "v_fma_mixhi_f16 %5, %11, %24, 0\n\t"                                                                              \
        "v_fma_mixhi_f16 %6, %13, %24, 0\n\t"                                                                              \
        "v_fma_mixhi_f16 %7, %15, %24, 0" TAIL                                                                             \
        : "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3),                          \
          "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)                           \
        : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]), "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(k2048))

// split8: halves as MFMA operands, and the block ends with the two wait states a VALU result needs before an MFMA reads it
// (the hazard recognizer does not see into inline assembly) -- conv_gemm, flow_branch, volume_tile: their next instruction is the MFMA.
__device__ __forceinline__ void split8(const f32x4 &u, const f32x4 &v, float k2048, f16x8 &hi, f16x8 &lo) {
    MFTX_SPLIT8_ASM("\n\ts_nop 1");
    hi = __builtin_bit_cast(f16x8, u32x4{h0, h1, h2, h3});
    lo = __builtin_bit_cast(f16x8, u32x4{l0, l1, l2, l3});
}
// split8_raw: halves as raw dwords, no wait states -- tile_conv: it stores them (split-form rows); where it does multiply
// them, the wait states follow its weight loads.
__device__ __forceinline__ void split8_raw(const f32x4 &u, const f32x4 &v, float k2048, u32x4 &hi, u32x4 &lo) {
    MFTX_SPLIT8_ASM("");
    hi = u32x4{h0, h1, h2, h3};
    lo = u32x4{l0, l1, l2, l3};
}
#undef MFTX_SPLIT8_ASM

// ... of 4 consecutive values (the same operations per value: the same bits); no wait states
__device__ __forceinline__ void split4(const f32x4 &u, float k2048, unsigned (&hi)[2], unsigned (&lo)[2]) {
    unsigned h0, h1, l0, l1;
    float r0, r1, r2, r3;
    asm("v_cvt_pk_f16_f32 %0, %8, %9\n\t"
        "v_cvt_pk_f16_f32 %1, %10, %11\n\t"
        "v_fma_mix_f32 %4, %0, -1.0, %8 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %5, %0, -1.0, %9 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %6, %1, -1.0, %10 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %7, %1, -1.0, %11 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %2, %4, %12, 0\n\t"
        "v_fma_mixlo_f16 %3, %6, %12, 0\n\t"
        "v_fma_mixhi_f16 %2, %5, %12, 0\n\t"
        "v_fma_mixhi_f16 %3, %7, %12, 0"
        : "=&v"(h0), "=&v"(h1), "=&v"(l0), "=&v"(l1), "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
        : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]), "s"(k2048));
    hi[0] = h0; hi[1] = h1; lo[0] = l0; lo[1] = l1;
}

// ... and of two values, as the piece that is slotted between two MFMAs of a K loop (5 instructions: they issue in the
// shadow of one 32-cycle MFMA).  No trailing wait states: the halves are consumed at least two MFMAs later, or stored.
__device__ __forceinline__ void split_pair(float x0, float x1, float k2048, unsigned &h, unsigned &l) {
    float r0, r1;
    asm("v_cvt_pk_f16_f32 %0, %4, %5\n\t"
        "v_fma_mix_f32 %2, %0, -1.0, %4 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %3, %0, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %2, %6, 0\n\t"
        "v_fma_mixhi_f16 %1, %3, %6, 0"
        : "=&v"(h), "=&v"(l), "=&v"(r0), "=&v"(r1)
        : "v"(x0), "v"(x1), "s"(k2048));
}

// One dword of a packed weight fragment: two consecutive k values of an MFMA operand row, their high halves (part 0) or their
// low halves (part 1) -- every pack kernel's word (split_halves: common.h, included before this header by every kernel file)
__device__ __forceinline__ unsigned frag_word(float v0, float v1, int part) {
    const unsigned a = split_halves(v0), b = split_halves(v1);
    return part ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
}

// Gate non-linearities of the GRU epilogues on the hardware exponential (v_exp_f32, ~1 ulp) and
// reciprocal: 16 values per lane and tile, where libm's expf / tanhf cost ~7 % of the q-gate kernel.
// Absolute error < 2e-7 on outputs in (-1, 1) -- four orders below the parity tolerance; the same
// code runs for every kernel, tile shape and batch, so results stay independent of all three.
__device__ __forceinline__ float fast_sigmoid(float s) { return __frcp_rn(1.f + __expf(-s)); }
__device__ __forceinline__ float fast_tanh(float s) {
    const float t = __expf(-2.f * fabsf(s));            // in (0, 1]: no overflow
    return copysignf((1.f - t) * __frcp_rn(1.f + t), s);
}

// h <- (1 - z) h + z q, with the contraction spelled out: the scalar and the vectorised epilogues (and every tile shape) must
// round alike, whatever the compiler would fuse in each
__device__ __forceinline__ float gru_blend(float z, float h, float q) { return __fmaf_rn(z, q, __fmul_rn(__fsub_rn(1.f, z), h)); }

// 2 x 2 mean in ATen's avg_pool2d order: ((a + b) + c + d) * 0.25, a b = top row, c d = bottom row
__device__ __forceinline__ float pool4(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

}  // namespace mftx

#endif  // __HIPCC__

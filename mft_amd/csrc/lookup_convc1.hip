// Correlation lookup FUSED into convc1 (core/corr.py:30-51 feeding core/update.py:152-153), split arithmetic.
//
// 323 of the lookup's 324 channels have exactly one consumer -- the 1 x 1 convolution convc1 -- 11 iterations out
// of 12.  Stand-alone, the lookup writes 37 MB of features per iteration (7 pairs of 512 x 512) that convc1 reads
// back and splits in registers.  Here the features never leave the CU: one workgroup owns a tile of up to 64 query
// cells; its four PRODUCER waves gather the cells' 10 x 10 windows (LDS-DMA, one dword per tap: what lies outside a
// level gets an out-of-range offset = grid_sample's zero padding, tap for tap), blend them, split the results into
// fp16 halves and park them in LDS in the A-operand layout of v_mfma_f32_32x32x16_f16; its four CONSUMER waves
// multiply them with convc1's weights (64 output channels per wave; the wave's weight fragments stream from L2
// straight into registers, three 16-wide k groups ahead -- no wave shares them, so LDS would add nothing) and write
// relu(. + bias) in the form convc2 reads.
//
//   unit      = (tile, pyramid level): 64 rows x 96 k -- the level's 81 window samples at k'' = 10 b + a (b: y
//               offset, a: x offset; a = 9 and k'' >= 90 carry zero weights), so that a sample's index is the index
//               of its upper-left tap in the 10 x 10 patch: every lane runs the same 24-sample loop on its own
//               quarter of a patch;
//   pipeline  = producers and consumers meet at ONE workgroup barrier per unit: barrier u certifies that unit u is
//               complete in A slot u & 1 and that the consumers are done with unit u - 1, whose slot then takes unit
//               u + 1 while the consumers multiply unit u.  Gathers run three units ahead of their conversion
//               (patch ring of three, counted vmcnt waits): the HBM round trip of a window hides under ~3 units of
//               matrix work.
//
// Results are independent of the tile size and of the batch: a row's 324 products are summed in the fixed order of
// the k groups, by one accumulator pair.
#include "common.h"
#include "profile.h"
#include "device_prims.h"

namespace mftx {
// (this variant's copy: lookup_convc1_shared.h says why)
struct LookupConvArgs {
    const float *lvl[4];
    long long stride[4];        // floats per query cell
    int hl[4], wl[4];
    int wb0, wb1;               // block-grid widths of levels 0, 1
    const float *coords;
    int cells;                  // P * h * w
    const void *wf;             // fused weights (mftx_pack_lookup_convc1_weights)
    const float *bias;
    float *out;
    int ld_out, out_split;
    int rpw;                    // cells per producer wave and tile: a tile is 4 rpw cells
    int n_tiles;
    int ablate;                 // tuning builds only (MFTX_LF_ABLATE): 1 no window gathers, 2 no MFMAs, 4 no conversion, 8 no weight loads, 16 no stores, 1024 LDS poisoned with NaNs first
};
}  // namespace mftx

#include "lookup_convc1_shared.h"

namespace mftx {

typedef __attribute__((address_space(3))) const unsigned lf_lds_u32;

constexpr int LF_PATCH = 400;                       // bytes per window patch: the 100 taps of a cell and level, patches of a unit back to back
constexpr int LF_PSLOT = 16 * LF_PATCH + 32;        // a unit's patches + 8 floats that stay zero (the last cell's dummy samples read them)
constexpr int LF_NP = 3;                            // patch ring (units) per producer wave: a unit's gather is issued two steps before its conversion

// ---------------------------------------------------------------------------------------------------------------
// producer waves (pw = 0..3): cells [pw rpw, (pw + 1) rpw) of every tile
// ---------------------------------------------------------------------------------------------------------------
struct LfProducer : LfProducerBase {
    // this lane's tap in DMA 4 i + e of a unit: the LDS addresses of its row entry and of its column entry in the table (round 6:
    // addresses, not packed indices -- the unpacking was 4 VALU instructions per DMA and lane, 100 per unit)
    lf_lds_u32 *tap_r[7][4], *tap_c[7][4];
    int ent[3];                  // (cell << 8 | j) of this lane's table entry in pass k (entries 64 k + lane of 16 x 10)
    static constexpr int PATCH_BYTES = LF_NP * LF_PSLOT;      // 19 296 per wave: 154 496 bytes of LDS in all (LfLayout)

    // VMEM operations of unit v's gather, and of the coordinate prefetch that follows a level-0 unit
#ifdef MFTX_TUNING
    __device__ __forceinline__ int n_gather(int v) const { return (v < U && !(p.ablate & 1)) ? ((((rpw + 3) & ~3) * 100 + 63) >> 6) : 0; }
#else
    __device__ __forceinline__ int n_gather(int v) const { return v < U ? ((((rpw + 3) & ~3) * 100 + 63) >> 6) : 0; }
#endif
    __device__ __forceinline__ int n_coord(int v) const { return (v < U && (v & 3) == 0 && (v >> 2) + 1 < my_tiles) ? 1 : 0; }

    // gather of unit v into patch slot v % 3.
    //   The VALU pipe of a SIMD is all a producer wave has (one instruction per four cycles), so the address arithmetic is
    // done ONCE per row and column of a window instead of once per tap: phase 1 forms, two cells per pass -- lane =
    // (cell & 1, row | column, j) --, the byte offset of window row j (or column j) inside the query's level slice, or a
    // large value where the row / column lies outside the level (any sum with it is out of range = a zero, as
    // grid_sample pads), into a small LDS table; phase 2 adds one row and one column entry per tap.
    struct GatherCtx { __amdgpu_buffer_rsrc_t rs; unsigned char *pdst; const unsigned *tb; int nd; };
    struct ConvCtx { float T[36]; float w00, w01, w10, w11; unsigned char *dst; const unsigned char *src; bool live; };

    // The address table of unit v: 160 row entries and 160 column entries (16 cells x 10), as three passes of rows and three of
    // columns -- entry 64 k + lane of a kind; the lane's (cell, j) of pass k were worked out once (ent[k]).  Every pass carries
    // ONE kind of entry, so no lane computes both forms and selects, and the multiplications are 24-bit (round 6: the table was
    // 2.1 k of the producer's 6.6 k cycles per step with three cells per pass and both kinds in every pass).
    // (All 16 cells, used or not: the last DMA of a short unit runs a few taps into the next cell's table entries, which must say
    // "outside" -- a stale entry could be a misaligned offset, and a misaligned dword of finite floats can be a NaN that the
    // next cell's zero-weight dummy samples would spread over a whole row.)
    __device__ __forceinline__ void table(int v) {
        const int k = v >> 2, l = v & 3;
        const float *base; long long stride; unsigned H, W, wb;
        level_geometry(v, base, stride, H, W, wb);
        const float inv = l == 0 ? 1.f : l == 1 ? 0.5f : l == 2 ? 0.25f : 0.125f;     // (x / 2^l, exactly)
        const bool blocked = l < 2;
        const unsigned rowmul = blocked ? wb * 128u : W * 4u;
        const unsigned stride4 = (unsigned)stride * 4u;
        const int cell0 = tile_of(k) * TR + pw * rpw;
        const float *cs = cslots + (k % 3) * 32;
        float cx[3], cy[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) { cx[q] = cs[2 * (ent[q] >> 8)]; cy[q] = cs[2 * (ent[q] >> 8) + 1]; }
#pragma unroll
        for (int q = 0; q < 3; ++q) {             // rows
            const int ci = ent[q] >> 8, j = ent[q] & 15;
            // clamp so that the int conversion is defined for wild coordinates
            const unsigned yy = (unsigned)((int)fminf(fmaxf(floorf(cy[q] * inv), -1.0e6f), 1.0e6f) - 4 + j);
            const unsigned val = (blocked ? __umul24(yy >> 2, rowmul) + (yy & 3u) * 32u : __umul24(yy, rowmul)) + __umul24((unsigned)ci, stride4);
            const bool ok = (ci < rpw) & (cell0 + ci < p.cells) & (yy < H);
            if (q < 2 || lane < 32) tab[ci * 32 + j] = ok ? val : 0x40000000u;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {             // columns
            const int ci = ent[q] >> 8, j = ent[q] & 15;
            const unsigned xx = (unsigned)((int)fminf(fmaxf(floorf(cx[q] * inv), -1.0e6f), 1.0e6f) - 4 + j);
            const unsigned val = blocked ? (xx >> 3) * 128u + (xx & 7u) * 4u : xx * 4u;
            const bool ok = (ci < rpw) & (cell0 + ci < p.cells) & (xx < W);
            if (q < 2 || lane < 32) tab[ci * 32 + 16 + j] = ok ? val : 0x40000000u;
        }
    }

    // what unit v's DMA groups need
    __device__ __forceinline__ GatherCtx gather_begin(int v) {
        GatherCtx G;
        const float *base; long long stride; unsigned H, W, wb;
        level_geometry(v, base, stride, H, W, wb);
        const int cell0 = tile_of(v >> 2) * TR + pw * rpw;
        G.pdst = patches + (v % 3) * LF_PSLOT;
        G.tb = tab;
        // ONE buffer descriptor per unit: this wave's cells are consecutive, their level slices lie `stride` floats apart --
        // the table has cell * stride folded into its row entries, so a tap's offset is still one addition
        const int c0 = __builtin_amdgcn_readfirstlane(cell0 < p.cells ? cell0 : 0);
        G.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base + (long long)c0 * stride), 0, (unsigned)rpw * (unsigned)stride * 4u, 0x00020000);
        // The unit's taps form ONE array -- cell after cell, 100 each -- and a DMA instruction fetches 64 consecutive ones:
        // 25 full instructions for 16 cells.  A lane's (cell, row, column) in DMA d never changes: their table addresses were
        // worked out once (tap_r / tap_c).  (Taps past the last cell: table entries that say "outside" -- zeros into a patch nobody reads.)
        G.nd = n_gather(v);
        return G;
    }

    // DMAs 4 i .. 4 i + 3 of a unit's gather: their table entries are read together, so the LDS latency shows once per four
    __device__ __forceinline__ void dma_group(const GatherCtx &G, int i) {
        unsigned o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = *tap_r[i][e] + *tap_c[i][e];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * i + e < G.nd) buf_load_lds4(G.rs, G.pdst + (4 * i + e) * 256, o[e]);
    }

    // conversion of unit v: lane (cell c16, quarter q) blends samples k'' = 24 q .. 24 q + 23 of its cell and stores
    // their halves into the A slot v & 1 -- in three chunks of eight samples, so that the DMAs of the next gather can be issued
    // between them (a DMA holds the wave that issues the NEXT one; VALU work slotted in between is free)
    // what the conversion of unit v needs apart from the taps -- bilinear weights, source, destination: worked out BEFORE the wait for
    // the unit's gather (it depends on the coordinates only; round 6: one LDS round trip less in the step's chain)
    __device__ __forceinline__ void conv_prepare(int v, ConvCtx &C) {
        float sx, sy;
        level_coords(v, sx, sy);
        const float fx = __fsub_rn(sx, floorf(sx)), fy = __fsub_rn(sy, floorf(sy));
        const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy);
        C.w00 = __fmul_rn(gx, gy); C.w01 = __fmul_rn(fx, gy); C.w10 = __fmul_rn(gx, fy); C.w11 = __fmul_rn(fx, fy);
        C.src = patches + (v % 3) * LF_PSLOT + c16 * LF_PATCH + q * 96;
        C.dst = lds + (v & 1) * LF_AUNIT + (pw * rpw + c16) * LF_AROW + q * 96;
        C.live = c16 < rpw;
    }
    __device__ __forceinline__ void conv_load(ConvCtx &C) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(C.src);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const f32x4 t = src[i];
            C.T[4 * i] = t[0]; C.T[4 * i + 1] = t[1]; C.T[4 * i + 2] = t[2]; C.T[4 * i + 3] = t[3];
        }
    }
    __device__ __forceinline__ void conv_chunk(const ConvCtx &C, int g8) {
        const float k2048 = 2048.f;
        unsigned h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 8 * g8 + 2 * e;
            const float v0 = lf_blend4(C.T[j], C.T[j + 1], C.T[j + 10], C.T[j + 11], C.w00, C.w01, C.w10, C.w11);
            const float v1 = lf_blend4(C.T[j + 1], C.T[j + 2], C.T[j + 11], C.T[j + 12], C.w00, C.w01, C.w10, C.w11);
            split_pair(v0, v1, k2048, h[e], l[e]);
        }
        if (C.live) {
            *reinterpret_cast<u32x4 *>(C.dst + g8 * 32) = u32x4{h[0], h[1], h[2], h[3]};
            *reinterpret_cast<u32x4 *>(C.dst + g8 * 32 + 16) = u32x4{l[0], l[1], l[2], l[3]};
        }
    }

    // One step of a producer: the gather of unit vg (-1: none) and the conversion of unit vc (-1: none).  vg's address table
    // first (VALU + LDS), then the wait for vc's patches (nothing of vg is in flight yet: only unit vc + 1's gather is
    // younger), vc's patch reads, and then vg's DMA groups with a chunk of vc's conversion behind each of the first three.
    // (A producer wave is one in-order instruction stream: measured, its step is the SUM of table, DMA issue and conversion
    // whatever the interleaving -- working the table out a step ahead, pass by pass between the DMAs, was 5 % slower.)
    __device__ __forceinline__ void work(int vg, int vc) {
        GatherCtx G{};
        ConvCtx C;
        if (vg >= 0) {
            table(vg);
            G = gather_begin(vg);
        }
#ifdef MFTX_TUNING
        if (p.ablate & 1) G.nd = 0;
        if (p.ablate & 4) vc = -1;
#endif
        if (vc >= 0) {
            conv_prepare(vc, C);
            wait_vmcnt_upto(younger(vc, 1));
            conv_load(C);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {            // (unrolled: tap_r / tap_c stay in registers)
            if (vg >= 0 && 4 * i < G.nd) dma_group(G, i);
            __builtin_amdgcn_sched_barrier(0);
            if (vc >= 0 && i < 3) conv_chunk(C, i);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (vg >= 0 && n_coord(vg)) coords_issue((vg >> 2) + 1);
    }

    // operations issued after unit v's gather at the moment unit v is converted: the coordinate prefetch behind it and the
    // gathers of the `ahead` units issued since, with theirs
    __device__ __forceinline__ int younger(int v, int ahead) const {
        int n = n_coord(v);
        for (int a = 1; a <= ahead; ++a) n += n_gather(v + a) + n_coord(v + a);
        return n;
    }

    // Per step u (the consumers multiply unit u) every producer converts its cells of unit u + 1 and issues the gather of
    // unit u + 3 (into the patch slot unit u left a step ago), interleaved (work()).
    __device__ __forceinline__ void run() {
        int tcount = 0; (void)tcount;
        LF_T(1);
        // my patch slots start out as zeros: the dummy samples of a cell (k'' = 10 b + 9, k'' >= 90: zero weights) read up to 8
        // taps past its 100 -- the next cell's, or the slot's pad, which no DMA reaches -- and must find finite values there
        for (int i = lane; i < LF_NP * LF_PSLOT / 16; i += 64) reinterpret_cast<f32x4 *>(patches)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int g = 64 * (4 * i + e) + lane;                    // this lane's tap in the unit's array
                const int cell = g / 100, t = g - 100 * cell, r = t / 10;
                lf_lds_u32 *tb3 = (lf_lds_u32 *)tab;
                tap_r[i][e] = tb3 + (cell < LF_CPP ? cell * 32 + r : 0);
                tap_c[i][e] = tb3 + (cell < LF_CPP ? cell * 32 + 16 + (t - 10 * r) : 0);
            }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int idx = min(64 * q + lane, 159);
            ent[q] = ((idx / 10) << 8) | (idx % 10);
        }
        coords_issue(0);
        wait_vmcnt_upto(0);
        LF_T(2);
        work(0, -1);
        LF_T(3);
        work(1 < U ? 1 : -1, -1);
        LF_T(3);
        work(2 < U ? 2 : -1, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        LF_T(5);
        for (int u = 0; u < U; ++u) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            LF_T(6);
            lds_barrier();                    // unit u is complete in its slot; the consumers are done with unit u - 1
            LF_T(7);
            work(u + 3 < U ? u + 3 : -1, u + 1 < U ? u + 1 : -1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the conversion's patch reads and A stores are complete)
            LF_T(5);
        }
    }
};

// convc1's packed fp32 weights [256][ld_w] (channel l * 81 + a * 9 + b of the lookup, core/corr.py:45-51) -> the fused
// kernel's fragment stream: for k group wg, consumer wave j, fragment x = 2 jt + (0: high, 1: low halves) and lane
// (col = lane & 31, kh = lane >> 5), the 8 halves of W[64 j + 32 jt + col][k'' = 16 (wg % 6) + 8 kh + e of level wg / 6]
// (The kernel whole, not only its index mapping: with the mapping as a callee of a shared body the wide variant's code comes out with two operands swapped.)
__global__ void pack_lookup_convc1_kernel(const float *__restrict__ w, int ld_w, uint4 *__restrict__ out) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;          // over 24 * 4 * 4 * 64 pieces of 16 bytes
    if (d >= LF_GROUPS * 4 * 4 * 64) return;
    const int lane = d & 63, x = (d >> 6) & 3, j = (d >> 8) & 3, wg = d >> 10;
    const int row = 64 * j + 32 * (x >> 1) + (lane & 31);
    const int lvl = wg / 6;
    _Float16 o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int kk = 16 * (wg - 6 * lvl) + 8 * (lane >> 5) + e;      // k'' = 10 b + a
        const int b = kk / 10, a = kk - 10 * b;
        float v = 0.f;
        if (kk < 90 && a < 9) v = w[(long long)row * ld_w + lvl * 81 + a * 9 + b];
        const _Float16 h = (_Float16)v;
        o[e] = (x & 1) ? (_Float16)((v - (float)h) * 2048.f) : h;
    }
    uint4 r;
    __builtin_memcpy(&r, o, 16);
    out[d] = r;
}

int launch_lookup_convc1(const float *const lvl[4], const float *coords, int P, int h, int w, const void *wf,
                         const float *bias, float *out, int ld_out, int out_split, hipStream_t s) {
    return lf_launch<LfProducer>(LookupConvArgs{}, lvl, coords, P, h, w, wf, bias, out, ld_out, out_split, s);
}

}  // namespace mftx

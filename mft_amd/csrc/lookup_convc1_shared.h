// What the two fused lookup + convc1 kernels have in common: lookup_convc1.hip (one dword per tap; the default) and
// lookup_convc1_wide.hip (16-byte pieces).  A library links exactly ONE of the two, and this header is the common part of that
// translation unit, host functions included.  Shared: the LDS layout, the trace buffer, the producers' common state, the
// CONSUMER waves (MFMA K loop + epilogue), the kernel itself, the weight packing's launcher and the launcher.  A variant adds
//   * BEFORE it includes this header (after common.h, profile.h and device_prims.h), its `struct LookupConvArgs`: the kernels'
//     arguments.  The two copies are the same but for `wide` in front of `ablate`; they stay copies because the layout of a
//     kernel's arguments is part of its code (the offsets it loads from), which one shared struct would move for one variant,
//   * its patch constants and `struct LfProducer : LfProducerBase` with
//         static constexpr int PATCH_BYTES                        LDS of one producer wave's patch ring
//         void run()                                              gather + conversion of its cells, unit by unit
//   * pack_lookup_convc1_kernel, declared below: convc1's weights in the K order of its conversion,
//   * launch_lookup_convc1 around lf_launch.
#pragma once

namespace mftx {

constexpr int LF_GROUPS = 24;                       // 16-wide k groups: 4 levels x 6
constexpr int LF_AROW = 400;                        // bytes per A row of a unit: 96 x 4 + 16 (rows r, r + 1 start 25 sixteen-byte slots apart: conflict-free ds_read_b128)
constexpr int LF_AUNIT = 64 * LF_AROW;              // 25 600
constexpr int LF_CPP = 16;                          // cells per producer wave and unit (at most)
constexpr unsigned LF_WBYTES = LF_GROUPS * 4 * 4 * 1024;     // fused weights: [group][wave][fragment][lane] x 16 bytes
constexpr unsigned LF_OOB = 0x80000000u;

// LDS: two A units | the four producer waves' patch rings (PATCH_BYTES each) | the consumers' epilogue stages | coordinate slots | address tables
template <int PATCH_BYTES>
struct LfLayout {
    static constexpr int OFF_PATCH = 2 * LF_AUNIT;                              // 51 200
    static constexpr int OFF_STAGE = OFF_PATCH + 4 * PATCH_BYTES;
    static constexpr int OFF_COORD = OFF_STAGE + 4 * 4096;                      // + 16 384
    static constexpr int OFF_TAB = OFF_COORD + 4 * 3 * 128;                     // + 1 536
    static constexpr int LDS = OFF_TAB + 4 * LF_CPP * 32 * 4;                   // + 8 192
    static_assert(LDS <= 160 * 1024, "lookup_convc1: the workgroup must fit the CU's LDS");
};

// Tuning builds only (-DMFTX_LF_TRACE): s_memtime stamps of workgroup 0's waves at the pipeline's events, read back with
// mftx_debug_lf_trace (tools/lf_trace.py): [wave][event] = (code << 56) | ticks
#ifdef MFTX_LF_TRACE
__device__ unsigned long long lf_trace_buf[8][128];
#define LF_T(code) do { if (blockIdx.x == 0 && tcount < 128) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
                        if ((threadIdx.x & 63) == 0) lf_trace_buf[threadIdx.x >> 6][tcount] = ((unsigned long long)(code) << 56) | (t_ & 0x00ffffffffffffffull); ++tcount; } } while (0)
#else
#define LF_T(code) do { } while (0)
#endif

__global__ void pack_lookup_convc1_kernel(const float *__restrict__ w, int ld_w, uint4 *__restrict__ out);

// the bilinear blend of four taps, spelled out: one multiply and three fused multiply-adds in THIS order.  Left to the compiler's
// contraction, the copies of the conversion that inlining makes (the prologue's and the loop's) may contract differently -- round 6
// saw exactly that after a code motion: 1-ulp differences between a cell converted as a workgroup's first tile and as its second,
// i.e. a pair's bits depending on its batch (tests/test_gpu_e2e.py::test_pair_bits_independent_of_batch_512, tools/lf_invariance.py).
__device__ __forceinline__ float lf_blend4(float t00, float t01, float t10, float t11, float w00, float w01, float w10, float w11) {
    return __builtin_fmaf(t11, w11, __builtin_fmaf(t10, w10, __builtin_fmaf(t01, w01, __fmul_rn(t00, w00))));
}

// ---------------------------------------------------------------------------------------------------------------
// producer waves (pw = 0..3): cells [pw rpw, (pw + 1) rpw) of every tile -- what both variants' producers hold and do
// ---------------------------------------------------------------------------------------------------------------
struct LfProducerBase {
    const LookupConvArgs &p;
    unsigned char *lds;
    int pw, lane, rpw, TR, my_tiles, U;
    int c16, q;                  // conversion: this lane's cell of the wave's 16 and its quarter of the cell's columns
    unsigned char *patches;      // the wave's patch ring
    float *cslots;               // coordinates of the wave's cells: three tiles' worth
    unsigned *tab;               // row / column offsets of the windows being gathered: [cell][32] (the variant's table() fills it)

    __device__ __forceinline__ int tile_of(int k) const { return (int)blockIdx.x + k * (int)gridDim.x; }

    // coordinates of tile k's cells of this wave -> slot k % 3 (32 dwords: 16 cells x (x, y))
    __device__ __forceinline__ void coords_issue(int k) {
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.coords), 0, (unsigned)p.cells * 8u, 0x00020000);
        const int cell0 = __builtin_amdgcn_readfirstlane(tile_of(k) * TR + pw * rpw);
        const int cell = cell0 + (lane >> 1);
        const bool ok = (lane >> 1) < rpw && cell < p.cells;
        if (lane < 32) buf_load_lds4(rc, cslots + (k % 3) * 32, ok ? (unsigned)cell * 8u + (unsigned)(lane & 1) * 4u : LF_OOB);
    }

    __device__ __forceinline__ void level_coords(int v, float &sx, float &sy) const {
        const int k = v >> 2, l = v & 3;
        const float2 c = reinterpret_cast<const float2 *>(cslots + (k % 3) * 32)[c16];
        const float inv = l == 0 ? 1.f : l == 1 ? 0.5f : l == 2 ? 0.25f : 0.125f;     // (x / 2^l, exactly)
        sx = c.x * inv;
        sy = c.y * inv;
    }

    __device__ __forceinline__ void level_geometry(int v, const float *&base, long long &stride, unsigned &H, unsigned &W, unsigned &wb) const {
        const int l = v & 3;
        base = l == 0 ? p.lvl[0] : l == 1 ? p.lvl[1] : l == 2 ? p.lvl[2] : p.lvl[3];
        stride = l == 0 ? p.stride[0] : l == 1 ? p.stride[1] : l == 2 ? p.stride[2] : p.stride[3];
        H = (unsigned)(l == 0 ? p.hl[0] : l == 1 ? p.hl[1] : l == 2 ? p.hl[2] : p.hl[3]);
        W = (unsigned)(l == 0 ? p.wl[0] : l == 1 ? p.wl[1] : l == 2 ? p.wl[2] : p.wl[3]);
        wb = (unsigned)(l == 0 ? p.wb0 : p.wb1);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// consumer waves (j = 0..3): output channels [64 j, 64 j + 64) of every tile; OFF_STAGE: where the variant's layout has the epilogue stages
// ---------------------------------------------------------------------------------------------------------------
template <bool OS, int OFF_STAGE>
__device__ __forceinline__ void lf_consumer(const LookupConvArgs &p, unsigned char *lds, int j, int lane, int U, int TR) {
    const int col = lane & 31, kh = lane >> 5;
    const unsigned char *a_lane = lds + col * LF_AROW + kh * 32;      // + slot, + 32 it rows, + 64 g, + 16 (low halves)
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.wf), 0, LF_WBYTES, 0x00020000);
    const unsigned w_lane = (unsigned)(j * 4096 + lane * 16);          // + 16384 group + 1024 fragment
    f16x8 wq[3][4];                    // weight fragments of three k groups: [jt = 0 hi, lo | jt = 1 hi, lo]
    auto wload = [&](int wg, f16x8 (&d)[4]) {
#ifdef MFTX_TUNING
        if (p.ablate & 8) return;
#endif
#pragma unroll
        for (int x = 0; x < 4; ++x)
            d[x] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rW, (unsigned)wg * 16384u + (unsigned)x * 1024u + w_lane, 0, 0));
    };
    wload(0, wq[0]); wload(1, wq[1]); wload(2, wq[2]);
    int wg_next = 3;
    // bias of this lane's four columns in the epilogue's row layout (columns 4 (lane & 7) .. + 3 of a 32-wide tile)
    f32x4 bias4[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) bias4[jt] = *reinterpret_cast<const f32x4 *>(p.bias + 64 * j + 32 * jt + 4 * (lane & 7));
    const __amdgpu_buffer_rsrc_t rOut = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (unsigned)((long long)p.cells * p.ld_out * 4), 0x00020000);
    float *st = reinterpret_cast<float *>(lds + OFF_STAGE + j * 4096);

    f32x16 acc[2][2], accx[2][2];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[it][jt][r] = 0.f; accx[it][jt][r] = 0.f; }

    int tcount = 0; (void)tcount;
    LF_T(1);
    for (int u = 0; u < U; ++u) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        LF_T(6);
        lds_barrier();
        LF_T(7);
        const unsigned char *A = a_lane + (u & 1) * LF_AUNIT;
        f16x8 ah[2][2], al[2][2];      // [register set][row tile]
        auto read_a = [&](int g, int set) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                ah[set][it] = *reinterpret_cast<const f16x8 *>(A + it * 32 * LF_AROW + g * 64);
                al[set][it] = *reinterpret_cast<const f16x8 *>(A + it * 32 * LF_AROW + g * 64 + 16);
            }
        };
        read_a(0, 0);
#pragma unroll
        for (int g = 0; g < 6; ++g) {
            const int set = g & 1;
            if (g < 5) read_a(g + 1, set ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            f16x8 (&w)[4] = wq[g % 3];
#ifdef MFTX_TUNING
            if (!(p.ablate & 2))
#endif
            {
            // product by product: consecutive MFMAs never wait for each other's accumulator
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) acc[it][jt] = mfma_f16(ah[set][it], w[2 * jt], acc[it][jt]);
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) accx[it][jt] = mfma_f16(ah[set][it], w[2 * jt + 1], accx[it][jt]);
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) accx[it][jt] = mfma_f16(al[set][it], w[2 * jt], accx[it][jt]);
            }
            __builtin_amdgcn_sched_barrier(0);
            wload(wg_next, wq[g % 3]);          // three k groups ahead of its use
            wg_next = wg_next == LF_GROUPS - 1 ? 0 : wg_next + 1;
            __builtin_amdgcn_sched_barrier(0);
        }
        LF_T(8);
        if ((u & 3) != 3) continue;
        // ---- the tile is complete: out = relu(acc + accx / 2048 + bias), through 4 KiB of the wave's own LDS so that a
        // lane holds 4 consecutive channels of a row (16-byte accesses; conv_gemm.hip's vectorised epilogue)
        const long long m_base = (long long)((int)blockIdx.x + (u >> 2) * (int)gridDim.x) * TR;
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                float *w = st + (4 * (lane >> 5)) * 32 + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    w[((r & 3) + 8 * (r >> 2)) * 32] = acc[it][jt][r] + accx[it][jt][r] * (1.f / 2048.f);
                    acc[it][jt][r] = 0.f;
                    accx[it][jt][r] = 0.f;
                }
                f32x4 v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = *reinterpret_cast<const f32x4 *>(st + (t * 8 + (lane >> 3)) * 32 + (lane & 7) * 4);
                const int nb = 64 * j + 32 * jt + 4 * (lane & 7);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int row = 32 * it + 8 * t + (lane >> 3);
                    const long long m = m_base + row;
#ifdef MFTX_TUNING
                    const bool ok = row < TR && m < p.cells && !(p.ablate & 16);
#else
                    const bool ok = row < TR && m < p.cells;
#endif
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = relu_keep_nan(v[t][e] + bias4[jt][e]);
                    if constexpr (OS) {
                        unsigned h0, h1, l0, l1;
                        const float k2048 = 2048.f;
                        split_pair(o[0], o[1], k2048, h0, l0);
                        split_pair(o[2], o[3], k2048, h1, l1);
                        const unsigned off = ok ? (unsigned)(m * p.ld_out * 4) + (unsigned)split_row_offset(nb) : LF_OOB;
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{h0, h1}, rOut, off, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{l0, l1}, rOut, off + 16u, 0, 0);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rOut, ok ? (unsigned)((m * p.ld_out + nb) * 4) : LF_OOB, 0, 0);
                    }
                }
            }
        LF_T(9);
    }
}

// The kernel: waves 0..3 consume, waves 4..7 produce.  Its text is here, its producer is the variant's: LfDefer makes the name
// depend on OS, so that it is looked up where the kernel is instantiated -- at the end of the variant's file.  (A shell per
// variant around a shared body was tried: behind the extra call the arguments end up in scratch memory.)
struct LfProducer;
template <bool> struct LfDefer { using Producer = LfProducer; };
template <bool OS>
__global__ __launch_bounds__(512, 2) void lookup_convc1_kernel(LookupConvArgs p) {
    using Producer = typename LfDefer<OS>::Producer;
    using L = LfLayout<Producer::PATCH_BYTES>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lf_lds[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#ifdef MFTX_TUNING
    if (p.ablate & 1024) {          // robustness check (tools/lf_stress.py): start from LDS full of NaNs -- nothing may depend on what it held
        for (int i = threadIdx.x; i < L::LDS / 4; i += blockDim.x) reinterpret_cast<unsigned *>(lf_lds)[i] = 0x7fc0beefu;
        __syncthreads();
    }
#endif
    const int TR = 4 * p.rpw;
    const int my_tiles = (p.n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;    // >= 1: the grid never exceeds n_tiles
    const int U = 4 * my_tiles;
    if (wid >= 4) {
        const int pw = wid - 4;
        Producer P{{p, lf_lds, pw, lane, p.rpw, TR, my_tiles, U,
                    lane & 15, lane >> 4,
                    lf_lds + L::OFF_PATCH + pw * Producer::PATCH_BYTES,
                    reinterpret_cast<float *>(lf_lds + L::OFF_COORD + pw * (3 * 128)),
                    reinterpret_cast<unsigned *>(lf_lds + L::OFF_TAB + pw * (LF_CPP * 32 * 4))}};
        P.run();
    } else {
        lf_consumer<OS, L::OFF_STAGE>(p, lf_lds, wid, lane, U, TR);
    }
}

#ifdef MFTX_LF_TRACE
extern "C" int mftx_debug_lf_trace(unsigned long long *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lf_trace_buf), sizeof(unsigned long long) * 8 * 128) != hipSuccess) return -1;
    unsigned long long z[8 * 128] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(lf_trace_buf), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

static int lf_num_cus() {
    static const int n = [] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        }
        return cus;
    }();
    return n;
}

int launch_pack_lookup_convc1(const float *w, int ld_w, void *out, hipStream_t s) {
    const int n = LF_GROUPS * 4 * 4 * 64;
    hipLaunchKernelGGL(pack_lookup_convc1_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, w, ld_w, reinterpret_cast<uint4 *>(out));
    return check_launch("pack_lookup_convc1");
}

bool lookup_convc1_applicable(int P, int h, int w, int ld_out) {
    const long long M = (long long)P * h * w;
    return M > 0 && M * ld_out * 4 < 0x7fffffffLL && M * 8 < 0x7fffffffLL;
}

// launch_lookup_convc1; a: zeros but for what the variant's arguments have of their own
template <class Producer>
int lf_launch(LookupConvArgs a, const float *const lvl[4], const float *coords, int P, int h, int w, const void *wf,
              const float *bias, float *out, int ld_out, int out_split, hipStream_t s) {
    constexpr int LDS = LfLayout<Producer::PATCH_BYTES>::LDS;
    const PyramidLayout L = pyramid_layout(h, w);
    for (int l = 0; l < 4; ++l) { a.lvl[l] = lvl[l]; a.stride[l] = L.stride[l]; a.hl[l] = L.h[l]; a.wl[l] = L.w[l]; }
    a.wb0 = L.wb[0]; a.wb1 = L.wb[1];
    a.coords = coords; a.cells = P * h * w;
    a.wf = wf; a.bias = bias; a.out = out; a.ld_out = ld_out; a.out_split = out_split;
    // tile = 4 rpw cells (rpw <= 16), sized so that the tiles come in whole rounds of the CUs: 7 x 4096 cells on 256
    // CUs are 512 tiles of 56, two per CU, instead of 448 of 64 (1.75)
    const int cus = lf_num_cus();
    const long long rounds = cdiv(cdiv(a.cells, 64), cus);
    const int tr0 = cdiv(a.cells, (int)(rounds * cus));
    a.rpw = cdiv(tr0, 4) < 1 ? 1 : cdiv(tr0, 4) > LF_CPP ? LF_CPP : cdiv(tr0, 4);
    a.n_tiles = cdiv(a.cells, 4 * a.rpw);
    static const int ablate = tune_env("MFTX_LF_ABLATE", 0);
    a.ablate = ablate;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(lookup_convc1_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(lookup_convc1_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        if (e != hipSuccess) return fail((int)e, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    // booked as the algorithmic BYTES the fused kernel really moves: the unique taps (10 x 10 per level), the coordinates and
    // convc1's 256 output channels -- not the 324-feature tensor it no longer writes; the flops of convc1 ride along
    ProfScope prof(PC_LOOKUP_FUSED, s, (double)a.cells * (4 * 100 * 4 + 8 + 256 * 4));
    const dim3 grid(a.n_tiles < cus ? a.n_tiles : cus);
    if (out_split) hipLaunchKernelGGL(lookup_convc1_kernel<true>, grid, dim3(512), LDS, s, a);
    else hipLaunchKernelGGL(lookup_convc1_kernel<false>, grid, dim3(512), LDS, s, a);
    return check_launch("lookup_convc1");
}

}  // namespace mftx

// Dense track store on the device: every frame's selected (template -> frame) result kept in the ".flowouX16" quantisation
// of codec.hip -- per-channel min/max, uint16, round-half-even -- as ONE 8-byte word per pixel (fx, fy, occl, sigma), and a
// point read-out of any N points over any T stored frames straight from the quantised data.
//
//   append : planes -> packed [H][W][4] uint16 + lohi [4][2] float32.  Two launches: per-block partial min/max of all four
//            channels in one pass; then every block re-reduces the partials (as quantize_kernel does) and quantises its pixels.
//            Per channel bitwise mftx_quantize_u16 of that plane alone: min and max do not depend on the order they are taken in.
//   unpack : packed + lohi -> planes, per channel bitwise mftx_dequantize_u16 (lo, hi read from device memory).
//   query  : chain.hip's sample_points_kernel, its taps dequantised with dequantize_kernel's dec() -- an out-of-frame tap is 0,
//            not dec(0) = lo.  Bitwise mftx_sample_points on the unpacked planes.
//
// Planes are read and written one float per lane (four pixels per thread in flight): their bases need 4-byte alignment only
// (flow y of a [2][H][W] tensor and the planes of a [4][H][W] buffer sit H * W floats apart, which is no multiple of 16
// bytes when H * W % 4 != 0).
// Compiled like chain.o: -ffp-contract=off (the float arithmetic is the reference's, operation by operation),
// -fno-slp-vectorize and no packed-fp32 instructions (EXEC-masked loads and stores next to the sampler's arithmetic).
#include "common.h"
#include "profile.h"
#include <cfloat>

namespace mftx {

constexpr int TS_T = 256;           // threads per block
constexpr int TS_B_MAX = 1024;      // blocks (= partial min/max octets) at most
constexpr int TS_PX = 4;            // pixels per thread and pass (and what sizes the grid)

struct Frame4 { const float *p[4]; };        // flow x, flow y, occlusion, sigma: [H * W] each
struct Frame4Out { float *p[4]; };

__device__ __forceinline__ void ts_block_minmax(float &lo, float &hi, float *sh /* [2 * TS_T / 64] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[2 * w] = lo; sh[2 * w + 1] = hi; }
    __syncthreads();
    lo = sh[0]; hi = sh[1];
#pragma unroll
    for (int i = 1; i < TS_T / 64; ++i) { lo = fminf(lo, sh[2 * i]); hi = fmaxf(hi, sh[2 * i + 1]); }
    __syncthreads();
}

// partial: [gridDim.x][4][2] = (min, max) of each channel over the block's pixels
__global__ __launch_bounds__(TS_T) void ts_minmax_kernel(Frame4 f, long long n, float *__restrict__ partial) {
    __shared__ float sh[2 * TS_T / 64];
    float lo[4], hi[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { lo[c] = FLT_MAX; hi[c] = -FLT_MAX; }
    // TS_PX pixels per pass, all their loads issued before the first use
    const long long stride = (long long)gridDim.x * TS_T;
    long long i = (long long)blockIdx.x * TS_T + threadIdx.x;
    for (; i + (TS_PX - 1) * stride < n; i += TS_PX * stride) {
        float v[TS_PX][4];
#pragma unroll
        for (int u = 0; u < TS_PX; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[u][c] = f.p[c][i + u * stride];
#pragma unroll
        for (int u = 0; u < TS_PX; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) { lo[c] = fminf(lo[c], v[u][c]); hi[c] = fmaxf(hi[c], v[u][c]); }
    }
    for (; i < n; i += stride) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = f.p[c][i];
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ts_block_minmax(lo[c], hi[c], sh);
        if (threadIdx.x == 0) {
            partial[8 * (long long)blockIdx.x + 2 * c] = lo[c];
            partial[8 * (long long)blockIdx.x + 2 * c + 1] = hi[c];
        }
    }
}

__global__ __launch_bounds__(TS_T) void ts_pack_kernel(Frame4 f, long long n, const float *__restrict__ partial, int n_partial,
                                                       ushort4 *__restrict__ packed, float *__restrict__ lohi) {
    __shared__ float sh[2 * TS_T / 64];
    float lo[4], range[4];
    bool flat[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float l = FLT_MAX, h = -FLT_MAX;
        for (int i = threadIdx.x; i < n_partial; i += TS_T) {
            l = fminf(l, partial[8 * i + 2 * c]);
            h = fmaxf(h, partial[8 * i + 2 * c + 1]);
        }
        ts_block_minmax(l, h, sh);
        if (blockIdx.x == 0 && threadIdx.x == 0) { lohi[2 * c] = l; lohi[2 * c + 1] = h; }
        lo[c] = l;
        range[c] = h - l;
        flat[c] = fabsf(range[c]) < 1e-8f;
    }
    // quantize_kernel's enc(), per channel
    auto enc = [&](int c, float v) -> unsigned short {
        if (flat[c]) return 0;
        const float u = (v - lo[c]) / range[c];
        return (unsigned short)rintf(u * 65535.f);
    };
    const long long stride = (long long)gridDim.x * TS_T;
    long long i = (long long)blockIdx.x * TS_T + threadIdx.x;
    for (; i + (TS_PX - 1) * stride < n; i += TS_PX * stride) {
        float v[TS_PX][4];
#pragma unroll
        for (int u = 0; u < TS_PX; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[u][c] = f.p[c][i + u * stride];
#pragma unroll
        for (int u = 0; u < TS_PX; ++u)
            packed[i + u * stride] = make_ushort4(enc(0, v[u][0]), enc(1, v[u][1]), enc(2, v[u][2]), enc(3, v[u][3]));
    }
    for (; i < n; i += stride)
        packed[i] = make_ushort4(enc(0, f.p[0][i]), enc(1, f.p[1][i]), enc(2, f.p[2][i]), enc(3, f.p[3][i]));
}

// dequantize_kernel's dec() for the four channels of one packed pixel
struct Dec4 {
    float lo[4], range[4];
    __device__ __forceinline__ explicit Dec4(const float *__restrict__ lohi) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { lo[c] = lohi[2 * c]; range[c] = lohi[2 * c + 1] - lohi[2 * c]; }
    }
    __device__ __forceinline__ float one(int c, unsigned v) const { return ((float)v / 65535.f) * range[c] + lo[c]; }
    __device__ __forceinline__ float4 operator()(uint2 q) const {
        return make_float4(one(0, q.x & 0xffffu), one(1, q.x >> 16), one(2, q.y & 0xffffu), one(3, q.y >> 16));
    }
};

__global__ __launch_bounds__(TS_T) void ts_unpack_kernel(const uint2 *__restrict__ packed, const float *__restrict__ lohi,
                                                         long long n, Frame4Out o) {
    const Dec4 dec(lohi);
    for (long long i = (long long)blockIdx.x * TS_T + threadIdx.x; i < n; i += (long long)gridDim.x * TS_T) {
        const float4 v = dec(packed[i]);
        o.p[0][i] = v.x; o.p[1][i] = v.y; o.p[2][i] = v.z; o.p[3][i] = v.w;
    }
}

// ---- point read-out ---------------------------------------------------------------------------------------------------------
// A workgroup owns a tile of TQ_P points x TQ_F requested frames.  Each of its four waves takes frames of the tile in turn with
// its lanes over the POINTS: neighbouring query points share cache lines of that frame, and a grid of queries reads
// near-contiguous 8-byte words.  The (x, y, occlusion, sigma) entries go to LDS and leave transposed: 16 consecutive lanes
// store the 16 consecutive frames of one point, a contiguous 256-byte run of a [N][frames][4] table, instead of 64 scattered
// 16-byte pieces per wave.
constexpr int TQ_P = 64, TQ_F = 16, TQ_FW = TQ_F / 4;      // (TQ_FW frames of the tile per wave)
constexpr int TQ_CHUNKS = 192;      // chunk descriptors per launch: 192 x 16 B = 3072 B of kernel arguments
struct ChunkSet { const uint2 *data[TQ_CHUNKS]; const float *lohi[TQ_CHUNKS]; };
static_assert(sizeof(ChunkSet) + 128 <= 4096, "kernel arguments of ts_query_kernel exceed 4 KB");

__global__ __launch_bounds__(256) void ts_query_kernel(ChunkSet cs, int c0, int nc, int fpc, const int *__restrict__ slots, int T,
                                                       int H, int W, float sx, float sy, int N, const float *__restrict__ xy,
                                                       float *__restrict__ table, long long row_stride, int column0) {
    __shared__ float4 tile[TQ_P][TQ_F + 1];       // (+ 1: the lanes of a wave, 17 x 16 bytes apart, spread over the banks)
    __shared__ int live[TQ_F];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform: the chunk descriptors are read with scalar loads
    const int i = blockIdx.x * TQ_P + lane;
    const int j0 = blockIdx.y * TQ_F;
    const bool have = i < N;
    // sample_points_kernel's sampler set-up, once per point
    const float px = have ? xy[2 * (long long)i] : 0.f, py = have ? xy[2 * (long long)i + 1] : 0.f;
    const float ix = ((px * sx - 1.f) + 1.f) / 2.f * (float)(W - 1);
    const float iy = ((py * sy - 1.f) + 1.f) / 2.f * (float)(H - 1);
    const float flx = floorf(ix), fly = floorf(iy);
    const float wx = ix - flx, wy = iy - fly;
    const int x0 = (int)fminf(fmaxf(flx, -1.0e6f), 1.0e6f);
    const int y0 = (int)fminf(fmaxf(fly, -1.0e6f), 1.0e6f);
    const float w00 = (1.f - wx) * (1.f - wy), w01 = wx * (1.f - wy), w10 = (1.f - wx) * wy, w11 = wx * wy;
    // The four taps' addresses are clamped into the frame and the loads are unconditional; a tap outside counts as 0 below.
    // So all TQ_FW frames' taps of this wave are in flight together instead of one bounds-tested gather after the other.
    const bool inx0 = x0 >= 0 && x0 < W, inx1 = x0 + 1 >= 0 && x0 + 1 < W, iny0 = y0 >= 0 && y0 < H, iny1 = y0 + 1 >= 0 && y0 + 1 < H;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x0 + 1, 0), W - 1), cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y0 + 1, 0), H - 1);
    const long long o00 = (long long)cy0 * W + cx0, o01 = (long long)cy0 * W + cx1, o10 = (long long)cy1 * W + cx0, o11 = (long long)cy1 * W + cx1;
    const long long frame_words = (long long)H * W;
    const uint2 *frame[TQ_FW];
    const float *lh[TQ_FW];
    bool ok[TQ_FW];
    const int jl = j0 + (lane & (TQ_F - 1));
    const int tile_slot = slots[jl < T ? jl : T - 1];          // the tile's TQ_F slots in one load, lane k holding frame k's
#pragma unroll
    for (int u = 0; u < TQ_FW; ++u) {
        const int k = wave + 4 * u, j = j0 + k;
        const int slot = __builtin_amdgcn_readlane(tile_slot, k);      // one frame per wave: scalar from here on
        const int c = slot >= 0 ? slot / fpc - c0 : -1;
        ok[u] = j < T && c >= 0 && c < nc;         // a slot of another launch's chunks, or of no chunk at all, is left alone
        const int cc = ok[u] ? c : 0, within = ok[u] ? slot % fpc : 0;      // (... and reads the launch's first frame, to no effect)
        frame[u] = cs.data[cc] + (long long)within * frame_words;
        lh[u] = cs.lohi[cc] + 8 * (long long)within;
        if (lane == 0) live[k] = ok[u];
    }
    uint2 q[TQ_FW][4];
#pragma unroll
    for (int u = 0; u < TQ_FW; ++u) { q[u][0] = frame[u][o00]; q[u][1] = frame[u][o01]; q[u][2] = frame[u][o10]; q[u][3] = frame[u][o11]; }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < TQ_FW; ++u) {
        const Dec4 dec(lh[u]);
        const float4 t00 = iny0 && inx0 ? dec(q[u][0]) : zero, t01 = iny0 && inx1 ? dec(q[u][1]) : zero;
        const float4 t10 = iny1 && inx0 ? dec(q[u][2]) : zero, t11 = iny1 && inx1 ? dec(q[u][3]) : zero;
        if (ok[u] && have)
            tile[lane][wave + 4 * u] = make_float4(px + (t00.x * w00 + t01.x * w01 + t10.x * w10 + t11.x * w11),
                                                   py + (t00.y * w00 + t01.y * w01 + t10.y * w10 + t11.y * w11),
                                                   t00.z * w00 + t01.z * w01 + t10.z * w10 + t11.z * w11,
                                                   t00.w * w00 + t01.w * w01 + t10.w * w10 + t11.w * w11);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TQ_P * TQ_F; e += 256) {
        const int p = e / TQ_F, k = e % TQ_F;
        const long long row = (long long)blockIdx.x * TQ_P + p;
        if (row < N && live[k])
            *reinterpret_cast<float4 *>(table + row * row_stride + 4 * ((long long)column0 + j0 + k)) = tile[p][k];
    }
}

static int ts_blocks(long long n) {
    const long long b = (n + (long long)TS_T * TS_PX - 1) / ((long long)TS_T * TS_PX);
    return (int)(b < 1 ? 1 : (b > TS_B_MAX ? TS_B_MAX : b));
}

static bool aligned_to(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

}  // namespace mftx

using namespace mftx;

extern "C" size_t mftx_trackstore_workspace_bytes(void) { return (size_t)TS_B_MAX * 8 * sizeof(float); }

extern "C" int mftx_trackstore_append(const float *flow, const float *occl, const float *sigma, int H, int W, uint16_t *packed,
                                      float *lohi, void *workspace, size_t workspace_bytes, void *stream) {
    if (!flow || !occl || !sigma || !packed || !lohi || !workspace) return fail(MFTX_E_ARG, "trackstore_append: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_append: H and W must be >= 2");
    if (!aligned_to(flow, 4) || !aligned_to(occl, 4) || !aligned_to(sigma, 4) || !aligned_to(lohi, 4) || !aligned_to(workspace, 4))
        return fail(MFTX_E_ALIGN, "trackstore_append: planes, lohi and workspace must be 4-byte aligned");
    if (!aligned_to(packed, 8)) return fail(MFTX_E_ALIGN, "trackstore_append: packed must be 8-byte aligned");
    if (workspace_bytes < mftx_trackstore_workspace_bytes()) return fail(MFTX_E_WORKSPACE, "trackstore_append: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)H * W;
    const int nb = ts_blocks(n);
    const Frame4 f{{flow, flow + n, occl, sigma}};
    float *partial = (float *)workspace;
    ProfScope prof(PC_GLUE, s, 40.0 * (double)n);         // 16 B/px read twice, 8 B/px written
    hipLaunchKernelGGL(ts_minmax_kernel, dim3(nb), dim3(TS_T), 0, s, f, n, partial);
    hipLaunchKernelGGL(ts_pack_kernel, dim3(nb), dim3(TS_T), 0, s, f, n, partial, nb, reinterpret_cast<ushort4 *>(packed), lohi);
    return check_launch("trackstore_append");
}

extern "C" int mftx_trackstore_unpack(const uint16_t *packed, const float *lohi, int H, int W, float *flow, float *occl,
                                      float *sigma, void *stream) {
    if (!packed || !lohi || !flow || !occl || !sigma) return fail(MFTX_E_ARG, "trackstore_unpack: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_unpack: H and W must be >= 2");
    if (!aligned_to(flow, 4) || !aligned_to(occl, 4) || !aligned_to(sigma, 4) || !aligned_to(lohi, 4))
        return fail(MFTX_E_ALIGN, "trackstore_unpack: planes and lohi must be 4-byte aligned");
    if (!aligned_to(packed, 8)) return fail(MFTX_E_ALIGN, "trackstore_unpack: packed must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)H * W;
    const Frame4Out o{{flow, flow + n, occl, sigma}};
    ProfScope prof(PC_GLUE, s, 24.0 * (double)n);
    hipLaunchKernelGGL(ts_unpack_kernel, dim3(ts_blocks(n)), dim3(TS_T), 0, s, reinterpret_cast<const uint2 *>(packed), lohi, n, o);
    return check_launch("trackstore_unpack");
}

extern "C" int mftx_trackstore_query(const uint16_t *const *chunks, const float *const *lohi_chunks, int n_chunks,
                                     int frames_per_chunk, const int *slots, int T, int H, int W, int N, const float *xy,
                                     float *table, long long row_stride, int column0, void *stream) {
    if (T < 0 || N < 0) return fail(MFTX_E_ARG, "trackstore_query: need T >= 0, N >= 0");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_query: H and W must be >= 2");
    if (T == 0 || N == 0) return 0;
    if (!chunks || !lohi_chunks || !slots || !xy || !table) return fail(MFTX_E_ARG, "trackstore_query: null pointer");
    if (n_chunks < 1 || frames_per_chunk < 1) return fail(MFTX_E_ARG, "trackstore_query: need n_chunks >= 1, frames_per_chunk >= 1");
    if (T > TQ_F * 65535) return fail(MFTX_E_ARG, "trackstore_query: at most %d frames per call", TQ_F * 65535);
    for (int c = 0; c < n_chunks; ++c) {
        if (!chunks[c] || !lohi_chunks[c]) return fail(MFTX_E_ARG, "trackstore_query: null chunk %d", c);
        if (!aligned_to(chunks[c], 8) || !aligned_to(lohi_chunks[c], 4))
            return fail(MFTX_E_ALIGN, "trackstore_query: chunk %d must be 8-byte, its lohi table 4-byte aligned", c);
    }
    if (column0 < 0 || row_stride % 4 || row_stride < 4 * ((long long)column0 + T))
        return fail(MFTX_E_ARG, "trackstore_query: row_stride must be a multiple of 4 floats that holds columns %d .. %lld", column0,
                    (long long)column0 + T - 1);
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "trackstore_query: the table must be 16-byte aligned");
    if (!aligned_to(slots, 4) || !aligned_to(xy, 4)) return fail(MFTX_E_ALIGN, "trackstore_query: slots and xy must be 4-byte aligned");
    // np.array([2/(W-1), 2/(H-1)]).astype(np.float32)  (double division, then rounded): chain.hip's scales()
    const float sx = (float)(2.0 / (double)(W - 1)), sy = (float)(2.0 / (double)(H - 1));
    // per (point, frame): 4 taps of 8 B, one table entry of 16 B
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, (32.0 + 16.0) * (double)N * (double)T);
    for (int c0 = 0; c0 < n_chunks; c0 += TQ_CHUNKS) {
        const int nc = n_chunks - c0 < TQ_CHUNKS ? n_chunks - c0 : TQ_CHUNKS;
        ChunkSet cs = {};
        for (int c = 0; c < nc; ++c) {
            cs.data[c] = reinterpret_cast<const uint2 *>(chunks[c0 + c]);
            cs.lohi[c] = lohi_chunks[c0 + c];
        }
        hipLaunchKernelGGL(ts_query_kernel, dim3(cdiv(N, TQ_P), cdiv(T, TQ_F)), dim3(256), 0, (hipStream_t)stream, cs, c0, nc,
                           frames_per_chunk, slots, T, H, W, sx, sy, N, xy, table, row_stride, column0);
        const int rc = check_launch("trackstore_query");
        if (rc) return rc;
    }
    return 0;
}

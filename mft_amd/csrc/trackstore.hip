// Dense track store on the device: every frame's selected (template -> frame) result kept in the ".flowouX16" quantisation
// of codec.hip -- per-channel min/max, uint16, round-half-even -- as ONE 8-byte word per pixel (fx, fy, occl, sigma), and a
// point read-out of any N points over any T stored frames straight from the quantised data.
//
//   append : planes -> packed [H][W][4] uint16 + lohi [4][2] float32.  Two launches: per-block partial min/max of all four
//            channels in one pass; then every block re-reduces the partials (as quantize_kernel does) and quantises its pixels.
//            Per channel bitwise mftx_quantize_u16 of that plane alone: min and max do not depend on the order they are taken in.
//   unpack : packed + lohi -> planes, per channel bitwise mftx_dequantize_u16 (lo, hi read from device memory).
//   query  : chain.hip's sample_points_kernel, its taps dequantised with QuantU16::dec -- an out-of-frame tap is 0,
//            not dec(0) = lo.  Bitwise mftx_sample_points on the unpacked planes.
//   locate : the inverse -- points given ON stored frames -> the template points they are the images of: a search over the
//            template's cells (bilinear patches solved by Newton steps, the winner a 64-bit integer atomic minimum) and a resolve
//            kernel.  Bitwise the numpy float32 restatement in mft_amd/trackstore.py.
//   invert : locate at every pixel centre of stored frames, as a scatter: each template cell writes its key onto the pixel
//            centres its box holds; the same resolve.  Bitwise locate with the pixel grid as its queries.
//   invert_atlas : invert of several stored frames onto ONE key plane, the entry's index in the key between sigma and cell.  invert
//            is these two kernels in their identity mode (one entry per plane, all 32 bits of the key's low word the cell).
//   flow_from : a plane of the atlas's inverse followed over T columns, each pixel on its winner's template -- query's sampler and
//            the chaining rule of DenseTrackStore.results_from in one launch, straight to planar flow, occlusion and sigma.
//   flow_from_best : the same with every entry that holds the source frame a candidate: per (pixel, column) the candidate whose
//            chained result has the smallest (occluded, sigma, rank) wins -- a 64-bit integer minimum in registers, one launch.
//   tracks_from_best : that choice for sparse points given on any number of source frames, behind locate's un-reduced rows: query's
//            tiles of 64 points x 16 columns, the candidates of a tile's source frame walked per wave, the winners out through LDS.
//   appearance : the video read along every track -- per template pixel and column unpack's dequantisation and warp_backward's sample of
//            the column's uint8 frame, masked by visibility and summed over the columns in order (sum, sum of squares, count; optionally
//            the per-column stack) in one launch.
//
// Shared with codec.hip: quant_u16.h (block_minmax, QuantU16's enc and dec).  Shared with chain.hip: grid_sample.h (the sampler's
// coordinate round trip, weights, order of summation, clamped taps; the host's grid_scales).
// Shared between the kernels here: TsSampler (query, flow_from, flow_from_best, tracks_from_best: grid_sample.h's sampler set up once
// per point, its taps' loads and their dequantised blend), ts_chain_behind (flow_from, flow_from_best, tracks_from_best: the chaining rule), ts_cell_tile (locate's search, the scatter: a tile's corners staged
// and the lane's InvCell), ts_solve_cell / ts_mix / ts_locate_key (search, scatter, both resolves), and on the host ts_cell_grids /
// ts_launch_inverse.
//
// Planes are read and written one float per lane (four pixels per thread in flight): their bases need 4-byte alignment only
// (flow y of a [2][H][W] tensor and the planes of a [4][H][W] buffer sit H * W floats apart, which is no multiple of 16
// bytes when H * W % 4 != 0).
// Compiled like chain.o: -ffp-contract=off (the float arithmetic rounds as the two headers write it),
// -fno-slp-vectorize and no packed-fp32 instructions (EXEC-masked loads and stores next to the sampler's arithmetic).
#include "common.h"
#include "grid_sample.h"
#include "profile.h"
#include "quant_u16.h"
#include <cfloat>

namespace mftx {

constexpr int TS_T = 256;           // threads per block
constexpr int TS_B_MAX = 1024;      // blocks (= partial min/max octets) at most
constexpr int TS_PX = 4;            // pixels per thread and pass (and what sizes the grid)

struct Frame4 { const float *p[4]; };        // flow x, flow y, occlusion, sigma: [H * W] each
struct Frame4Out { float *p[4]; };

// partial: [gridDim.x][4][2] = (min, max) of each channel over the block's pixels
__device__ __forceinline__ void ts_minmax_body(const Frame4 &f, long long n, float *__restrict__ partial, float *sh) {
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
        block_minmax<TS_T>(lo[c], hi[c], sh);
        if (threadIdx.x == 0) {
            partial[8 * (long long)blockIdx.x + 2 * c] = lo[c];
            partial[8 * (long long)blockIdx.x + 2 * c + 1] = hi[c];
        }
    }
}

__global__ __launch_bounds__(TS_T) void ts_minmax_kernel(Frame4 f, long long n, float *__restrict__ partial) {
    __shared__ float sh[2 * TS_T / 64];
    ts_minmax_body(f, n, partial, sh);
}

__device__ __forceinline__ void ts_pack_body(const Frame4 &f, long long n, const float *__restrict__ partial, int n_partial,
                                             ushort4 *__restrict__ packed, float *__restrict__ lohi, float *sh) {
    QuantU16 qu[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float l = FLT_MAX, h = -FLT_MAX;
        for (int i = threadIdx.x; i < n_partial; i += TS_T) {
            l = fminf(l, partial[8 * i + 2 * c]);
            h = fmaxf(h, partial[8 * i + 2 * c + 1]);
        }
        block_minmax<TS_T>(l, h, sh);
        if (blockIdx.x == 0 && threadIdx.x == 0) { lohi[2 * c] = l; lohi[2 * c + 1] = h; }
        qu[c] = QuantU16::of(l, h);
    }
    auto enc4 = [&](float x, float y, float z, float w) { return make_ushort4(qu[0].enc(x), qu[1].enc(y), qu[2].enc(z), qu[3].enc(w)); };
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
            packed[i + u * stride] = enc4(v[u][0], v[u][1], v[u][2], v[u][3]);
    }
    for (; i < n; i += stride)
        packed[i] = enc4(f.p[0][i], f.p[1][i], f.p[2][i], f.p[3][i]);
}

__global__ __launch_bounds__(TS_T) void ts_pack_kernel(Frame4 f, long long n, const float *__restrict__ partial, int n_partial,
                                                       ushort4 *__restrict__ packed, float *__restrict__ lohi) {
    __shared__ float sh[2 * TS_T / 64];
    ts_pack_body(f, n, partial, n_partial, packed, lohi, sh);
}

// append_multi: the two kernels above for up to TSM_F frames per launch, frame j = blockIdx.y.  The frames' descriptors travel in
// the kernel arguments (as chain.hip's MultiSet does); frame j's partials are rows j * gridDim.x .. of the workspace, and its
// blocks do exactly what the single-frame kernels' blocks do: the same bits.
constexpr int TSM_F = 64;           // frames per launch: 64 x 48 B = 3072 B of kernel arguments
struct MultiFrame { const float *p[4]; ushort4 *packed; float *lohi; };
struct MultiFrameSet { MultiFrame f[TSM_F]; };
static_assert(sizeof(MultiFrameSet) + 64 <= 4096, "kernel arguments of the append_multi kernels exceed 4 KB");

__global__ __launch_bounds__(TS_T) void ts_minmax_multi_kernel(MultiFrameSet fs, long long n, float *__restrict__ partial) {
    __shared__ float sh[2 * TS_T / 64];
    const MultiFrame &m = fs.f[blockIdx.y];
    const Frame4 f{{m.p[0], m.p[1], m.p[2], m.p[3]}};
    ts_minmax_body(f, n, partial + 8 * (long long)blockIdx.y * gridDim.x, sh);
}

__global__ __launch_bounds__(TS_T) void ts_pack_multi_kernel(MultiFrameSet fs, long long n, const float *__restrict__ partial) {
    __shared__ float sh[2 * TS_T / 64];
    const MultiFrame &m = fs.f[blockIdx.y];
    const Frame4 f{{m.p[0], m.p[1], m.p[2], m.p[3]}};
    ts_pack_body(f, n, partial + 8 * (long long)blockIdx.y * gridDim.x, (int)gridDim.x, m.packed, m.lohi, sh);
}

// the four channels of one packed pixel dequantised, (lo, hi) per channel from a lohi table
struct Dec4 {
    QuantU16 qu[4];
    __device__ __forceinline__ explicit Dec4(const float *__restrict__ lohi) {
#pragma unroll
        for (int c = 0; c < 4; ++c) qu[c] = QuantU16::of(lohi[2 * c], lohi[2 * c + 1]);
    }
    __device__ __forceinline__ float4 operator()(uint2 q) const {
        return make_float4(qu[0].dec(q.x & 0xffffu), qu[1].dec(q.x >> 16), qu[2].dec(q.y & 0xffffu), qu[3].dec(q.y >> 16));
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

// grid_sample.h's sampler at one point (px, py) of an H x W frame, set up once and used on any number of stored frames.  The
// four taps' addresses are clamped into the frame so that their loads are unconditional -- a caller issues the loads of several
// frames before the first mix(), and they are all in flight together instead of one bounds-tested gather after the other; a
// tap outside the frame counts as 0 in mix().
struct TsSampler {
    Bilinear w;
    ClampedTaps t;
    __device__ __forceinline__ TsSampler(float px, float py, float sx, float sy, int H, int W) {
        const GridSample s = grid_sample_at(px, py, sx, sy, H, W);
        w = s.w;
        t = clamped_taps(s, H, W);
    }
    __device__ __forceinline__ void load(const uint2 *__restrict__ frame, uint2 (&q)[4]) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = frame[t.o[k]];
    }
    // (flow x, flow y, occlusion, sigma) at the point: the taps dequantised, then blended
    __device__ __forceinline__ float4 mix(const Dec4 &dec, const uint2 (&q)[4]) const {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        return w.blend(t.in(0) ? dec(q[0]) : zero, t.in(1) ? dec(q[1]) : zero, t.in(2) ? dec(q[2]) : zero, t.in(3) ? dec(q[3]) : zero);
    }
};

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
    const float px = have ? xy[2 * (long long)i] : 0.f, py = have ? xy[2 * (long long)i + 1] : 0.f;
    const TsSampler smp(px, py, sx, sy, H, W);          // once per point
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
    for (int u = 0; u < TQ_FW; ++u) smp.load(frame[u], q[u]);       // all TQ_FW frames' taps of this wave in flight together
#pragma unroll
    for (int u = 0; u < TQ_FW; ++u) {
        const float4 m = smp.mix(Dec4(lh[u]), q[u]);
        if (ok[u] && have) tile[lane][wave + 4 * u] = make_float4(px + m.x, py + m.y, m.z, m.w);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TQ_P * TQ_F; e += 256) {
        const int p = e / TQ_F, k = e % TQ_F;
        const long long row = (long long)blockIdx.x * TQ_P + p;
        if (row < N && live[k])
            *reinterpret_cast<float4 *>(table + row * row_stride + 4 * ((long long)column0 + j0 + k)) = tile[p][k];
    }
}

// ---- locate: the stored map inverted at points given ON a stored frame ------------------------------------------------------------
// Template cell (i, j) .. (i + 1, j + 1) is mapped by the bilinear patch F(u, v) = A + u e + v g + u v h of its corner images
// A = M(i, j), B = M(i, j + 1), C = M(i + 1, j), D = M(i + 1, j + 1), M(i, j) = (j + fx, i + fy) dequantised.  A cell can hold
// the query Q only if Q is in the corners' bounding box widened by TL_EPS; there TL_NEWTON Newton steps on F - Q = 0 from the
// cell's centre, (u, v) clamped into [0, 1], and the cell is a candidate iff (u, v) were finite and |F - Q| <= TL_EPS in both
// coordinates at the clamped (u, v).  The winner is the smallest key (occluded, sigma, cell) as ONE 64-bit integer -- bit 63
// occlusion > threshold, bits 62..32 the bits of sigma (a sigma that is not > 0 counts as +0), bits 31..0 the cell -- so the
// minimum does not depend on the order it is taken in.  mft_amd/trackstore.py (_solve_cells, _locate_host) is the same
// arithmetic in numpy float32, operation by operation: + - * / only, no contraction (this file's flags).
constexpr float TL_EPS = 0.0009765625f;        // 2^-10 px
constexpr int TL_NEWTON = 6;
constexpr int TL_TW = 32, TL_TH = 8;           // cells per workgroup: one per lane, a wave owns two rows of 32
constexpr unsigned long long TL_NONE = ~0ull;

struct LocCell { float ax, ay, bx, by, cx, cy, dx, dy; };

__device__ __forceinline__ float ts_clamp01(float t) { return t < 0.f ? 0.f : (t > 1.f ? 1.f : t); }

// -> candidate?  (u, v) are the clamped solution either way.
__device__ __forceinline__ bool ts_solve_cell(const LocCell &c, float qx, float qy, float &u, float &v) {
    const float ex = c.bx - c.ax, ey = c.by - c.ay, gx = c.cx - c.ax, gy = c.cy - c.ay;
    const float hx = ((c.ax - c.bx) - c.cx) + c.dx, hy = ((c.ay - c.by) - c.cy) + c.dy;
    u = 0.5f; v = 0.5f;
#pragma unroll 1
    for (int it = 0; it < TL_NEWTON; ++it) {
        const float uv = u * v;
        const float rx = (((c.ax + u * ex) + v * gx) + uv * hx) - qx;
        const float ry = (((c.ay + u * ey) + v * gy) + uv * hy) - qy;
        const float j00 = ex + v * hx, j01 = gx + u * hx, j10 = ey + v * hy, j11 = gy + u * hy;
        const float det = j00 * j11 - j01 * j10;
        const float du = (rx * j11 - ry * j01) / det, dv = (ry * j00 - rx * j10) / det;
        u = u - du;
        v = v - dv;
    }
    const bool finite = fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX;
    u = ts_clamp01(u); v = ts_clamp01(v);          // (a NaN stays one; `finite` has refused it already)
    const float uv = u * v;
    const float rx = (((c.ax + u * ex) + v * gx) + uv * hx) - qx;
    const float ry = (((c.ay + u * ey) + v * gy) + uv * hy) - qy;
    return finite && fabsf(rx) <= TL_EPS && fabsf(ry) <= TL_EPS;
}

// the sampler's four weights and its order of summation at the patch's solution (u, v)
__device__ __forceinline__ float ts_mix(float a, float b, float c, float d, float u, float v) { return Bilinear::at(u, v).blend(a, b, c, d); }

__device__ __forceinline__ unsigned long long ts_locate_key(float occl, float sigma, float thr, unsigned cell) {
    const float s = sigma > 0.f ? sigma : 0.f;
    return ((unsigned long long)(occl > thr ? 1u : 0u) << 63) | ((unsigned long long)(__float_as_uint(s) & 0x7fffffffu) << 32) | cell;
}

struct InvCell {                    // what a lane (or, read from it, a whole wave) needs of one cell
    LocCell c;
    float oa, ob, oc, od, sa, sb, sc, sd;      // the corners' occlusion and sigma
    float lox, hix, loy, hiy;                  // the widened box: empty for a lane without a cell
    unsigned cell;                             // key_hi | i * (W - 1) + j
};

// The workgroup's tile of TL_TH x TL_TW cells from (i0, j0) on: its corners (M x, M y, occlusion, sigma) staged into `corner`, and
// the calling lane's cell built from them, lane li * TL_TW + lj owning cell (i0 + li, j0 + lj).
__device__ __forceinline__ InvCell ts_cell_tile(const uint2 *__restrict__ frame, const float *__restrict__ lohi, int i0, int j0, int H,
                                                int W, unsigned key_hi, float4 (*corner)[TL_TW + 1]) {
    const Dec4 dec(lohi);
    for (int e = threadIdx.x; e < (TL_TH + 1) * (TL_TW + 1); e += 256) {
        const int ci = e / (TL_TW + 1), cj = e % (TL_TW + 1);
        const int i = min(i0 + ci, H - 1), j = min(j0 + cj, W - 1);           // (a ragged tile's cells beyond the frame are never used)
        const float4 t = dec(frame[(long long)i * W + j]);
        corner[ci][cj] = make_float4((float)j + t.x, (float)i + t.y, t.z, t.w);
    }
    __syncthreads();
    const int li = threadIdx.x / TL_TW, lj = threadIdx.x % TL_TW;
    const float4 ta = corner[li][lj], tb = corner[li][lj + 1], tc = corner[li + 1][lj], td = corner[li + 1][lj + 1];
    InvCell t = {{ta.x, ta.y, tb.x, tb.y, tc.x, tc.y, td.x, td.y}, ta.z, tb.z, tc.z, td.z, ta.w, tb.w, tc.w, td.w,
                 FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX, key_hi | (unsigned)((i0 + li) * (W - 1) + (j0 + lj))};
    if (i0 + li < H - 1 && j0 + lj < W - 1) {
        t.lox = fminf(fminf(t.c.ax, t.c.bx), fminf(t.c.cx, t.c.dx)) - TL_EPS;
        t.hix = fmaxf(fmaxf(t.c.ax, t.c.bx), fmaxf(t.c.cx, t.c.dx)) + TL_EPS;
        t.loy = fminf(fminf(t.c.ay, t.c.by), fminf(t.c.cy, t.c.dy)) - TL_EPS;
        t.hiy = fmaxf(fmaxf(t.c.ay, t.c.by), fmaxf(t.c.cy, t.c.dy)) + TL_EPS;
    }
    return t;
}

// Grid: cell tiles x frame groups (blockIdx.x = group * tiles + tile).  A group is the run order[group_start[g] ..
// group_start[g + 1]) of queries given on one frame.  Each wave tests 64 queries at a time against the box of its 64 cells, a
// query per lane; only the queries that pass are walked one by one, each lane with its own cell.
__global__ __launch_bounds__(256) void ts_locate_search_kernel(const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis,
                                                               const int *__restrict__ group_start, const int *__restrict__ order,
                                                               int tiles_x, int tiles, int H, int W, const float *__restrict__ xy,
                                                               float thr, unsigned long long *__restrict__ keys) {
    __shared__ float4 corner[TL_TH + 1][TL_TW + 1];       // (M x, M y, occlusion, sigma) of the tile's corners
    const int g = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int i0 = (tile / tiles_x) * TL_TH, j0 = (tile % tiles_x) * TL_TW;
    const uint2 *__restrict__ frame = frames[g];          // (asked for before the queries: the tile's loads hang on it)
    const int lane = threadIdx.x & 63;
    // the wave's first 64 queries are fetched while the tile is staged (a group of few queries is one pass of the loop below)
    int k0 = group_start[g];
    const int k_end = group_start[g + 1];
    int p = k0 + lane < k_end ? order[k0 + lane] : -1;
    float px = 0.f, py = 0.f;
    if (p >= 0) { px = xy[2 * (long long)p]; py = xy[2 * (long long)p + 1]; }
    const InvCell t = ts_cell_tile(frame, lohis[g], i0, j0, H, W, 0u, corner);
    // the union of the boxes of the wave's cells: a query outside it is in no lane's box
    float wlox = t.lox, whix = t.hix, wloy = t.loy, whiy = t.hiy;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        wlox = fminf(wlox, __shfl_xor(wlox, off));
        whix = fmaxf(whix, __shfl_xor(whix, off));
        wloy = fminf(wloy, __shfl_xor(wloy, off));
        whiy = fmaxf(whiy, __shfl_xor(whiy, off));
    }
    for (;;) {
        unsigned long long hits = __ballot(p >= 0 && px >= wlox && px <= whix && py >= wloy && py <= whiy);
        while (hits) {
            const int b = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            const float qx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px), b));
            const float qy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py), b));
            const int q = __builtin_amdgcn_readlane(p, b);
            unsigned long long key = TL_NONE;
            if (qx >= t.lox && qx <= t.hix && qy >= t.loy && qy <= t.hiy) {
                float u, v;
                if (ts_solve_cell(t.c, qx, qy, u, v))
                    key = ts_locate_key(ts_mix(t.oa, t.ob, t.oc, t.od, u, v), ts_mix(t.sa, t.sb, t.sc, t.sd, u, v), thr, t.cell);
            }
            if (__any(key != TL_NONE)) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long other = __shfl_xor(key, off);
                    key = other < key ? other : key;
                }
                if (lane == 0) atomicMin(keys + q, key);
            }
        }
        k0 += 64;
        if (k0 >= k_end) break;
        p = k0 + lane < k_end ? order[k0 + lane] : -1;
        if (p >= 0) { px = xy[2 * (long long)p]; py = xy[2 * (long long)p + 1]; }
    }
}

// The answer to one query (qx, qy) on frame g from its key: the winning cell solved again with the same device function.
// -> the cell, -1 (and a row of NaN) where the key names none.
__device__ __forceinline__ int ts_resolve(const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis, int g, int H,
                                          int W, unsigned long long key, float qx, float qy, float4 &row) {
    const float nan = __uint_as_float(0x7fc00000u);
    row = make_float4(nan, nan, nan, nan);
    if (key == TL_NONE || (key & 0xffffffffull) >= (unsigned long long)(H - 1) * (W - 1)) return -1;     // (only cells of the frame are ever keyed)
    const int cell = (int)(unsigned)(key & 0xffffffffull);
    const int i = cell / (W - 1), j = cell % (W - 1);
    const uint2 *__restrict__ frame = frames[g];
    const Dec4 dec(lohis[g]);
    const long long o = (long long)i * W + j;
    const float4 ta = dec(frame[o]), tb = dec(frame[o + 1]), tc = dec(frame[o + W]), td = dec(frame[o + W + 1]);
    const LocCell c = {(float)j + ta.x, (float)i + ta.y, (float)(j + 1) + tb.x, (float)i + tb.y,
                       (float)j + tc.x, (float)(i + 1) + tc.y, (float)(j + 1) + td.x, (float)(i + 1) + td.y};
    float u, v;
    ts_solve_cell(c, qx, qy, u, v);
    row = make_float4((float)j + u, (float)i + v, ts_mix(ta.z, tb.z, tc.z, td.z, u, v), ts_mix(ta.w, tb.w, tc.w, td.w, u, v));
    return cell;
}

// One lane per query, in the caller's order.
__global__ __launch_bounds__(256) void ts_locate_resolve_kernel(const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis,
                                                                const int *__restrict__ group_of, int H, int W, int N,
                                                                const float *__restrict__ xy, const unsigned long long *__restrict__ keys,
                                                                float *__restrict__ table, int *__restrict__ cell_out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float4 row;
    const int cell = ts_resolve(frames, lohis, group_of[n], H, W, keys[n], xy[2 * (long long)n], xy[2 * (long long)n + 1], row);
    *reinterpret_cast<float4 *>(table + 4 * (long long)n) = row;
    cell_out[n] = cell;
}

// ---- invert: locate at EVERY pixel centre of a stored frame, the other way round ---------------------------------------------------
// The search kernel's work is tiles x queries; with the H * W pixel centres as the queries a cell would be tested against every
// pixel of the frame.  Here every template cell writes itself onto the few pixel centres its widened box can hold: the same box
// test, the same ts_solve_cell, the same key, the same atomic minimum per query -- so the candidate sets, and with them the bits, are
// those of locate on the pixel grid.  Work is the cells plus the area of their boxes, and each stored frame is read once.
constexpr int TI_INLINE = 16;       // a cell whose clipped range holds at most this many centres is walked by its own lane

// The pixel centres lo <= q <= hi can hold, as the integers a .. b clipped to 0 .. n - 1 (a superset: floor and ceil).  The bounds
// are limited in FLOAT before they are converted: an infinite or huge bound gives the frame's edge, a NaN bound an empty range
// (fmaxf / fminf return their other operand), never an undefined conversion.
__device__ __forceinline__ void ts_centre_range(float lo, float hi, int n, int &a, int &b) {
    a = (int)fminf(fmaxf(floorf(lo), 0.f), (float)n);
    b = (int)fminf(fmaxf(ceilf(hi), -1.f), (float)(n - 1));
    a = min(max(a, 0), n);          // ((float)n is n itself below 2^24; this keeps the range inside the frame beyond that too)
    b = min(max(b, -1), n - 1);
}

__device__ __forceinline__ float ts_lane_f(float v, int b) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b)); }

// the cell tested at pixel centre (x, y) of the frame whose keys start at `keys`: 0 <= x < W, 0 <= y < H is the caller's business
__device__ __forceinline__ void ts_invert_try(const InvCell &t, int x, int y, int W, float thr, unsigned long long *__restrict__ keys) {
    const float qx = (float)x, qy = (float)y;
    if (qx >= t.lox && qx <= t.hix && qy >= t.loy && qy <= t.hiy) {
        float u, v;
        if (ts_solve_cell(t.c, qx, qy, u, v))
            atomicMin(keys + ((long long)y * W + x),
                      ts_locate_key(ts_mix(t.oa, t.ob, t.oc, t.od, u, v), ts_mix(t.sa, t.sb, t.sc, t.sd, u, v), thr, t.cell));
    }
}

// ---- invert_atlas: several stored frames (the entries of a track atlas that hold one video frame) scattered onto ONE key plane ------
// Plane g is built from the stored frames j = first_of[g] .. first_of[g + 1] - 1, listed in ascending rank.  Entry k = j - first_of[g]
// goes into bits 31..24 of the key's low word, above the 24 bits of the cell: the minimum is locate's (occluded, sigma, cell) with
// the rank put between sigma and cell, i.e. per-entry invert followed by the minimum of (occluded, sigma, rank) over the entries.
// invert is the same two kernels in their identity mode, first_of == nullptr (uniform per launch): plane g is stored frame g
// alone, and the key's low word is locate's -- the cell in all 32 bits, so neither limit below binds it.
constexpr int TA_ENTRIES = 256;                 // entries per plane (8 bits of the key)
constexpr long long TA_CELLS = 1ll << 24;       // cells per frame (24 bits of the key)

// Grid: cell tiles x stored frames (blockIdx.x = j * tiles + tile), a cell per lane, the tile staged as the search kernel stages
// it.  The plane of frame j is the last g with first_of[g] <= j.  Phase 1: a lane whose range holds at most TI_INLINE centres
// walks it.  Phase 2: the wave takes the larger cells one at a time, its 64 lanes striding over the range, so that a torn cell's
// frame-sized box costs area / 64 solves per lane.
__global__ __launch_bounds__(256) void ts_atlas_scatter_kernel(const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis,
                                                               const int *__restrict__ first_of, int G, int tiles_x, int tiles, int H, int W,
                                                               float thr, unsigned long long *__restrict__ keys) {
    __shared__ float4 corner[TL_TH + 1][TL_TW + 1];
    const int j = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    int g = j, e = 0;
    if (first_of) {
        int hi = G - 1;
        g = 0;
        while (g < hi) {
            const int mid = (g + hi + 1) >> 1;
            if (first_of[mid] <= j) g = mid; else hi = mid - 1;
        }
        e = j - first_of[g];
        if (e < 0 || e >= TA_ENTRIES || j >= first_of[g + 1]) return;    // (block-uniform: a table that is not what it should be writes nothing)
    }
    keys += (long long)g * H * W;
    const int lane = threadIdx.x & 63;
    const InvCell t = ts_cell_tile(frames[j], lohis[j], (tile / tiles_x) * TL_TH, (tile % tiles_x) * TL_TW, H, W, (unsigned)e << 24, corner);
    int x0, x1, y0, y1;
    ts_centre_range(t.lox, t.hix, W, x0, x1);
    ts_centre_range(t.loy, t.hiy, H, y0, y1);
    const int bw = max(x1 - x0 + 1, 0), bh = max(y1 - y0 + 1, 0);          // bw <= W, bh <= H: the product is at most H * W < 2^31
    const int count = bw * bh;                                             // (0 for a lane without a cell: its box is empty)
    // phase 1
    const int n1 = count <= TI_INLINE ? count : 0;
    for (int k = 0; k < n1; ++k) ts_invert_try(t, x0 + k % bw, y0 + k / bw, W, thr, keys);
    // phase 2: `big` and everything read from lane b are wave-uniform
    unsigned long long big = __ballot(count > TI_INLINE);
    while (big) {
        const int b = __ffsll((long long)big) - 1;
        big &= big - 1;
        const InvCell s = {{ts_lane_f(t.c.ax, b), ts_lane_f(t.c.ay, b), ts_lane_f(t.c.bx, b), ts_lane_f(t.c.by, b),
                            ts_lane_f(t.c.cx, b), ts_lane_f(t.c.cy, b), ts_lane_f(t.c.dx, b), ts_lane_f(t.c.dy, b)},
                           ts_lane_f(t.oa, b), ts_lane_f(t.ob, b), ts_lane_f(t.oc, b), ts_lane_f(t.od, b),
                           ts_lane_f(t.sa, b), ts_lane_f(t.sb, b), ts_lane_f(t.sc, b), ts_lane_f(t.sd, b),
                           ts_lane_f(t.lox, b), ts_lane_f(t.hix, b), ts_lane_f(t.loy, b), ts_lane_f(t.hiy, b),
                           (unsigned)__builtin_amdgcn_readlane((int)t.cell, b)};
        const int sx0 = __builtin_amdgcn_readlane(x0, b), sy0 = __builtin_amdgcn_readlane(y0, b);
        const int sbw = __builtin_amdgcn_readlane(bw, b), scount = __builtin_amdgcn_readlane(count, b);
        for (int k = lane; k < scount; k += 64) ts_invert_try(s, sx0 + k % sbw, sy0 + k / sbw, W, thr, keys);
    }
}

// One lane per pixel of plane g (blockIdx.x = g * blocks + block): the query is the pixel's centre, and the winning entry's cell is
// solved again.  Identity mode has no entries: rank_of is not read, and entry_out may be null.
__global__ __launch_bounds__(256) void ts_atlas_resolve_kernel(const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis,
                                                               const int *__restrict__ first_of, const int *__restrict__ rank_of, int blocks,
                                                               int H, int W, const unsigned long long *__restrict__ keys,
                                                               float *__restrict__ table, int *__restrict__ cell_out, int *__restrict__ entry_out) {
    const int g = blockIdx.x / blocks;
    const int p = (blockIdx.x % blocks) * 256 + threadIdx.x;
    if (p >= H * W) return;
    const long long n = (long long)g * H * W + p;
    unsigned long long key = keys[n];
    const float nan = __uint_as_float(0x7fc00000u);
    float4 row = make_float4(nan, nan, nan, nan);
    int cell = -1, entry = -1;
    if (key != TL_NONE) {
        int j = g;
        if (first_of) {
            j = first_of[g] + (int)((key >> 24) & 0xffu);
            if (j >= first_of[g + 1]) j = -1;
            key = (key & ~0xffffffffull) | (key & 0xffffffull);
        }
        if (j >= 0) {
            cell = ts_resolve(frames, lohis, j, H, W, key, (float)(p % W), (float)(p / W), row);
            if (cell >= 0) entry = first_of ? rank_of[j] : 0;
        }
    }
    *reinterpret_cast<float4 *>(table + 4 * n) = row;
    cell_out[n] = cell;
    if (entry_out) entry_out[n] = entry;
}

// ---- flow_from: the dense results FROM a video frame to T frames, across the templates of a track atlas -----------------------------
// What invert_atlas leaves per pixel of the source frame -- the winner's template point (Px, Py), its occlusion and sigma there,
// and the winner's rank -- followed through the columns' stored frames of THAT winner's template: ts_query_kernel's read-out of
// (Px, Py) and the chaining rule of DenseTrackStore.results_from, straight to planar results.  A lane owns a pixel, lanes along
// x: neighbouring pixels mostly share a winner and map to neighbouring template points, so their taps share cache lines, and
// each of the four output planes of a column leaves as contiguous 256-byte runs per wave.  The lane reads its table row and
// entry, looks up its row and sets the sampler up ONCE, then walks its workgroup's columns TF_FW at a time, all their taps in
// flight.  The winner differs between lanes, so the columns' frame and lohi pointers are per-lane loads from the [R][T] tables.
// A lane that is not found and a column its template does not cover load nothing and write the fill (NaN, NaN, 1, +inf).
// Grid: pixel blocks x column blocks of `cols` columns -- ONE launch.
constexpr int TF_FW = 4;            // columns whose taps a lane keeps in flight
constexpr int TF_COLS = 16;         // columns per workgroup unless the caller says otherwise

// The chaining rule of DenseTrackStore.results_from: src = (Px, Py, occlusion, sigma) of the inverse at pixel (x, y), m the
// template's stored result sampled at (Px, Py) -> flow x, flow y, occlusion, sigma of the pixel.  Query's row, (Px + m.x,
// Py + m.y, m.z, m.w), chained behind the inverse.  The maximum keeps a NaN of either operand, as torch.maximum does (fmaxf drops
// it).  The root is taken in float64 and rounded once, as results_from takes it: the float32 sum is exact in float64, its
// float64 root is correctly rounded, and because 53 >= 2 * 24 + 2 rounding that once more gives the correctly rounded float32
// root -- whatever this unit's float32 sqrtf is compiled to.
__device__ __forceinline__ float4 ts_chain_behind(const float4 &src, const float4 &m, float x, float y) {
    const float qx = src.x + m.x, qy = src.y + m.y, od = m.z, sd = m.w;
    const float ss = src.w * src.w + sd * sd;
    return make_float4(qx - x, qy - y, src.z != src.z ? src.z : (od != od ? od : fmaxf(src.z, od)), (float)sqrt((double)ss));
}

__global__ __launch_bounds__(256) void ts_flow_from_kernel(const float4 *__restrict__ table, const int *__restrict__ entry,
                                                           const int *__restrict__ row_of, const uint2 *const *__restrict__ frames,
                                                           const float *const *__restrict__ lohis, int n_ranks, int R, int T, int cols,
                                                           int H, int W, float sx, float sy, float *__restrict__ flow,
                                                           float *__restrict__ occl, float *__restrict__ sigma) {
    const long long n = (long long)H * W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const long long first = (long long)blockIdx.y * cols;
    if (first >= T) return;
    const int t0 = (int)first, t1 = (int)(first + cols < T ? first + cols : T);
    const int e = entry[p];
    int row = -1;
    if (e >= 0 && e < n_ranks) row = row_of[e];
    const bool found = row >= 0 && row < R;             // (a table that is not what it should be reads nothing)
    float4 src = make_float4(0.f, 0.f, 0.f, 0.f);
    if (found) src = table[p];
    const float x = (float)(int)(p % W), y = (float)(int)(p / W);
    const TsSampler smp(src.x, src.y, sx, sy, H, W);     // ts_query_kernel's sampler at the template point, once per pixel
    const long long tb = (long long)(found ? row : 0) * T;
    const float nan = __uint_as_float(0x7fc00000u), inf = __uint_as_float(0x7f800000u);
    for (int t = t0; t < t1; t += TF_FW) {
        const uint2 *frame[TF_FW];
        const float *lh[TF_FW];
        bool ok[TF_FW];
#pragma unroll
        for (int u = 0; u < TF_FW; ++u) {
            frame[u] = nullptr; lh[u] = nullptr;
            if (found && t + u < t1) { frame[u] = frames[tb + t + u]; lh[u] = lohis[tb + t + u]; }
        }
        uint2 q[TF_FW][4];
        float l[TF_FW][8];
#pragma unroll
        for (int u = 0; u < TF_FW; ++u) {
            ok[u] = frame[u] != nullptr && lh[u] != nullptr;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[u][k] = make_uint2(0u, 0u);
#pragma unroll
            for (int k = 0; k < 8; ++k) l[u][k] = 0.f;
            if (ok[u]) {
                smp.load(frame[u], q[u]);
#pragma unroll
                for (int k = 0; k < 8; ++k) l[u][k] = lh[u][k];
            }
        }
#pragma unroll
        for (int u = 0; u < TF_FW; ++u) {
            if (t + u >= t1) continue;
            const float4 r = ts_chain_behind(src, smp.mix(Dec4(l[u]), q[u]), x, y);
            float fx = r.x, fy = r.y, oc = r.z, sg = r.w;
            if (!ok[u]) { fx = nan; fy = nan; oc = 1.f; sg = inf; }
            const long long c = t + u;
            flow[2 * c * n + p] = fx;
            flow[(2 * c + 1) * n + p] = fy;
            occl[c * n + p] = oc;
            sigma[c * n + p] = sg;
        }
    }
}

// ---- flow_from_best: the template chosen per (pixel, column) among ALL entries that hold the source frame -----------------------------
// ts_flow_from_kernel follows each pixel on the ONE entry that won the source frame's inverse.  Here every candidate k = 0 .. E - 1
// (the entries that hold the source frame, ascending rank) brings its OWN inverse plane -- tables[k], cells[k]: per-entry invert --
// and for every column the candidate whose CHAINED result is best wins:
//   key = (occluded << 39) | (sigma field << 8) | rank,  occluded = !(occlusion <= thr),
//   sigma field = 0x7fffffff for a NaN sigma, the bits of sigma where sigma > 0, 0 otherwise,
// the smallest key: visible before occluded, then the lowest chained sigma, then the lowest rank.  Not ts_locate_key in two respects:
// a NaN occlusion counts as occluded and a NaN sigma sorts behind every number, +inf included -- among alternatives a NaN never
// beats a number.  A candidate has a key for a pixel-column iff it found the pixel (cell >= 0) and its template covers the column.
// A lane owns a pixel, lanes along x, as in ts_flow_from_kernel; but the candidate list is the same for every pixel, so row_of[k],
// rank_of[k] and the frame and lohi pointers of (candidate, column) are wave-uniform (scalar loads) and only cells[k][p] and
// tables[k][p] are per lane.  Loop order: column groups of TF_FW outside, candidates inside.  The running best of a group -- key and
// four values per column -- stays in registers whatever the workgroup's column count is, the sampler is set up again per
// (candidate, group) from the candidate's row (16 bytes, out of the cache after the first group), and the TF_FW columns' taps of a
// candidate are all in flight.  The comparison is a 64-bit integer compare in registers: no atomics, no LDS, and each of the five
// output planes is written once per pixel-column, in contiguous 256-byte runs per wave.
// Grid: pixel blocks x column blocks of `cols` columns -- ONE launch.
constexpr int TFB_COLS = 16;        // columns per workgroup unless the caller says otherwise
constexpr int TFB_ENTRIES = 256;    // candidates (8 bits of the key)

__global__ __launch_bounds__(256) void ts_flow_best_kernel(const float4 *__restrict__ tables, const int *__restrict__ cells,
                                                           const int *__restrict__ rank_of, const int *__restrict__ row_of,
                                                           const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis,
                                                           int E, int R, int T, int cols, int H, int W, float sx, float sy, float thr,
                                                           float *__restrict__ flow, float *__restrict__ occl, float *__restrict__ sigma,
                                                           int *__restrict__ entry) {
    const long long n = (long long)H * W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const long long first = (long long)blockIdx.y * cols;
    if (first >= T) return;
    const int t0 = (int)first, t1 = (int)(first + cols < T ? first + cols : T);
    const float x = (float)(int)(p % W), y = (float)(int)(p / W);
    const float nan = __uint_as_float(0x7fc00000u), inf = __uint_as_float(0x7f800000u);
    for (int t = t0; t < t1; t += TF_FW) {
        unsigned long long best[TF_FW];
        float bx[TF_FW], by[TF_FW], bo[TF_FW], bs[TF_FW];
#pragma unroll
        for (int u = 0; u < TF_FW; ++u) { best[u] = TL_NONE; bx[u] = nan; by[u] = nan; bo[u] = 1.f; bs[u] = inf; }
        for (int k = 0; k < E; ++k) {
            // wave-uniform: the candidate's row, rank and its columns' frames
            const int row = row_of[k];
            if (row < 0 || row >= R) continue;            // (a table that is not what it should be reads nothing)
            const unsigned long long rank = (unsigned long long)(rank_of[k] & 0xff);
            const long long tb = (long long)row * T;
            const uint2 *frame[TF_FW];
            const float *lh[TF_FW];
            bool ok[TF_FW], any = false;
#pragma unroll
            for (int u = 0; u < TF_FW; ++u) {
                frame[u] = nullptr; lh[u] = nullptr;
                if (t + u < t1) { frame[u] = frames[tb + t + u]; lh[u] = lohis[tb + t + u]; }
                ok[u] = frame[u] != nullptr && lh[u] != nullptr;
                any = any || ok[u];
            }
            if (!any) continue;
            // per lane: did this candidate find the pixel, and where on its template
            if (cells[(long long)k * n + p] < 0) continue;
            const float4 src = tables[(long long)k * n + p];
            const TsSampler smp(src.x, src.y, sx, sy, H, W);     // ts_query_kernel's sampler at the candidate's template point
            uint2 q[TF_FW][4];
            float l[TF_FW][8];
#pragma unroll
            for (int u = 0; u < TF_FW; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[u][j] = make_uint2(0u, 0u);
#pragma unroll
                for (int j = 0; j < 8; ++j) l[u][j] = 0.f;
                if (ok[u]) {
                    smp.load(frame[u], q[u]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) l[u][j] = lh[u][j];
                }
            }
#pragma unroll
            for (int u = 0; u < TF_FW; ++u) {
                if (!ok[u]) continue;
                const float4 r = ts_chain_behind(src, smp.mix(Dec4(l[u]), q[u]), x, y);
                const float fx = r.x, fy = r.y, oc = r.z, sg = r.w;
                const unsigned field = sg != sg ? 0x7fffffffu : (sg > 0.f ? __float_as_uint(sg) : 0u);
                const unsigned long long key = ((unsigned long long)(oc <= thr ? 0u : 1u) << 39) | ((unsigned long long)field << 8) | rank;
                if (key < best[u]) { best[u] = key; bx[u] = fx; by[u] = fy; bo[u] = oc; bs[u] = sg; }
            }
        }
#pragma unroll
        for (int u = 0; u < TF_FW; ++u) {
            if (t + u >= t1) continue;
            const long long c = t + u;
            flow[2 * c * n + p] = bx[u];
            flow[(2 * c + 1) * n + p] = by[u];
            occl[c * n + p] = bo[u];
            sigma[c * n + p] = bs[u];
            entry[c * n + p] = best[u] == TL_NONE ? -1 : (int)(best[u] & 0xffull);
        }
    }
}

// ---- tracks_from_best: ts_flow_best_kernel's choice for sparse POINTS, given on any number of source frames --------------------------
// The sparse sibling of ts_flow_best_kernel in the shape of ts_query_kernel.  Step A (mftx_trackstore_locate, the points repeated per
// candidate) has left `located` [Q][4] and `cells` [Q]: source frame after source frame ("group") and, within a group of n points and E
// candidates, candidate after candidate -- row = first row of the group + k * n + i.  The host has sorted the points by source frame
// and cut every group into tiles of at most TP_P points, so a tile's candidate list is wave-uniform: rank_of, row_of and the frame and
// lohi pointers of (candidate, column) are scalar loads, and only the cell and the located row are per lane.
//   tiles  [n_tiles][2]: (group, first point of the tile within its group)
//   groups [G][5]      : (first row of step A, points, first sorted point, first candidate, one past the last candidate)
//   order  [N]         : sorted point -> the caller's row
// A workgroup owns a tile x `cols` columns, walked in chunks of TP_F: each of its four waves takes every fourth column of the chunk
// with its lanes over the POINTS and, per candidate in order, sets TsSampler up at the candidate's template point, has its TP_FW
// columns' taps in flight, chains (the pixel is (0, 0): q - 0 is exact), keys and keeps the running minimum and its four values in
// registers.  The winners go to a padded LDS tile and leave transposed after ONE barrier per chunk (two tiles in turn: a wave that is
// a chunk ahead writes the other one): 16 consecutive lanes write the 16 consecutive columns of one point, 256-byte runs of
// table [N][T][4] and 64-byte runs of entry [N][T], at the caller's row.  Every lane reaches every barrier: a lane without a point, a
// candidate that did not find the point and a column beyond T are predicated.  An index that is not inside its table reads nothing.
constexpr int TP_P = 64, TP_F = 16, TP_FW = TP_F / 4;
constexpr int TP_COLS = 16;         // columns per workgroup unless the caller says otherwise
constexpr int TP_ENTRIES = 256;     // candidates per group (8 bits of the key)

__global__ __launch_bounds__(256) void ts_tracks_best_kernel(const float4 *__restrict__ located, const int *__restrict__ cells,
                                                             const int *__restrict__ tiles, const int *__restrict__ groups,
                                                             const int *__restrict__ rank_of, const int *__restrict__ row_of,
                                                             const int *__restrict__ order, const uint2 *const *__restrict__ frames,
                                                             const float *const *__restrict__ lohis, int G, int C, int Q, int N, int R,
                                                             int T, int cols, int H, int W, float sx, float sy, float thr,
                                                             float4 *__restrict__ table, int *__restrict__ entry) {
    __shared__ float4 tile[2][TP_P][TP_F + 1];      // (+ 1: the lanes of a wave, 17 x 16 bytes apart, spread over the banks)
    __shared__ int etile[2][TP_P][TP_F + 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long first_col = (long long)blockIdx.y * cols;
    const int t0 = (int)(first_col < T ? first_col : T), t1 = (int)(first_col + cols < T ? first_col + cols : T);
    // the tile and its group: block-uniform
    const int g = tiles[2 * (long long)blockIdx.x], first = tiles[2 * (long long)blockIdx.x + 1];
    int row0 = 0, n = 0, point0 = 0, c0 = 0, c1 = 0;
    if (g >= 0 && g < G) {
        const int *gr = groups + 5 * (long long)g;
        row0 = gr[0]; n = gr[1]; point0 = gr[2]; c0 = gr[3]; c1 = gr[4];
    }
    bool valid = n > 0 && first >= 0 && first < n && point0 >= 0 && (long long)point0 + n <= N;
    if (!(c0 >= 0 && c0 <= c1 && c1 <= C && c1 - c0 <= TP_ENTRIES && row0 >= 0 && (long long)row0 + (long long)(c1 - c0) * n <= Q)) c1 = c0 = 0;
    if (!valid) { c0 = c1 = 0; n = 0; }
    const int i = first + lane;
    const bool have = valid && i < n;
    const int in_tile = valid ? (n - first < TP_P ? n - first : TP_P) : 0;
    const float nan = __uint_as_float(0x7fc00000u), inf = __uint_as_float(0x7f800000u);
    int buf = 0;
    for (int tc = t0; tc < t1; tc += TP_F, buf ^= 1) {
        unsigned long long best[TP_FW];
        float bx[TP_FW], by[TP_FW], bo[TP_FW], bs[TP_FW];
#pragma unroll
        for (int u = 0; u < TP_FW; ++u) { best[u] = TL_NONE; bx[u] = nan; by[u] = nan; bo[u] = 1.f; bs[u] = inf; }
        for (int k = c0; k < c1; ++k) {
            // wave-uniform: the candidate's row, rank and its columns' frames
            const int row = row_of[k];
            if (row < 0 || row >= R) continue;            // (a table that is not what it should be reads nothing)
            const unsigned long long rank = (unsigned long long)(rank_of[k] & 0xff);
            const long long tb = (long long)row * T;
            const uint2 *frame[TP_FW];
            const float *lh[TP_FW];
            bool ok[TP_FW], any = false;
#pragma unroll
            for (int u = 0; u < TP_FW; ++u) {
                const int t = tc + wave + 4 * u;
                frame[u] = nullptr; lh[u] = nullptr;
                if (t < t1) { frame[u] = frames[tb + t]; lh[u] = lohis[tb + t]; }
                ok[u] = frame[u] != nullptr && lh[u] != nullptr;
                any = any || ok[u];
            }
            if (!any) continue;
            // per lane: did this candidate find the point, and where on its template
            const long long at = (long long)row0 + (long long)(k - c0) * n + i;
            int cell = -1;
            if (have) cell = cells[at];
            const bool found = cell >= 0;
            float4 src = make_float4(0.f, 0.f, 0.f, 0.f);
            if (found) src = located[at];
            const TsSampler smp(src.x, src.y, sx, sy, H, W);     // ts_query_kernel's sampler at the candidate's template point
            uint2 q[TP_FW][4];
            float l[TP_FW][8];
#pragma unroll
            for (int u = 0; u < TP_FW; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[u][j] = make_uint2(0u, 0u);
#pragma unroll
                for (int j = 0; j < 8; ++j) l[u][j] = 0.f;
                if (ok[u]) {
                    if (found) smp.load(frame[u], q[u]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) l[u][j] = lh[u][j];
                }
            }
#pragma unroll
            for (int u = 0; u < TP_FW; ++u) {
                const float4 r = ts_chain_behind(src, smp.mix(Dec4(l[u]), q[u]), 0.f, 0.f);
                const float sg = r.w;
                const unsigned field = sg != sg ? 0x7fffffffu : (sg > 0.f ? __float_as_uint(sg) : 0u);
                const unsigned long long key = ((unsigned long long)(r.z <= thr ? 0u : 1u) << 39) | ((unsigned long long)field << 8) | rank;
                if (ok[u] && found && key < best[u]) { best[u] = key; bx[u] = r.x; by[u] = r.y; bo[u] = r.z; bs[u] = sg; }
            }
        }
#pragma unroll
        for (int u = 0; u < TP_FW; ++u) {
            tile[buf][lane][wave + 4 * u] = make_float4(bx[u], by[u], bo[u], bs[u]);
            etile[buf][lane][wave + 4 * u] = best[u] == TL_NONE ? -1 : (int)(best[u] & 0xffull);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < TP_P * TP_F; e += 256) {
            const int p = e / TP_F, k = e % TP_F;
            const int t = tc + k;
            if (p < in_tile && t < t1) {
                const int dst = order[(long long)point0 + first + p];
                if (dst >= 0 && dst < N) {
                    table[(long long)dst * T + t] = tile[buf][p][k];
                    entry[(long long)dst * T + t] = etile[buf][p][k];
                }
            }
        }
    }
}

// ---- appearance: the video sampled along every track, reduced over the columns ---------------------------------------------------------
// Per template pixel (x, y) and column k (a stored frame and the video frame that belongs to it, [H][W][C] uint8):
//   (fx, fy, o, s) = the stored frame's word at the pixel, dequantised (ts_unpack_kernel's bits);  px = (float)x + fx, py = (float)y + fy;
//   c[ch] = warp_backward_kernel's sample of the image at (px, py): grid_sample_at, the taps (float)u8, 0 outside, Bilinear::blend;
//   visible = o <= thr && s <= sigma_max && 0 <= px <= W - 1 && 0 <= py <= H - 1     (every comparison false on NaN);
//   d = c - (float)reference;  where visible: sum += d, sumsq += d * d, count += 1 -- over k in order, float32, no contraction.
// A lane owns a template pixel, lanes along x: the packed words of a wave are one contiguous run of 512 bytes per column, and the taps
// of neighbouring pixels share cache lines.  The lane walks ALL columns TAP_NF at a time: their packed words are loaded together, then
// their samplers are set up and their 4 x C tap bytes are all in flight (clamped addresses: the loads are unconditional), then the
// columns are reduced in order into 2 C + 1 registers -- no atomics, no LDS, and the reduction is never split over columns.  The
// frame, lohi and image pointers and the lohi values of a column are the same for every lane (scalar loads).  STACK: per column also
// warped = (uint8)rint(clamp(c, 0, 255)) where visible, `fill` elsewhere, and visible -- each where its pointer is not null; without it
// nothing is written per column.
// A group's columns beyond T read column T - 1 once more and are dropped.
// Grid: pixel blocks of 256 -- ONE launch whatever T is.
constexpr int TAP_NF = 4;           // columns in flight: 2, 4 and 8 were measured and time the same; the siblings' 4
// What the pointer tables name is device memory that nothing writes while the kernel runs: said to the compiler, a pointer read from a
// table is no generic (flat) address -- the words and the bytes are global loads, the lohi table a scalar load of constant memory.
typedef const __attribute__((address_space(1))) unsigned long long *TapWords;       // (a packed pixel: x = the low half)
typedef const __attribute__((address_space(1))) uint8_t *TapBytes;
typedef const __attribute__((address_space(4))) float *TapLohi;

template <int C, bool STACK>
__global__ __launch_bounds__(256) void ts_appearance_kernel(const uint2 *const *__restrict__ frames, const float *const *__restrict__ lohis,
                                                            const uint8_t *const *__restrict__ images, int T, int H, int W, float sx,
                                                            float sy, const uint8_t *__restrict__ reference, float thr, float smax,
                                                            int fill, float *__restrict__ sum, float *__restrict__ sumsq,
                                                            int *__restrict__ count, uint8_t *__restrict__ warped,
                                                            uint8_t *__restrict__ visible) {
    const long long n = (long long)H * W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float x = (float)(int)(p % W), y = (float)(int)(p / W);
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    constexpr int NF = TAP_NF;
    float ref[C], s[C], ss[C];
    int cnt = 0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        ref[ch] = reference ? (float)reference[p * C + ch] : 0.f;
        s[ch] = 0.f; ss[ch] = 0.f;
    }
    for (int t = 0; t < T; t += NF) {
        uint2 q[NF];
        float l[NF][8];
        TapBytes img[NF];
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int tt = t + u < T ? t + u : T - 1;          // wave-uniform: the three pointers are scalar loads, and so is the lohi table
            const unsigned long long word = ((TapWords)frames[tt])[p];
            q[u] = make_uint2((unsigned)word, (unsigned)(word >> 32));
            const TapLohi lh = (TapLohi)lohis[tt];
#pragma unroll
            for (int k = 0; k < 8; ++k) l[u][k] = lh[k];
            img[u] = (TapBytes)images[tt];
        }
        Bilinear w[NF];
        bool in[NF][4], vis[NF];
        uint8_t b[NF][4][C];
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const float4 v = Dec4(l[u])(q[u]);
            const float px = x + v.x, py = y + v.y;
            vis[u] = v.z <= thr && v.w <= smax && px >= 0.f && px <= xmax && py >= 0.f && py <= ymax;
            const GridSample g = grid_sample_at(px, py, sx, sy, H, W);
            const ClampedTaps tp = clamped_taps(g, H, W);
            w[u] = g.w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                in[u][k] = tp.in(k);
#pragma unroll
                for (int ch = 0; ch < C; ++ch) b[u][k][ch] = img[u][tp.o[k] * C + ch];
            }
        }
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            if (t + u >= T) continue;
            float c[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                c[ch] = w[u].blend(in[u][0] ? (float)b[u][0][ch] : 0.f, in[u][1] ? (float)b[u][1][ch] : 0.f,
                                   in[u][2] ? (float)b[u][2][ch] : 0.f, in[u][3] ? (float)b[u][3][ch] : 0.f);
                const float d = c[ch] - ref[ch];
                if (vis[u]) { s[ch] = s[ch] + d; ss[ch] = ss[ch] + d * d; }
            }
            if (vis[u]) ++cnt;
            if (STACK) {
                const long long at = (long long)(t + u) * n + p;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    int level = fill;
                    if (vis[u]) level = (int)rintf(fminf(fmaxf(c[ch], 0.f), 255.f));          // (c is finite wherever the pixel is visible)
                    if (warped) warped[at * C + ch] = (uint8_t)level;
                }
                if (visible) visible[at] = vis[u] ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) { sum[ch * n + p] = s[ch]; sumsq[ch * n + p] = ss[ch]; }
    count[p] = cnt;
}

template <int C>
static void ts_appearance_launch(bool stack, dim3 grid, hipStream_t s, const uint2 *const *frames, const float *const *lohis,
                                 const uint8_t *const *images, int T, int H, int W, float sx, float sy, const uint8_t *reference, float thr,
                                 float smax, int fill, float *sum, float *sumsq, int *count, uint8_t *warped, uint8_t *visible) {
    if (stack)
        hipLaunchKernelGGL((ts_appearance_kernel<C, true>), grid, dim3(256), 0, s, frames, lohis, images, T, H, W, sx, sy, reference, thr,
                           smax, fill, sum, sumsq, count, warped, visible);
    else
        hipLaunchKernelGGL((ts_appearance_kernel<C, false>), grid, dim3(256), 0, s, frames, lohis, images, T, H, W, sx, sy, reference, thr,
                           smax, fill, sum, sumsq, count, warped, visible);
}

template <typename... A>
static void ts_appearance_channels(int C, A... a) {
    switch (C) {
        case 1: ts_appearance_launch<1>(a...); break;
        case 2: ts_appearance_launch<2>(a...); break;
        case 3: ts_appearance_launch<3>(a...); break;
        default: ts_appearance_launch<4>(a...); break;
    }
}

static int ts_blocks(long long n) {
    const long long b = (n + (long long)TS_T * TS_PX - 1) / ((long long)TS_T * TS_PX);
    return (int)(b < 1 ? 1 : (b > TS_B_MAX ? TS_B_MAX : b));
}

static bool aligned_to(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// The grids of locate, invert and invert_atlas over an H x W frame: its cell tiles, one workgroup each per tile frame, and its
// blocks of 256 pixels, one workgroup each per block plane.  `fits`: both products are grids of one launch.
struct CellGrids { int tiles_x; long long tiles, blocks; bool fits; };
static CellGrids ts_cell_grids(int H, int W, long long tile_frames, long long block_planes) {
    CellGrids g;
    g.tiles_x = cdiv(W - 1, TL_TW);
    g.tiles = (long long)g.tiles_x * cdiv(H - 1, TL_TH);
    g.blocks = ((long long)H * W + 255) / 256;
    g.fits = g.tiles * tile_frames <= 0x7fffffffLL && g.blocks * block_planes <= 0x7fffffffLL;
    return g;
}

// The launches of invert_atlas, and of invert as its identity mode (first_of and rank_of null, J == G, entry null or not): the G
// key planes reset, the J stored frames scattered onto them, every pixel of every plane resolved.
static int ts_launch_inverse(const char *who, const uint16_t *const *frames, const float *const *lohis, const int *first_of,
                             const int *rank_of, int G, int J, const CellGrids &cg, int H, int W, float thr, unsigned long long *keys,
                             float *table, int *cell, int *entry, hipStream_t s) {
    const uint2 *const *words = reinterpret_cast<const uint2 *const *>(frames);
    hipError_t e = hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)G * H * W, s);
    if (e != hipSuccess) return fail((int)e, "%s: %s", who, hipGetErrorString(e));
    if (J > 0) {
        hipLaunchKernelGGL(ts_atlas_scatter_kernel, dim3((unsigned)(cg.tiles * J)), dim3(256), 0, s, words, lohis, first_of, G, cg.tiles_x,
                           (int)cg.tiles, H, W, thr, keys);
        const int rc = check_launch(who);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ts_atlas_resolve_kernel, dim3((unsigned)(cg.blocks * G)), dim3(256), 0, s, words, lohis, first_of, rank_of,
                       (int)cg.blocks, H, W, keys, table, cell, entry);
    return check_launch(who);
}

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

extern "C" size_t mftx_trackstore_append_multi_workspace_bytes(int T) {
    return T > 0 ? (size_t)T * mftx_trackstore_workspace_bytes() : 0;
}

extern "C" int mftx_trackstore_append_multi(int T, const float *const *flow, const float *const *occl, const float *const *sigma,
                                            int H, int W, uint16_t *const *packed, float *const *lohi, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    if (T < 0) return fail(MFTX_E_ARG, "trackstore_append_multi: need T >= 0");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_append_multi: H and W must be >= 2");
    if (T == 0) return 0;
    if (!flow || !occl || !sigma || !packed || !lohi || !workspace) return fail(MFTX_E_ARG, "trackstore_append_multi: null pointer");
    for (int j = 0; j < T; ++j) {
        if (!flow[j] || !occl[j] || !sigma[j] || !packed[j] || !lohi[j]) return fail(MFTX_E_ARG, "trackstore_append_multi: null pointer of frame %d", j);
        if (!aligned_to(flow[j], 4) || !aligned_to(occl[j], 4) || !aligned_to(sigma[j], 4) || !aligned_to(lohi[j], 4))
            return fail(MFTX_E_ALIGN, "trackstore_append_multi: planes and lohi of frame %d must be 4-byte aligned", j);
        if (!aligned_to(packed[j], 8)) return fail(MFTX_E_ALIGN, "trackstore_append_multi: packed of frame %d must be 8-byte aligned", j);
    }
    if (!aligned_to(workspace, 4)) return fail(MFTX_E_ALIGN, "trackstore_append_multi: workspace must be 4-byte aligned");
    if (workspace_bytes < mftx_trackstore_append_multi_workspace_bytes(T))
        return fail(MFTX_E_WORKSPACE, "trackstore_append_multi: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)H * W;
    const int nb = ts_blocks(n);
    ProfScope prof(PC_GLUE, s, 40.0 * (double)n * T);
    for (int j0 = 0; j0 < T; j0 += TSM_F) {
        const int nf = T - j0 < TSM_F ? T - j0 : TSM_F;
        MultiFrameSet fs = {};
        for (int j = 0; j < nf; ++j)
            fs.f[j] = MultiFrame{{flow[j0 + j], flow[j0 + j] + n, occl[j0 + j], sigma[j0 + j]},
                                 reinterpret_cast<ushort4 *>(packed[j0 + j]), lohi[j0 + j]};
        float *partial = (float *)workspace + 8 * (long long)j0 * TS_B_MAX;         // (frame j0 + j: rows j * nb .. of this launch's part)
        hipLaunchKernelGGL(ts_minmax_multi_kernel, dim3(nb, nf), dim3(TS_T), 0, s, fs, n, partial);
        hipLaunchKernelGGL(ts_pack_multi_kernel, dim3(nb, nf), dim3(TS_T), 0, s, fs, n, partial);
        const int rc = check_launch("trackstore_append_multi");
        if (rc) return rc;
    }
    return 0;
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
    float sx, sy;
    grid_scales(H, W, sx, sy);
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

extern "C" int mftx_trackstore_locate(const uint16_t *const *frames, const float *const *lohis, const int *group_start, int G,
                                      const int *order, const int *group_of, int H, int W, int N, const float *xy,
                                      float occlusion_threshold, unsigned long long *keys, float *table, int *cell, void *stream) {
    if (N < 0 || G < 0) return fail(MFTX_E_ARG, "trackstore_locate: need N >= 0, G >= 0");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_locate: H and W must be >= 2");
    if (N == 0) return 0;
    if (!frames || !lohis || !group_start || !order || !group_of || !xy || !keys || !table || !cell)
        return fail(MFTX_E_ARG, "trackstore_locate: null pointer");
    if (G < 1 || G > N) return fail(MFTX_E_ARG, "trackstore_locate: need 1 <= G <= N frame groups");
    if ((long long)(H - 1) * (W - 1) > 0x7fffffffLL) return fail(MFTX_E_ARG, "trackstore_locate: more than 2^31 - 1 cells");
    const CellGrids cg = ts_cell_grids(H, W, G, 0);
    if (!cg.fits) return fail(MFTX_E_ARG, "trackstore_locate: %lld cell tiles x %d frame groups exceed one grid", cg.tiles, G);
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8) || !aligned_to(keys, 8))
        return fail(MFTX_E_ALIGN, "trackstore_locate: the pointer tables and the keys must be 8-byte aligned");
    if (!aligned_to(group_start, 4) || !aligned_to(order, 4) || !aligned_to(group_of, 4) || !aligned_to(xy, 4) || !aligned_to(cell, 4))
        return fail(MFTX_E_ALIGN, "trackstore_locate: group_start, order, group_of, xy and cell must be 4-byte aligned");
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "trackstore_locate: the table must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // per tile and group: 33 x 9 packed corners; per query: its coordinates in every wave, a key, a row, a cell index
    ProfScope prof(PC_CHAIN, s, 8.0 * (TL_TW + 1) * (TL_TH + 1) * (double)cg.tiles * G + (8.0 + 8.0 + 16.0 + 4.0) * (double)N);
    hipError_t e = hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)N, s);
    if (e != hipSuccess) return fail((int)e, "trackstore_locate: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(ts_locate_search_kernel, dim3((unsigned)(cg.tiles * G)), dim3(256), 0, s, reinterpret_cast<const uint2 *const *>(frames),
                       lohis, group_start, order, cg.tiles_x, (int)cg.tiles, H, W, xy, occlusion_threshold, keys);
    int rc = check_launch("trackstore_locate");
    if (rc) return rc;
    hipLaunchKernelGGL(ts_locate_resolve_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, reinterpret_cast<const uint2 *const *>(frames), lohis,
                       group_of, H, W, N, xy, keys, table, cell);
    return check_launch("trackstore_locate");
}

extern "C" int mftx_trackstore_invert(const uint16_t *const *frames, const float *const *lohis, int G, int H, int W,
                                      float occlusion_threshold, unsigned long long *keys, float *table, int *cell, void *stream) {
    if (G < 0) return fail(MFTX_E_ARG, "trackstore_invert: need G >= 0");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_invert: H and W must be >= 2");
    if (G == 0) return 0;
    if (!frames || !lohis || !keys || !table || !cell) return fail(MFTX_E_ARG, "trackstore_invert: null pointer");
    if ((long long)H * W > 0x7fffffffLL) return fail(MFTX_E_ARG, "trackstore_invert: more than 2^31 - 1 pixels (and cells)");
    const CellGrids cg = ts_cell_grids(H, W, G, G);
    if (!cg.fits)
        return fail(MFTX_E_ARG, "trackstore_invert: %lld cell tiles (%lld pixel blocks) x %d frames exceed one grid", cg.tiles, cg.blocks, G);
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8) || !aligned_to(keys, 8))
        return fail(MFTX_E_ALIGN, "trackstore_invert: the pointer tables and the keys must be 8-byte aligned");
    if (!aligned_to(cell, 4)) return fail(MFTX_E_ALIGN, "trackstore_invert: cell must be 4-byte aligned");
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "trackstore_invert: the table must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // per tile and frame: 33 x 9 packed corners; per pixel: its key set, (at least once) lowered and read, a row, a cell index, and
    // the winning cell's four corners once more
    ProfScope prof(PC_CHAIN, s, 8.0 * (TL_TW + 1) * (TL_TH + 1) * (double)cg.tiles * G +
                                    (8.0 + 8.0 + 8.0 + 16.0 + 4.0 + 32.0) * (double)G * H * W);
    return ts_launch_inverse("trackstore_invert", frames, lohis, nullptr, nullptr, G, G, cg, H, W, occlusion_threshold, keys, table, cell,
                             nullptr, s);
}

extern "C" int mftx_trackstore_invert_atlas(const uint16_t *const *frames, const float *const *lohis, const int *first_of,
                                            const int *rank_of, int G, int J, int H, int W, float occlusion_threshold,
                                            unsigned long long *keys, float *table, int *cell, int *entry, void *stream) {
    if (G < 0 || J < 0) return fail(MFTX_E_ARG, "trackstore_invert_atlas: need G >= 0, J >= 0");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_invert_atlas: H and W must be >= 2");
    if ((long long)(H - 1) * (W - 1) > TA_CELLS) return fail(MFTX_E_ARG, "trackstore_invert_atlas: more than 2^24 cells");
    if ((long long)J > (long long)TA_ENTRIES * G)
        return fail(MFTX_E_ARG, "trackstore_invert_atlas: %d stored frames in %d planes: more than %d entries in a plane", J, G, TA_ENTRIES);
    if (G == 0) return 0;
    if (!first_of || !keys || !table || !cell || !entry || (J > 0 && (!frames || !lohis || !rank_of)))
        return fail(MFTX_E_ARG, "trackstore_invert_atlas: null pointer");
    const CellGrids cg = ts_cell_grids(H, W, J, G);
    if (!cg.fits)
        return fail(MFTX_E_ARG, "trackstore_invert_atlas: %lld cell tiles x %d frames (%lld pixel blocks x %d planes) exceed one grid", cg.tiles,
                    J, cg.blocks, G);
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8) || !aligned_to(keys, 8))
        return fail(MFTX_E_ALIGN, "trackstore_invert_atlas: the pointer tables and the keys must be 8-byte aligned");
    if (!aligned_to(first_of, 4) || !aligned_to(rank_of, 4) || !aligned_to(cell, 4) || !aligned_to(entry, 4))
        return fail(MFTX_E_ALIGN, "trackstore_invert_atlas: first_of, rank_of, cell and entry must be 4-byte aligned");
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "trackstore_invert_atlas: the table must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // per tile and stored frame: 33 x 9 packed corners; per pixel of a plane: its key set and read, a row, a cell, an entry, the
    // winning cell's four corners once more; per pixel of a stored frame: (at least) one key lowered
    ProfScope prof(PC_CHAIN, s, 8.0 * (TL_TW + 1) * (TL_TH + 1) * (double)cg.tiles * J +
                                    (8.0 + 8.0 + 16.0 + 4.0 + 4.0 + 32.0) * (double)G * H * W + 8.0 * (double)J * H * W);
    return ts_launch_inverse("trackstore_invert_atlas", frames, lohis, first_of, rank_of, G, J, cg, H, W, occlusion_threshold, keys, table,
                             cell, entry, s);
}

extern "C" int mftx_trackstore_flow_from(const float *table, const int *entry, const int *row_of, const uint16_t *const *frames,
                                         const float *const *lohis, int n_ranks, int R, int T, int H, int W, int columns_per_block,
                                         float *flow, float *occl, float *sigma, void *stream) {
    if (T < 0) return fail(MFTX_E_ARG, "trackstore_flow_from: need T >= 0");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_flow_from: H and W must be >= 2");
    if (columns_per_block < 0) return fail(MFTX_E_ARG, "trackstore_flow_from: columns_per_block must be >= 0 (0: the default)");
    if (T == 0) return 0;
    if (n_ranks < 1 || R < 1) return fail(MFTX_E_ARG, "trackstore_flow_from: need n_ranks >= 1, R >= 1");
    const struct { const void *p; const char *name; } ptrs[] = {{table, "table"}, {entry, "entry"}, {row_of, "row_of"}, {frames, "frames"},
                                                                {lohis, "lohis"}, {flow, "flow"}, {occl, "occl"}, {sigma, "sigma"}};
    for (const auto &a : ptrs)
        if (!a.p) return fail(MFTX_E_ARG, "trackstore_flow_from: null pointer: %s", a.name);
    if ((long long)H * W > 0x7fffffffLL) return fail(MFTX_E_ARG, "trackstore_flow_from: more than 2^31 - 1 pixels");
    const int cols = columns_per_block ? columns_per_block : TF_COLS;
    const long long blocks = ((long long)H * W + 255) / 256, col_blocks = ((long long)T + cols - 1) / cols;
    if (col_blocks > 65535)
        return fail(MFTX_E_ARG, "trackstore_flow_from: T = %d in blocks of %d columns: more than 65535 column blocks", T, cols);
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "trackstore_flow_from: table must be 16-byte aligned");
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8))
        return fail(MFTX_E_ALIGN, "trackstore_flow_from: the pointer tables frames and lohis must be 8-byte aligned");
    for (const auto &a : ptrs)
        if (!aligned_to(a.p, 4)) return fail(MFTX_E_ALIGN, "trackstore_flow_from: %s must be 4-byte aligned", a.name);
    float sx, sy;
    grid_scales(H, W, sx, sy);
    hipStream_t s = (hipStream_t)stream;
    // per pixel and column block: a table row and an entry; per pixel and column: two pointers, a lohi table (shared between the
    // lanes of one winner), 4 taps of 8 B, 16 B of results
    ProfScope prof(PC_CHAIN, s, 20.0 * (double)H * W * (double)col_blocks + (32.0 + 16.0) * (double)H * W * (double)T);
    hipLaunchKernelGGL(ts_flow_from_kernel, dim3((unsigned)blocks, (unsigned)col_blocks), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(table), entry, row_of, reinterpret_cast<const uint2 *const *>(frames), lohis, n_ranks,
                       R, T, cols, H, W, sx, sy, flow, occl, sigma);
    return check_launch("trackstore_flow_from");
}

extern "C" int mftx_trackstore_flow_from_best(const float *tables, const int *cells, const int *rank_of, const int *row_of,
                                              const uint16_t *const *frames, const float *const *lohis, int E, int R, int T, int H, int W,
                                              float occlusion_threshold, int columns_per_block, float *flow, float *occl, float *sigma,
                                              int *entry, void *stream) {
    if (T < 0 || E < 0) return fail(MFTX_E_ARG, "trackstore_flow_from_best: need T >= 0, E >= 0");
    if (E > TFB_ENTRIES) return fail(MFTX_E_ARG, "trackstore_flow_from_best: %d candidates: more than %d", E, TFB_ENTRIES);
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_flow_from_best: H and W must be >= 2");
    if (columns_per_block < 0) return fail(MFTX_E_ARG, "trackstore_flow_from_best: columns_per_block must be >= 0 (0: the default)");
    if ((long long)H * W > 0x7fffffffLL) return fail(MFTX_E_ARG, "trackstore_flow_from_best: more than 2^31 - 1 pixels");
    if (T == 0) return 0;
    if (E > 0 && R < 1) return fail(MFTX_E_ARG, "trackstore_flow_from_best: need R >= 1");
    const struct { const void *p; const char *name; bool always; } ptrs[] = {
        {tables, "tables", false}, {cells, "cells", false}, {rank_of, "rank_of", false}, {row_of, "row_of", false}, {frames, "frames", false},
        {lohis, "lohis", false}, {flow, "flow", true}, {occl, "occl", true}, {sigma, "sigma", true}, {entry, "entry", true}};
    for (const auto &a : ptrs)           // (without candidates nothing but the results is touched)
        if (!a.p && (a.always || E > 0)) return fail(MFTX_E_ARG, "trackstore_flow_from_best: null pointer: %s", a.name);
    const int cols = columns_per_block ? columns_per_block : TFB_COLS;
    const long long blocks = ((long long)H * W + 255) / 256, col_blocks = ((long long)T + cols - 1) / cols;
    if (col_blocks > 65535)
        return fail(MFTX_E_ARG, "trackstore_flow_from_best: T = %d in blocks of %d columns: more than 65535 column blocks", T, cols);
    if (!aligned16(tables)) return fail(MFTX_E_ALIGN, "trackstore_flow_from_best: tables must be 16-byte aligned");
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8))
        return fail(MFTX_E_ALIGN, "trackstore_flow_from_best: the pointer tables frames and lohis must be 8-byte aligned");
    for (const auto &a : ptrs)
        if (!aligned_to(a.p, 4)) return fail(MFTX_E_ALIGN, "trackstore_flow_from_best: %s must be 4-byte aligned", a.name);
    float sx, sy;
    grid_scales(H, W, sx, sy);
    hipStream_t s = (hipStream_t)stream;
    // per pixel, candidate and group of TF_FW columns: a row and a cell; per pixel, column and candidate (at most): 4 taps of 8 B; per
    // pixel and column: 20 B of results
    ProfScope prof(PC_CHAIN, s, 20.0 * (double)H * W * (double)E * (double)((T + TF_FW - 1) / TF_FW) +
                                    32.0 * (double)H * W * (double)T * (double)E + 20.0 * (double)H * W * (double)T);
    hipLaunchKernelGGL(ts_flow_best_kernel, dim3((unsigned)blocks, (unsigned)col_blocks), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(tables), cells, rank_of, row_of, reinterpret_cast<const uint2 *const *>(frames), lohis, E,
                       R, T, cols, H, W, sx, sy, occlusion_threshold, flow, occl, sigma, entry);
    return check_launch("trackstore_flow_from_best");
}

extern "C" int mftx_trackstore_tracks_from_best(const float *located, const int *cells, const int *tiles, const int *groups,
                                                const int *rank_of, const int *row_of, const int *order,
                                                const uint16_t *const *frames, const float *const *lohis, int n_tiles, int G, int C,
                                                int max_candidates, int Q, int N, int R, int T, int H, int W, float occlusion_threshold,
                                                int columns_per_block, float *table, int *entry, void *stream) {
    if (N < 0 || T < 0 || n_tiles < 0 || G < 0 || C < 0 || Q < 0 || max_candidates < 0)
        return fail(MFTX_E_ARG, "trackstore_tracks_from_best: need N, T, n_tiles, G, C, Q, max_candidates >= 0");
    if (max_candidates > TP_ENTRIES)
        return fail(MFTX_E_ARG, "trackstore_tracks_from_best: %d candidates in a group: more than %d", max_candidates, TP_ENTRIES);
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_tracks_from_best: H and W must be >= 2");
    if (columns_per_block < 0) return fail(MFTX_E_ARG, "trackstore_tracks_from_best: columns_per_block must be >= 0 (0: the default)");
    if ((long long)H * W > 0x7fffffffLL) return fail(MFTX_E_ARG, "trackstore_tracks_from_best: more than 2^31 - 1 pixels");
    if (N == 0 || T == 0) return 0;
    if (n_tiles < 1 || G < 1 || G > n_tiles || n_tiles > N)
        return fail(MFTX_E_ARG, "trackstore_tracks_from_best: need 1 <= G <= n_tiles <= N groups and tiles of the N points");
    if (max_candidates > C || (C > 0 && (R < 1 || Q < 1)))
        return fail(MFTX_E_ARG, "trackstore_tracks_from_best: with candidates need R >= 1, Q >= 1 and max_candidates <= C");
    const struct { const void *p; const char *name; bool always; } ptrs[] = {
        {located, "located", false}, {cells, "cells", false}, {rank_of, "rank_of", false}, {row_of, "row_of", false}, {frames, "frames", false},
        {lohis, "lohis", false}, {tiles, "tiles", true}, {groups, "groups", true}, {order, "order", true}, {table, "table", true},
        {entry, "entry", true}};
    for (const auto &a : ptrs)           // (without candidates nothing but the tiles and the results is touched)
        if (!a.p && (a.always || C > 0)) return fail(MFTX_E_ARG, "trackstore_tracks_from_best: null pointer: %s", a.name);
    const int cols = columns_per_block ? columns_per_block : TP_COLS;
    const long long col_blocks = ((long long)T + cols - 1) / cols;
    if (col_blocks > 65535)
        return fail(MFTX_E_ARG, "trackstore_tracks_from_best: T = %d in blocks of %d columns: more than 65535 column blocks", T, cols);
    if (!aligned16(located)) return fail(MFTX_E_ALIGN, "trackstore_tracks_from_best: located must be 16-byte aligned");
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "trackstore_tracks_from_best: table must be 16-byte aligned");
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8))
        return fail(MFTX_E_ALIGN, "trackstore_tracks_from_best: the pointer tables frames and lohis must be 8-byte aligned");
    for (const auto &a : ptrs)
        if (!aligned_to(a.p, 4)) return fail(MFTX_E_ALIGN, "trackstore_tracks_from_best: %s must be 4-byte aligned", a.name);
    float sx, sy;
    grid_scales(H, W, sx, sy);
    hipStream_t s = (hipStream_t)stream;
    // per point, candidate and chunk of TP_F columns: a row and a cell in each wave; per point, column and candidate (at most): 4 taps
    // of 8 B; per point and column: 20 B of results
    ProfScope prof(PC_CHAIN, s, 20.0 * 4.0 * (double)Q * (double)((T + TP_F - 1) / TP_F) + 32.0 * (double)Q * (double)T + 20.0 * (double)N * (double)T);
    hipLaunchKernelGGL(ts_tracks_best_kernel, dim3((unsigned)n_tiles, (unsigned)col_blocks), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(located), cells, tiles, groups, rank_of, row_of, order,
                       reinterpret_cast<const uint2 *const *>(frames), lohis, G, C, Q, N, R, T, cols, H, W, sx, sy, occlusion_threshold,
                       reinterpret_cast<float4 *>(table), entry);
    return check_launch("trackstore_tracks_from_best");
}


extern "C" int mftx_trackstore_appearance(const uint16_t *const *frames, const float *const *lohis, const uint8_t *const *images, int T,
                                          int C, int H, int W, const uint8_t *reference, float occlusion_threshold, float sigma_max,
                                          int fill, float *sum, float *sumsq, int *count, uint8_t *warped, uint8_t *visible, void *stream) {
    if (T < 0) return fail(MFTX_E_ARG, "trackstore_appearance: need T >= 0");
    if (C < 1 || C > 4) return fail(MFTX_E_ARG, "trackstore_appearance: C = %d: need 1 .. 4 channels", C);
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "trackstore_appearance: H and W must be >= 2");
    if ((long long)H * W > 0x7fffffffLL) return fail(MFTX_E_ARG, "trackstore_appearance: more than 2^31 - 1 pixels");
    if (fill < 0 || fill > 255) return fail(MFTX_E_ARG, "trackstore_appearance: fill = %d: need 0 .. 255", fill);
    if (T == 0) return 0;
    const struct { const void *p; const char *name; } ptrs[] = {{frames, "frames"}, {lohis, "lohis"}, {images, "images"}, {sum, "sum"},
                                                                {sumsq, "sumsq"}, {count, "count"}};
    for (const auto &a : ptrs)
        if (!a.p) return fail(MFTX_E_ARG, "trackstore_appearance: null pointer: %s", a.name);
    if (!aligned_to(frames, 8) || !aligned_to(lohis, 8) || !aligned_to(images, 8))
        return fail(MFTX_E_ALIGN, "trackstore_appearance: the pointer tables frames, lohis and images must be 8-byte aligned");
    if (!aligned_to(sum, 4) || !aligned_to(sumsq, 4) || !aligned_to(count, 4))
        return fail(MFTX_E_ALIGN, "trackstore_appearance: sum, sumsq and count must be 4-byte aligned");
    float sx, sy;
    grid_scales(H, W, sx, sy);
    hipStream_t s = (hipStream_t)stream;
    const bool stack = warped != nullptr || visible != nullptr;
    const double n = (double)H * W;
    // per pixel and column: a packed word and (with no reuse between neighbours counted) C image bytes, with the stack C + 1 bytes out;
    // per pixel: the reference and 8 C + 4 bytes of results
    ProfScope prof(PC_CHAIN, s, (8.0 + C + (warped ? C : 0.0) + (visible ? 1.0 : 0.0)) * n * (double)T + (9.0 * C + 4.0) * n);
    const dim3 grid((unsigned)(((long long)H * W + 255) / 256));
    ts_appearance_channels(C, stack, grid, s, reinterpret_cast<const uint2 *const *>(frames), lohis, images, T, H, W, sx, sy, reference,
                           occlusion_threshold, sigma_max, fill, sum, sumsq, count, warped, visible);
    return check_launch("trackstore_appearance");
}

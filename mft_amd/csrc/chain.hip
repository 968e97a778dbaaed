// MFT flow chaining and per-pixel best-chain selection (HBM-bound).
//
// chain (MFT/MFT.py:233-239, MFT/results.py:87-136), per pixel g = (x, y):
//   p     = g + flowL
//   B(X)  = bilinear sample of X at p, zeros outside, align_corners=True, after
//           the reference's normalise (MFT/utils/interpolation.py:69-72) /
//           un-normalise round trip, reproduced here in fp32
//   flow  = (p + B(flowR)) - g ;  occl = max(occlL, B(occlR)) ;
//   sigma = sqrt(sigmaL^2 + B(sigmaR)^2)
// select (MFT/MFT.py:112-143, MFT/results.py:250-265): first arg-max over the
// candidates of -sigma, with -inf where occl > thr; then occl = 1 where the
// selected flow leaves the image.
//
// The reference does 3 grid_samples + ~25 launches per candidate and a
// stack/max/gather pass; here one thread owns a pixel, walks the K candidates,
// and keeps the running best in registers: (32 K + 16) B/pixel of traffic.
// Every kernel here gives the same bits for the same operands -- chain -> all-gather -> select (multi-GPU) is bitwise the
// fused single-GPU kernel, planar and packed and multi-template variants agree -- because each piece of arithmetic is
// written once: B (coordinate round trip, weights, order of the sum, both tap policies) in grid_sample.h, which
// trackstore.hip shares; the chaining rule in `chained()`; the selection in `consider()`; the two walks over the candidates
// in `MFTX_BEST_BATCHED` and `best_sequential()`.
// Compiled with -ffp-contract=off: no FMA contraction, products and sums round
// exactly as written.
#include "common.h"
#include "grid_sample.h"
#include "profile.h"
#include <initializer_list>

namespace mftx {

struct Planes { const float *flow, *occl, *sigma; };
struct Chained { float fx, fy, occ, sig; };

// NaN handling follows torch: a NaN sampled occlusion propagates through
// maximum(); fmaxf would drop it, so patch it up explicitly.
__device__ __forceinline__ float max_nanprop(float a, float b) {
    return (a != a || b != b) ? NAN : fmaxf(a, b);
}

// Pixel g = (x, y) with its left flow: p = g + flowL and the sampler there.
struct ChainPrep { float px, py, gx, gy; GridSample s; };

__device__ __forceinline__ ChainPrep chain_prep(float lfx, float lfy, int H, int W, int x, int y, float sx, float sy) {
    const float gx = (float)x, gy = (float)y;
    const float px = gx + lfx, py = gy + lfy;
    return ChainPrep{px, py, gx, gy, grid_sample_at(px, py, sx, sy, H, W)};
}

// The chaining rule: the left operand's occlusion and sigma with r = B(flow x, flow y, occlusion, sigma of the right operand).
__device__ __forceinline__ Chained chained(const ChainPrep &c, float locc, float lsig, const float4 &r) {
    Chained o;
    o.fx = (c.px + r.x) - c.gx;
    o.fy = (c.py + r.y) - c.gy;
    o.occ = max_nanprop(locc, r.z);
    o.sig = sqrtf(lsig * lsig + r.w * r.w);
    return o;
}

// planar right operand: bounds-tested taps
__device__ __forceinline__ Chained chain_px(const Planes &L, const Planes &R, int H, int W, int x, int y,
                                           float sx, float sy) {
    const long long pix = (long long)y * W + x;
    const long long plane = (long long)H * W;
    const ChainPrep c = chain_prep(L.flow[pix], L.flow[plane + pix], H, W, x, y, sx, sy);
    return chained(c, L.occl[pix], L.sigma[pix],
                   make_float4(grid_sample(c.s, R.flow, H, W), grid_sample(c.s, R.flow + plane, H, W),
                               grid_sample(c.s, R.occl, H, W), grid_sample(c.s, R.sigma, H, W)));
}

__global__ __launch_bounds__(256) void chain_kernel(Planes L, Planes R, int H, int W, float sx, float sy,
                                                    float *flowO, float *occlO, float *sigmaO) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const Chained c = chain_px(L, R, H, W, x, y, sx, sy);
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    flowO[pix] = c.fx; flowO[plane + pix] = c.fy; occlO[pix] = c.occ; sigmaO[pix] = c.sig;
}

// warp_backward (MFT/results.py:116-136): out[c] = B(img[c]) at p = g + flow
__global__ __launch_bounds__(256) void warp_backward_kernel(const float *__restrict__ flow,
                                                            const float *__restrict__ img, int C, int H, int W,
                                                            float sx, float sy, float *__restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    const GridSample s = grid_sample_at((float)x + flow[pix], (float)y + flow[plane + pix], sx, sy, H, W);
    for (int c = 0; c < C; ++c) out[c * plane + pix] = grid_sample(s, img + c * plane, H, W);
}

struct CandSet {
    int K;
    Planes L[MFTX_MAX_CANDIDATES];
    Planes R[MFTX_MAX_CANDIDATES];
};

struct Best { float score = 0.f; Chained c = {0.f, 0.f, 0.f, 0.f}; int k = 0; };      // (consider() takes candidate 0 whatever this holds)

__device__ __forceinline__ void consider(Best &b, const Chained &c, int k, float thr) {
    // torch: scores = -sigma; scores[occl > thr] = -inf; max(dim=0) keeps the
    // first maximal index (a NaN score wins over everything, first NaN kept).
    const float score = (c.occ > thr) ? -INFINITY : -c.sig;
    bool take;
    if (k == 0) take = true;
    else if (b.score != b.score) take = false;          // current best is NaN
    else if (score != score) take = true;               // NaN beats numbers
    else take = score > b.score;                        // strict: first max wins
    if (take) { b.score = score; b.c = c; b.k = k; }
}

__device__ __forceinline__ void write_selected(const Best &b, int H, int W, int x, int y, float *flowO,
                                               float *occlO, float *sigmaO, int8_t *chosen) {
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    const float qx = (float)x + b.c.fx, qy = (float)y + b.c.fy;
    const bool invalid = (qx < 0.f) | (qy < 0.f) | (qx >= (float)W) | (qy >= (float)H);
    flowO[pix] = b.c.fx;
    flowO[plane + pix] = b.c.fy;
    occlO[pix] = invalid ? 1.f : b.c.occ;
    sigmaO[pix] = b.c.sig;
    if (chosen) chosen[pix] = (int8_t)b.k;
}

__global__ __launch_bounds__(256) void chain_select_kernel(CandSet cs, float thr, int H, int W, float sx,
                                                           float sy, float *flowO, float *occlO, float *sigmaO,
                                                           int8_t *chosen) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    Best b;
    for (int k = 0; k < cs.K; ++k) consider(b, chain_px(cs.L[k], cs.R[k], H, W, x, y, sx, sy), k, thr);
    write_selected(b, H, W, x, y, flowO, occlO, sigmaO, chosen);
}

struct SelSet {
    int K;
    Planes C[MFTX_MAX_CANDIDATES];
};

__global__ __launch_bounds__(256) void select_kernel(SelSet ss, float thr, int H, int W, float *flowO,
                                                     float *occlO, float *sigmaO, int8_t *chosen) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    Best b;
    for (int k = 0; k < ss.K; ++k) {
        Chained c;
        c.fx = ss.C[k].flow[pix]; c.fy = ss.C[k].flow[plane + pix];
        c.occ = ss.C[k].occl[pix]; c.sig = ss.C[k].sigma[pix];
        consider(b, c, k, thr);
    }
    write_selected(b, H, W, x, y, flowO, occlO, sigmaO, chosen);
}

// ---- PACKED right operands ([H][W][4] = fx, fy, occl, sigma per pixel, written by the upsampler): each bilinear
// tap is ONE 16-byte gather instead of four 4-byte ones, blended by the same Bilinear::blend and chained by the same
// chained() as the planar operands: bitwise equal results.
struct PackedSet {
    int K;
    Planes L[MFTX_MAX_CANDIDATES];
    const float4 *R[MFTX_MAX_CANDIDATES];
};

__device__ __forceinline__ void write_selected4(const Best (&b)[4], int H, int W, int x, int y, float *flowO,
                                                float *occlO, float *sigmaO, int8_t *chosen) {
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    float ox[4], oy[4], oo[4], os[4];
    char4 ck;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float qx = (float)(x + i) + b[i].c.fx, qy = (float)y + b[i].c.fy;
        const bool invalid = (qx < 0.f) | (qy < 0.f) | (qx >= (float)W) | (qy >= (float)H);
        ox[i] = b[i].c.fx; oy[i] = b[i].c.fy; oo[i] = invalid ? 1.f : b[i].c.occ; os[i] = b[i].c.sig;
    }
    ck.x = (signed char)b[0].k; ck.y = (signed char)b[1].k; ck.z = (signed char)b[2].k; ck.w = (signed char)b[3].k;
    *reinterpret_cast<float4 *>(flowO + pix) = make_float4(ox[0], ox[1], ox[2], ox[3]);
    *reinterpret_cast<float4 *>(flowO + plane + pix) = make_float4(oy[0], oy[1], oy[2], oy[3]);
    *reinterpret_cast<float4 *>(occlO + pix) = make_float4(oo[0], oo[1], oo[2], oo[3]);
    *reinterpret_cast<float4 *>(sigmaO + pix) = make_float4(os[0], os[1], os[2], os[3]);
    if (chosen) *reinterpret_cast<char4 *>(chosen + pix) = ck;
}

// One pixel per thread, right operands PACKED: 4 coalesced 4-byte loads of the left planes + 4 sixteen-byte gathers
// per candidate instead of 4 + 16 four-byte gathers (the planar kernel is bound by the texture-address rate of
// its gathers).  Taps outside the image are read at a clamped address and replaced by zeros afterwards (no branches).
__device__ __forceinline__ float4 packed_tap(const float4 *R, int H, int W, int yy, int xx) {
    bool in;
    const float4 v = R[clamped_tap(H, W, yy, xx, in)];
    return in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void packed_taps(const float4 *R, const GridSample &s, int H, int W, float4 (&t)[4]) {
    t[0] = packed_tap(R, H, W, s.y0, s.x0);
    t[1] = packed_tap(R, H, W, s.y0, s.x0 + 1);
    t[2] = packed_tap(R, H, W, s.y0 + 1, s.x0);
    t[3] = packed_tap(R, H, W, s.y0 + 1, s.x0 + 1);
}

__device__ __forceinline__ Chained chained(const ChainPrep &c, float locc, float lsig, const float4 (&t)[4]) {
    return chained(c, locc, lsig, c.s.w.blend(t[0], t[1], t[2], t[3]));
}

// The chain of a candidate is two dependent memory round trips (left planes -> tap addresses -> taps); walked candidate by
// candidate that is 2 K round trips per thread and the kernel is latency-bound (24 us for 63 MB at K = 7).  `Set` is anything
// with candidate k's left planes in L[k] and its packed right operand in R[k] (PackedSet, MultiTmpl).
template <class Set>
__device__ __forceinline__ Best best_sequential(const Set &cs, int K, float thr, int H, int W, int x, int y, float sx, float sy) {
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    Best b;
    for (int k = 0; k < K; ++k) {
        const Planes L = cs.L[k];
        const ChainPrep c = chain_prep(L.flow[pix], L.flow[plane + pix], H, W, x, y, sx, sy);
        float4 t[4];
        packed_taps(cs.R[k], c.s, H, W, t);
        consider(b, chained(c, L.occl[pix], L.sigma[pix], t), k, thr);
    }
    return b;
}

// With K <= KB, a compile-time bound of at most 8, ALL left planes are loaded first, then the taps in batches of four candidates:
// 1 + ceil(K / 4) round trips.  K is KB itself (every `< K` folds) or a run-time value, uniform per block.  A macro, not a
// function: as a function the compiler simplifies the body on its own before it inlines it, and both kernels came out different
// from the body written in place -- chain_select_packed_kernel<7> 2 % slower, and chain_select_multi_kernel<8, 12> with the
// operands of the blend's sums swapped, which NaN bits show ("One sampler").  That order is the compiler's: an upgrade
// may change it, and tests/test_gpu_chain_family.py (every variant against select, NaN as int32) shows it.  Expands in a
// kernel's scope: it reads pix, plane, thr, H, W, x, y, sx, sy there.
#define MFTX_BEST_BATCHED(b, cs, KB, K)                                                                                          \
    {                                                                                                                            \
        float lfx[KB], lfy[KB], loc[KB], lsg[KB];                                                                                \
        _Pragma("unroll") for (int k = 0; k < KB; ++k) {                                                                         \
            if (k < K) {                                                                                                         \
                lfx[k] = cs.L[k].flow[pix]; lfy[k] = cs.L[k].flow[plane + pix];                                                  \
                loc[k] = cs.L[k].occl[pix]; lsg[k] = cs.L[k].sigma[pix];                                                         \
            }                                                                                                                    \
        }                                                                                                                        \
        _Pragma("unroll") for (int k0 = 0; k0 < KB; k0 += 4) {                                                                   \
            ChainPrep c[4];                                                                                                      \
            float4 tp[4][4];                                                                                                     \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                      \
                if (k0 + j < K) {                                                                                                \
                    c[j] = chain_prep(lfx[k0 + j], lfy[k0 + j], H, W, x, y, sx, sy);                                             \
                    packed_taps(cs.R[k0 + j], c[j].s, H, W, tp[j]);                                                              \
                }                                                                                                                \
            }                                                                                                                    \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                        \
                if (k0 + j < K) consider(b, chained(c[j], loc[k0 + j], lsg[k0 + j], tp[j]), k0 + j, thr);                        \
        }                                                                                                                        \
    }

template <int KT>    // KT = number of candidates (1..8): batched taps; or 0: any K, candidate by candidate
__global__ __launch_bounds__(256) void chain_select_packed_kernel(PackedSet ps, float thr, int H, int W, float sx,
                                                                  float sy, float *flowO, float *occlO, float *sigmaO,
                                                                  int8_t *chosen) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    Best b;
    if constexpr (KT == 0) b = best_sequential(ps, ps.K, thr, H, W, x, y, sx, sy);
    else MFTX_BEST_BATCHED(b, ps, KT, KT)
    write_selected(b, H, W, x, y, flowO, occlO, sigmaO, chosen);
}

__global__ __launch_bounds__(256) void select4_kernel(SelSet ss, float thr, int H, int W, float *flowO, float *occlO,
                                                      float *sigmaO, int8_t *chosen) {
    const int x = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
    const int y = blockIdx.y;
    if (x >= W) return;
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    Best b[4];
    for (int k = 0; k < ss.K; ++k) {
        const float4 fx = *reinterpret_cast<const float4 *>(ss.C[k].flow + pix);
        const float4 fy = *reinterpret_cast<const float4 *>(ss.C[k].flow + plane + pix);
        const float4 oc = *reinterpret_cast<const float4 *>(ss.C[k].occl + pix);
        const float4 sg = *reinterpret_cast<const float4 *>(ss.C[k].sigma + pix);
        consider(b[0], Chained{fx.x, fy.x, oc.x, sg.x}, k, thr);
        consider(b[1], Chained{fx.y, fy.y, oc.y, sg.y}, k, thr);
        consider(b[2], Chained{fx.z, fy.z, oc.z, sg.z}, k, thr);
        consider(b[3], Chained{fx.w, fy.w, oc.w, sg.w}, k, thr);
    }
    write_selected4(b, H, W, x, y, flowO, occlO, sigmaO, chosen);
}

// ---- MANY TEMPLATES of one video in one launch (mft_amd/multi.py): template j = blockIdx.z chains its own K[j] candidates
// and selects among them with chain_select_packed_kernel's two walks -- the output of template j is bitwise what
// mftx_chain_select_packed gives for that template's candidates alone.  K is a run-time value below the compile-time bound
// KMAX, uniform per block (no divergence).  The descriptors travel by value in the kernel arguments (they are read with
// scalar loads, indexed by blockIdx.z); a launch's argument block is limited to 4 KB, hence TN templates per launch.  The
// right operands the templates share (the finite-delta pairs of a frame) are read once from HBM and then from L2 /
// Infinity Cache by the other templates' blocks.
template <int KMAX>
struct MultiTmpl {
    int K;
    Planes L[KMAX];
    const float4 *R[KMAX];
    float *flowO, *occlO, *sigmaO;
    int8_t *chosen;
};
constexpr int MULTI_TN8 = 12;      // 12 x 296 B = 3552 B
constexpr int MULTI_TN16 = 6;      //  6 x 552 B = 3312 B
template <int KMAX, int TN>
struct MultiSet { MultiTmpl<KMAX> t[TN]; };
static_assert(sizeof(MultiSet<8, MULTI_TN8>) + 32 <= 4096 && sizeof(MultiSet<MFTX_MAX_CANDIDATES, MULTI_TN16>) + 32 <= 4096,
              "kernel arguments of chain_select_multi_kernel exceed 4 KB");

template <int KMAX, int TN>     // KMAX = 8: batched taps; KMAX = 16: any K, candidate by candidate
__global__ __launch_bounds__(256) void chain_select_multi_kernel(MultiSet<KMAX, TN> ms, float thr, int H, int W, float sx,
                                                                 float sy) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const MultiTmpl<KMAX> &t = ms.t[blockIdx.z];
    const int K = t.K;
    const long long pix = (long long)y * W + x, plane = (long long)H * W;
    Best b;
    if constexpr (KMAX > 8) b = best_sequential(t, K, thr, H, W, x, y, sx, sy);
    else MFTX_BEST_BATCHED(b, t, KMAX, K)
    write_selected(b, H, W, x, y, t.flowO, t.occlO, t.sigmaO, t.chosen);
}
#undef MFTX_BEST_BATCHED

// ---- point read-out of many templates' results in one launch (MFT/point_tracking.py:6-27: warp_forward_points + sample).
// Point i belongs to template tmpl[i] and sits at (xy[2 i], xy[2 i + 1]) on that template's frame: its flow / occlusion /
// sigma planes are sampled there with grid_sample.h's sampler (bilinear, zeros outside, align_corners=True, after the
// normalise / un-normalise round trip) and (x + fx, y + fy, occlusion, sigma) goes, as ONE 16-byte store, to row i, column
// `column` of the caller's table.  One thread per point; a launch carries the planes of up to SAMPLE_TN templates in its
// arguments and leaves the points of other templates alone.
constexpr int SAMPLE_TN = 128;     // 128 x 24 B = 3072 B
struct SampleSet { Planes t[SAMPLE_TN]; };
static_assert(sizeof(SampleSet) + 64 <= 4096, "kernel arguments of sample_points_kernel exceed 4 KB");

__global__ __launch_bounds__(256) void sample_points_kernel(SampleSet ss, int t0, int nt, int H, int W, float sx, float sy,
                                                            int N, const int *__restrict__ tmpl, const float *__restrict__ xy,
                                                            float *__restrict__ table, long long row_stride, int column) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int j = tmpl[i] - t0;
    if (j < 0 || j >= nt) return;
    const Planes P = ss.t[j];
    const long long plane = (long long)H * W;
    const float px = xy[2 * (long long)i], py = xy[2 * (long long)i + 1];
    const GridSample s = grid_sample_at(px, py, sx, sy, H, W);
    const float4 o = make_float4(px + grid_sample(s, P.flow, H, W), py + grid_sample(s, P.flow + plane, H, W),
                                 grid_sample(s, P.occl, H, W), grid_sample(s, P.sigma, H, W));
    *reinterpret_cast<float4 *>(table + (long long)i * row_stride + 4 * (long long)column) = o;
}

}  // namespace mftx

using namespace mftx;

// float4 access to every plane: W % 4 == 0 and all bases 16-byte aligned
static bool vec4_ok(int W, std::initializer_list<const void *> ptrs) {
    if (W % 4) return false;
    for (const void *p : ptrs) if (p != nullptr && !aligned16(p)) return false;
    return true;
}

extern "C" int mftx_chain(const float *flowL, const float *occlL, const float *sigmaL, const float *flowR,
                          const float *occlR, const float *sigmaR, int H, int W, float *flowO, float *occlO,
                          float *sigmaO, void *stream) {
    if (!flowL || !occlL || !sigmaL || !flowR || !occlR || !sigmaR || !flowO || !occlO || !sigmaO)
        return fail(MFTX_E_ARG, "chain: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "chain: H and W must be >= 2");
    float sx, sy;
    grid_scales(H, W, sx, sy);
    Planes L{flowL, occlL, sigmaL}, R{flowR, occlR, sigmaR};
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, 48.0 * H * W);
    hipLaunchKernelGGL(chain_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, L, R, H, W, sx, sy,
                       flowO, occlO, sigmaO);
    return check_launch("chain");
}

extern "C" int mftx_warp_backward(const float *flow, const float *img, int C, int H, int W, float *out,
                                  void *stream) {
    if (!flow || !img || !out) return fail(MFTX_E_ARG, "warp_backward: null pointer");
    if (C < 1 || H < 2 || W < 2) return fail(MFTX_E_ARG, "warp_backward: need C >= 1, H, W >= 2");
    float sx, sy;
    grid_scales(H, W, sx, sy);
    hipLaunchKernelGGL(warp_backward_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, flow, img,
                       C, H, W, sx, sy, out);
    return check_launch("warp_backward");
}

extern "C" int mftx_select(int K, const float *const *flow, const float *const *occl, const float *const *sigma,
                           float thr, int H, int W, float *flowO, float *occlO, float *sigmaO, int8_t *chosen,
                           void *stream) {
    if (K < 1 || K > MFTX_MAX_CANDIDATES) return fail(MFTX_E_ARG, "select: K must be in 1..%d", MFTX_MAX_CANDIDATES);
    if (!flow || !occl || !sigma || !flowO || !occlO || !sigmaO) return fail(MFTX_E_ARG, "select: null pointer");
    if (H < 1 || W < 1) return fail(MFTX_E_ARG, "select: bad size");
    SelSet ss;
    ss.K = K;
    for (int k = 0; k < K; ++k) {
        if (!flow[k] || !occl[k] || !sigma[k]) return fail(MFTX_E_ARG, "select: null candidate %d", k);
        ss.C[k] = Planes{flow[k], occl[k], sigma[k]};
    }
    bool v4 = vec4_ok(W, {flowO, occlO, sigmaO}) && (chosen == nullptr || (reinterpret_cast<uintptr_t>(chosen) & 3) == 0);
    for (int k = 0; k < K && v4; ++k) v4 = vec4_ok(W, {flow[k], occl[k], sigma[k]});
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, (16.0 * K + 16.0) * H * W);
    if (v4)
        hipLaunchKernelGGL(select4_kernel, dim3(cdiv(W, 256), H), dim3(64), 0, (hipStream_t)stream, ss, thr, H, W,
                           flowO, occlO, sigmaO, chosen);
    else
        hipLaunchKernelGGL(select_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, ss, thr, H, W,
                           flowO, occlO, sigmaO, chosen);
    return check_launch("select");
}

extern "C" int mftx_chain_select(int K, const float *const *flowL, const float *const *occlL,
                                 const float *const *sigmaL, const float *const *flowR,
                                 const float *const *occlR, const float *const *sigmaR, float thr, int H, int W,
                                 float *flowO, float *occlO, float *sigmaO, int8_t *chosen, void *stream) {
    if (K < 1 || K > MFTX_MAX_CANDIDATES)
        return fail(MFTX_E_ARG, "chain_select: K must be in 1..%d", MFTX_MAX_CANDIDATES);
    if (!flowL || !occlL || !sigmaL || !flowR || !occlR || !sigmaR || !flowO || !occlO || !sigmaO)
        return fail(MFTX_E_ARG, "chain_select: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "chain_select: H and W must be >= 2");
    CandSet cs;
    cs.K = K;
    for (int k = 0; k < K; ++k) {
        if (!flowL[k] || !occlL[k] || !sigmaL[k] || !flowR[k] || !occlR[k] || !sigmaR[k])
            return fail(MFTX_E_ARG, "chain_select: null candidate %d", k);
        cs.L[k] = Planes{flowL[k], occlL[k], sigmaL[k]};
        cs.R[k] = Planes{flowR[k], occlR[k], sigmaR[k]};
    }
    float sx, sy;
    grid_scales(H, W, sx, sy);
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, (32.0 * K + 16.0) * H * W);
    hipLaunchKernelGGL(chain_select_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, cs, thr, H,
                       W, sx, sy, flowO, occlO, sigmaO, chosen);
    return check_launch("chain_select");
}

extern "C" int mftx_chain_select_packed(int K, const float *const *flowL, const float *const *occlL,
                                        const float *const *sigmaL, const float *const *packedR, float thr, int H,
                                        int W, float *flowO, float *occlO, float *sigmaO, int8_t *chosen, void *stream) {
    if (K < 1 || K > MFTX_MAX_CANDIDATES)
        return fail(MFTX_E_ARG, "chain_select_packed: K must be in 1..%d", MFTX_MAX_CANDIDATES);
    if (!flowL || !occlL || !sigmaL || !packedR || !flowO || !occlO || !sigmaO)
        return fail(MFTX_E_ARG, "chain_select_packed: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "chain_select_packed: H and W must be >= 2");
    PackedSet ps;
    ps.K = K;
    for (int k = 0; k < K; ++k) {
        if (!flowL[k] || !occlL[k] || !sigmaL[k] || !packedR[k])
            return fail(MFTX_E_ARG, "chain_select_packed: null candidate %d", k);
        if (!aligned16(packedR[k])) return fail(MFTX_E_ALIGN, "chain_select_packed: packed operands must be 16-byte aligned");
        ps.L[k] = Planes{flowL[k], occlL[k], sigmaL[k]};
        ps.R[k] = reinterpret_cast<const float4 *>(packedR[k]);
    }
    float sx, sy;
    grid_scales(H, W, sx, sy);
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, (32.0 * K + 16.0) * H * W);
#define CSP_LAUNCH(KT)                                                                                               \
    hipLaunchKernelGGL(chain_select_packed_kernel<KT>, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, ps, thr, H, \
                       W, sx, sy, flowO, occlO, sigmaO, chosen)
    switch (K) {
        case 1: CSP_LAUNCH(1); break;
        case 2: CSP_LAUNCH(2); break;
        case 3: CSP_LAUNCH(3); break;
        case 4: CSP_LAUNCH(4); break;
        case 5: CSP_LAUNCH(5); break;
        case 6: CSP_LAUNCH(6); break;
        case 7: CSP_LAUNCH(7); break;
        case 8: CSP_LAUNCH(8); break;
        default: CSP_LAUNCH(0); break;
    }
#undef CSP_LAUNCH
    return check_launch("chain_select_packed");
}

template <int KMAX, int TN>
static void launch_multi(int n, const int *K, const float *const *flowL, const float *const *occlL,
                         const float *const *sigmaL, const float *const *packedR, float thr, int H, int W, float sx,
                         float sy, float *const *flowO, float *const *occlO, float *const *sigmaO, int8_t *const *chosen,
                         hipStream_t stream) {
    MultiSet<KMAX, TN> ms = {};
    for (int j = 0, c = 0; j < n; ++j) {
        MultiTmpl<KMAX> &t = ms.t[j];
        t.K = K[j];
        for (int k = 0; k < K[j]; ++k, ++c) {
            t.L[k] = Planes{flowL[c], occlL[c], sigmaL[c]};
            t.R[k] = reinterpret_cast<const float4 *>(packedR[c]);
        }
        t.flowO = flowO[j]; t.occlO = occlO[j]; t.sigmaO = sigmaO[j];
        t.chosen = chosen ? chosen[j] : nullptr;
    }
    hipLaunchKernelGGL((chain_select_multi_kernel<KMAX, TN>), dim3(cdiv(W, 256), H, n), dim3(256), 0, stream, ms, thr, H, W,
                       sx, sy);
}

extern "C" int mftx_chain_select_multi(int T, const int *K, const float *const *flowL, const float *const *occlL,
                                       const float *const *sigmaL, const float *const *packedR, float thr, int H, int W,
                                       float *const *flowO, float *const *occlO, float *const *sigmaO,
                                       int8_t *const *chosen, void *stream) {
    if (T < 1) return fail(MFTX_E_ARG, "chain_select_multi: T must be >= 1");
    if (!K || !flowL || !occlL || !sigmaL || !packedR || !flowO || !occlO || !sigmaO)
        return fail(MFTX_E_ARG, "chain_select_multi: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "chain_select_multi: H and W must be >= 2");
    int maxK = 0;
    long long total = 0;
    for (int j = 0; j < T; ++j) {
        if (K[j] < 1 || K[j] > MFTX_MAX_CANDIDATES)
            return fail(MFTX_E_ARG, "chain_select_multi: K[%d] must be in 1..%d", j, MFTX_MAX_CANDIDATES);
        if (!flowO[j] || !occlO[j] || !sigmaO[j]) return fail(MFTX_E_ARG, "chain_select_multi: null output of template %d", j);
        for (int k = 0; k < K[j]; ++k, ++total) {
            if (!flowL[total] || !occlL[total] || !sigmaL[total] || !packedR[total])
                return fail(MFTX_E_ARG, "chain_select_multi: null candidate %d of template %d", k, j);
            if (!aligned16(packedR[total]))
                return fail(MFTX_E_ALIGN, "chain_select_multi: packed operands must be 16-byte aligned");
        }
        maxK = K[j] > maxK ? K[j] : maxK;
    }
    float sx, sy;
    grid_scales(H, W, sx, sy);
    // bytes per pixel: every left operand (16) and every output (16) once, every DISTINCT right operand (16) once
    double bytes = 0.0;
    if (prof_enabled()) {
        long long distinct = 0;
        for (long long c = 0; c < total; ++c) {
            bool seen = false;
            for (long long d = 0; d < c && !seen; ++d) seen = packedR[d] == packedR[c];
            distinct += !seen;
        }
        bytes = (16.0 * total + 16.0 * distinct + 16.0 * T) * H * W;
    }
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, bytes);
    const int per = maxK <= 8 ? MULTI_TN8 : MULTI_TN16;
    for (int j0 = 0, c0 = 0; j0 < T; j0 += per) {
        const int n = T - j0 < per ? T - j0 : per;
        if (maxK <= 8)
            launch_multi<8, MULTI_TN8>(n, K + j0, flowL + c0, occlL + c0, sigmaL + c0, packedR + c0, thr, H, W, sx, sy,
                                       flowO + j0, occlO + j0, sigmaO + j0, chosen ? chosen + j0 : nullptr, (hipStream_t)stream);
        else
            launch_multi<MFTX_MAX_CANDIDATES, MULTI_TN16>(n, K + j0, flowL + c0, occlL + c0, sigmaL + c0, packedR + c0, thr, H,
                                                          W, sx, sy, flowO + j0, occlO + j0, sigmaO + j0,
                                                          chosen ? chosen + j0 : nullptr, (hipStream_t)stream);
        for (int j = j0; j < j0 + n; ++j) c0 += K[j];
        const int rc = check_launch("chain_select_multi");
        if (rc) return rc;
    }
    return 0;
}

extern "C" int mftx_sample_points(int T, const float *const *flow, const float *const *occl, const float *const *sigma,
                                  int H, int W, int N, const int *tmpl, const float *xy, float *table,
                                  long long row_stride, int column, void *stream) {
    if (T < 1 || N < 0) return fail(MFTX_E_ARG, "sample_points: need T >= 1, N >= 0");
    if (!flow || !occl || !sigma) return fail(MFTX_E_ARG, "sample_points: null pointer");
    if (H < 2 || W < 2) return fail(MFTX_E_ARG, "sample_points: H and W must be >= 2");
    for (int j = 0; j < T; ++j)
        if (!flow[j] || !occl[j] || !sigma[j]) return fail(MFTX_E_ARG, "sample_points: null planes of template %d", j);
    if (N == 0) return 0;
    if (!tmpl || !xy || !table) return fail(MFTX_E_ARG, "sample_points: null pointer");
    if (column < 0 || row_stride < 4 * ((long long)column + 1) || row_stride % 4)
        return fail(MFTX_E_ARG, "sample_points: row_stride must be a multiple of 4 floats that holds column %d", column);
    if (!aligned16(table)) return fail(MFTX_E_ALIGN, "sample_points: the table must be 16-byte aligned");
    float sx, sy;
    grid_scales(H, W, sx, sy);
    // per point: template index + xy (12 B), 4 taps of 4 planes (64 B), one table entry (16 B)
    ProfScope prof(PC_CHAIN, (hipStream_t)stream, (12.0 + 64.0 + 16.0) * N);
    for (int t0 = 0; t0 < T; t0 += SAMPLE_TN) {
        const int nt = T - t0 < SAMPLE_TN ? T - t0 : SAMPLE_TN;
        SampleSet ss = {};
        for (int j = 0; j < nt; ++j) ss.t[j] = Planes{flow[t0 + j], occl[t0 + j], sigma[t0 + j]};
        hipLaunchKernelGGL(sample_points_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, ss, t0, nt, H, W, sx,
                           sy, N, tmpl, xy, table, row_stride, column);
        const int rc = check_launch("sample_points");
        if (rc) return rc;
    }
    return 0;
}

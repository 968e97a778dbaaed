// Forward splat (FlowOUTrackingResult.warp_forward: MFT/results.py:190-248 with MFT/utils/interpolation.py:234-309) and the
// demo overlays built on it (demo.py:116-146), bitwise reproducible.
//
// Every kept template pixel (x, y) spreads its value over the four pixels around dst = g + flow:
//   x0 = floor(x), x1 = x0 + 1 (likewise y); THEN x is clamped to [0, W-1], y to [0, H-1], and so are the four corner
//   coordinates; wx0 = x1 - x, wx1 = x - x0, wy0 = y1 - y, wy1 = y - y0; the four fp32 products go
//   wx0*wy0 -> (y0, x0), wx0*wy1 -> (y1, x0), wx1*wy0 -> (y0, x1), wx1*wy1 -> (y1, x1)
// -- operation for operation the torch path of mft_amd/results.py (this unit is built like chain.o: no FMA contraction, no
// packed fp32).  A pixel whose destination is not finite contributes nothing.
//
// The sums are 64-bit INTEGERS: q_w = rint(w * 2^S) (half-even; a corner with q_w == 0 is dropped), v_q = the integer value
// (V = 0) or rint((double)v * 2^V); per corner acc[c][p] += v_q[c] * q_w and cnt[p] += q_w by a 64-bit atomic add without
// return.  Integer addition is associative, so the accumulator -- and everything resolved from it -- does not depend on the
// order the atomics arrive in; float atomics would.  The host picks S and V so that no sum can leave 62 bits
// (mft_amd/ops.py: splat_plan).  The accumulator is planar [C + 1][H][W] (plane C = cnt) and one thread owns one source
// pixel, consecutive lanes consecutive pixels: under a smooth flow one atomic wave-instruction covers a near-contiguous
// run of one plane.
#include "common.h"

namespace mftx {

__device__ __forceinline__ void add64(long long *p, long long v) {
    // result unused: an atomic add without return; two's complement, so the unsigned add is the signed one
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
}

// the four destination pixels and quantised weights of the source pixel (xi, yi); false: the destination is not finite
__device__ __forceinline__ bool splat_corners(float fx, float fy, int xi, int yi, int H, int W, double wscale,
                                              long long (&p)[4], long long (&q)[4]) {
    const float x = (float)xi + fx, y = (float)yi + fy;
    if (!__builtin_isfinite(x) || !__builtin_isfinite(y)) return false;
    // clamp the float before the int conversion (as chain_px does); anything beyond +-1e6 clamps to the border below anyway
    const int x0 = (int)fminf(fmaxf(floorf(x), -1.0e6f), 1.0e6f);
    const int y0 = (int)fminf(fmaxf(floorf(y), -1.0e6f), 1.0e6f);
    const float xc = fminf(fmaxf(x, 0.f), (float)(W - 1));
    const float yc = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const int x0c = min(max(x0, 0), W - 1), x1c = min(max(x0 + 1, 0), W - 1);
    const int y0c = min(max(y0, 0), H - 1), y1c = min(max(y0 + 1, 0), H - 1);
    const float wx0 = (float)x1c - xc, wx1 = xc - (float)x0c;
    const float wy0 = (float)y1c - yc, wy1 = yc - (float)y0c;
    const float w[4] = {wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1};
    p[0] = (long long)y0c * W + x0c; p[1] = (long long)y1c * W + x0c;
    p[2] = (long long)y0c * W + x1c; p[3] = (long long)y1c * W + x1c;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = (long long)rint((double)w[j] * wscale);
    return true;
}

__device__ __forceinline__ long long quantise(float v, double vscale) {
    return __builtin_isfinite(v) ? (long long)rint((double)v * vscale) : 0;
}
__device__ __forceinline__ long long quantise(uint8_t v, double) { return (long long)v; }

template <typename T>
__global__ __launch_bounds__(256) void splat_forward_kernel(const float *__restrict__ flow, const T *__restrict__ img,
                                                            const uint8_t *__restrict__ mask, int C, int H, int W,
                                                            double wscale, double vscale, long long *__restrict__ acc) {
    const long long n = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask != nullptr && mask[i] == 0) return;
    const int yi = (int)(i / W), xi = (int)(i - (long long)yi * W);
    long long p[4], q[4];
    if (!splat_corners(flow[i], flow[n + i], xi, yi, H, W, wscale, p, q)) return;
    for (int c = 0; c < C; ++c) {
        const long long v = quantise(img[i * C + c], vscale);
        long long *plane = acc + (long long)c * n;
        if (v != 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (q[j] != 0) add64(plane + p[j], v * q[j]);
        }
    }
    long long *cnt = acc + (long long)C * n;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (q[j] != 0) add64(cnt + p[j], q[j]);
}

// out [H][W][C] = (float)((double)acc / ((double)cnt * 2^V)) where cnt > 0, else `fill`; clear: zero what was read
__global__ __launch_bounds__(256) void splat_resolve_kernel(long long *__restrict__ acc, int C, long long n, double vscale,
                                                            float fill, int clear, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long cnt = acc[(long long)C * n + i];
    if (cnt > 0) {
        const double den = (double)cnt * vscale;
        for (int c = 0; c < C; ++c) {
            out[i * C + c] = (float)((double)acc[(long long)c * n + i] / den);
            if (clear) acc[(long long)c * n + i] = 0;
        }
        if (clear) acc[(long long)C * n + i] = 0;
    } else {
        for (int c = 0; c < C; ++c) out[i * C + c] = fill;
    }
}

// ---- the edit overlay (vis.draw_edit): the BGRA edit's integer channels (b a, g a, r a, a) are splatted for template
// pixels that are visible (occlusion < 0.5; a NaN compares false, as in torch) and inside the edit (a > 0)
__global__ __launch_bounds__(256) void edit_splat_kernel(const float *__restrict__ flow, const float *__restrict__ occl,
                                                         const uchar4 *__restrict__ edit, int H, int W, double wscale,
                                                         long long *__restrict__ acc) {
    const long long n = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uchar4 e = edit[i];
    if (!(occl[i] < 0.5f) || e.w == 0) return;
    const int yi = (int)(i / W), xi = (int)(i - (long long)yi * W);
    long long p[4], q[4];
    if (!splat_corners(flow[i], flow[n + i], xi, yi, H, W, wscale, p, q)) return;
    const long long a = e.w;
    const long long v[5] = {(long long)e.x * a, (long long)e.y * a, (long long)e.z * a, a, 1};      // plane 4 = cnt
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        if (v[c] == 0) continue;
        long long *plane = acc + (long long)c * n;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q[j] != 0) add64(plane + p[j], v[c] * q[j]);
    }
}

// resolve + blend + clear: colour_c = trunc(clip((float)(acc_c / (cnt * 255)))), alpha = (float)(acc_a / cnt) / alpha_div,
// gray = cv2's 14-bit BGR2GRAY, out = trunc(clip(colour + gray * (1 - alpha))) in fp32 (vis.blend_with_alpha_premult);
// a pixel nothing reached has colour = alpha = 0
__global__ __launch_bounds__(256) void edit_composite_kernel(long long *__restrict__ acc, const uint8_t *__restrict__ frame,
                                                             long long n, float alpha_div, uint8_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = frame[3 * i], g = frame[3 * i + 1], r = frame[3 * i + 2];
    const float gray = (float)((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14);
    const long long cnt = acc[4 * n + i];
    float colour[3] = {0.f, 0.f, 0.f}, alpha = 0.f;
    if (cnt > 0) {
        const double dc = (double)cnt;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = (float)((double)acc[c * n + i] / (dc * 255.0));
            colour[c] = (float)(uint8_t)fminf(fmaxf(v, 0.f), 255.f);
            acc[c * n + i] = 0;
        }
        alpha = __fdiv_rn((float)((double)acc[3 * n + i] / dc), alpha_div);
        acc[3 * n + i] = 0;
        acc[4 * n + i] = 0;
    }
    const float keep = 1.f - alpha;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = (uint8_t)fminf(fmaxf(colour[c] + gray * keep, 0.f), 255.f);
}

// ---- the point overlay (vis.draw_dots): one wave per point writes its disc, fp64 as numpy evaluates it
__global__ __launch_bounds__(64) void overlay_dots_kernel(uint8_t *__restrict__ out, int H, int W,
                                                          const float *__restrict__ table, long long row_stride, int r,
                                                          double limit, uchar4 colour) {
    const float *row = table + (long long)blockIdx.x * row_stride;
    const float xf = row[0], yf = row[1], oc = row[2];
    if (oc > 0.5f || !__builtin_isfinite(xf) || !__builtin_isfinite(yf)) return;
    const double x = (double)xf, y = (double)yf;
    if (fabs(x) > 1.0e9 || fabs(y) > 1.0e9) return;                 // nowhere near the frame (and cx, cy stay small)
    const long long cx = (long long)rint(x), cy = (long long)rint(y);
    const int side = 2 * r + 1;
    for (int t = threadIdx.x; t < side * side; t += 64) {
        const int dy = t / side - r, dx = t - (t / side) * side - r;
        const long long px = dx + cx, py = dy + cy;
        const double ex = (double)px - x, ey = (double)py - y;
        if (ex * ex + ey * ey <= limit && px >= 0 && px < W && py >= 0 && py < H) {
            uint8_t *o = out + 3 * (py * W + px);
            o[0] = colour.x; o[1] = colour.y; o[2] = colour.z;
        }
    }
}

__global__ __launch_bounds__(256) void copy_u8_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

}  // namespace mftx

using namespace mftx;

static unsigned pixel_blocks(int H, int W) { return (unsigned)(((long long)H * W + 255) / 256); }

extern "C" int mftx_splat_forward(const float *flow, const void *img, int img_dtype, const uint8_t *mask, int C, int H, int W,
                                  int S, int V, long long *acc, void *stream) {
    if (!flow || !img || !acc) return fail(MFTX_E_ARG, "splat_forward: null pointer");
    if (C < 1 || H < 1 || W < 1) return fail(MFTX_E_ARG, "splat_forward: need C, H, W >= 1");
    if ((long long)H * W > (1ll << 29)) return fail(MFTX_E_ARG, "splat_forward: frame too large");
    if (img_dtype != MFTX_SPLAT_F32 && img_dtype != MFTX_SPLAT_U8) return fail(MFTX_E_ARG, "splat_forward: img_dtype must be 0 (float32) or 1 (uint8)");
    if (S < 16 || S > 24) return fail(MFTX_E_ARG, "splat_forward: S must be in 16..24 (got %d)", S);
    if (img_dtype == MFTX_SPLAT_U8 ? V != 0 : (V < 12 || V > 23))
        return fail(MFTX_E_ARG, "splat_forward: V must be 0 for integer values, 12..23 for float values (got %d)", V);
    const double wscale = (double)(1ll << S), vscale = (double)(1ll << V);
    if (img_dtype == MFTX_SPLAT_U8)
        hipLaunchKernelGGL(splat_forward_kernel<uint8_t>, dim3(pixel_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, flow,
                           static_cast<const uint8_t *>(img), mask, C, H, W, wscale, vscale, acc);
    else
        hipLaunchKernelGGL(splat_forward_kernel<float>, dim3(pixel_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, flow,
                           static_cast<const float *>(img), mask, C, H, W, wscale, vscale, acc);
    return check_launch("splat_forward");
}

extern "C" int mftx_splat_resolve(long long *acc, int C, int H, int W, int V, float fill, int clear, float *out, void *stream) {
    if (!acc || !out) return fail(MFTX_E_ARG, "splat_resolve: null pointer");
    if (C < 1 || H < 1 || W < 1) return fail(MFTX_E_ARG, "splat_resolve: need C, H, W >= 1");
    if (V < 0 || V > 23) return fail(MFTX_E_ARG, "splat_resolve: V must be in 0..23 (got %d)", V);
    hipLaunchKernelGGL(splat_resolve_kernel, dim3(pixel_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, acc, C,
                       (long long)H * W, (double)(1ll << V), fill, clear, out);
    return check_launch("splat_resolve");
}

extern "C" int mftx_overlay_edit(const float *flow, const float *occl, const uint8_t *edit, const uint8_t *frame, int H, int W,
                                 int S, float alpha_div, long long *acc, uint8_t *out, void *stream) {
    // edit == NULL: composite only (of what acc holds); out == NULL: splat only -- the two launches one by one, for measurements
    if (!acc || (!edit && !out)) return fail(MFTX_E_ARG, "overlay_edit: null pointer");
    if ((edit && (!flow || !occl)) || (out && !frame)) return fail(MFTX_E_ARG, "overlay_edit: null pointer");
    if (H < 1 || W < 1) return fail(MFTX_E_ARG, "overlay_edit: bad size");
    if ((long long)H * W > (1ll << 29)) return fail(MFTX_E_ARG, "overlay_edit: frame too large");
    if (S < 16 || S > 24) return fail(MFTX_E_ARG, "overlay_edit: S must be in 16..24 (got %d)", S);
    if (alpha_div != 255.f && alpha_div != 1.f) return fail(MFTX_E_ARG, "overlay_edit: alpha_div must be 255 or 1");
    if (reinterpret_cast<uintptr_t>(edit) & 3) return fail(MFTX_E_ALIGN, "overlay_edit: the edit must be 4-byte aligned");
    if (edit) {
        hipLaunchKernelGGL(edit_splat_kernel, dim3(pixel_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, flow, occl,
                           reinterpret_cast<const uchar4 *>(edit), H, W, (double)(1ll << S), acc);
        const int rc = check_launch("overlay_edit (splat)");
        if (rc) return rc;
    }
    if (out)
        hipLaunchKernelGGL(edit_composite_kernel, dim3(pixel_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, acc, frame,
                           (long long)H * W, alpha_div, out);
    return check_launch("overlay_edit (composite)");
}

extern "C" int mftx_overlay_dots(const uint8_t *frame, uint8_t *out, int H, int W, const float *table, long long row_stride,
                                 int N, double radius, int b, int g, int r, void *stream) {
    if (!frame || !out) return fail(MFTX_E_ARG, "overlay_dots: null pointer");
    if (H < 1 || W < 1 || N < 0) return fail(MFTX_E_ARG, "overlay_dots: bad size");
    if ((long long)H * W > (1ll << 29)) return fail(MFTX_E_ARG, "overlay_dots: frame too large");
    if (!(radius >= 0.0 && radius <= 256.0)) return fail(MFTX_E_ARG, "overlay_dots: radius must be in 0..256");
    if (N > 0 && (!table || row_stride < 3)) return fail(MFTX_E_ARG, "overlay_dots: need a table with row_stride >= 3");
    const long long bytes = 3ll * H * W;
    if (out != frame) {
        const long long blocks = (bytes + 255) / 256;
        hipLaunchKernelGGL(copy_u8_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream,
                           frame, out, bytes);
        const int rc = check_launch("overlay_dots (copy)");
        if (rc) return rc;
    }
    if (N == 0) return 0;
    const uchar4 colour = make_uchar4((unsigned char)b, (unsigned char)g, (unsigned char)r, 0);
    hipLaunchKernelGGL(overlay_dots_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, out, H, W, table, row_stride,
                       (int)ceil(radius), (radius + 0.5) * (radius + 0.5), colour);
    return check_launch("overlay_dots");
}

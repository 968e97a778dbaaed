// The reference's bilinear sampler (MFT/utils/interpolation.py:69-72 + grid_sample: zeros outside, align_corners=True), written
// ONCE for every kernel that must give its bits: chain.hip (chain, warp_backward, the chain_select family, sample_points) and
// trackstore.hip (query, flow_from, flow_from_best; locate's blend of a cell's corners).  Everything is float32, operation by
// operation as the reference does it; every unit that includes this is compiled with -ffp-contract=off, so products and sums
// round exactly as written here.
#pragma once
#include <hip/hip_runtime.h>

namespace mftx {

// np.array([2/(W-1), 2/(H-1)]).astype(np.float32)  (double division, then rounded)
static inline void grid_scales(int H, int W, float &sx, float &sy) {
    sx = (float)(2.0 / (double)(W - 1));
    sy = (float)(2.0 / (double)(H - 1));
}

// The four weights of a point (wx, wy) in the unit cell and the order the four terms are summed in.
struct Bilinear {
    float w00, w01, w10, w11;
    __device__ __forceinline__ static Bilinear at(float wx, float wy) {
        const float w00 = (1.f - wx) * (1.f - wy), w01 = wx * (1.f - wy), w10 = (1.f - wx) * wy, w11 = wx * wy;
        return Bilinear{w00, w01, w10, w11};
    }
    __device__ __forceinline__ float blend(float a, float b, float c, float d) const { return a * w00 + b * w01 + c * w10 + d * w11; }
    __device__ __forceinline__ float4 blend(const float4 &a, const float4 &b, const float4 &c, const float4 &d) const {
        return make_float4(blend(a.x, b.x, c.x, d.x), blend(a.y, b.y, c.y, d.y), blend(a.z, b.z, c.z, d.z), blend(a.w, b.w, c.w, d.w));
    }
};

// The sampler at the pixel-space point (px, py) of an H x W frame: the taps are (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
// (y0 + 1, x0 + 1), in blend()'s order.
struct GridSample {
    int x0, y0;
    Bilinear w;
};

__device__ __forceinline__ GridSample grid_sample_at(float px, float py, float sx, float sy, int H, int W) {
    // normalise: p * float32(2/(W-1)) - 1 ; un-normalise: ((g + 1) / 2) * (W - 1)
    const float ix = ((px * sx - 1.f) + 1.f) / 2.f * (float)(W - 1);
    const float iy = ((py * sy - 1.f) + 1.f) / 2.f * (float)(H - 1);
    const float flx = floorf(ix), fly = floorf(iy);
    const float wx = ix - flx, wy = iy - fly;
    // the float is limited before the int conversion: anything beyond +-1e6 is outside every frame either way
    const int x0 = (int)fminf(fmaxf(flx, -1.0e6f), 1.0e6f);
    const int y0 = (int)fminf(fmaxf(fly, -1.0e6f), 1.0e6f);
    return GridSample{x0, y0, Bilinear::at(wx, wy)};
}

// ---- tap policy 1: the read is bounds-tested, a tap outside the frame is 0
__device__ __forceinline__ float tap(const float *pl, int H, int W, int yy, int xx) {
    return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? pl[(long long)yy * W + xx] : 0.f;
}

__device__ __forceinline__ float grid_sample(const GridSample &s, const float *pl, int H, int W) {
    return s.w.blend(tap(pl, H, W, s.y0, s.x0), tap(pl, H, W, s.y0, s.x0 + 1), tap(pl, H, W, s.y0 + 1, s.x0), tap(pl, H, W, s.y0 + 1, s.x0 + 1));
}

// ---- tap policy 2: the address is clamped into the frame, so that the load is unconditional (a caller issues many before it
// uses the first), and `in` says whether the tap counts: where it does not, the caller puts 0 in its place.
__device__ __forceinline__ long long clamped_tap(int H, int W, int yy, int xx, bool &in) {
    in = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W);
    const int cy = min(max(yy, 0), H - 1), cx = min(max(xx, 0), W - 1);
    return (long long)cy * W + cx;
}

struct ClampedTaps {          // (the four taps in blend()'s order)
    long long o[4];
    bool inx[2], iny[2];
    __device__ __forceinline__ bool in(int k) const { return iny[k >> 1] && inx[k & 1]; }
};

__device__ __forceinline__ ClampedTaps clamped_taps(const GridSample &s, int H, int W) {
    const int x0 = s.x0, y0 = s.y0;
    ClampedTaps t;
    t.inx[0] = x0 >= 0 && x0 < W; t.inx[1] = x0 + 1 >= 0 && x0 + 1 < W; t.iny[0] = y0 >= 0 && y0 < H; t.iny[1] = y0 + 1 >= 0 && y0 + 1 < H;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x0 + 1, 0), W - 1), cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y0 + 1, 0), H - 1);
    t.o[0] = (long long)cy0 * W + cx0; t.o[1] = (long long)cy0 * W + cx1; t.o[2] = (long long)cy1 * W + cx0; t.o[3] = (long long)cy1 * W + cx1;
    return t;
}

}  // namespace mftx

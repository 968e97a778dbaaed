// The ".flowouX16" quantisation of MFT/utils/io.py:495-512 (write) and :548-551 (read), per channel:
//   lb = min(x), ub = max(x)
//   q  = uint16(round_half_even( (x - lb) / (ub - lb) * 65535 ))     (all zeros if |ub - lb| < 1e-8)
//   x' = (float(q) / 65535) * (ub - lb) + lb
// in float32, operation by operation as numpy does it (the units that include this are compiled with -ffp-contract=off).
// Written ONCE for codec.hip (one channel per call) and trackstore.hip (four channels in one 8-byte word per pixel).
#pragma once
#include <hip/hip_runtime.h>

namespace mftx {

// (min, max) over a workgroup of THREADS lanes, the result in every lane.  Min and max do not depend on the order they are taken in.
template <int THREADS>
__device__ __forceinline__ void block_minmax(float &lo, float &hi, float *sh /* [2 * THREADS / 64] */) {
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
    for (int i = 1; i < THREADS / 64; ++i) { lo = fminf(lo, sh[2 * i]); hi = fmaxf(hi, sh[2 * i + 1]); }
    __syncthreads();
}

struct QuantU16 {
    float lo, range;
    bool flat;
    __device__ __forceinline__ static QuantU16 of(float lo, float hi) {
        const float range = hi - lo;
        return QuantU16{lo, range, fabsf(range) < 1e-8f};
    }
    __device__ __forceinline__ unsigned short enc(float v) const {
        if (flat) return 0;
        const float u = (v - lo) / range;
        return (unsigned short)rintf(u * 65535.f);
    }
    __device__ __forceinline__ float dec(unsigned q) const { return ((float)q / 65535.f) * range + lo; }
};

}  // namespace mftx

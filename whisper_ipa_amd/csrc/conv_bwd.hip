// Conv stem of the AudioEncoder in the fine-tune step (f32): the two elementwise passes that wipa_gemm cannot express.
//   conv1 (k3, p1) and conv2 (k3, s2, p1) run as GEMMs over overlapping rows (wipa_gemm_desc row groups) and keep their
//   PRE-activation values; their weight gradients are K-major GEMMs over the same overlapping views.  What is left:
//   - forward:  x = gelu(z2) + positional table                                   (stem_gelu_pos_kernel)
//   - backward: dz1 = gelu'(z1) * overlap-add of the three conv2 input-gradient taps (conv2_dx_kernel)
// Both are deterministic: every output element is written by exactly one thread, which adds its terms in a fixed order,
// so a clip's values do not depend on the batch it is computed in.
#include "wipa_common.h"

namespace {

// d/dz of the exact-erf GELU, the series of wipa_gelu_bwd (train.hip)
__device__ __forceinline__ float stem_gelu_grad(float z) {
    const float cdf = 0.5f * (1.0f + erf_fast(z * 0.70710678118654752440f));
    const float pdf = 0.3989422804014327f * __builtin_amdgcn_exp2f(-0.72134752044448170f * z * z);  // exp(-z^2/2)/sqrt(2 pi)
    return cdf + z * pdf;
}

// x[(b*N + t)*d + c] = gelu(z[(b*N + t)*d + c]) + pos[t*d + c]; one thread per four channels
__global__ __launch_bounds__(256) void stem_gelu_pos_kernel(const float* __restrict__ z, const float* __restrict__ pos,
                                                            float* __restrict__ x, int64_t n4, int N, int d4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t row = i / d4;
    const int c4 = (int)(i - row * d4);
    const int t = (int)(row % N);
    const f32x4 a = *reinterpret_cast<const f32x4*>(z + i * 4);
    const f32x4 p = *reinterpret_cast<const f32x4*>(pos + ((int64_t)t * d4 + c4) * 4);
    *reinterpret_cast<f32x4*>(x + i * 4) =
        f32x4{gelu_erf(a[0]) + p[0], gelu_erf(a[1]) + p[1], gelu_erf(a[2]) + p[2], gelu_erf(a[3]) + p[3]};
}

// conv2 (k3, s2, p1): position t reads the conv1 frames 2t-1, 2t, 2t+1 through taps 0, 1, 2.  Frame s therefore receives
//   s even:  tap 1 of t = s/2
//   s odd:   tap 2 of t = (s-1)/2, then tap 0 of t = (s+1)/2 when that position exists (the last odd frame has one tap only)
// rows 2N .. 2N + zero_rows - 1 of every clip are written as zero (the halo rows of the conv1 weight-gradient GEMM).
__global__ __launch_bounds__(256) void conv2_dx_kernel(const float* __restrict__ taps, int64_t taps_cs, const float* __restrict__ z1,
                                                       int64_t z1_cs, float* __restrict__ dz1, int64_t dz1_cs, int64_t n4, int N,
                                                       int rows, int d4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t row = i / d4;
    const int c = (int)(i - row * d4) * 4;
    const int b = (int)(row / rows);
    const int s = (int)(row - (int64_t)b * rows);
    const int d = d4 * 4;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (s < 2 * N) {
        const float* tp = taps + (int64_t)b * taps_cs + c;
        const int t = s >> 1;
        if ((s & 1) == 0) {
            g = *reinterpret_cast<const f32x4*>(tp + ((int64_t)t * 3 + 1) * d);
        } else {
            g = *reinterpret_cast<const f32x4*>(tp + ((int64_t)t * 3 + 2) * d);
            if (t + 1 < N) g += *reinterpret_cast<const f32x4*>(tp + ((int64_t)(t + 1) * 3) * d);
        }
        const f32x4 z = *reinterpret_cast<const f32x4*>(z1 + (int64_t)b * z1_cs + (int64_t)s * d + c);
        g = f32x4{g[0] * stem_gelu_grad(z[0]), g[1] * stem_gelu_grad(z[1]), g[2] * stem_gelu_grad(z[2]), g[3] * stem_gelu_grad(z[3])};
    }
    *reinterpret_cast<f32x4*>(dz1 + (int64_t)b * dz1_cs + (int64_t)s * d + c) = g;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int wipa_conv_stem_gelu_pos(const float* z, const float* pos, float* x, int B, int N, int d, wipa_stream_t stream) {
    WIPA_REQUIRE(z && pos && x && B > 0 && N > 0 && d > 0 && d % 4 == 0, "wipa_conv_stem_gelu_pos: bad arguments (B=%d N=%d d=%d)", B, N, d);
    WIPA_REQUIRE(aligned16(z) && aligned16(pos) && aligned16(x), "wipa_conv_stem_gelu_pos: pointers must be 16-byte aligned");
    const int64_t n4 = (int64_t)B * N * (d / 4);
    WIPA_REQUIRE((n4 + 255) / 256 < (int64_t)1 << 31, "wipa_conv_stem_gelu_pos: too many elements");
    hipLaunchKernelGGL(stem_gelu_pos_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, pos, x, n4, N, d / 4);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_conv2_dx(const float* taps, int64_t taps_clip_stride, const float* z1, int64_t z1_clip_stride, float* dz1,
                             int64_t dz1_clip_stride, int B, int N, int d, int zero_rows, wipa_stream_t stream) {
    WIPA_REQUIRE(taps && z1 && dz1 && B > 0 && N > 0 && d > 0 && d % 4 == 0 && zero_rows >= 0,
                 "wipa_conv2_dx: bad arguments (B=%d N=%d d=%d zero_rows=%d)", B, N, d, zero_rows);
    const int64_t rows = 2 * (int64_t)N + zero_rows;
    WIPA_REQUIRE(taps_clip_stride >= (int64_t)N * 3 * d && z1_clip_stride >= 2 * (int64_t)N * d && dz1_clip_stride >= rows * d,
                 "wipa_conv2_dx: a clip stride is shorter than the clip's rows");
    WIPA_REQUIRE(taps_clip_stride % 4 == 0 && z1_clip_stride % 4 == 0 && dz1_clip_stride % 4 == 0 && aligned16(taps) && aligned16(z1) &&
                     aligned16(dz1),
                 "wipa_conv2_dx: pointers and clip strides must be 16-byte aligned");
    const int64_t n4 = (int64_t)B * rows * (d / 4);
    WIPA_REQUIRE(rows < (1 << 30) && (n4 + 255) / 256 < (int64_t)1 << 31, "wipa_conv2_dx: too many elements");
    hipLaunchKernelGGL(conv2_dx_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, taps, taps_clip_stride, z1,
                       z1_clip_stride, dz1, dz1_clip_stride, n4, N, (int)rows, d / 4);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

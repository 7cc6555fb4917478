// Low-rank adapters (LoRA) on a frozen linear: y += gain * (x A^T) Bm^T with A [r, K], Bm [N, r], 4 <= r <= 64.
// Forward, backward and merge for the fine-tune step and for Whisper.set_adapter (include/wipa.h).
//
// Every contraction here has one side of length r, which the tile GEMMs of gemm.hip serve worst (K in whole 32-float steps,
// 128 x 128 tiles a few per cent full).  All of them run on the exact f32 MFMA (v_mfma_f32_16x16x4_f32: bit-equal to an fmaf
// chain), operands read from global memory straight into fragments, one wave per output tile, no float atomics:
//   rows kernel   out[M, r]  = scale * X[M, Kc] * W      eight waves of a workgroup cut Kc, summed in wave order through LDS
//                 (u = x A^T with W = A as stored;  du = gain * dy Bm with W = Bm as stored)
//   wide kernel   out[M, C] (+)= scale * S[M, r] * W     one wave per 16 rows x 64 columns, the whole of r in one go
//                 (y += gain * u Bm^T;  dx (+)= du A)
//   chunk kernel  P[chunk][r, C] = S[rows of the chunk, r]^T * G[rows of the chunk, C]   one wave per chunk x 64 columns
//                 (dB^T from u and dy;  dA from du and x), the chunks added in ascending order by the finish kernel.
//
// Two operand forms feed an MFMA whose lane l = (lr = l & 15, g = l >> 4) supplies A[row lr][k slot g] and B[k slot g][col lr]:
//   k-contiguous (the contraction index runs along a row of the array): one 16-byte load at [row lr][k0 + 4g ..] feeds four
//     MFMAs, step e taking element e, i.e. k = k0 + 4g + e -- the k order inside a 16-wide step is permuted, identically on
//     both sides of the product;
//   k-by-row (the contraction index is the array's row): one 16-byte load at [k0 + g][c0 + 4 lr ..] feeds four column tiles,
//     tile t holding the columns c0 + 4 lr + t, so that the results of a lane are again four consecutive floats.
#include "wipa_common.h"

namespace {

constexpr int ROWS_WAVES = 8;    // waves of a rows-kernel workgroup: 2048 rows are 128 workgroups, 1024 waves
constexpr int CHUNK_MIN_ROWS = 64;
constexpr int CHUNK_MAX = 128;

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// out[M, r] = scale * X[M, Kc] * W.  W_BY_ROW = false: W [r, Kc] (k-contiguous; u = x A^T).  true: W [Kc, r] (du = dy Bm).
// One workgroup per 16 rows; wave w takes the 16-wide k steps w, w + 8, ...; wave 0 adds the eight partial tiles in wave order.
template <bool W_BY_ROW>
__device__ __forceinline__ void rows_tile(const float* __restrict__ X, int64_t ldx, const float* __restrict__ W, float* __restrict__ out,
                                          int M, int Kc, int r, float scale, int m0, float* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int JT = (r + 15) >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row = m0 + lr;
    const bool rok = row < M;
    const float* xp = X + (int64_t)(rok ? row : 0) * ldx;
    for (int k0 = wave * 16; k0 < Kc; k0 += ROWS_WAVES * 16) {
        const int k = k0 + 4 * g;
        const bool kok = k < Kc;
        const f32x4 xf = ld4(xp + k, rok && kok);
        if (!W_BY_ROW) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < JT) {
                    const int j = 16 * t + lr;
                    const f32x4 wf = ld4(W + (int64_t)j * Kc + k, j < r && kok);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t] = mma(wf[e], xf[e], acc[t]);  // acc[t][e] = out[m0 + lr][16t + 4g + e]
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 wf = ld4(W + (int64_t)(k + e) * r + 4 * lr, kok && 4 * lr < r);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mma(xf[e], wf[t], acc[t]);  // acc[t][e'] = out[m0 + 4g + e'][4 lr + t]
            }
        }
    }
    if (wave != 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) lds[((wave - 1) * 16 + t * 4 + e) * 64 + lane] = acc[t][e];
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < ROWS_WAVES; ++w)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][e] += lds[((w - 1) * 16 + t * 4 + e) * 64 + lane];
    if (!W_BY_ROW) {
        if (rok)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int j = 16 * t + 4 * g;
                if (j < r) *reinterpret_cast<f32x4*>(out + (int64_t)row * r + j) = acc[t] * scale;
            }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + 4 * g + e;
            if (m < M && 4 * lr < r)
                *reinterpret_cast<f32x4*>(out + (int64_t)m * r + 4 * lr) = f32x4{acc[0][e], acc[1][e], acc[2][e], acc[3][e]} * scale;
        }
    }
}

// out[M, C] (+)= scale * S[M, r] * W on the 16 rows from m0 and the 64 columns from c0 (one wave).
// W_BY_ROW = false: W [C, r] (y += gain * u Bm^T).  true: W [r, C] (dx (+)= du A).  add: out is read and added to.
template <bool W_BY_ROW>
__device__ __forceinline__ void wide_tile(const float* __restrict__ S, const float* __restrict__ W, float* __restrict__ out, int64_t ldo,
                                          int M, int C, int r, float scale, bool add, int m0, int c0) {
    const int lane = threadIdx.x & 63;
    const int lr = lane & 15, g = lane >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row = m0 + lr;
    const bool rok = row < M;
    const float* sp = S + (int64_t)(rok ? row : 0) * r;
    for (int k0 = 0; k0 < r; k0 += 16) {
        const int k = k0 + 4 * g;
        const bool kok = k < r;
        const f32x4 sf = ld4(sp + k, rok && kok);
        if (!W_BY_ROW) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int n = c0 + 16 * t + lr;
                const f32x4 wf = ld4(W + (int64_t)n * r + k, n < C && kok);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = mma(wf[e], sf[e], acc[t]);  // acc[t][e] = out[m0 + lr][c0 + 16t + 4g + e]
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 wf = ld4(W + (int64_t)(k + e) * C + c0 + 4 * lr, kok && c0 + 4 * lr < C);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mma(sf[e], wf[t], acc[t]);  // acc[t][e'] = out[m0 + 4g + e'][c0 + 4 lr + t]
            }
        }
    }
    if (!W_BY_ROW) {
        if (rok)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int n = c0 + 16 * t + 4 * g;
                if (n < C) {
                    f32x4* o = reinterpret_cast<f32x4*>(out + (int64_t)row * ldo + n);
                    f32x4 v = acc[t] * scale;
                    if (add) v += *o;
                    *o = v;
                }
            }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + 4 * g + e, c = c0 + 4 * lr;
            if (m < M && c < C) {
                f32x4* o = reinterpret_cast<f32x4*>(out + (int64_t)m * ldo + c);
                f32x4 v = f32x4{acc[0][e], acc[1][e], acc[2][e], acc[3][e]} * scale;
                if (add) v += *o;
                *o = v;
            }
        }
    }
}

// P[r, C] (row stride C) = sum over the rows m in [mlo, mhi) of S[m, :r]^T G[m, c0 .. c0 + 63]  (one wave; rows ascending)
__device__ __forceinline__ void chunk_tile(const float* __restrict__ S, const float* __restrict__ G, int64_t ldg, float* __restrict__ P,
                                           int mlo, int mhi, int C, int r, int c0) {
    const int lane = threadIdx.x & 63;
    const int lr = lane & 15, g = lane >> 4;
    const int JT = (r + 15) >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t][s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c = c0 + 4 * lr;
    const bool cok = c < C;
#pragma unroll 2
    for (int m = mlo; m < mhi; m += 4) {
        const int mm = m + g;
        const bool ok = mm < mhi;
        const f32x4 gf = ld4(G + (int64_t)(ok ? mm : mlo) * ldg + c, ok && cok);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < JT) {
                const int j = 16 * t + lr;
                const float sv = (ok && j < r) ? S[(int64_t)mm * r + j] : 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[t][s] = mma(sv, gf[s], acc[t][s]);  // acc[t][s][e] = P[16t + 4g + e][c0 + 4 lr + s]
            }
        }
    }
    if (cok)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 16 * t + 4 * g + e;
                if (j < r) *reinterpret_cast<f32x4*>(P + (int64_t)j * C + c) = f32x4{acc[t][0][e], acc[t][1][e], acc[t][2][e], acc[t][3][e]};
            }
}

__global__ __launch_bounds__(ROWS_WAVES * 64) void lora_u_kernel(const float* x, int64_t ldx, const float* A, float* u, int M, int K, int r) {
    __shared__ float lds[(ROWS_WAVES - 1) * 16 * 64];
    rows_tile<false>(x, ldx, A, u, M, K, r, 1.f, blockIdx.x * 16, lds);
}

// blockIdx.x: 16 rows; blockIdx.y * 4 + wave: 64 columns
__global__ __launch_bounds__(256) void lora_y_kernel(const float* u, const float* Bm, float* y, int64_t ldy, int M, int N, int r, float gain) {
    const int c0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 64;
    if (c0 >= N) return;
    wide_tile<false>(u, Bm, y, ldy, M, N, r, gain, true, blockIdx.x * 16, c0);
}

// backward, first launch.  Workgroups [0, n_du): du = gain * dy Bm, 16 rows each (eight waves cut N).  The rest: eight waves each, one
// (chunk, 64 columns of N) task per wave: PB[chunk] = u^T dy over the chunk's rows.
__global__ __launch_bounds__(ROWS_WAVES * 64) void lora_bwd1_kernel(const float* dy, int64_t ldy, const float* u, const float* Bm, float* du,
                                                                    float* PB, int M, int N, int r, float gain, int n_du, int n_chunk,
                                                                    int chunk_rows) {
    __shared__ float lds[(ROWS_WAVES - 1) * 16 * 64];
    if ((int)blockIdx.x < n_du) {
        rows_tile<true>(dy, ldy, Bm, du, M, N, r, gain, blockIdx.x * 16, lds);
        return;
    }
    const int cb = (N + 63) / 64;
    const int task = ((int)blockIdx.x - n_du) * ROWS_WAVES + (threadIdx.x >> 6);
    if (task >= n_chunk * cb) return;
    const int ch = task / cb, c0 = (task % cb) * 64;
    const int mlo = ch * chunk_rows, mhi = min(M, mlo + chunk_rows);
    chunk_tile(u, dy, ldy, PB + (int64_t)ch * r * N, mlo, mhi, N, r, c0);
}

// backward, second launch (du is complete).  Tasks [0, n_pa): PA[chunk] = du^T x over the chunk's rows, one per wave.  Then, with dx:
// dx (+)= du A, one 16 x 64 tile per wave.
__global__ __launch_bounds__(256) void lora_bwd2_kernel(const float* du, const float* x, int64_t ldx, const float* A, float* PA, float* dx,
                                                        int64_t lddx, int accumulate_dx, int M, int K, int r, int n_chunk, int chunk_rows) {
    const int cb = (K + 63) / 64;
    const int n_pa = n_chunk * cb;
    int task = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task < n_pa) {
        const int ch = task / cb, c0 = (task % cb) * 64;
        const int mlo = ch * chunk_rows, mhi = min(M, mlo + chunk_rows);
        chunk_tile(du, x, ldx, PA + (int64_t)ch * r * K, mlo, mhi, K, r, c0);
        return;
    }
    task -= n_pa;
    if (dx == nullptr || task >= ((M + 15) / 16) * cb) return;
    wide_tile<true>(du, A, dx, lddx, M, K, r, 1.f, accumulate_dx != 0, (task / cb) * 16, (task % cb) * 64);
}

// backward, third launch: dA[j][k] = sum over chunks (ascending) of PA[chunk][j][k];  dB[n][j] = gain * the same sum of PB[chunk][j][n]
__global__ __launch_bounds__(256) void lora_finish_kernel(const float* PA, const float* PB, float* dA, float* dB, int K, int N, int r,
                                                          int n_chunk, float gain) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nA = (int64_t)r * K, nB = (int64_t)r * N;
    if (i < nA) {
        float s = 0.f;
        for (int c = 0; c < n_chunk; ++c) s += PA[c * nA + i];
        dA[i] = s;
    } else if (i < nA + nB) {
        const int64_t q = i - nA;
        float s = 0.f;
        for (int c = 0; c < n_chunk; ++c) s += PB[c * nB + q];
        dB[(q % N) * r + q / N] = gain * s;
    }
}

// W[n][k .. k+3] = cast(base + s * sum_j Bm[n][j] A[j][k]), j ascending: an fmaf chain from zero, one fmaf with the base, one rounding
template <typename T>
__global__ __launch_bounds__(256) void lora_merge_kernel(T* W, int64_t ldw, const T* base, int64_t ldb, const float* __restrict__ A,
                                                         const float* __restrict__ Bm, int N, int K, int r, float s) {
    const int k = (blockIdx.y * 64 + (threadIdx.x & 63)) * 4;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K || n >= N) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* bp = Bm + (int64_t)n * r;
    for (int j = 0; j < r; ++j) {
        const float b = bp[j];
        const f32x4 a = *reinterpret_cast<const f32x4*>(A + (int64_t)j * K + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(b, a[e], acc[e]);
    }
    const T* src = base + (int64_t)n * ldb + k;
    T* dst = W + (int64_t)n * ldw + k;
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = from_f32<T>(fmaf(s, acc[e], to_f32<T>(src[e])));
}

struct Chunks {
    int n, rows;
};
// row chunks of the sums over m: at least CHUNK_MIN_ROWS rows (a multiple of 4), at most CHUNK_MAX chunks
inline Chunks chunks_of(int M) {
    int n = (M + CHUNK_MIN_ROWS - 1) / CHUNK_MIN_ROWS;
    if (n > CHUNK_MAX) n = CHUNK_MAX;
    if (n < 1) n = 1;
    int rows = ((M + n - 1) / n + 3) / 4 * 4;
    return Chunks{(M + rows - 1) / rows, rows};
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

int check_shape(const char* who, int M, int K, int N, int r) {
    WIPA_REQUIRE(r >= 4 && r <= 64 && r % 4 == 0, "%s: r = %d: the rank is a multiple of 4 in 4..64", who, r);
    WIPA_REQUIRE(M > 0, "%s: M = %d: at least one row", who, M);
    WIPA_REQUIRE(K > 0 && K % 4 == 0, "%s: K = %d: a positive multiple of 4", who, K);
    WIPA_REQUIRE(N > 0 && N % 4 == 0, "%s: N = %d: a positive multiple of 4", who, N);
    return WIPA_OK;
}

#define LORA_PTR(who, p) WIPA_REQUIRE((p) != nullptr && aligned16(p), "%s: %s: a 16-byte aligned device pointer", who, #p)

}  // namespace

extern "C" size_t wipa_lora_workspace_bytes(int M, int K, int N, int r) {
    if (M <= 0 || K <= 0 || N <= 0 || r <= 0) return 0;
    const Chunks c = chunks_of(M);
    return sizeof(float) * ((size_t)M * r + (size_t)c.n * r * ((size_t)N + K));
}

extern "C" int wipa_lora_fwd(const float* x, int64_t ldx, const float* A, const float* Bm, float* y, int64_t ldy, float* u, int M, int K,
                             int N, int r, float gain, wipa_stream_t stream) {
    const char* who = "wipa_lora_fwd";
    if (int rc = check_shape(who, M, K, N, r)) return rc;
    LORA_PTR(who, x);
    LORA_PTR(who, A);
    LORA_PTR(who, Bm);
    LORA_PTR(who, y);
    LORA_PTR(who, u);
    WIPA_REQUIRE(ldx >= K && ldx % 4 == 0, "%s: ldx = %lld: a multiple of 4, at least K = %d", who, (long long)ldx, K);
    WIPA_REQUIRE(ldy >= N && ldy % 4 == 0, "%s: ldy = %lld: a multiple of 4, at least N = %d", who, (long long)ldy, N);
    hipStream_t s = (hipStream_t)stream;
    const int mb = (M + 15) / 16;
    hipLaunchKernelGGL(lora_u_kernel, dim3(mb), dim3(ROWS_WAVES * 64), 0, s, x, ldx, A, u, M, K, r);
    hipLaunchKernelGGL(lora_y_kernel, dim3(mb, (N + 255) / 256), dim3(256), 0, s, u, Bm, y, ldy, M, N, r, gain);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_lora_bwd(const float* dy, int64_t ldy, const float* x, int64_t ldx, const float* u, const float* A, const float* Bm,
                             float* dA, float* dB, float* dx, int64_t lddx, int accumulate_dx, int M, int K, int N, int r, float gain,
                             void* workspace, size_t workspace_bytes, wipa_stream_t stream) {
    const char* who = "wipa_lora_bwd";
    if (int rc = check_shape(who, M, K, N, r)) return rc;
    LORA_PTR(who, dy);
    LORA_PTR(who, x);
    LORA_PTR(who, u);
    LORA_PTR(who, A);
    LORA_PTR(who, Bm);
    LORA_PTR(who, dA);
    LORA_PTR(who, dB);
    LORA_PTR(who, workspace);
    WIPA_REQUIRE(ldy >= N && ldy % 4 == 0, "%s: ldy = %lld: a multiple of 4, at least N = %d", who, (long long)ldy, N);
    WIPA_REQUIRE(ldx >= K && ldx % 4 == 0, "%s: ldx = %lld: a multiple of 4, at least K = %d", who, (long long)ldx, K);
    if (dx) {
        WIPA_REQUIRE(aligned16(dx), "%s: dx: a 16-byte aligned device pointer (or NULL)", who);
        WIPA_REQUIRE(lddx >= K && lddx % 4 == 0, "%s: lddx = %lld: a multiple of 4, at least K = %d", who, (long long)lddx, K);
    }
    const size_t need = wipa_lora_workspace_bytes(M, K, N, r);
    WIPA_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes = %zu: wipa_lora_workspace_bytes(M, K, N, r) is %zu", who, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const Chunks c = chunks_of(M);
    float* du = (float*)workspace;
    float* PB = du + (size_t)M * r;
    float* PA = PB + (size_t)c.n * r * N;
    const int mb = (M + 15) / 16;
    const int tasks_b = c.n * ((N + 63) / 64);
    hipLaunchKernelGGL(lora_bwd1_kernel, dim3(mb + (tasks_b + ROWS_WAVES - 1) / ROWS_WAVES), dim3(ROWS_WAVES * 64), 0, s, dy, ldy, u, Bm, du,
                       PB, M, N, r, gain, mb, c.n, c.rows);
    const int kb = (K + 63) / 64;
    const int tasks_2 = c.n * kb + (dx ? mb * kb : 0);
    hipLaunchKernelGGL(lora_bwd2_kernel, dim3((tasks_2 + 3) / 4), dim3(256), 0, s, du, x, ldx, A, PA, dx, lddx, accumulate_dx, M, K, r, c.n,
                       c.rows);
    const int64_t n_out = (int64_t)r * ((int64_t)K + N);
    hipLaunchKernelGGL(lora_finish_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, PA, PB, dA, dB, K, N, r, c.n, gain);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_lora_merge(void* W, int64_t ldw, int dtype, const void* base, int64_t ld_base, const float* A, const float* Bm, int N,
                               int K, int r, float s, wipa_stream_t stream) {
    const char* who = "wipa_lora_merge";
    if (int rc = check_shape(who, 1, K, N, r)) return rc;
    WIPA_REQUIRE(dtype == WIPA_F32 || dtype == WIPA_BF16, "%s: dtype = %d: WIPA_F32 or WIPA_BF16", who, dtype);
    LORA_PTR(who, W);
    LORA_PTR(who, base);
    LORA_PTR(who, A);
    LORA_PTR(who, Bm);
    WIPA_REQUIRE(ldw >= K && ldw % 4 == 0, "%s: ldw = %lld: a multiple of 4, at least K = %d", who, (long long)ldw, K);
    WIPA_REQUIRE(ld_base >= K && ld_base % 4 == 0, "%s: ld_base = %lld: a multiple of 4, at least K = %d", who, (long long)ld_base, K);
    const dim3 grid((N + 3) / 4, (K + 255) / 256);
    if (dtype == WIPA_F32)
        hipLaunchKernelGGL((lora_merge_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (float*)W, ldw, (const float*)base, ld_base, A,
                           Bm, N, K, r, s);
    else
        hipLaunchKernelGGL((lora_merge_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, (__bf16*)W, ldw, (const __bf16*)base, ld_base,
                           A, Bm, N, K, r, s);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

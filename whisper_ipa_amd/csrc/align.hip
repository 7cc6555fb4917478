// K15: word-timestamp alignment.  Replaces the numeric core of openai-whisper timing.py find_alignment (which mlx_whisper ports;
// [UPSTREAM-UNVERIFIED], restated from memory and pinned to the local transformers copy of the same chain): the softmax over a
// window's own frames, the z-score over the token axis, the width-7 median filter, the sum over alignment heads, and the
// dynamic-time-warping recurrence with its backtrace -- for a whole batch of windows.
//
// Alignment weights, per decoder layer that has alignment heads (two launches):
//   align_stats_kernel    grid (64-frame chunk, head, clip): lane = frame, the lane keeps its key row in registers (64 floats), the four
//                         waves stride the token rows; per row one wave max and one wave sum of exp(s - chunk max) -> (m, s) per
//                         (clip, head, row, chunk).  Rows and chunks outside the clip's own n_tokens / n_frames are never touched.
//   align_weights_kernel  grid (58-frame tile, clip): 64 columns = 58 frames + a 3-frame halo on each side, reflected at both ends of
//                         the clip's OWN frame range, so a lane is a column and a wave needs no tail handling.  Per head, in the
//                         caller's list order: the chunk statistics of every row are merged in chunk order (M = max m_c, S = sum s_c
//                         exp(m_c - M)); w = exp(s - M) / S lands in LDS for all rows of the tile ([T][64] f32, 112 KB at T = 448);
//                         mean and population std per column over the clip's rows (two passes, four row groups added in a fixed
//                         order); z-score in place; the 7-tap median by a 13-exchange network; out[b][t][f] += median.  One thread
//                         owns a cell for every head, layers follow each other on the stream: the head sum has one fixed order and
//                         needs no atomics.  A reflected halo column recomputes its source frame's column, so its z-score is that
//                         frame's z-score bit for bit -- padding after the z-score, as upstream pads.
// The scores are plain f32 FMA chains over the 64 head dimensions in index order (bf16 operands are exact in f32; f32 operands are
// exact f32 products), the same function in both kernels, so exp(s - M) never exceeds 1.  VALU dot products, not MFMA: the work is
// T x 1500 x 64 per (head, clip) -- 1.5 % of the teacher-forced pass's FLOPs at whisper-small -- and a lane-owns-a-column layout
// makes the frame reflection, the per-clip ranges and the bit-equal independence from the rest of the batch trivial.  Nothing
// about the speed of this shape had been measured before it was written; tools/align_bench.py is where it is measured.
//
// Batched DTW (dtw_kernel): one wave per clip, lane l owns the strip of R = ceil(N / 64) token rows [l R, (l + 1) R).  The wave
// walks anti-diagonals: at step s lane l computes column j = s - l + 1 of its rows top to bottom.  Its upper neighbour's value
// comes from lane l - 1 with one __shfl_up per step, the diagonal one is the value shuffled in the step before, the left ones are
// its own registers.  cost[i][j] = (-x[i-1][j-1]) + c is ONE f32 add per cell with upstream's strict-less tie rule, so cost, trace
// and path equal the float32 restatement bit for bit whatever the evaluation order.  2-bit trace codes are packed 16 to a word
// in caller scratch (a lane flushes a row's word every 16 columns); lane 0 walks the backtrace, re-reading a word only when it
// leaves it, and the wave reverses the path in place.
#include <mutex>

#include "wipa_common.h"

namespace {

constexpr int TILE = 64, HALO = 3, INNER = TILE - 2 * HALO;  // 58 frames per weights tile
constexpr int CHUNK = 64;                                     // frames per statistics chunk
constexpr int WG = 256, WAVES = WG / 64;
constexpr int DTW_MAX_R = (WIPA_ALIGN_MAX_TOKENS + 63) / 64;  // 7 rows per lane
constexpr int TRACE_LD = (WIPA_ALIGN_MAX_FRAMES + 15) / 16;   // 94 words per token row

struct HeadList {
    int n;
    int h[WIPA_ALIGN_MAX_HEADS];
};

template <typename T>
__device__ __forceinline__ void load_row64(const T* p, float (&r)[64]) {
    const Vec16<T>* v = reinterpret_cast<const Vec16<T>*>(p);
    constexpr int E = Vec16<T>::EPL;
#pragma unroll
    for (int i = 0; i < 64 / E; ++i) {
        const Vec16<T> x = v[i];
#pragma unroll
        for (int e = 0; e < E; ++e) r[i * E + e] = x.get(e);
    }
}

// s = sum_d q[d] k[d], d ascending, one FMA per term.  q is wave-uniform.
template <typename T>
__device__ __forceinline__ float score64(const T* q, const float (&k)[64]) {
    const Vec16<T>* v = reinterpret_cast<const Vec16<T>*>(q);
    constexpr int E = Vec16<T>::EPL;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 64 / E; ++i) {
        const Vec16<T> x = v[i];
#pragma unroll
        for (int e = 0; e < E; ++e) acc = fmaf(x.get(e), k[i * E + e], acc);
    }
    return acc;
}

template <typename T>
__global__ __launch_bounds__(WG) void align_stats_kernel(const T* __restrict__ q, const T* __restrict__ k, int64_t k_bs, int64_t k_hs, int Tq,
                                                        int d, int Ta, HeadList heads, const int32_t* __restrict__ n_tokens,
                                                        const int32_t* __restrict__ n_frames, float2* __restrict__ stats, int n_chunks) {
    const int c = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nf = min(max(n_frames[b], 0), Ta), nt = min(max(n_tokens[b], 0), Tq);
    if (c * CHUNK >= nf) return;
    const int h = heads.h[j];
    const int f = c * CHUNK + lane;
    const bool valid = f < nf;
    float kr[64];
    load_row64(k + (int64_t)b * k_bs + (int64_t)h * k_hs + (int64_t)(valid ? f : 0) * 64, kr);
    for (int t = wave; t < nt; t += WAVES) {
        const float s = valid ? score64(q + ((int64_t)b * Tq + t) * d + h * 64, kr) : -INFINITY;
        const float m = wave_reduce_max(s);
        const float sum = wave_reduce_sum(valid ? expf(s - m) : 0.f);
        if (lane == 0) stats[(((int64_t)b * heads.n + j) * Tq + t) * n_chunks + c] = make_float2(m, sum);
    }
}

__device__ __forceinline__ void cswap(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}
// median of seven: 13 compare-exchanges (Devillard's opt_med7), the median ends in p[3]
__device__ __forceinline__ float median7(float (&p)[7]) {
    cswap(p[0], p[5]); cswap(p[0], p[3]); cswap(p[1], p[6]);
    cswap(p[2], p[4]); cswap(p[0], p[1]); cswap(p[3], p[5]);
    cswap(p[2], p[6]); cswap(p[2], p[3]); cswap(p[3], p[6]);
    cswap(p[4], p[5]); cswap(p[1], p[4]); cswap(p[1], p[3]);
    cswap(p[3], p[4]);
    return p[3];
}

template <typename T>
__global__ __launch_bounds__(WG) void align_weights_kernel(const T* __restrict__ q, const T* __restrict__ k, int64_t k_bs, int64_t k_hs, int Tq,
                                                          int d, int Ta, HeadList heads, const int32_t* __restrict__ n_tokens,
                                                          const int32_t* __restrict__ n_frames, const float2* __restrict__ stats,
                                                          int n_chunks, float* __restrict__ out, int64_t ld_out, float divisor) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tile = lds;                       // [Tq][TILE]
    float* row_m = tile + (size_t)Tq * TILE;  // [Tq]
    float* row_s = row_m + Tq;                // [Tq]
    float* part_a = row_s + Tq;               // [WAVES][TILE]
    float* part_b = part_a + WAVES * TILE;    // [WAVES][TILE]

    const int tl = blockIdx.x, b = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
    const int nf = min(max(n_frames[b], 0), Ta), nt = min(max(n_tokens[b], 0), Tq);
    const int f0 = tl * INNER;
    if (f0 >= nf || nt == 0) return;
    const bool filter = nf > HALO;  // upstream leaves an input of <= 3 frames unfiltered
    int fr = f0 - HALO + lane;      // this lane's frame, reflected into the clip's own range
    if (filter) {
        if (fr < 0) fr = -fr;
        if (fr >= nf) fr = 2 * (nf - 1) - fr;
    }
    const bool col_valid = fr >= 0 && fr < nf;  // false only for columns the tile's live cells never read
    const int live_chunks = (nf + CHUNK - 1) / CHUNK;
    const float inv_nt = 1.f / (float)nt;

    for (int j = 0; j < heads.n; ++j) {
        const int h = heads.h[j];
        for (int t = tid; t < nt; t += WG) {
            const float2* st = stats + (((int64_t)b * heads.n + j) * Tq + t) * n_chunks;
            float M = -INFINITY;
            for (int c = 0; c < live_chunks; ++c) M = fmaxf(M, st[c].x);
            float S = 0.f;
            for (int c = 0; c < live_chunks; ++c) S += st[c].y * expf(st[c].x - M);
            row_m[t] = M;
            row_s[t] = S;
        }
        float kr[64];
        load_row64(k + (int64_t)b * k_bs + (int64_t)h * k_hs + (int64_t)(col_valid ? fr : 0) * 64, kr);
        __syncthreads();
        for (int t = wave; t < nt; t += WAVES) {
            const float s = score64(q + ((int64_t)b * Tq + t) * d + h * 64, kr);
            tile[t * TILE + lane] = col_valid ? expf(s - row_m[t]) / row_s[t] : 0.f;
        }
        __syncthreads();
        {  // column statistics over the clip's rows: the wave is the row group, the lane the column
            float a = 0.f;
            for (int t = wave; t < nt; t += WAVES) a += tile[t * TILE + lane];
            part_a[wave * TILE + lane] = a;
            __syncthreads();
            const float mean = (((part_a[lane] + part_a[TILE + lane]) + part_a[2 * TILE + lane]) + part_a[3 * TILE + lane]) * inv_nt;
            float v = 0.f;
            for (int t = wave; t < nt; t += WAVES) {
                const float dlt = tile[t * TILE + lane] - mean;
                v = fmaf(dlt, dlt, v);
            }
            part_b[wave * TILE + lane] = v;
            __syncthreads();
            const float var = (((part_b[lane] + part_b[TILE + lane]) + part_b[2 * TILE + lane]) + part_b[3 * TILE + lane]) * inv_nt;
            const float sd = sqrtf(var);
            for (int t = wave; t < nt; t += WAVES) tile[t * TILE + lane] = (tile[t * TILE + lane] - mean) / sd;
        }
        __syncthreads();
        const bool last = divisor != 0.f && j == heads.n - 1;
        for (int idx = tid; idx < nt * INNER; idx += WG) {
            const int t = idx / INNER, c = idx - t * INNER;
            if (f0 + c >= nf) continue;
            const float* p = tile + t * TILE + c;  // columns c .. c + 6 are frames f0 + c - 3 .. f0 + c + 3
            float v;
            if (filter) {
                float w[7] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
                v = median7(w);
            } else {
                v = p[HALO];
            }
            float* o = out + ((int64_t)b * Tq + t) * ld_out + f0 + c;
            const float acc = *o + v;
            *o = last ? acc / divisor : acc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(WG) void token_probs_kernel(const float* __restrict__ logits, int64_t ldl, int row0, const int32_t* __restrict__ tokens,
                                                        const int32_t* __restrict__ n_tokens, int Tq, int eot, float* __restrict__ probs) {
    __shared__ float red[WAVES];
    const int m = row0 + blockIdx.x, b = m / Tq, t = m - b * Tq;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tok = t + 1 < min(n_tokens[b], Tq) ? tokens[m + 1] : -1;
    if (tok < 0 || tok >= eot) {  // uniform over the block
        if (tid == 0) probs[m] = 0.f;
        return;
    }
    const float* row = logits + (int64_t)blockIdx.x * ldl;
    float mx = -INFINITY;
    for (int v = tid; v < eot; v += WG) mx = fmaxf(mx, row[v]);
    mx = wave_reduce_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int v = tid; v < eot; v += WG) sum += expf(row[v] - mx);
    sum = wave_reduce_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) probs[m] = expf(row[tok] - mx) / (((red[0] + red[1]) + red[2]) + red[3]);
}

__global__ __launch_bounds__(64) void dtw_kernel(const float* __restrict__ mat, int64_t mat_bs, int64_t ld, int first_row, int rows_avail,
                                                const int32_t* __restrict__ n_rows, const int32_t* __restrict__ n_cols,
                                                uint32_t* __restrict__ trace_all, int64_t trace_bs, int32_t* __restrict__ text_idx,
                                                int32_t* __restrict__ time_idx, int64_t ld_path, int32_t* __restrict__ path_len) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = n_rows[b], M = n_cols[b];
    // the entry point has checked the host copies; a device array that disagrees with them gets an empty path, never a wild index
    if (N <= 0 || M <= 0 || N > WIPA_ALIGN_MAX_TOKENS || M > WIPA_ALIGN_MAX_FRAMES || first_row + N > rows_avail || N + M > ld_path ||
        (int64_t)N * TRACE_LD > trace_bs) {
        if (lane == 0) path_len[b] = 0;
        return;
    }
    const int R = (N + 63) >> 6;
    const int i0 = lane * R;  // first row of the strip, 0-based
    const float* x = mat + (int64_t)b * mat_bs + (int64_t)(first_row + i0) * ld;
    uint32_t* trace = trace_all + (int64_t)b * trace_bs;
    float prev[DTW_MAX_R];
    uint32_t acc[DTW_MAX_R];
#pragma unroll
    for (int r = 0; r < DTW_MAX_R; ++r) {
        prev[r] = INFINITY;  // cost[i][0], i >= 1
        acc[r] = 0u;
    }
    float bottom = INFINITY;                     // the strip's last row at the column computed last
    float diag_in = lane == 0 ? 0.f : INFINITY;  // cost[row above the strip][j - 1]: cost[0][0] = 0 for lane 0's first column
    const int steps = M + (N - 1) / R;
#pragma unroll 2
    for (int s = 0; s < steps; ++s) {
        float up_in = __shfl_up(bottom, 1, 64);  // cost[row above the strip][j]: lane l - 1 computed column j one step ago
        if (lane == 0) up_in = INFINITY;         // cost[0][j], j >= 1
        const int j = s - lane + 1;
        if (j >= 1 && j <= M && i0 < N) {
            float above_old = diag_in, above_new = up_in;
            const int sh = 2 * ((j - 1) & 15);
            const bool flush = (j & 15) == 0 || j == M;
#pragma unroll
            for (int r = 0; r < DTW_MAX_R; ++r) {
                if (r < R && i0 + r < N) {
                    const float c0 = above_old, c1 = above_new, c2 = prev[r];
                    float c;
                    uint32_t code;
                    if (c0 < c1 && c0 < c2) {
                        c = c0; code = 0u;
                    } else if (c1 < c0 && c1 < c2) {
                        c = c1; code = 1u;
                    } else {
                        c = c2; code = 2u;
                    }
                    const float v = (-x[(int64_t)r * ld + (j - 1)]) + c;
                    above_old = prev[r];
                    above_new = v;
                    prev[r] = v;
                    acc[r] |= code << sh;
                    if (flush) {
                        trace[(int64_t)(i0 + r) * TRACE_LD + ((j - 1) >> 4)] = acc[r];
                        acc[r] = 0u;
                    }
                }
            }
            bottom = above_new;
            diag_in = up_in;
        }
    }
    // lane 0 reads what all lanes wrote: one wave, one CU, one L1 -- the stores only have to have left the wave
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    int32_t* text = text_idx + (int64_t)b * ld_path;
    int32_t* time = time_idx + (int64_t)b * ld_path;
    int len = 0;
    if (lane == 0) {
        int i = N, j = M, held = -1;
        uint32_t word = 0u;
        while ((i > 0 || j > 0) && len < N + M) {
            text[len] = i - 1;
            time[len] = j - 1;
            ++len;
            uint32_t code;
            if (i == 0) {
                code = 2u;
            } else if (j == 0) {
                code = 1u;
            } else {
                const int at = (i - 1) * TRACE_LD + ((j - 1) >> 4);
                if (at != held) {
                    word = trace[at];
                    held = at;
                }
                code = (word >> (2 * ((j - 1) & 15))) & 3u;
            }
            if (code == 0u) {
                --i; --j;
            } else if (code == 1u) {
                --i;
            } else {
                --j;
            }
        }
        path_len[b] = len;
    }
    len = __shfl(len, 0, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (int a = lane; a < len / 2; a += 64) {  // the backtrace ran from the end: reverse in place
        const int z = len - 1 - a;
        const int32_t ta = text[a], tz = text[z], ma = time[a], mz = time[z];
        text[a] = tz; text[z] = ta;
        time[a] = mz; time[z] = ma;
    }
}

size_t weights_lds_bytes(int T) { return ((size_t)T * TILE + 2 * (size_t)T + 2 * WAVES * TILE) * sizeof(float); }

int weights_attrs() {
    static std::once_flag once;  // the limit is a property of the loaded code object: set once per process
    static hipError_t err = hipSuccess;
    std::call_once(once, [] {
        const int lds = (int)weights_lds_bytes(WIPA_ALIGN_MAX_TOKENS);
        const void* fns[2] = {reinterpret_cast<const void*>(&align_weights_kernel<float>), reinterpret_cast<const void*>(&align_weights_kernel<__bf16>)};
        for (const void* f : fns) {
            const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) err = e;
        }
    });
    WIPA_CHECK_HIP(err);
    return WIPA_OK;
}

}  // namespace

extern "C" size_t wipa_align_weights_scratch_bytes(int B, int T, int n_heads, int n_audio_ctx) {
    if (B <= 0 || T <= 0 || n_heads <= 0 || n_audio_ctx <= 0) return 0;
    return (size_t)B * n_heads * T * ((n_audio_ctx + CHUNK - 1) / CHUNK) * sizeof(float2);
}

extern "C" int wipa_align_weights(const void* q, const void* k, int64_t k_bs, int64_t k_hs, int dtype, int B, int T, int d, int n_audio_ctx,
                                  const int32_t* heads_host, int n_heads, const int32_t* n_tokens, const int32_t* n_frames, void* scratch,
                                  size_t scratch_bytes, float* out, int64_t ld_out, float divisor, wipa_stream_t s) {
    WIPA_REQUIRE(q && k && heads_host && n_tokens && n_frames && scratch && out, "wipa_align_weights: null pointer");
    WIPA_REQUIRE(dtype == WIPA_F32 || dtype == WIPA_BF16, "wipa_align_weights: dtype %d", dtype);
    WIPA_REQUIRE(B > 0 && T > 0 && T <= WIPA_ALIGN_MAX_TOKENS, "wipa_align_weights: B=%d T=%d (T at most %d)", B, T, WIPA_ALIGN_MAX_TOKENS);
    WIPA_REQUIRE(n_audio_ctx > 0 && n_audio_ctx <= WIPA_ALIGN_MAX_FRAMES && ld_out >= n_audio_ctx,
                 "wipa_align_weights: n_audio_ctx=%d (at most %d) ld_out=%lld", n_audio_ctx, WIPA_ALIGN_MAX_FRAMES, (long long)ld_out);
    WIPA_REQUIRE(d > 0 && d % 64 == 0, "wipa_align_weights: d=%d is not a multiple of the head width 64", d);
    WIPA_REQUIRE(n_heads >= 1 && n_heads <= WIPA_ALIGN_MAX_HEADS, "wipa_align_weights: %d heads (1..%d a layer)", n_heads, WIPA_ALIGN_MAX_HEADS);
    WIPA_REQUIRE(k_hs >= (int64_t)n_audio_ctx * 64 && k_bs >= k_hs * (d / 64), "wipa_align_weights: key strides %lld / %lld", (long long)k_bs,
                 (long long)k_hs);
    HeadList hl;
    hl.n = n_heads;
    for (int j = 0; j < WIPA_ALIGN_MAX_HEADS; ++j) hl.h[j] = 0;
    for (int j = 0; j < n_heads; ++j) {
        WIPA_REQUIRE(heads_host[j] >= 0 && heads_host[j] < d / 64, "wipa_align_weights: head %d of %d", heads_host[j], d / 64);
        hl.h[j] = heads_host[j];
    }
    const size_t need = wipa_align_weights_scratch_bytes(B, T, n_heads, n_audio_ctx);
    WIPA_REQUIRE(scratch_bytes >= need, "wipa_align_weights: scratch too small (%zu < %zu)", scratch_bytes, need);
    {
        const int rc = weights_attrs();
        if (rc != WIPA_OK) return rc;
    }
    const int n_chunks = (n_audio_ctx + CHUNK - 1) / CHUNK, n_tiles = (n_audio_ctx + INNER - 1) / INNER;
    const size_t lds = weights_lds_bytes(T);
    float2* st = (float2*)scratch;
    if (dtype == WIPA_F32) {
        hipLaunchKernelGGL(align_stats_kernel<float>, dim3(n_chunks, n_heads, B), dim3(WG), 0, (hipStream_t)s, (const float*)q, (const float*)k, k_bs,
                           k_hs, T, d, n_audio_ctx, hl, n_tokens, n_frames, st, n_chunks);
        WIPA_LAUNCH_CHECK();
        hipLaunchKernelGGL(align_weights_kernel<float>, dim3(n_tiles, B), dim3(WG), lds, (hipStream_t)s, (const float*)q, (const float*)k, k_bs, k_hs,
                           T, d, n_audio_ctx, hl, n_tokens, n_frames, st, n_chunks, out, ld_out, divisor);
    } else {
        hipLaunchKernelGGL(align_stats_kernel<__bf16>, dim3(n_chunks, n_heads, B), dim3(WG), 0, (hipStream_t)s, (const __bf16*)q, (const __bf16*)k,
                           k_bs, k_hs, T, d, n_audio_ctx, hl, n_tokens, n_frames, st, n_chunks);
        WIPA_LAUNCH_CHECK();
        hipLaunchKernelGGL(align_weights_kernel<__bf16>, dim3(n_tiles, B), dim3(WG), lds, (hipStream_t)s, (const __bf16*)q, (const __bf16*)k, k_bs,
                           k_hs, T, d, n_audio_ctx, hl, n_tokens, n_frames, st, n_chunks, out, ld_out, divisor);
    }
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_token_probs(const float* logits, int64_t ldl, int row0, int rows, const int32_t* tokens, const int32_t* n_tokens, int B, int T,
                                int eot, float* probs, wipa_stream_t s) {
    WIPA_REQUIRE(logits && tokens && n_tokens && probs, "wipa_token_probs: null pointer");
    WIPA_REQUIRE(B > 0 && T > 0 && rows > 0 && row0 >= 0 && (int64_t)row0 + rows <= (int64_t)B * T, "wipa_token_probs: rows [%d, %d + %d) of %d x %d",
                 row0, row0, rows, B, T);
    WIPA_REQUIRE(eot >= 1 && ldl >= eot, "wipa_token_probs: eot=%d ldl=%lld", eot, (long long)ldl);
    hipLaunchKernelGGL(token_probs_kernel, dim3(rows), dim3(WG), 0, (hipStream_t)s, logits, ldl, row0, tokens, n_tokens, T, eot, probs);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" size_t wipa_dtw_scratch_bytes(int B, int max_rows) {
    if (B <= 0 || max_rows <= 0) return 0;
    return (size_t)B * max_rows * TRACE_LD * sizeof(uint32_t);
}

extern "C" int wipa_dtw_batch(const float* matrix, int64_t batch_stride, int64_t ld, int first_row, int rows_avail, const int32_t* n_rows,
                              const int32_t* n_cols, const int32_t* n_rows_host, const int32_t* n_cols_host, int B, void* scratch,
                              size_t scratch_bytes, int32_t* text_idx, int32_t* time_idx, int64_t ld_path, int32_t* path_len, wipa_stream_t s) {
    WIPA_REQUIRE(B >= 0, "wipa_dtw_batch: B %d is negative", B);
    if (B == 0) return WIPA_OK;
    WIPA_REQUIRE(n_rows_host && n_cols_host, "wipa_dtw_batch: null host sizes");
    WIPA_REQUIRE(first_row >= 0 && rows_avail >= 0, "wipa_dtw_batch: first_row %d rows_avail %d", first_row, rows_avail);
    int max_rows = 0;
    for (int b = 0; b < B; ++b) {
        const int N = n_rows_host[b], M = n_cols_host[b];
        WIPA_REQUIRE(N >= 0 && N <= WIPA_ALIGN_MAX_TOKENS, "wipa_dtw_batch: clip %d: %d token rows (0..%d)", b, N, WIPA_ALIGN_MAX_TOKENS);
        if (N == 0) continue;
        WIPA_REQUIRE(M >= 1 && M <= WIPA_ALIGN_MAX_FRAMES, "wipa_dtw_batch: clip %d: %d frames (1..%d)", b, M, WIPA_ALIGN_MAX_FRAMES);
        WIPA_REQUIRE(first_row + N <= rows_avail, "wipa_dtw_batch: clip %d: rows [%d, %d) of %d", b, first_row, first_row + N, rows_avail);
        WIPA_REQUIRE(M <= ld && (int64_t)N + M <= ld_path, "wipa_dtw_batch: clip %d: %d x %d exceeds ld %lld or the path room %lld", b, N, M,
                     (long long)ld, (long long)ld_path);
        max_rows = N > max_rows ? N : max_rows;
    }
    WIPA_REQUIRE(matrix && n_rows && n_cols && text_idx && time_idx && path_len, "wipa_dtw_batch: null pointer");
    WIPA_REQUIRE(batch_stride >= (int64_t)rows_avail * ld, "wipa_dtw_batch: batch stride %lld below %d rows of %lld", (long long)batch_stride,
                 rows_avail, (long long)ld);
    WIPA_REQUIRE(max_rows == 0 || (scratch && scratch_bytes >= wipa_dtw_scratch_bytes(B, max_rows)), "wipa_dtw_batch: scratch too small (%zu < %zu)",
                 scratch_bytes, wipa_dtw_scratch_bytes(B, max_rows));
    const int64_t trace_bs = max_rows == 0 ? 0 : (int64_t)(scratch_bytes / sizeof(uint32_t) / B);
    hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(64), 0, (hipStream_t)s, matrix, batch_stride, ld, first_row, rows_avail, n_rows, n_cols,
                       (uint32_t*)scratch, trace_bs, text_idx, time_idx, ld_path, path_len);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

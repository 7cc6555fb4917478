// The row routines the decode step's tails share: 16-byte row loads / stores, the (value, lowest column) arg-max, the prompt-walk tests,
// the next step's input row (embedding + first LayerNorm) and the tails' read of the position.  Moved here, text unchanged, from
// elementwise.hip when the beam tail (beam.hip) became their second user; both files include it inside their own translation unit, so
// every kernel of elementwise.hip compiles to the instructions it had.
#pragma once
#include "wipa_common.h"

namespace {

template <typename TI>
__device__ __forceinline__ f32x4 ld4(const TI* p);
template <>
__device__ __forceinline__ f32x4 ld4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <>
__device__ __forceinline__ f32x4 ld4<__bf16>(const __bf16* p) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <typename TO>
__device__ __forceinline__ void st4(TO* p, f32x4 v);
template <>
__device__ __forceinline__ void st4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <>
__device__ __forceinline__ void st4<__bf16>(__bf16* p, f32x4 v) {
    *reinterpret_cast<bf16x4*>(p) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
}

// ------------------------------------------------------------------ block reductions
struct MaxIdx {
    float v;
    int i;
};
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) {
    // larger value wins; on ties the LOWER index (argmax returns the first maximum)
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}
__device__ __forceinline__ MaxIdx wave_argmax(MaxIdx m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MaxIdx other;
        other.v = __shfl_xor(m.v, o, 64);
        other.i = __shfl_xor(m.i, o, 64);
        m = better(m, other);
    }
    return m;
}

constexpr int GS_THREADS = 1024;
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int GS_MAXQ = 16;  // the register-resident row: 16 quads per thread, V <= 65536 (every Whisper vocabulary)

// the prompt walk: the column after p holds a prompt token already, the step picks nothing; and the mask of a column that is picked
__device__ __forceinline__ bool in_prompt(int p, int n_init) { return p + 1 < n_init; }
__device__ __forceinline__ const float* step_mask(int p, int n_init, const float* mask_first, const float* mask_always) {
    return (p + 1 == n_init) ? mask_first : mask_always;
}

__device__ __forceinline__ f32x4 emb_row_ld4(const void* emb, int emb_dtype, const float* emb_scale, int tok, int D, int c) {
    if (emb_dtype == WIPA_F32) return *reinterpret_cast<const f32x4*>((const float*)emb + (int64_t)tok * D + c);
    if (emb_dtype == WIPA_BF16) return ld4<__bf16>((const __bf16*)emb + (int64_t)tok * D + c);
    // e4m3fn codes x per-row scale, rounded to bf16 like embed_fp8_kernel
    const unsigned int u = *reinterpret_cast<const unsigned int*>((const unsigned char*)emb + (int64_t)tok * D + c);
    const float sc = emb_scale[tok];
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, true);
    return f32x4{(float)(__bf16)(lo[0] * sc), (float)(__bf16)(lo[1] * sc), (float)(__bf16)(hi[0] * sc), (float)(__bf16)(hi[1] * sc)};
}

// threads 0..255 of the workgroup embed token `tok` at position `pp` into xr[D] and write LayerNorm(xr) to yr[D]; EVERY thread
// of the workgroup must call it (three workgroup barriers); s_red: 4 floats of LDS
template <typename TO>
__device__ __forceinline__ void row_embed_layernorm(int tid, int tok, int pp, const void* emb, int emb_dtype, const float* emb_scale,
                                                    const float* pos_emb, float* xr, const float* w, const float* b, TO* yr, int D,
                                                    float eps, float* s_red) {
    const int lane = tid & 63, wave = tid >> 6;
    const bool active = tid < 256;
    f32x4 v[2], ww[2], bb[2];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid * 4 + 1024 * i;
        v[i] = ww[i] = bb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (active && c < D) {
            const f32x4 a = emb_row_ld4(emb, emb_dtype, emb_scale, tok, D, c);
            const f32x4 q = *reinterpret_cast<const f32x4*>(pos_emb + (int64_t)pp * D + c);
            ww[i] = *reinterpret_cast<const f32x4*>(w + c);
            bb[i] = *reinterpret_cast<const f32x4*>(b + c);
            v[i] = a + q;
            *reinterpret_cast<f32x4*>(xr + c) = v[i];
            sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    sum = wave_reduce_sum(sum);
    if (active && lane == 0) s_red[wave] = sum;
    __syncthreads();
    const float mean = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / (float)D;
    __syncthreads();
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (active && c < D) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                sq += d * d;
            }
        }
    }
    sq = wave_reduce_sum(sq);
    if (active && lane == 0) s_red[wave] = sq;
    __syncthreads();
    const float rstd = rsqrtf(((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (active && c < D) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * ww[i][e] + bb[i][e];
            st4<TO>(yr + c, o);
        }
    }
}

// The tails' read of the position.  volatile: ONE load per thread at the kernel's start, never re-materialised by the compiler after
// a barrier -- the last workgroup to arrive overwrites *pos while slower workgroups are still between their barriers and their exit
// (the sampling tails' draw counter reads this value live, too)
__device__ __forceinline__ int tail_pos(const int32_t* pos) { return *(volatile const int32_t*)pos; }

struct RulesDev {
    int tb, nt, max_init;  // timestamp_begin, <|notimestamps|>, max_initial_timestamp_index (< 0: no cap)
};

}  // namespace

// The streaming softmax of the one-query-row attention kernels (VALU, Vec16<T> lanes), spelled once.
//
// decode_attn_kernel, decode_attn_multi_kernel (attention.hip) and the two cross-block kernels (decode_fused.hip) must give
// bit-identical results for the same query and cache (the fused decode step against the unfused one, the prompt prefill
// against the stepwise prompt, the LDS-staged stream against the plain one): they do because every one of them expands the
// SAME text below, in the same order.  Change the arithmetic here and every path changes with it.
//
// Decomposition shared by all users: a 64-dim key row is LPK = 64 / EPL lanes of 16 bytes (lane c of the row holds dims
// c*EPL ..), G rows ride in one wave-wide load (lane group g), U such groups are in flight per step, the lane groups are merged
// by shuffles at the end and, where four waves split the keys, the waves are merged through LDS.
//
// The load is a function; the step and the merges are MACROS over the caller's locals: as __forceinline__ functions they
// compiled to different code (commuted v_pk_fma_f32 operands, other registers) in decode_attn_kernel / decode_attn_multi_kernel,
// as text they leave every kernel as it was.  The macros expect EPL, LPK, G (constexpr) and g, Tk (lane group, key count) in scope.
#pragma once
#include "wipa_common.h"

constexpr float NEG_BIG = -1.0e30f;   // score of a masked key; running max before the first key
constexpr float NEG_TEST = -1.0e29f;  // "is masked" threshold: such a key's probability is an exact 0, not exp(-huge)

// Key or value row min(t, last) of a head (rows rs elements apart; base already points at this lane's 16 bytes).  Rows past the
// end are clamped, not skipped: the load stays unconditional and the step masks the score.  NT: non-temporal, for a cache that
// a step reads exactly once (the cached cross K / V).
template <bool NT = true, typename T>
__device__ __forceinline__ Vec16<T> load_row_clamped(const T* base, int t, int last, int64_t rs) {
    Vec16<T> r;
    if constexpr (NT) {
        typedef decltype(r.v) VT;
        r.v = __builtin_nontemporal_load(reinterpret_cast<const VT*>(base + (int64_t)min(t, last) * rs));
    } else {
        r = *reinterpret_cast<const Vec16<T>*>(base + (int64_t)min(t, last) * rs);
    }
    return r;
}

// One step: the scores of the lane's U_ keys t0 + u*G + g against QF, then the online-softmax update of (M, L, ACC[EPL]).
#define WIPA_STREAM_STEP(U_, QF, KA, VA, t0, M, L, ACC)                                                      \
    do {                                                                                                     \
        float s[U_];                                                                                         \
        _Pragma("unroll") for (int u = 0; u < U_; ++u) {                                                     \
            float a = 0.f;                                                                                   \
            _Pragma("unroll") for (int e = 0; e < EPL; ++e) a = fmaf(QF[e], KA[u].get(e), a);                \
            _Pragma("unroll") for (int o = 1; o < LPK; o <<= 1) a += __shfl_xor(a, o, 64);                   \
            s[u] = ((t0) + u * G + g < Tk) ? a : NEG_BIG;                                                    \
        }                                                                                                    \
        float m_new = M;                                                                                     \
        _Pragma("unroll") for (int u = 0; u < U_; ++u) m_new = fmaxf(m_new, s[u]);                           \
        const float alpha = __expf(M - m_new);                                                               \
        L *= alpha;                                                                                          \
        _Pragma("unroll") for (int e = 0; e < EPL; ++e) ACC[e] *= alpha;                                     \
        _Pragma("unroll") for (int u = 0; u < U_; ++u) {                                                     \
            const float pr = (s[u] <= NEG_TEST) ? 0.f : __expf(s[u] - m_new);                                \
            L += pr;                                                                                         \
            _Pragma("unroll") for (int e = 0; e < EPL; ++e) ACC[e] = fmaf(pr, VA[u].get(e), ACC[e]);         \
        }                                                                                                    \
        M = m_new;                                                                                           \
    } while (0)

// Merge the partial softmax states (M, L, ACC[N]) of the lanes that differ in the lane-index bits FROM .. TO/2.
#define WIPA_LANE_MERGE(FROM, TO, N, M, L, ACC)                                                              \
    _Pragma("unroll") for (int o = (FROM); o < (TO); o <<= 1) {                                              \
        const float m_o = __shfl_xor(M, o, 64);                                                              \
        const float l_o = __shfl_xor(L, o, 64);                                                              \
        const float m_n = fmaxf(M, m_o);                                                                     \
        const float a = __expf(M - m_n), bsc = __expf(m_o - m_n);                                            \
        L = L * a + l_o * bsc;                                                                               \
        _Pragma("unroll") for (int e = 0; e < (N); ++e) ACC[e] = ACC[e] * a + __shfl_xor(ACC[e], o, 64) * bsc; \
        M = m_n;                                                                                             \
    }

// Four waves split the keys of one query: every wave leaves its merged state in LDS (S_ACC[4][64], S_M[4], S_L[4]) ...
#define WIPA_WAVE_MERGE_STORE(S_ACC, S_M, S_L, M, L, ACC)                                                    \
    if (lane < LPK) {                                                                                        \
        _Pragma("unroll") for (int e = 0; e < EPL; ++e) S_ACC[wave][c * EPL + e] = ACC[e];                   \
        if (lane == 0) {                                                                                     \
            S_M[wave] = M;                                                                                   \
            S_L[wave] = L;                                                                                   \
        }                                                                                                    \
    }
// ... and, after a barrier, one thread per output dim dd combines the four in wave order and stores the result to DST.
#define WIPA_WAVE_MERGE_OUT(S_ACC, S_M, S_L, dd, DST)                                                        \
    do {                                                                                                     \
        const float mm = fmaxf(fmaxf(S_M[0], S_M[1]), fmaxf(S_M[2], S_M[3]));                                \
        float num = 0.f, den = 0.f;                                                                          \
        _Pragma("unroll") for (int w = 0; w < 4; ++w) {                                                      \
            const float sc = __expf(S_M[w] - mm);                                                            \
            num += S_ACC[w][dd] * sc;                                                                        \
            den += S_L[w] * sc;                                                                              \
        }                                                                                                    \
        DST = from_f32<T>(num / den);                                                                        \
    } while (0)

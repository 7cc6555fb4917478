// Attention kernels (head_dim = 64; q and k arrive pre-scaled by 64^-0.25 each).
//   * attn_generic_kernel  : f32-math flash-style kernel for any (Tq, Tk), causal or not,
//                            T in {f32, bf16} storage.  Parity path + decoder self-attn.
//   * flash_enc_bf16_kernel: K5 encoder self-attention on bf16 MFMA 32x32x16 (swapped
//                            QK^T so a P row is lane-local; P feeds PV from registers).
//   * decode_cross_attn_kernel: K11, one query per (b,h) against the cached cross K/V,
//                            HBM-bound streaming with 16-byte coalesced loads.
// Replaces MultiHeadAttention.qkv_attention of mlx_whisper.whisper
// (call sites scripts/train_whisper_ipa.py:223,232; scripts/transcribe_single.py:54-55).
#include <cstring>

#include "attn_stream.h"
#include "wipa_common.h"

namespace {

// =============================================================================
// generic attention, f32 math
// =============================================================================
struct AttnParams {
    const char* q;
    const char* k;
    const char* v;
    char* out;
    const int32_t* tk_dev;
    const int32_t* q_row_dev;
    float* lse;  // optional [B, H, Tq]: log-sum-exp of every score row (saved for the backward pass)
    int64_t q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, v_bs, v_rs, v_hs, o_bs, o_rs, o_hs;
    int Tq, Tk, causal, H;
};

// Ragged prompts (left-padded rows; wipa_decode_attn_ragged, wipa_attention_ragged): row b's first visible key.  The RAGGED instantiations
// take it; the others keep AttnParams' layout and their code.
// Candidate groups (best-of-N sampling; wipa_decode_cross_attn_grouped): the B rows are B / n_group clips x n_group candidates and K / V
// hold one entry per CLIP: row b reads clip b / n_group.  The GROUPED instantiations take the count; the others keep their arguments
// and their code.
// Beams (wipa_decode_attn_beam): the B rows are B / n_group clips x n_group beams, and a beam's history is spread over the physical cache
// rows of its clip: key t of row b lies in physical row b - b % n_group + anc[b][t].  The BEAM instantiations take the table; the others keep
// their arguments and their code.
template <bool RAGGED, bool GROUPED = false, bool BEAM = false>
struct AttnArgs : AttnParams {};
template <>
struct AttnArgs<true> : AttnParams {
    const int32_t* k_start;  // int32 [B], device
};
template <>
struct AttnArgs<false, true> : AttnParams {
    int n_group;
};
template <>
struct AttnArgs<false, false, true> : AttnParams {
    const uint8_t* anc;  // uint8 [B][anc_ld], device: the group-local physical row that holds column t of row b's history
    int64_t anc_ld;
    int n_group;
};

constexpr int GA_LD = 68;  // padded f32 row (64 + 4): conflict-free ds_read_b128 across 16 keys

// RAGGED (causal self-attention over left-padded prompt rows, Tq == Tk): query i of row b sees keys k_start[b] .. i.  As in
// decode_attn_kernel the row's K / V base moves up by k_start[b] rows and Tk shrinks by as much, so a live query walks its keys in the
// tiles it would walk in a batch of its own; a padding query (i < k_start[b]) sees the row's first own key: finite, and nobody reads it.
template <typename T, bool RAGGED = false>
__global__ __launch_bounds__(256) void attn_generic_kernel(AttnArgs<RAGGED> p) {
    __shared__ __attribute__((aligned(16))) float Ks[64 * GA_LD];
    __shared__ __attribute__((aligned(16))) float Vs[64 * GA_LD];
    constexpr int EPL = Vec16<T>::EPL;
    const int tid = threadIdx.x;
    const int ql = tid >> 4, kl = tid & 15;
    const int h = blockIdx.y, b = blockIdx.z;
    int k_first = 0;  // a constant 0 without RAGGED
    if constexpr (RAGGED) k_first = p.k_start[b];
    const int Tk = p.Tk + (p.tk_dev ? *p.tk_dev : 0) - k_first;
    const int qi = blockIdx.x * 16 + ql;
    const int qc = min(qi, p.Tq - 1);
    const int q_row0 = p.q_row_dev ? *p.q_row_dev : 0;
    const T* qp = reinterpret_cast<const T*>(p.q) + b * p.q_bs + (int64_t)(q_row0 + qc) * p.q_rs + h * p.q_hs;
    float q[64];
#pragma unroll
    for (int c = 0; c < 64 / EPL; ++c) {
        Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(qp + c * EPL);
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[c * EPL + e] = v.get(e);
    }
    float acc[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) acc[d] = 0.f;
    float m = NEG_BIG, l = 0.f;
    int kmax = p.causal ? (qc + (Tk - p.Tq)) : (Tk - 1);  // last visible key of this query
    if constexpr (RAGGED) kmax = max(kmax, 0);
    // staging role: key row srow, 16-element segment sseg
    const int srow = tid >> 2, sseg = (tid & 3) * 16;
    const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_bs + h * p.k_hs;
    const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_bs + h * p.v_hs;
    if constexpr (RAGGED) {
        kb += (int64_t)k_first * p.k_rs;
        vb += (int64_t)k_first * p.v_rs;
    }
    // causal: no query of this block sees keys beyond the block's last query
    const int q_last = min(blockIdx.x * 16 + 15, p.Tq - 1);
    int k_end = p.causal ? min(Tk, q_last + (Tk - p.Tq) + 1) : Tk;
    if constexpr (RAGGED) k_end = max(k_end, 1);
    for (int k0 = 0; k0 < k_end; k0 += 64) {
        __syncthreads();
        {
            const int key = k0 + srow;
            float kv[16], vv[16];
            if (key < Tk) {
                const T* kp = kb + (int64_t)key * p.k_rs + sseg;
                const T* vp = vb + (int64_t)key * p.v_rs + sseg;
#pragma unroll
                for (int c = 0; c < 16 / EPL; ++c) {
                    Vec16<T> a = *reinterpret_cast<const Vec16<T>*>(kp + c * EPL);
                    Vec16<T> bb = *reinterpret_cast<const Vec16<T>*>(vp + c * EPL);
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        kv[c * EPL + e] = a.get(e);
                        vv[c * EPL + e] = bb.get(e);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) kv[e] = vv[e] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                *reinterpret_cast<f32x4*>(&Ks[srow * GA_LD + sseg + 4 * c]) =
                    f32x4{kv[4 * c], kv[4 * c + 1], kv[4 * c + 2], kv[4 * c + 3]};
                *reinterpret_cast<f32x4*>(&Vs[srow * GA_LD + sseg + 4 * c]) =
                    f32x4{vv[4 * c], vv[4 * c + 1], vv[4 * c + 2], vv[4 * c + 3]};
            }
        }
        __syncthreads();
        float s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = kl + 16 * i;
            const float* kr = &Ks[kk * GA_LD];
            float a = 0.f;
#pragma unroll
            for (int d4 = 0; d4 < 16; ++d4) {
                const f32x4 k4 = *reinterpret_cast<const f32x4*>(kr + 4 * d4);
                a = fmaf(q[4 * d4], k4[0], a);
                a = fmaf(q[4 * d4 + 1], k4[1], a);
                a = fmaf(q[4 * d4 + 2], k4[2], a);
                a = fmaf(q[4 * d4 + 3], k4[3], a);
            }
            s[i] = (k0 + kk <= kmax) ? a : NEG_BIG;
        }
        const float m_new = fmaxf(fmaxf(fmaxf(m, s[0]), fmaxf(s[1], s[2])), s[3]);
        const float alpha = __expf(m - m_new);
        l *= alpha;
#pragma unroll
        for (int d = 0; d < 64; ++d) acc[d] *= alpha;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float pr = (s[i] <= NEG_TEST) ? 0.f : __expf(s[i] - m_new);
            l += pr;
            const float* vr = &Vs[(kl + 16 * i) * GA_LD];
#pragma unroll
            for (int d4 = 0; d4 < 16; ++d4) {
                const f32x4 v4 = *reinterpret_cast<const f32x4*>(vr + 4 * d4);
                acc[4 * d4] = fmaf(pr, v4[0], acc[4 * d4]);
                acc[4 * d4 + 1] = fmaf(pr, v4[1], acc[4 * d4 + 1]);
                acc[4 * d4 + 2] = fmaf(pr, v4[2], acc[4 * d4 + 2]);
                acc[4 * d4 + 3] = fmaf(pr, v4[3], acc[4 * d4 + 3]);
            }
        }
        m = m_new;
    }
    // merge the 16 key lanes of this query (consecutive lanes of one wave)
    WIPA_LANE_MERGE(1, 16, 64, m, l, acc);
    if (qi < p.Tq) {
        const float inv = 1.f / l;
        if (p.lse && kl == 0) p.lse[((int64_t)b * gridDim.y + h) * p.Tq + qi] = m + __logf(l);
        T* op = reinterpret_cast<T*>(p.out) + b * p.o_bs + (int64_t)qi * p.o_rs + h * p.o_hs;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (kl == j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) op[4 * j + e] = from_f32<T>(acc[4 * j + e] * inv);
            }
        }
    }
}

// ---- the same attention on the f32 MFMA, for float32 with at least one 16-query fragment (the teacher-forced decoder of a
// fine-tune step: 64 target positions against 64 causal keys, and against the 1500 encoder positions -- 0.5 ms per layer on
// the VALU kernel above).  64 queries per workgroup, wave w owns queries 16w .. 16w+15 with the query row as MFMA fragment
// in registers and walks the keys in tiles of 64 staged as K [key][d] and V^T [d][key].  The keys sit on the ROW side of the
// score product, S[key][q], so a lane ends up holding 4 consecutive keys of one query: after the softmax these ARE the
// fragment of O[q][d] += sum_key P[q][key] V[key][d] (no LDS round trip for P; attention_bwd.hip uses the same orientation).
// Online softmax per query: its 64 scores of a tile are spread over the 4 lanes (frow = query, fq = 0..3).
__global__ __launch_bounds__(256) void attn_fwd_f32_mfma_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) float Ks[64 * GA_LD];
    __shared__ __attribute__((aligned(16))) float VsT[64 * GA_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * 64;
    const int qi = q0 + 16 * wave + frow;
    const int qc = min(qi, p.Tq - 1);
    f32x4 qx[4];
    {
        const float* qp = reinterpret_cast<const float*>(p.q) + b * p.q_bs + (int64_t)qc * p.q_rs + h * p.q_hs + 4 * fq;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qx[ks] = *reinterpret_cast<const f32x4*>(qp + 16 * ks);
    }
    f32x4 O[4];  // O[j][r] <-> query q0 + 16 wave + 4 fq + r, d = 16 j + frow
#pragma unroll
    for (int j = 0; j < 4; ++j) O[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG_BIG, l = 0.f;  // of query frow; l is this lane's share (its 16 keys of every tile)
    const int off = p.Tk - p.Tq;
    const int kmax = p.causal ? qc + off : p.Tk - 1;  // last visible key of the lane's query
    const int q_last = min(q0 + 63, p.Tq - 1);
    const int k_end = p.causal ? min(p.Tk, q_last + off + 1) : p.Tk;
    const int srow = tid >> 2, sseg = (tid & 3) * 16;
    const float* kb = reinterpret_cast<const float*>(p.k) + b * p.k_bs + h * p.k_hs;
    const float* vb = reinterpret_cast<const float*>(p.v) + b * p.v_bs + h * p.v_hs;
    for (int k0 = 0; k0 < k_end; k0 += 64) {
        __syncthreads();
        {
            const int key = k0 + srow;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, bb = {0.f, 0.f, 0.f, 0.f};
                if (key < p.Tk) {
                    a = *reinterpret_cast<const f32x4*>(kb + (int64_t)key * p.k_rs + sseg + 4 * c);
                    bb = *reinterpret_cast<const f32x4*>(vb + (int64_t)key * p.v_rs + sseg + 4 * c);
                }
                *reinterpret_cast<f32x4*>(&Ks[srow * GA_LD + sseg + 4 * c]) = a;
#pragma unroll
                for (int e = 0; e < 4; ++e) VsT[(sseg + 4 * c + e) * GA_LD + srow] = bb[e];
            }
        }
        __syncthreads();
        f32x4 S[4];  // S[i][e] <-> key k0 + 16 i + 4 fq + e, query = the lane's
        float mx = NEG_BIG;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            S[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(&Ks[(16 * i + frow) * GA_LD + 16 * ks + 4 * fq]);
                Mma<float>::run(kf, qx[ks], S[i]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (k0 + 16 * i + 4 * fq + e > kmax) S[i][e] = NEG_BIG;
                mx = fmaxf(mx, S[i][e]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        if (__any(m_new > m)) {
            const float alpha = __expf(m - m_new);
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = __shfl(alpha, 4 * fq + r, 64);  // lane 4fq + r holds query 4fq + r of this wave
#pragma unroll
                for (int j = 0; j < 4; ++j) O[j][r] *= ar;
            }
            m = m_new;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pr = (S[i][e] <= NEG_TEST) ? 0.f : __expf(S[i][e] - m);
                S[i][e] = pr;
                l += pr;
            }
        // O[q][d] += sum_key P[q][key] V[key][d]   (k-step i = keys 16i .. 16i+15 of the tile)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 vt = *reinterpret_cast<const f32x4*>(&VsT[(16 * j + frow) * GA_LD + 16 * i + 4 * fq]);
                Mma<float>::run(S[i], vt, O[j]);
            }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (p.lse && fq == 0 && qi < p.Tq) p.lse[((int64_t)b * gridDim.y + h) * p.Tq + qi] = m + __logf(l);
    const float inv = 1.f / l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float ir = __shfl(inv, 4 * fq + r, 64);
        const int qq = q0 + 16 * wave + 4 * fq + r;
        if (qq < p.Tq) {
            float* op = reinterpret_cast<float*>(p.out) + b * p.o_bs + (int64_t)qq * p.o_rs + h * p.o_hs + frow;
#pragma unroll
            for (int j = 0; j < 4; ++j) op[16 * j] = O[j][r] * ir;
        }
    }
}

// =============================================================================
// K11 decode-step cross-attention
// =============================================================================
// WPH = waves per (b,h): 4 (the workgroup's waves split the keys; long caches, e.g. 1500 cross keys) or
// 1 (every wave owns one head and walks all its keys; short self-attention caches: no LDS merge, 4x fewer workgroups).
// NT: non-temporal loads (a cache read exactly once per step: the cached cross K / V); off for the growing self-attention cache,
// which the next step reads again.  Round 4: the self-attention of a decode step takes WPH = 4 with NT off once the cache can
// exceed 32 keys -- a wave of the one-wave form walks 32 keys per dependent round trip (7 of them at 224 keys: 6.6 us at 32
// keys, 9.9 us at 64, growing), four waves take 128 per round trip.
// RAGGED (left-padded prompt rows, wipa_decode_attn_ragged): row b sees the keys k_start[b] .. Tk - 1 only.  The row's K / V base
// pointers move up by k_start[b] rows and Tk shrinks by as much -- no mask: the row walks exactly the keys, in exactly the lane and
// wave partition, it would walk if it were decoded alone with an unpadded prompt, and the clamped loads never touch a padding row.
// A query at a padding column (below k_start[b]) sees its own key only.  A separate instantiation: the kernels of calls without
// prompts keep their arguments and their code.
// GROUPED (candidate groups): K / V of row b are those of clip b / n_group; nothing else differs.
// BEAM (beams over an ancestor table, wipa_decode_attn_beam): key t of row b is loaded from physical row b - b % n_group + anc[b][t] --
// one byte per key ahead of the row's load, the same clamped index for both.  The key partition over lanes and waves, the clamp and the
// streaming softmax are the text below, so a BEAM row does the arithmetic of a plain row on a physically gathered cache.
template <typename T, int WPH, bool NT = (WPH == 4), bool RAGGED = false, bool GROUPED = false, bool BEAM = false>
__global__ __launch_bounds__(256) void decode_attn_kernel(AttnArgs<RAGGED, GROUPED, BEAM> p) {
    constexpr int EPL = Vec16<T>::EPL;  // elements per 16-byte load
    constexpr int LPK = 64 / EPL;       // lanes per key row (64 dims)
    constexpr int G = 64 / LPK;         // keys per wave instruction
    constexpr int U = 4;                // independent key groups in flight per iteration
    __shared__ float s_m[4], s_l[4];
    __shared__ float s_acc[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = WPH == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wave, b = blockIdx.y;
    if (WPH == 1 && h >= p.H) return;  // no workgroup barrier on this path
    const int kw = WPH == 4 ? wave : 0;
    const int g = lane / LPK, c = lane % LPK;
    const int Tk_all = p.Tk + (p.tk_dev ? *p.tk_dev : 0);
    const int q_row0 = p.q_row_dev ? *p.q_row_dev : 0;
    int k_first = 0;  // a constant 0 without RAGGED
    if constexpr (RAGGED) k_first = min(p.k_start[b], q_row0);
    const int Tk = Tk_all - k_first;
    float qf[EPL];
    {
        const T* qp = reinterpret_cast<const T*>(p.q) + b * p.q_bs + (int64_t)q_row0 * p.q_rs + h * p.q_hs + c * EPL;
        Vec16<T> qv = *reinterpret_cast<const Vec16<T>*>(qp);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[e] = qv.get(e);
    }
    int kvb = b;  // the cache entry the row reads: its own, or its clip's
    if constexpr (GROUPED) kvb = b / p.n_group;
    const T* Kb = reinterpret_cast<const T*>(p.k) + kvb * p.k_bs + h * p.k_hs + c * EPL;
    const T* Vb = reinterpret_cast<const T*>(p.v) + kvb * p.v_bs + h * p.v_hs + c * EPL;
    if constexpr (RAGGED) {
        Kb += (int64_t)k_first * p.k_rs;
        Vb += (int64_t)k_first * p.v_rs;
    }
    const int64_t k_rs = p.k_rs, v_rs = p.v_rs;
    const uint8_t* anc_row = nullptr;  // BEAM only: Kb / Vb then point at the first physical row of the row's clip
    if constexpr (BEAM) {
        const int64_t back = (int64_t)(b % p.n_group);
        Kb -= back * p.k_bs;
        Vb -= back * p.v_bs;
        anc_row = p.anc + (int64_t)b * p.anc_ld;
    }
    float m = NEG_BIG, l = 0.f;
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    // One register set (U K-rows + U V-rows in flight per lane), latency hidden by the other waves of the CU.
    // A register double-buffer measured the same 5.4 TB/s stand-alone but needs 135 VGPRs; the lean form keeps
    // the kernel small enough to share a SIMD with the 2 x 212-VGPR waves of the encoder GEMM of another
    // in-flight pass (see bench.py --pipeline), where it can use the HBM bandwidth the GEMM leaves idle.
    constexpr int STEP = WPH * G * U;
    auto key_group = [&](int t0) {  // a lambda on purpose: the same text straight in the loop compiles to other code
        Vec16<T> ka[U], va[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // cross-attention (NT): 3.5 GB per step read exactly once -> non-temporal (nt) loads
            if constexpr (BEAM) {
                const int t = min(t0 + u * G + g, Tk - 1);  // load_row_clamped's clamp, taken first: the table is read at the same index
                const int64_t phys = min((int)anc_row[t], p.n_group - 1);  // a table entry never leaves the clip's rows
                ka[u] = load_row_clamped<NT>(Kb + phys * p.k_bs, t, Tk - 1, k_rs);
                va[u] = load_row_clamped<NT>(Vb + phys * p.v_bs, t, Tk - 1, v_rs);
            } else {
                ka[u] = load_row_clamped<NT>(Kb, t0 + u * G + g, Tk - 1, k_rs);
                va[u] = load_row_clamped<NT>(Vb, t0 + u * G + g, Tk - 1, v_rs);
            }
        }
        WIPA_STREAM_STEP(U, qf, ka, va, t0, m, l, acc);
    };
    for (int t0 = kw * G * U; t0 < Tk; t0 += STEP) key_group(t0);
    // merge the G key groups of this wave (lanes with equal c)
    WIPA_LANE_MERGE(LPK, 64, EPL, m, l, acc);
    if (WPH == 1) {
        if (lane < LPK) {
            const float inv = 1.f / l;
            T* op = reinterpret_cast<T*>(p.out) + b * p.o_bs + h * p.o_hs + c * EPL;
#pragma unroll
            for (int e = 0; e < EPL; ++e) op[e] = from_f32<T>(acc[e] * inv);
        }
        return;
    }
    WIPA_WAVE_MERGE_STORE(s_acc, s_m, s_l, m, l, acc);
    __syncthreads();
    if (tid < 64) WIPA_WAVE_MERGE_OUT(s_acc, s_m, s_l, tid, reinterpret_cast<T*>(p.out)[b * p.o_bs + h * p.o_hs + tid]);
}

// Prompt prefill: the NQ prompt positions of a clip attend to the SAME cached cross K/V, so one pass over the cache serves
// all of them (the per-position decode step would stream the 3.5 GB cache NQ times).  Same decomposition and the same
// per-query arithmetic order as decode_attn_kernel<T, 4>: 4 waves split the keys, LDS merge; q / out rows are (b, t).
template <typename T, int NQ, bool GROUPED = false>
__global__ __launch_bounds__(256) void decode_attn_multi_kernel(AttnArgs<false, GROUPED> p) {
    constexpr int EPL = Vec16<T>::EPL;
    constexpr int LPK = 64 / EPL;
    constexpr int G = 64 / LPK;
    constexpr int U = 4;
    __shared__ float s_m[NQ][4], s_l[NQ][4];
    __shared__ float s_acc[NQ][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    const int g = lane / LPK, c = lane % LPK;
    const int Tk = p.Tk;
    float qf[NQ][EPL];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const T* qp = reinterpret_cast<const T*>(p.q) + b * p.q_bs + (int64_t)t * p.q_rs + h * p.q_hs + c * EPL;
        Vec16<T> qv = *reinterpret_cast<const Vec16<T>*>(qp);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[t][e] = qv.get(e);
    }
    int kvb = b;
    if constexpr (GROUPED) kvb = b / p.n_group;
    const T* Kb = reinterpret_cast<const T*>(p.k) + kvb * p.k_bs + h * p.k_hs + c * EPL;
    const T* Vb = reinterpret_cast<const T*>(p.v) + kvb * p.v_bs + h * p.v_hs + c * EPL;
    const int64_t k_rs = p.k_rs, v_rs = p.v_rs;
    float m[NQ], l[NQ], acc[NQ][EPL];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        m[t] = NEG_BIG;
        l[t] = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[t][e] = 0.f;
    }
    constexpr int STEP = 4 * G * U;
    for (int t0 = wave * G * U; t0 < Tk; t0 += STEP) {
        Vec16<T> ka[U], va[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ka[u] = load_row_clamped(Kb, t0 + u * G + g, Tk - 1, k_rs);
            va[u] = load_row_clamped(Vb, t0 + u * G + g, Tk - 1, v_rs);
        }
#pragma unroll
        for (int t = 0; t < NQ; ++t) WIPA_STREAM_STEP(U, qf[t], ka, va, t0, m[t], l[t], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        WIPA_LANE_MERGE(LPK, 64, EPL, m[t], l[t], acc[t]);
        WIPA_WAVE_MERGE_STORE(s_acc[t], s_m[t], s_l[t], m[t], l[t], acc[t]);
    }
    __syncthreads();
    if (tid < 64 * NQ) {
        const int t = tid >> 6, dd = tid & 63;
        WIPA_WAVE_MERGE_OUT(s_acc[t], s_m[t], s_l[t], dd, reinterpret_cast<T*>(p.out)[b * p.o_bs + (int64_t)t * p.o_rs + h * p.o_hs + dd]);
    }
}

// =============================================================================
// K5 encoder flash attention, bf16 MFMA 32x32x16
// =============================================================================
constexpr int FA_ROWB = 128;                // bytes per LDS row (64 bf16)
constexpr int FA_TILE = 64 * FA_ROWB;       // 8 KiB
constexpr float LOG2E = 1.4426950408889634f;

// The online softmax of one 64-key tile, one text for the three flash kernels (a macro over their locals: as a __forceinline__
// function over references it compiled to different code in all three).  In: S[2], the raw scores S^T of tile kt in the 32x32
// accumulator layout -- element i of S[u] in lane half hh is key 64 kt + 32u + 8(i>>2) + 4hh + (i&3), the lane's query is its
// column.  Out: S holds p = exp2(S*log2e - m); O[2] is rescaled when the running max moved; m (log2 domain) and l are updated,
// l being the lane half's share of the row sum until WIPA_FLASH_SOFTMAX_FINISH adds the two halves.
//   * The ragged last tile is masked behind a scalar BRANCH, which the empty asm keeps one: if-converted, the 32 compares and
//     selects ran on every tile and cost as much VALU time as the softmax itself.
//   * Every tile holds at least one real key, so m_new is finite; a masked score gives exp2(-1e30) = 0 without a test.
//   * p as one FMA + v_exp, two scores per VALU slot (v_pk_fma_f32 / v_pk_add_f32); only the exponentials stay scalar.
//   * The rescale is wave-uniform (__any): the running max rarely moves after the first tiles.
#define WIPA_FLASH_SOFTMAX_TILE()                                                                  \
    do {                                                                                           \
        if (kt * 64 + 64 > T) {                                                                    \
            asm volatile("" ::: "memory");                                                         \
            _Pragma("unroll") for (int u = 0; u < 2; ++u)                                          \
                _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                   \
                    const int key = kt * 64 + 32 * u + (i & 3) + 8 * (i >> 2) + 4 * hh;            \
                    if (key >= T) S[u][i] = NEG_BIG;                                               \
                }                                                                                  \
        }                                                                                          \
        float mx = NEG_BIG;                                                                        \
        _Pragma("unroll") for (int u = 0; u < 2; ++u)                                              \
            _Pragma("unroll") for (int i = 0; i < 16; ++i) mx = fmaxf(mx, S[u][i]);                \
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                                                    \
        const float m_new = fmaxf(m, mx * LOG2E);                                                  \
        f32x2 psum2 = {0.f, 0.f};                                                                  \
        const f32x2 l2e = {LOG2E, LOG2E}, mneg = {-m_new, -m_new};                                 \
        _Pragma("unroll") for (int u = 0; u < 2; ++u)                                              \
            _Pragma("unroll") for (int i = 0; i < 16; i += 2) {                                    \
                const f32x2 x = __builtin_elementwise_fma(f32x2{S[u][i], S[u][i + 1]}, l2e, mneg); \
                const f32x2 pv = {__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};       \
                S[u][i] = pv.x;                                                                    \
                S[u][i + 1] = pv.y;                                                                \
                psum2 += pv;                                                                       \
            }                                                                                      \
        const float psum = psum2.x + psum2.y;                                                      \
        if (__any(m_new > m)) {                                                                    \
            const float alpha = __builtin_amdgcn_exp2f(m - m_new);                                 \
            l *= alpha;                                                                            \
            _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                       \
                O[0][i] *= alpha;                                                                  \
                O[1][i] *= alpha;                                                                  \
            }                                                                                      \
            m = m_new;                                                                             \
        }                                                                                          \
        l += psum;                                                                                 \
    } while (0)
#define WIPA_FLASH_SOFTMAX_FINISH() l += __shfl_xor(l, 32, 64)

// blockDim.x / 64 = 4 or 8 waves: 128 or 256 queries share every K / V^T tile (8 waves halve the L2->LDS fill per FLOP).
__global__ __launch_bounds__(512) void flash_enc_bf16_kernel(const __bf16* __restrict__ qk, int64_t ldqk,
                                                             const __bf16* __restrict__ vt, int64_t ldvt,
                                                             __bf16* __restrict__ out, int64_t ldo, int H, int T) {
    __shared__ __attribute__((aligned(16))) char smem[4 * FA_TILE];  // [buf][K tile | V^T tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const int D = H * 64;
    const int nw = blockDim.x >> 6;
    const int q0 = blockIdx.x * (nw * 32) + wave * 32;
    const int nkt = (T + 63) / 64;

    // Q fragments: B operand of S^T = K * Q^T.  lane (r,hh) holds Q[q0+r][16s + 8hh + 0..7]
    bf16x8 qf[4];
    {
        const int qrow = min(q0 + r, T - 1);
        const __bf16* qp = qk + ((int64_t)b * T + qrow) * ldqk + h * 64 + 8 * hh;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
    }
    // Staging by LDS-DMA (buffer_load_dwordx4 ... lds): no VGPR round trip, no ds_write.  A 1-KiB piece is 8 tile rows of
    // 128 B; lane l lands at byte 16 l of the piece, i.e. (row l>>3, physical chunk l&7), and fetches the SOURCE chunk
    // (l&7) ^ ((row>>1)&7) -- the same XOR the fragment reads apply.  Wave w moves pieces 2w, 2w+1 of the K tile and of
    // the V^T tile.  Keys beyond T are out of the K resource's range and read as zero; V^T is zero there already.
    typedef __attribute__((address_space(3))) void* lds_t;
    const __bf16* kbase = qk + (int64_t)b * T * ldqk + D + h * 64;
    const __bf16* vbase = vt + ((int64_t)b * D + h * 64) * ldvt;
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (int)(((int64_t)(T - 1) * ldqk + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, (int)(((int64_t)63 * ldvt + ldvt) * 2), 0x00020000);
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int ppw = 8 / nw;  // 1-KiB pieces of each tile per wave: 2 (four waves) or 1 (eight)
    int offK[2], offV[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = 8 * (ppw * wv + i) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        offK[i] = row * (int)ldqk * 2 + c * 16;   // + k0 * ldqk * 2 (scalar)
        offV[i] = row * (int)ldvt * 2 + c * 16;   // + k0 * 2 (scalar)
    }
    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * 2 * FA_TILE + (ppw * wv) * 1024;
        const int k0 = kt * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i < ppw) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, (lds_t)(base + i * 1024), 16, offK[i], k0 * (int)ldqk * 2, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, (lds_t)(base + FA_TILE + i * 1024), 16, offV[i], k0 * 2, 0, 0);
            }
        }
    };

    f32x16 O[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) O[0][i] = O[1][i] = 0.f;
    float m = NEG_BIG, l = 0.f;  // m in the log2 domain (scores * log2e)
    const int rsw = (r >> 1) & 7;  // swizzle term of rows 32x + r

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) stage(kt + 1, (kt + 1) & 1);
        const char* kbuf = smem + (kt & 1) * 2 * FA_TILE;
        const char* vbuf = kbuf + FA_TILE;
        f32x16 S[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int i = 0; i < 16; ++i) S[u][i] = 0.f;
            const char* krow = kbuf + (32 * u + r) * FA_ROWB;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(krow + (((2 * s + hh) ^ rsw) << 4));
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], S[u], 0, 0, 0);
            }
        }
        WIPA_FLASH_SOFTMAX_TILE();
        // O^T += V^T * P^T : P^T comes straight from the S accumulators (k order of the
        // 32x32 C layout: element j of half hh is key 16s' + 8(j>>2) + 4hh + (j&3))
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                bf16x8 pb;
#pragma unroll
                for (int j = 0; j < 8; ++j) pb[j] = (__bf16)S[u][8 * sp + j];
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const char* vrow = vbuf + (32 * dt + r) * FA_ROWB + 8 * hh;
                    const int c0 = 4 * u + 2 * sp;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow + ((c0 ^ rsw) << 4));
                    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vrow + (((c0 + 1) ^ rsw) << 4));
                    const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb, O[dt], 0, 0, 0);
                    // keep the dt = 0 / dt = 1 reads apart: merged into ds_read2st64_b64 their halves land in the wrong
                    // register pairs and cost 24 v_mov per tile on the (busier) VALU
                    asm volatile("" ::: "memory");
                }
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    WIPA_FLASH_SOFTMAX_FINISH();
    const int qrow = q0 + r;
    if (qrow < T) {
        const float inv = 1.f / l;
        __bf16* op = out + ((int64_t)b * T + qrow) * ldo + h * 64 + 4 * hh;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                bf16x4 o = {(__bf16)(O[dt][4 * g4] * inv), (__bf16)(O[dt][4 * g4 + 1] * inv),
                            (__bf16)(O[dt][4 * g4 + 2] * inv), (__bf16)(O[dt][4 * g4 + 3] * inv)};
                *reinterpret_cast<bf16x4*>(op + 32 * dt + 8 * g4) = o;
            }
    }
}

// =============================================================================
// K5 in f32 (the reference's own dtype: set_dtype(float32)): encoder flash attention on the f32 MFMA
// (v_mfma_f32_32x32x2_f32, exact f32 products, f32 accumulation).  Same structure as the bf16 kernel:
// S^T = K Q^T so that a lane owns one query column, P stays in the S accumulators and feeds O^T += V^T P^T.
// The contraction index of an f32 MFMA step is 2 wide (lane half hh picks the element), so
//   * Q is held as qf[s] = Q[q][2s + hh] and the K tile is stored with even and odd k separated
//     ([key][parity][32]): a lane reads its 32 operands of a key row with 8 ds_read_b128;
//   * the keys of P^T are contracted in the order the 32x32 accumulator layout holds them
//     (step s of half hh = key 8(s>>2) + 4hh + (s&3)), which are 4 consecutive keys per ds_read_b128 of V^T.
// V arrives [key][d]; the staging transposes it into the V^T tile.
constexpr int FF_LD = 68;                  // floats per LDS row: 64 + 4 (conflict-free ds_read_b128 down a column)
constexpr int FF_TILE = 64 * FF_LD;        // floats per operand tile

// The K half of the staging: this thread's 16 consecutive k (segment kseg) of one key, in rk, to the key's LDS row.
// Exact kernel: even and odd k separated, even k -> [0, 32), odd k -> [32, 64) of the row.  Split kernel: as they come.
__device__ __forceinline__ void stage_k_parity(float* krow, int kseg, const f32x4 (&rk)[4]) {
    float* kt = krow + 8 * kseg;
    *reinterpret_cast<f32x4*>(kt) = f32x4{rk[0][0], rk[0][2], rk[1][0], rk[1][2]};
    *reinterpret_cast<f32x4*>(kt + 4) = f32x4{rk[2][0], rk[2][2], rk[3][0], rk[3][2]};
    *reinterpret_cast<f32x4*>(kt + 32) = f32x4{rk[0][1], rk[0][3], rk[1][1], rk[1][3]};
    *reinterpret_cast<f32x4*>(kt + 36) = f32x4{rk[2][1], rk[2][3], rk[3][1], rk[3][3]};
}
__device__ __forceinline__ void stage_k_plain(float* krow, int kseg, const f32x4 (&rk)[4]) {
    float* kt = krow + 16 * kseg;
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(kt + 4 * c) = rk[c];
}

// The scaffold of the two f32 kernels, as text over the kernel's locals (q, k, v, out, their row strides and T are the kernel's
// arguments).  A kernel supplies its Q fragments, the K half of the staging (STAGE_K: one of the two functions above) and the
// two product blocks, which stay in the kernel as plain text between the TILE macros.
#define WIPA_FLASH_F32_INDICES()                                                                                 \
    __shared__ __attribute__((aligned(16))) float smem[4 * FF_TILE]; /* [buf][K tile | V^T tile], 69 632 B */    \
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;                                               \
    const int r = lane & 31, hh = lane >> 5;                                                                     \
    const int h = blockIdx.y, b = blockIdx.z;                                                                    \
    const int q0 = blockIdx.x * 128 + wave * 32;                                                                 \
    const int nkt = (T + 63) / 64

// staging roles.  K: key row tid>>2, 16 consecutive k (segment tid&3).  V: key tid&63, 16 consecutive d (tid>>6); V arrives
// [key][d] and is transposed into the V^T tile.  Then the accumulators and the first tile.
#define WIPA_FLASH_F32_STAGING(STAGE_K)                                                                          \
    const int krow = tid >> 2, kseg = tid & 3;                                                                   \
    const int vkey = tid & 63, vseg = tid >> 6;                                                                  \
    const float* kg = k + (int64_t)b * T * ldk + h * 64 + 16 * kseg;                                             \
    const float* vg = v + (int64_t)b * T * ldv + h * 64 + 16 * vseg;                                             \
    f32x4 rk[4], rv[4];                                                                                          \
    auto gload = [&](int kt) {                                                                                   \
        const float* kp = kg + (int64_t)min(kt * 64 + krow, T - 1) * ldk;                                        \
        const float* vp = vg + (int64_t)min(kt * 64 + vkey, T - 1) * ldv;                                        \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                          \
            rk[c] = *reinterpret_cast<const f32x4*>(kp + 4 * c);                                                 \
            rv[c] = *reinterpret_cast<const f32x4*>(vp + 4 * c);                                                 \
        }                                                                                                        \
    };                                                                                                           \
    auto swrite = [&](int buf) {                                                                                 \
        STAGE_K(smem + buf * 2 * FF_TILE + krow * FF_LD, kseg, rk);                                              \
        float* vt = smem + buf * 2 * FF_TILE + FF_TILE + (16 * vseg) * FF_LD + vkey; /* V^T[d][key] */           \
        _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                            \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) vt[(4 * c + e) * FF_LD] = rv[c][e];                    \
    };                                                                                                           \
    f32x16 O[2];                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 16; ++i) O[0][i] = O[1][i] = 0.f;                                      \
    float m = NEG_BIG, l = 0.f; /* m in the log2 domain */                                                       \
    gload(0);                                                                                                    \
    swrite(0);                                                                                                   \
    __syncthreads()

// inside for (kt): the next tile's global loads fly over this tile's products and are written to the other buffer behind them
#define WIPA_FLASH_F32_TILE_BEGIN()                                                                              \
    if (kt + 1 < nkt) gload(kt + 1);                                                                             \
    const float* kbuf = smem + (kt & 1) * 2 * FF_TILE;                                                           \
    const float* vbuf = kbuf + FF_TILE;                                                                          \
    f32x16 S[2]
#define WIPA_FLASH_F32_TILE_END()                                                                                \
    if (kt + 1 < nkt) swrite((kt + 1) & 1);                                                                      \
    __syncthreads()

#define WIPA_FLASH_F32_TAIL()                                                                                    \
    WIPA_FLASH_SOFTMAX_FINISH();                                                                                 \
    const int qrow = q0 + r;                                                                                     \
    if (qrow < T) {                                                                                              \
        const float inv = 1.f / l;                                                                               \
        float* op = out + ((int64_t)b * T + qrow) * ldo + h * 64 + 4 * hh;                                       \
        _Pragma("unroll") for (int dt = 0; dt < 2; ++dt)                                                         \
            _Pragma("unroll") for (int g4 = 0; g4 < 4; ++g4)                                                     \
                *reinterpret_cast<f32x4*>(op + 32 * dt + 8 * g4) =                                               \
                    f32x4{O[dt][4 * g4] * inv, O[dt][4 * g4 + 1] * inv, O[dt][4 * g4 + 2] * inv, O[dt][4 * g4 + 3] * inv}; \
    }

__global__ __launch_bounds__(256, 2) void flash_enc_f32_kernel(const float* __restrict__ q, int64_t ldq,
                                                               const float* __restrict__ k, int64_t ldk,
                                                               const float* __restrict__ v, int64_t ldv,
                                                               float* __restrict__ out, int64_t ldo, int T) {
    WIPA_FLASH_F32_INDICES();
    float qf[32];
    {
        const float* qp = q + ((int64_t)b * T + min(q0 + r, T - 1)) * ldq + h * 64 + hh;
#pragma unroll
        for (int s = 0; s < 32; ++s) qf[s] = qp[2 * s];
    }
    WIPA_FLASH_F32_STAGING(stage_k_parity);
    for (int kt = 0; kt < nkt; ++kt) {
        WIPA_FLASH_F32_TILE_BEGIN();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int i = 0; i < 16; ++i) S[u][i] = 0.f;
            const float* kr = kbuf + (32 * u + r) * FF_LD + 32 * hh;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(kr + 4 * c);
#pragma unroll
                for (int e = 0; e < 4; ++e) S[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[4 * c + e], S[u], 0, 0, 0);
            }
        }
        WIPA_FLASH_SOFTMAX_TILE();
        // O^T[d][q] += V^T[d][key] P^T[key][q]; step s of accumulator element s: key 32u + 8(s>>2) + 4hh + (s&3)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const float* vr = vbuf + (32 * dt + r) * FF_LD + 32 * u + 4 * hh;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 vf = *reinterpret_cast<const f32x4*>(vr + 8 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[e], S[u][4 * g + e], O[dt], 0, 0, 0);
                }
            }
        WIPA_FLASH_F32_TILE_END();
    }
    WIPA_FLASH_F32_TAIL();
}

// K5 in f32, fast form: every product on the bf16 MFMA (32x32x16) with the f32 operands split in registers.  The scores
// S^T = K Q^T use THREE terms per operand and the six largest cross products (error ~2^-24: an error eps in a score is a
// relative error eps*|s| in its probability, and scores can be large); O^T += V^T P^T -- probabilities in [0, 1] against
// values -- uses two terms per operand and three products, as the f32 tile GEMMs do.  9 bf16 MFMAs replace 16 f32-MFMA
// equivalents that run 16x slower; the conversions (VALU) set the pace.  K tile [key][64 d], V^T tile [d][64 keys], f32.
__global__ __launch_bounds__(256, 2) void flash_enc_f32s_kernel(const float* __restrict__ q, int64_t ldq,
                                                                const float* __restrict__ k, int64_t ldk,
                                                                const float* __restrict__ v, int64_t ldv,
                                                                float* __restrict__ out, int64_t ldo, int T) {
    WIPA_FLASH_F32_INDICES();
    // Q fragments (B operand): lane (r, hh) holds Q[q0+r][16s + 8hh + 0..7], split once
    bf16x8 qh[4], qm[4], ql[4];
    {
        const float* qp = q + ((int64_t)b * T + min(q0 + r, T - 1)) * ldq + h * 64 + 8 * hh;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            split_bf16x3(*reinterpret_cast<const f32x4*>(qp + 16 * s), *reinterpret_cast<const f32x4*>(qp + 16 * s + 4), qh[s], qm[s], ql[s]);
    }
    WIPA_FLASH_F32_STAGING(stage_k_plain);
    for (int kt = 0; kt < nkt; ++kt) {
        WIPA_FLASH_F32_TILE_BEGIN();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int i = 0; i < 16; ++i) S[u][i] = 0.f;
            const float* kr = kbuf + (32 * u + r) * FF_LD + 8 * hh;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8 kh, km, kl;
                split_bf16x3(*reinterpret_cast<const f32x4*>(kr + 16 * s), *reinterpret_cast<const f32x4*>(kr + 16 * s + 4), kh, km, kl);
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qh[s], S[u], 0, 0, 0);  // smallest terms first
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(km, qm[s], S[u], 0, 0, 0);
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, ql[s], S[u], 0, 0, 0);
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(km, qh[s], S[u], 0, 0, 0);
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qm[s], S[u], 0, 0, 0);
                S[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qh[s], S[u], 0, 0, 0);
            }
        }
        WIPA_FLASH_SOFTMAX_TILE();
        // O^T += V^T P^T; MFMA k slot j of half hh is key 16 sp + 8 (j>>2) + 4 hh + (j&3) of the 32-key block u
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                bf16x8 ph, pl;
                split_bf16x2(f32x4{S[u][8 * sp], S[u][8 * sp + 1], S[u][8 * sp + 2], S[u][8 * sp + 3]},
                             f32x4{S[u][8 * sp + 4], S[u][8 * sp + 5], S[u][8 * sp + 6], S[u][8 * sp + 7]}, ph, pl);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const float* vr = vbuf + (32 * dt + r) * FF_LD + 32 * u + 16 * sp + 4 * hh;
                    bf16x8 vh, vl;
                    split_bf16x2(*reinterpret_cast<const f32x4*>(vr), *reinterpret_cast<const f32x4*>(vr + 8), vh, vl);
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, pl, O[dt], 0, 0, 0);
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl, ph, O[dt], 0, 0, 0);
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, ph, O[dt], 0, 0, 0);
                }
            }
        WIPA_FLASH_F32_TILE_END();
    }
    WIPA_FLASH_F32_TAIL();
}

#undef WIPA_FLASH_F32_INDICES
#undef WIPA_FLASH_F32_STAGING
#undef WIPA_FLASH_F32_TILE_BEGIN
#undef WIPA_FLASH_F32_TILE_END
#undef WIPA_FLASH_F32_TAIL
#undef WIPA_FLASH_SOFTMAX_TILE
#undef WIPA_FLASH_SOFTMAX_FINISH

}  // namespace

// 16-byte row loads: every stride of q, k and v keeps the alignment of the base pointers
static bool attn_strides_aligned(const wipa_attn_desc* d) {
    const int64_t al = d->dtype == WIPA_BF16 ? 8 : 4;
    return d->q_rs % al == 0 && d->k_rs % al == 0 && d->v_rs % al == 0 && d->q_hs % al == 0 && d->k_hs % al == 0 && d->v_hs % al == 0 &&
           d->q_bs % al == 0 && d->k_bs % al == 0 && d->v_bs % al == 0;
}

static void fill_attn_params(const wipa_attn_desc* d, AttnParams& p) {
    p.q = (const char*)d->q;
    p.k = (const char*)d->k;
    p.v = (const char*)d->v;
    p.out = (char*)d->out;
    p.tk_dev = d->tk_dev;
    p.q_row_dev = d->q_row_dev;
    p.lse = d->lse;
    p.q_bs = d->q_bs; p.q_rs = d->q_rs; p.q_hs = d->q_hs;
    p.k_bs = d->k_bs; p.k_rs = d->k_rs; p.k_hs = d->k_hs;
    p.v_bs = d->v_bs; p.v_rs = d->v_rs; p.v_hs = d->v_hs;
    p.o_bs = d->o_bs; p.o_rs = d->o_rs; p.o_hs = d->o_hs;
    p.Tq = d->Tq;
    p.Tk = d->Tk;
    p.causal = d->causal;
    p.H = d->H;
}

extern "C" int wipa_attention(const wipa_attn_desc* d, wipa_stream_t stream) { return wipa_attention_as(d, d ? d->Tq : 0, stream); }

// wipa_attention with the kernel chosen as for path_tq query rows per batch entry.  The grouped prompt pass hands the G x P query rows
// of a clip's candidates to one batch entry (non-causal cross-attention: every query row's arithmetic is its own, whatever rows sit
// next to it) and must stay on the kernel its P rows alone would take.
int wipa_attention_as(const wipa_attn_desc* d, int path_tq, wipa_stream_t stream) {
    WIPA_REQUIRE(d && d->q && d->k && d->v && d->out, "wipa_attention: null pointer");
    WIPA_REQUIRE(d->B > 0 && d->H > 0 && d->Tq > 0, "wipa_attention: bad shape");
    WIPA_REQUIRE(d->dtype == WIPA_F32 || d->dtype == WIPA_BF16, "wipa_attention: bad dtype %d", d->dtype);
    WIPA_REQUIRE(attn_strides_aligned(d), "wipa_attention: strides must keep 16-byte alignment");
    AttnArgs<false> p;
    fill_attn_params(d, p);
    dim3 grid((d->Tq + 15) / 16, d->H, d->B);
    // float32 with whole 16-query fragments and no device-side offsets (teacher-forced decoder, fine-tune step): f32 MFMA kernel;
    // the few-row prefill and everything bf16 stay on the VALU kernel.  WIPA_ATTN_FWD=valu keeps it for A/B runs.
    static const bool valu = [] { const char* e = getenv("WIPA_ATTN_FWD"); return e && !strcmp(e, "valu"); }();
    if (d->dtype == WIPA_F32 && !valu && path_tq >= 16 && !d->tk_dev && !d->q_row_dev && d->o_rs % 4 == 0 && d->o_hs % 4 == 0 &&
        d->o_bs % 4 == 0) {
        hipLaunchKernelGGL(attn_fwd_f32_mfma_kernel, dim3((d->Tq + 63) / 64, d->H, d->B), dim3(256), 0, (hipStream_t)stream, p);
        WIPA_LAUNCH_CHECK();
        return WIPA_OK;
    }
    if (d->dtype == WIPA_F32)
        hipLaunchKernelGGL((attn_generic_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((attn_generic_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// the causal self-attention of a ragged prompt pass: always the f32-math VALU kernel (the f32 MFMA form declines device-side offsets,
// and the rows' starts are one)
extern "C" int wipa_attention_ragged(const wipa_attn_desc* d, const int32_t* starts_dev, wipa_stream_t stream) {
    WIPA_REQUIRE(d && d->q && d->k && d->v && d->out && starts_dev, "wipa_attention_ragged: null pointer (starts_dev is required)");
    WIPA_REQUIRE(d->B > 0 && d->H > 0 && d->Tq > 0, "wipa_attention_ragged: bad shape");
    WIPA_REQUIRE(d->dtype == WIPA_F32 || d->dtype == WIPA_BF16, "wipa_attention_ragged: bad dtype %d", d->dtype);
    WIPA_REQUIRE(attn_strides_aligned(d), "wipa_attention_ragged: strides must keep 16-byte alignment");
    WIPA_REQUIRE(d->causal && d->Tq == d->Tk && !d->tk_dev && !d->q_row_dev && !d->lse,
                 "wipa_attention_ragged: causal self-attention with Tq == Tk (Tq=%d Tk=%d), no device-side offsets, no lse", d->Tq, d->Tk);
    AttnArgs<true> p;
    fill_attn_params(d, p);
    p.k_start = starts_dev;
    dim3 grid((d->Tq + 15) / 16, d->H, d->B);
    if (d->dtype == WIPA_F32)
        hipLaunchKernelGGL((attn_generic_kernel<float, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((attn_generic_kernel<__bf16, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_flash_attn_enc_bf16(const void* qk, int64_t ldqk, const void* vt, int64_t ldvt, void* out, int64_t ldo,
                                        int B, int H, int T, wipa_stream_t stream) {
    WIPA_REQUIRE(qk && vt && out, "wipa_flash_attn_enc_bf16: null pointer");
    WIPA_REQUIRE(ldqk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0, "wipa_flash_attn_enc_bf16: ld alignment");
    WIPA_REQUIRE(ldvt >= ((T + 63) / 64) * 64, "wipa_flash_attn_enc_bf16: ldvt=%lld must cover ceil64(T)", (long long)ldvt);
    WIPA_REQUIRE(B > 0 && H > 0 && T > 0, "wipa_flash_attn_enc_bf16: bad shape");
    static const int q128 = [] { const char* e = getenv("WIPA_FLASH_Q128"); return e ? atoi(e) : 0; }();
    const int nw = (T > 256 && !q128) ? 8 : 4;
    dim3 grid((T + nw * 32 - 1) / (nw * 32), H, B);
    hipLaunchKernelGGL(flash_enc_bf16_kernel, grid, dim3(nw * 64), 0, (hipStream_t)stream, (const __bf16*)qk, ldqk,
                       (const __bf16*)vt, ldvt, (__bf16*)out, ldo, H, T);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_flash_attn_enc_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                       float* out, int64_t ldo, int B, int H, int T, int f32_split, wipa_stream_t stream) {
    WIPA_REQUIRE(q && k && v && out, "wipa_flash_attn_enc_f32: null pointer");
    WIPA_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0, "wipa_flash_attn_enc_f32: row strides must be multiples of 4");
    WIPA_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)v % 16) == 0 && ((uintptr_t)out % 16) == 0,
                 "wipa_flash_attn_enc_f32: operands must be 16-byte aligned");
    WIPA_REQUIRE(B > 0 && H > 0 && T > 0, "wipa_flash_attn_enc_f32: bad shape");
    dim3 grid((T + 127) / 128, H, B);
    // exact f32 products unless the caller opted into the split-bf16 kernel
    if (!f32_split)
        hipLaunchKernelGGL(flash_enc_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, q, ldq, k, ldk, v, ldv, out, ldo, T);
    else
        hipLaunchKernelGGL(flash_enc_f32s_kernel, grid, dim3(256), 0, (hipStream_t)stream, q, ldq, k, ldk, v, ldv, out, ldo, T);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_decode_attn(const wipa_attn_desc* d, wipa_stream_t stream) {
    WIPA_REQUIRE(d && d->q && d->k && d->v && d->out, "wipa_decode_attn: null pointer");
    WIPA_REQUIRE(d->B > 0 && d->H > 0 && d->Tq == 1, "wipa_decode_attn: one query row per (b,h) (Tq=%d)", d->Tq);
    WIPA_REQUIRE(d->dtype == WIPA_F32 || d->dtype == WIPA_BF16, "wipa_decode_attn: bad dtype %d", d->dtype);
    WIPA_REQUIRE(attn_strides_aligned(d), "wipa_decode_attn: strides must keep 16-byte alignment");
    AttnArgs<false> p;
    fill_attn_params(d, p);
    // short caches (the growing self-attention cache, <= n_text_ctx keys): default-policy loads, and four waves per head
    // (WIPA_SELF_ATTN_WAVES=1: the one-wave-per-head form of rounds 1-3); long ones (cached cross K / V): 4 waves, nt loads
    const bool short_cache = d->Tk + (d->tk_dev ? 448 : 0) <= 512;
    static const int self_waves = [] { const char* e = getenv("WIPA_SELF_ATTN_WAVES"); return e ? atoi(e) : 4; }();
    if (short_cache && self_waves == 4) {
        dim3 grid(d->H, d->B);
        if (d->dtype == WIPA_F32)
            hipLaunchKernelGGL((decode_attn_kernel<float, 4, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL((decode_attn_kernel<__bf16, 4, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
    } else if (short_cache) {
        dim3 grid((d->H + 3) / 4, d->B);
        if (d->dtype == WIPA_F32)
            hipLaunchKernelGGL((decode_attn_kernel<float, 1>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL((decode_attn_kernel<__bf16, 1>), grid, dim3(256), 0, (hipStream_t)stream, p);
    } else {
        dim3 grid(d->H, d->B);
        if (d->dtype == WIPA_F32)
            hipLaunchKernelGGL((decode_attn_kernel<float, 4>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL((decode_attn_kernel<__bf16, 4>), grid, dim3(256), 0, (hipStream_t)stream, p);
    }
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// wipa_decode_attn for the growing self-attention cache of rows with left-padded prompts: row b sees keys starts_dev[b] .. Tk - 1
extern "C" int wipa_decode_attn_ragged(const wipa_attn_desc* d, const int32_t* starts_dev, wipa_stream_t stream) {
    WIPA_REQUIRE(d && d->q && d->k && d->v && d->out && starts_dev, "wipa_decode_attn_ragged: null pointer (starts_dev is required)");
    WIPA_REQUIRE(d->B > 0 && d->H > 0 && d->Tq == 1, "wipa_decode_attn_ragged: one query row per (b,h) (Tq=%d)", d->Tq);
    WIPA_REQUIRE(d->dtype == WIPA_F32 || d->dtype == WIPA_BF16, "wipa_decode_attn_ragged: bad dtype %d", d->dtype);
    WIPA_REQUIRE(attn_strides_aligned(d), "wipa_decode_attn_ragged: strides must keep 16-byte alignment");
    WIPA_REQUIRE(d->q_row_dev && d->tk_dev, "wipa_decode_attn_ragged: the query row and the key count come from the device (q_row_dev, tk_dev)");
    AttnArgs<true> p;
    fill_attn_params(d, p);
    p.k_start = starts_dev;
    dim3 grid(d->H, d->B);  // the four-wave, default-policy form the self-attention cache takes in wipa_decode_attn
    if (d->dtype == WIPA_F32)
        hipLaunchKernelGGL((decode_attn_kernel<float, 4, false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((decode_attn_kernel<__bf16, 4, false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// wipa_decode_attn for the self-attention cache of beams: row b's key t lies in physical row b - b % n_group + anc[b][t]
extern "C" int wipa_decode_attn_beam(const wipa_attn_desc* d, const uint8_t* anc, int64_t anc_ld, int n_group, wipa_stream_t stream) {
    WIPA_REQUIRE(d && d->q && d->k && d->v && d->out && anc, "wipa_decode_attn_beam: null pointer (anc is required)");
    WIPA_REQUIRE(d->B > 0 && d->H > 0 && d->Tq == 1, "wipa_decode_attn_beam: one query row per (b,h) (Tq=%d)", d->Tq);
    WIPA_REQUIRE(d->dtype == WIPA_F32 || d->dtype == WIPA_BF16, "wipa_decode_attn_beam: bad dtype %d", d->dtype);
    WIPA_REQUIRE(attn_strides_aligned(d), "wipa_decode_attn_beam: strides must keep 16-byte alignment");
    WIPA_REQUIRE(n_group >= 1 && n_group <= 16 && d->B % n_group == 0, "wipa_decode_attn_beam: n_group=%d outside 1..16 or not dividing B=%d", n_group,
                 d->B);
    const int max_keys = d->Tk + (d->tk_dev ? 448 : 0);
    WIPA_REQUIRE(max_keys <= 512 && anc_ld >= (d->tk_dev ? 1 : d->Tk), "wipa_decode_attn_beam: Tk=%d keys (a short, growing cache of at most 512) / anc_ld=%lld",
                 d->Tk, (long long)anc_ld);
    AttnArgs<false, false, true> p;
    fill_attn_params(d, p);
    p.anc = anc;
    p.anc_ld = anc_ld;
    p.n_group = n_group;
    dim3 grid(d->H, d->B);  // the four-wave, default-policy form the self-attention cache takes in wipa_decode_attn
    if (d->dtype == WIPA_F32)
        hipLaunchKernelGGL((decode_attn_kernel<float, 4, false, false, false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((decode_attn_kernel<__bf16, 4, false, false, false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// q [B][n_q][H*64] against the cached cross K/V of a clip, kv [B][2H][Tk][64] (K heads then V heads); out like q
static wipa_attn_desc cross_attn_desc(const void* q, const void* kv, void* out, int B, int H, int Tk, int n_q, int dtype) {
    wipa_attn_desc d;
    memset(&d, 0, sizeof(d));
    const size_t e = wipa_dtype_size(dtype);
    d.q = q; d.k = kv; d.v = (const char*)kv + (size_t)H * Tk * 64 * e; d.out = out;
    d.q_bs = (int64_t)n_q * H * 64; d.q_rs = (int64_t)H * 64; d.q_hs = 64;
    d.k_bs = (int64_t)2 * H * Tk * 64; d.k_rs = 64; d.k_hs = (int64_t)Tk * 64;
    d.v_bs = d.k_bs; d.v_rs = 64; d.v_hs = d.k_hs;
    d.o_bs = d.q_bs; d.o_rs = d.q_rs; d.o_hs = 64;
    d.B = B; d.H = H; d.Tq = n_q; d.Tk = Tk; d.causal = 0; d.dtype = dtype;
    return d;
}

extern "C" int wipa_decode_cross_attn(const void* q, const void* kv, void* out, int B, int H, int Tk, int dtype,
                                      wipa_stream_t stream) {
    WIPA_REQUIRE(q && kv && out, "wipa_decode_cross_attn: null pointer");
    WIPA_REQUIRE(B > 0 && H > 0 && Tk > 0, "wipa_decode_cross_attn: bad shape");
    WIPA_REQUIRE(dtype == WIPA_F32 || dtype == WIPA_BF16, "wipa_decode_cross_attn: bad dtype %d", dtype);
    const wipa_attn_desc d = cross_attn_desc(q, kv, out, B, H, Tk, 1, dtype);
    return wipa_decode_attn(&d, stream);
}

extern "C" int wipa_decode_cross_attn_multi(const void* q, const void* kv, void* out, int B, int H, int Tk, int n_q, int dtype,
                                            wipa_stream_t stream) {
    WIPA_REQUIRE(q && kv && out, "wipa_decode_cross_attn_multi: null pointer");
    WIPA_REQUIRE(B > 0 && H > 0 && Tk > 0 && n_q >= 1 && n_q <= 4, "wipa_decode_cross_attn_multi: bad shape (n_q=%d)", n_q);
    WIPA_REQUIRE(dtype == WIPA_F32 || dtype == WIPA_BF16, "wipa_decode_cross_attn_multi: bad dtype %d", dtype);
    if (n_q == 1) return wipa_decode_cross_attn(q, kv, out, B, H, Tk, dtype, stream);
    const wipa_attn_desc d = cross_attn_desc(q, kv, out, B, H, Tk, n_q, dtype);
    AttnArgs<false> p;
    fill_attn_params(&d, p);
    const dim3 grid(H, B);
    hipStream_t s = (hipStream_t)stream;
#define WIPA_MULTI(T, NQ) hipLaunchKernelGGL((decode_attn_multi_kernel<T, NQ>), grid, dim3(256), 0, s, p)
    if (dtype == WIPA_F32) {
        if (n_q == 2) WIPA_MULTI(float, 2); else if (n_q == 3) WIPA_MULTI(float, 3); else WIPA_MULTI(float, 4);
    } else {
        if (n_q == 2) WIPA_MULTI(__bf16, 2); else if (n_q == 3) WIPA_MULTI(__bf16, 3); else WIPA_MULTI(__bf16, 4);
    }
#undef WIPA_MULTI
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}


// Candidate groups: the cached cross-attention of B = clips x n_group rows against the K / V of B / n_group clips -- the long-cache form
// of wipa_decode_attn (four waves, nt loads) for one query row, decode_attn_multi_kernel for 2..4, in their GROUPED instantiations.
extern "C" int wipa_decode_cross_attn_grouped(const void* q, const void* kv, void* out, int B, int H, int Tk, int n_q, int n_group, int dtype,
                                              wipa_stream_t stream) {
    WIPA_REQUIRE(q && kv && out, "wipa_decode_cross_attn_grouped: null pointer");
    WIPA_REQUIRE(B > 0 && H > 0 && Tk > 0 && n_q >= 1 && n_q <= 4, "wipa_decode_cross_attn_grouped: bad shape (n_q=%d)", n_q);
    WIPA_REQUIRE(n_group >= 1 && B % n_group == 0, "wipa_decode_cross_attn_grouped: %d rows are no multiple of n_group=%d", B, n_group);
    WIPA_REQUIRE(dtype == WIPA_F32 || dtype == WIPA_BF16, "wipa_decode_cross_attn_grouped: bad dtype %d", dtype);
    if (n_group == 1) return wipa_decode_cross_attn_multi(q, kv, out, B, H, Tk, n_q, dtype, stream);
    const wipa_attn_desc d = cross_attn_desc(q, kv, out, B, H, Tk, n_q, dtype);
    WIPA_REQUIRE(attn_strides_aligned(&d), "wipa_decode_cross_attn_grouped: strides must keep 16-byte alignment");
    AttnArgs<false, true> p;
    fill_attn_params(&d, p);
    p.n_group = n_group;
    const dim3 grid(H, B);
    hipStream_t s = (hipStream_t)stream;
    if (n_q == 1) {
        // the forms wipa_decode_attn chooses between for Tk keys without device-side offsets: up to 512 keys the default-policy
        // loads of a short cache (four waves, or one per head with WIPA_SELF_ATTN_WAVES=1), above that four waves and nt loads
        static const int self_waves = [] { const char* e = getenv("WIPA_SELF_ATTN_WAVES"); return e ? atoi(e) : 4; }();
        if (Tk <= 512 && self_waves == 4) {
            if (dtype == WIPA_F32) hipLaunchKernelGGL((decode_attn_kernel<float, 4, false, false, true>), grid, dim3(256), 0, s, p);
            else hipLaunchKernelGGL((decode_attn_kernel<__bf16, 4, false, false, true>), grid, dim3(256), 0, s, p);
        } else if (Tk <= 512) {
            const dim3 grid1((H + 3) / 4, B);
            if (dtype == WIPA_F32) hipLaunchKernelGGL((decode_attn_kernel<float, 1, false, false, true>), grid1, dim3(256), 0, s, p);
            else hipLaunchKernelGGL((decode_attn_kernel<__bf16, 1, false, false, true>), grid1, dim3(256), 0, s, p);
        } else if (dtype == WIPA_F32)
            hipLaunchKernelGGL((decode_attn_kernel<float, 4, true, false, true>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((decode_attn_kernel<__bf16, 4, true, false, true>), grid, dim3(256), 0, s, p);
    } else {
#define WIPA_MULTI_G(T, NQ) hipLaunchKernelGGL((decode_attn_multi_kernel<T, NQ, true>), grid, dim3(256), 0, s, p)
        if (dtype == WIPA_F32) {
            if (n_q == 2) WIPA_MULTI_G(float, 2); else if (n_q == 3) WIPA_MULTI_G(float, 3); else WIPA_MULTI_G(float, 4);
        } else {
            if (n_q == 2) WIPA_MULTI_G(__bf16, 2); else if (n_q == 3) WIPA_MULTI_G(__bf16, 3); else WIPA_MULTI_G(__bf16, 4);
        }
#undef WIPA_MULTI_G
    }
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

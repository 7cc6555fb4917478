// K3 LayerNorm, K8 embedding, K13 greedy step, K9 masked cross-entropy, small utilities.
// All HBM-bound row kernels: one wave (LayerNorm) or one workgroup (vocab reductions) per
// row, 8/16-byte vector loads, wave64 shuffle reductions, f32 math.
#include <string.h>

#include "wipa_common.h"
#include "philox.h"
#include "step_rows.h"  // ld4 / st4, MaxIdx, GS_THREADS, row_embed_layernorm, tail_pos, RulesDev: shared with beam.hip

namespace {

// ------------------------------------------------------------------ LayerNorm
constexpr int LN_MAXV = 8;  // D <= 8 * 256 = 2048

// NV = ceil(D / 256) vector iterations per lane: a compile-time bound sized to D keeps the register
// count (and so the waves per SIMD) where an HBM-bound kernel needs it -- with the generic bound of 8
// hipcc hoisted every load and allocated 208 VGPRs = 2 waves/SIMD = 2.1 TB/s on the encoder rows.
template <typename TI, typename TO, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const TI* __restrict__ x, int64_t ldx, TO* __restrict__ y,
                                                        int64_t ldy, const float* __restrict__ w,
                                                        const float* __restrict__ b, int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const TI* xr = x + (int64_t)row * ldx;
    TO* yr = y + (int64_t)row * ldy;
    f32x4 v[NV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < D) {
            v[i] = ld4<TI>(xr + c);
            sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        } else {
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float mean = wave_reduce_sum(sum) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < D) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                sq += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_reduce_sum(sq) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane * 4 + 256 * i;
        if (c < D) {
            const f32x4 ww = *reinterpret_cast<const f32x4*>(w + c);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(b + c);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * ww[e] + bb[e];
            st4<TO>(yr + c, o);
        }
    }
}

// Decode-step variant: ONE workgroup per row (few rows -> spread them over many CUs), fused with
// the fixed-order sum of the split-K partial slabs of the preceding residual GEMM.
constexpr int LN_MAX_SLABS = 16;  // NS = 4 (the split-K residual GEMMs) or 16 (one slab per head from the fused out projections)
template <typename TO, int NS = 4>
__global__ __launch_bounds__(256) void add_slabs_layernorm_kernel(float* __restrict__ x, int64_t ldx,
                                                                   const float* __restrict__ slabs, int n_slabs,
                                                                   int64_t slab_stride, TO* __restrict__ y, int64_t ldy,
                                                                   const float* __restrict__ w, const float* __restrict__ b,
                                                                   int D, float eps) {
    __shared__ float s_red[4];
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* xr = x + (int64_t)row * ldx;
    f32x4 v[2], ww[2], bb[2];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid * 4 + 1024 * i;
        v[i] = ww[i] = bb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < D) {
            // every load of the row (x, up to NS slabs, w, b) is issued before the first use:
            // one memory round trip instead of one per slab
            v[i] = *reinterpret_cast<const f32x4*>(xr + c);
            f32x4 sl[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s)
                sl[s] = (s < n_slabs) ? *reinterpret_cast<const f32x4*>(slabs + (int64_t)s * slab_stride + (int64_t)row * ldx + c)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
            ww[i] = *reinterpret_cast<const f32x4*>(w + c);
            bb[i] = *reinterpret_cast<const f32x4*>(b + c);
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < n_slabs) v[i] += sl[s];  // fixed order s = 0, 1, ...
            if (n_slabs > 0) *reinterpret_cast<f32x4*>(xr + c) = v[i];
            sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    sum = wave_reduce_sum(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    const float mean = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / (float)D;
    __syncthreads();
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (c < D) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                sq += d * d;
            }
        }
    }
    sq = wave_reduce_sum(sq);
    if (lane == 0) s_red[wave] = sq;
    __syncthreads();
    const float rstd = rsqrtf(((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / (float)D + eps);
    TO* yr = y + (int64_t)row * ldy;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid * 4 + 1024 * i;
        if (c < D) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * ww[i][e] + bb[i][e];
            st4<TO>(yr + c, o);
        }
    }
}

// ------------------------------------------------------------------ embedding
// RAGGED (left-padded prompt rows, wipa_embed_tokens_ragged): the token of column p takes the position row p - start[b] (padding
// columns, below start[b], row 0); a separate instantiation, `start` is not looked at otherwise
template <typename TE, bool RAGGED = false>
__global__ __launch_bounds__(256) void embed_kernel(const int32_t* __restrict__ tokens, int64_t ld_tok, int T, int t_start,
                                                    const int32_t* __restrict__ pos_dev, const TE* __restrict__ emb,
                                                    const float* __restrict__ pos_emb, float* __restrict__ x, int D,
                                                    const int32_t* __restrict__ start) {
    const int row = blockIdx.x;  // b*T + t
    const int b = row / T, t = row - b * T;
    const int p = t_start + (pos_dev ? *pos_dev : 0) + t;
    const int tok = tokens[(int64_t)b * ld_tok + p];
    const TE* e = emb + (int64_t)tok * D;
    int pp = p;
    if constexpr (RAGGED) pp = max(p - start[b], 0);
    const float* pe = pos_emb + (int64_t)pp * D;
    float* xr = x + (int64_t)row * D;
    for (int c = threadIdx.x * 4; c < D; c += 1024) {
        const f32x4 a = ld4<TE>(e + c);
        const f32x4 q = *reinterpret_cast<const f32x4*>(pe + c);
        *reinterpret_cast<f32x4*>(xr + c) = a + q;
    }
}

// fp8 (e4m3fn) token embedding: row `tok` of the codes times its per-row scale (the same matrix and scales serve as the
// logits weights, where the scale is per output column)
__global__ __launch_bounds__(256) void embed_fp8_kernel(const int32_t* __restrict__ tokens, int64_t ld_tok, int T, int t_start,
                                                        const int32_t* __restrict__ pos_dev, const unsigned char* __restrict__ emb,
                                                        const float* __restrict__ emb_scale, const float* __restrict__ pos_emb,
                                                        float* __restrict__ x, int D) {
    const int row = blockIdx.x;
    const int b = row / T, t = row - b * T;
    const int p = t_start + (pos_dev ? *pos_dev : 0) + t;
    const int tok = tokens[(int64_t)b * ld_tok + p];
    const unsigned char* e = emb + (int64_t)tok * D;
    const float sc = emb_scale[tok];
    const float* pe = pos_emb + (int64_t)p * D;
    float* xr = x + (int64_t)row * D;
    for (int c = threadIdx.x * 4; c < D; c += 1024) {
        const unsigned int u = *reinterpret_cast<const unsigned int*>(e + c);
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, true);
        const f32x4 q = *reinterpret_cast<const f32x4*>(pe + c);
        // the dequantised value is rounded to bf16 like every stored weight of the bf16 model (code * scale is not exact in bf16)
        const f32x4 a = {(float)(__bf16)(lo[0] * sc), (float)(__bf16)(lo[1] * sc), (float)(__bf16)(hi[0] * sc), (float)(__bf16)(hi[1] * sc)};
        *reinterpret_cast<f32x4*>(xr + c) = a + q;
    }
}

// ------------------------------------------------------------------ block reductions
// Block reductions of a GS_THREADS workgroup (lane, wave: of the calling thread): the wave tree, lane 0's LDS write, ONE barrier, then
// every thread folds the waves IN ORDER -- the order that makes the fused and the unfused step agree bit for bit.  s_v / s_i / s_sum:
// GS_WAVES slots of LDS each.  The fold hands the value back as a float and the column by reference: kept in a MaxIdx it compiles to
// the same compares with their operands swapped.
__device__ __forceinline__ float fold_waves_argmax(const float* s_v, const int* s_i, int& idx) {
    MaxIdx bm{s_v[0], s_i[0]};
#pragma unroll
    for (int w = 1; w < GS_WAVES; ++w) bm = better(bm, MaxIdx{s_v[w], s_i[w]});
    idx = bm.i;
    return bm.v;
}
__device__ __forceinline__ MaxIdx block_argmax(MaxIdx m, int lane, int wave, float* s_v, int* s_i) {
    m = wave_argmax(m);
    if (lane == 0) {
        s_v[wave] = m.v;
        s_i[wave] = m.i;
    }
    __syncthreads();
    m.v = fold_waves_argmax(s_v, s_i, m.i);
    return m;
}
__device__ __forceinline__ float block_sum(float v, int lane, int wave, float* s_sum) {
    v = wave_reduce_sum(v);
    if (lane == 0) s_sum[wave] = v;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < GS_WAVES; ++w) tot += s_sum[w];
    return tot;
}

// The commit of a picked token.  at: the row's column p (at[0] the previous token, at[1] the new one).  The EOT latch (a row whose
// previous token is eot takes eot again and adds no log-probability), the log-probability sum, the token store and the count of rows
// still running.  Two forms.  commit_by_thread0 (the step kernels): thread 0 does all of it.  commit (the tails): EVERY thread
// computes `next` from values all of them hold -- no single-thread section that hands a value to the workgroup through LDS: the
// pattern whose merge-kernel instance misbehaved, DESIGN.md section 8 -- and thread 0 alone writes.  logprob: log_softmax of the
// filtered row at `pick`.
__device__ __forceinline__ void commit_by_thread0(int32_t* at, int eot, int pick, float logprob, float* sum_logprob, int32_t* not_done) {
    if (threadIdx.x == 0) {
        const int prev = at[0];
        int next = pick;
        if (prev == eot) {
            next = eot;
        } else {
            *sum_logprob += logprob;
        }
        at[1] = next;
        if (next != eot) atomicAdd(not_done, 1);
    }
}
__device__ __forceinline__ int commit(int32_t* at, int eot, int pick, float logprob, float* sum_logprob, int32_t* not_done) {
    const int prev = at[0];
    const int next = (prev == eot) ? eot : pick;
    if (threadIdx.x == 0) {
        if (prev != eot) *sum_logprob += logprob;
        at[1] = next;
        if (next != eot) atomicAdd(not_done, 1);
    }
    return next;
}

// the plain filtered row's arg-max (lowest column on ties) and sum of exponentials against it: log_softmax at the arg-max = -log(tot)
struct RowScan {
    MaxIdx top;
    float tot;
};

__global__ __launch_bounds__(GS_THREADS) void greedy_step_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                                 const float* __restrict__ mask_first,
                                                                 const float* __restrict__ mask_always,
                                                                 int32_t* __restrict__ tokens, int64_t ld_tok,
                                                                 const int32_t* __restrict__ pos_dev, int n_init, int eot,
                                                                 float* __restrict__ sum_logprobs,
                                                                 int32_t* __restrict__ not_done) {
    __shared__ float s_v[GS_WAVES];
    __shared__ int s_i[GS_WAVES];
    __shared__ float s_sum[GS_WAVES];
    const int b = blockIdx.x;
    const int p = *pos_dev;
    if (in_prompt(p, n_init)) return;
    const float* mask = step_mask(p, n_init, mask_first, mask_always);
    const float* row = logits + (int64_t)b * ldl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    MaxIdx m{-INFINITY, 0x7fffffff};
    for (int i = tid; i < V; i += GS_THREADS) {
        const float v = row[i] + mask[i];
        m = better(m, MaxIdx{v, i});
    }
    const MaxIdx bm = block_argmax(m, lane, wave, s_v, s_i);
    float se = 0.f;
    for (int i = tid; i < V; i += GS_THREADS) se += __expf(row[i] + mask[i] - bm.v);
    const float tot = block_sum(se, lane, wave, s_sum);
    commit_by_thread0(tokens + ((int64_t)b * ld_tok + p), eot, bm.i, -logf(tot), sum_logprobs + b, not_done);
}

// Register-resident scan for V <= 65536 (every Whisper vocabulary): the filtered row is fetched ONCE with 16-byte loads
// that are all in flight together (13 per thread for V = 51 865), the arg-max and the sum of exponentials both run out of
// registers.  The two-pass scalar kernel above took 30 us per step on 64 rows (latency-bound: 2 x 51 dependent loads).
__device__ __forceinline__ RowScan row_scan_reg(const float* __restrict__ row, const float* __restrict__ mask, int V, float* s_v, int* s_i,
                                                float* s_sum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = V >> 2;
    f32x4 vals[GS_MAXQ];
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
        if (qi < nq) {
            vals[j] = *reinterpret_cast<const f32x4*>(row + 4 * qi) + *reinterpret_cast<const f32x4*>(mask + 4 * qi);
        } else {
            vals[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
    }
    const int ti = 4 * nq + tid;  // the (V mod 4) trailing elements
    const bool has_tail = tid < 4 && ti < V;
    const float tailv = has_tail ? row[ti] + mask[ti] : -INFINITY;
    MaxIdx m{tailv, has_tail ? ti : 0x7fffffff};
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
#pragma unroll
        for (int e = 0; e < 4; ++e) m = better(m, MaxIdx{vals[j][e], qi < nq ? 4 * qi + e : 0x7fffffff});
    }
    const MaxIdx bm = block_argmax(m, lane, wave, s_v, s_i);
    float se = __expf(tailv - bm.v);
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) se += __expf(vals[j][e] - bm.v);
    return RowScan{bm, block_sum(se, lane, wave, s_sum)};
}

__global__ __launch_bounds__(GS_THREADS) void greedy_step_reg_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                                     const float* __restrict__ mask_first,
                                                                     const float* __restrict__ mask_always,
                                                                     int32_t* __restrict__ tokens, int64_t ld_tok,
                                                                     const int32_t* __restrict__ pos_dev, int n_init, int eot,
                                                                     float* __restrict__ sum_logprobs,
                                                                     int32_t* __restrict__ not_done) {
    __shared__ float s_v[GS_WAVES];
    __shared__ int s_i[GS_WAVES];
    __shared__ float s_sum[GS_WAVES];
    const int b = blockIdx.x;
    const int p = *pos_dev;
    if (in_prompt(p, n_init)) return;
    const float* mask = step_mask(p, n_init, mask_first, mask_always);
    const RowScan sc = row_scan_reg(logits + (int64_t)b * ldl, mask, V, s_v, s_i, s_sum);
    commit_by_thread0(tokens + ((int64_t)b * ld_tok + p), eot, sc.top.i, -logf(sc.tot), sum_logprobs + b, not_done);
}

// ------------------------------------------------------------------ decode-step tail / head (round 4)
// A decode step used to end with greedy_step + advance_pos and the next one to begin with embed + the first LayerNorm: four
// launches of 4-16 us whose only content is a few dependent round trips.  greedy_tail_kernel does all of it in the launch that
// already owns the row: arg-max / log-prob of the filtered logits (greedy_step_reg_kernel's arithmetic, unchanged), the EOT
// latch, then x = tok_emb[next] + pos_emb[p + 1] and LayerNorm(x) with the first block's attn_ln for position p + 1, and -- by
// the LAST workgroup to finish (device counter) -- the position advance.  embed_layernorm_kernel is the same row routine alone:
// wipa_decoder_run launches it once before the first step (the prompt walk, forced histories and the first step after a
// prefill start from tokens the tail has not embedded).  The row routine repeats add_slabs_layernorm_kernel's reduction order
// (256 threads, float4 per thread, wave shuffle tree, ((s0+s1)+(s2+s3))), so fused and unfused steps agree bit for bit.
struct TailParams {
    const float* logits; int64_t ldl; int V;
    const float* mask_first; const float* mask_always;
    int32_t* tokens; int64_t ld_tok;
    int32_t* pos; int64_t* posd; int32_t* done_counter;
    int n_init, eot, n_ctx;
    float* sum_logprobs; int32_t* not_done;
    const void* emb; int emb_dtype; const float* emb_scale; const float* pos_emb;
    float* x; const float* ln_w; const float* ln_b; void* y; int D; float eps;
    const float* part; int n_part;  // wipa_logits_greedy's partials [B][3][n_part] instead of the logits (part != nullptr)
};

// Ragged prompts (left-padded rows, one shared column counter): row b's own tokens start at column start[b] (int32 [B], device), so
// its position-embedding index and its sampling counter are column - start[b].  A SEPARATE instantiation of every tail
// (template <..., bool RAGGED>): the kernels of calls without prompts keep their arguments and their code.
template <bool RAGGED>
struct TailArgs : TailParams {};
template <>
struct TailArgs<true> : TailParams {
    const int32_t* start;
};

// the row's position-embedding index at column `col`: clamped to the table, and with ragged prompts counted from the row's own start
template <bool RAGGED>
__device__ __forceinline__ int pos_row(const TailArgs<RAGGED>& q, int b, int col) {
    int pp = min(col, q.n_ctx - 1);
    if constexpr (RAGGED) pp = max(pp - q.start[b], 0);  // padding columns, below start[b], take row 0
    return pp;
}

template <typename TO, bool RAGGED = false>
__global__ __launch_bounds__(256) void embed_layernorm_kernel(TailArgs<RAGGED> q) {
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int p = *q.pos;
    const int tok = q.tokens[(int64_t)b * q.ld_tok + p];
    row_embed_layernorm<TO>(threadIdx.x, tok, pos_row(q, b, p), q.emb, q.emb_dtype, q.emb_scale, q.pos_emb, q.x + (int64_t)b * q.D, q.ln_w,
                            q.ln_b, (TO*)q.y + (int64_t)b * q.D, q.D, q.eps, s_red);
}

// What every tail does after `next` is known (every thread of the workgroup calls it with the same p and next): the next step's
// input row -- the embedding of the chosen token at position p + 1, then the first block's LayerNorm -- and the position advance by
// the LAST workgroup to arrive.  Every thread of every workgroup read *pos at its start (tail_pos) and has used it before the row
// routine's barriers, i.e. before its workgroup's counter increment -- no workgroup can still see the old position late.
// Needs *done_counter == 0 at launch and one launch in flight per state blob: wipa_decoder_run / _prefill zero the counter
// at the start of every call (a launch that died mid-grid must not leave later calls without a position advance)
template <typename TO, bool RAGGED>
__device__ __forceinline__ void tail_finish(const TailArgs<RAGGED>& q, int p, int next, float* s_red) {
    const int b = blockIdx.x;
    row_embed_layernorm<TO>(threadIdx.x, next, pos_row(q, b, p + 1), q.emb, q.emb_dtype, q.emb_scale, q.pos_emb, q.x + (int64_t)b * q.D,
                            q.ln_w, q.ln_b, (TO*)q.y + (int64_t)b * q.D, q.D, q.eps, s_red);
    if (threadIdx.x == 0) {
        const int arrived = atomicAdd(q.done_counter, 1);  // counts arrivals only: what the step wrote reaches the next launch at the kernel boundary
        if (arrived == (int)gridDim.x - 1) {
            *q.done_counter = 0;
            *q.pos = p + 1;
            *q.posd = (int64_t)(p + 1) * q.D;
        }
    }
}

template <typename TO, bool RAGGED = false>
__global__ __launch_bounds__(GS_THREADS) void greedy_tail_kernel(TailArgs<RAGGED> q) {
    __shared__ float s_v[GS_WAVES];
    __shared__ int s_i[GS_WAVES];
    __shared__ float s_sum[GS_WAVES];
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = tail_pos(q.pos);
    int next;
    if (in_prompt(p, q.n_init)) {  // the token is already in place (uniform branch: p is the same for every thread)
        next = q.tokens[(int64_t)b * q.ld_tok + p + 1];
    } else if (q.part) {
        // the logits GEMM left one (max, sum exp, arg-max) per wave of its grid for this row: merge them -- (value, lowest column)
        // for the arg-max, then sum_i s_i exp(m_i - M) in a fixed order (per thread ascending, wave tree, waves in order)
        const float* pm = q.part + (int64_t)b * 3 * q.n_part;
        const float* ps = pm + q.n_part;
        const int* pi = reinterpret_cast<const int*>(pm + 2 * q.n_part);
        MaxIdx m{-INFINITY, 0x7fffffff};
        for (int i = tid; i < q.n_part; i += GS_THREADS) m = better(m, MaxIdx{pm[i], pi[i]});
        const MaxIdx bm = block_argmax(m, lane, wave, s_v, s_i);
        float se = 0.f;
        for (int i = tid; i < q.n_part; i += GS_THREADS) se += ps[i] * __expf(pm[i] - bm.v);
        const float tot = block_sum(se, lane, wave, s_sum);
        next = commit(q.tokens + ((int64_t)b * q.ld_tok + p), q.eot, bm.i, -logf(tot), q.sum_logprobs + b, q.not_done);
    } else {
        const float* mask = step_mask(p, q.n_init, q.mask_first, q.mask_always);
        const RowScan sc = row_scan_reg(q.logits + (int64_t)b * q.ldl, mask, q.V, s_v, s_i, s_sum);
        next = commit(q.tokens + ((int64_t)b * q.ld_tok + p), q.eot, sc.top.i, -logf(sc.tot), q.sum_logprobs + b, q.not_done);
    }
    tail_finish<TO>(q, p, next, s_red);
}

// ------------------------------------------------------------------ timestamp rules in the step's tail
// ApplyTimestampRules of openai-whisper's decoding.py (the algorithm of transformers' WhisperTimeStampLogitsProcessor; mlx_whisper's
// port of it is [UPSTREAM-UNVERIFIED]) on the row the tail already holds in registers.  The rules depend on the row's OWN history
// tokens[b][n_init .. p] (seq) and on a comparison of probability masses, so they cannot be a static vocabulary mask:
//   nt column -inf;  last = seq[-1] >= tb, pen = len(seq) < 2 or seq[-2] >= tb:  last and pen -> no timestamp, last and not pen ->
//   no text below eot;  t = the LAST timestamp of seq in order (a forced history need not be monotone): timestamps below t (below
//   t + 1 unless last and not pen) -inf;  first sampled position: text -inf and timestamps capped at tb + max_initial;  then, over
//   the row as it stands, logsumexp(timestamps) > max(text) -> text -inf.
// Every rule kills a column RANGE, so the filtered row is: text columns (< tb) alive from text_lo on, bar nt; timestamp columns alive
// in [ts_lo, ts_hi].  Two reductions, text side and timestamp side, each (max, lowest column) then a sum of exponentials in the
// fixed order of greedy_tail_kernel (per thread ascending, wave tree, waves in order); the mass comparison and the log-probability
// of the winner come from those four numbers.  Like greedy_tail_kernel, every thread computes `next` from values all of them hold.
struct RowPick {
    int next;        // the arg-max of the filtered row (lowest column on ties)
    float logprob;   // log_softmax of the filtered row at next (thread 0 of the workgroup only)
};

// SAMPLE (temperature above 0): on the SAME filtered row l, next = argmax_c (l[c] / T + g_c) over the alive columns, lowest column on
// ties -- the Gumbel-max form of Categorical(softmax(l / T)): a third (max, lowest column) reduction, no prefix sum, the same result
// in any reduction order.  g_c comes from Philox4x32-10 (philox.h) with key (seed_lo, seed_hi) and counter (c >> 2, p | attempt << 16,
// stream_lo[b], stream_hi[b]); word c & 3 belongs to column c, so one call serves one f32x4 quad of the row, and a quad with nothing
// alive draws nothing.  Rule 5 and the log-probability stay on the UNTEMPERED row: logprob = l[next] - logsumexp(l), with the
// log-sum-exp of the greedy branch (same sums, same order), so it is a fixed function of the row's logits.
// RULES = false: the plain filtered row (r.tb = V: every column is on the text side, no history scan).
// rec: the caller's sampling record (wipa.h: wipa_sample_record_bytes): u32 seed_lo, seed_hi, attempt, f32 1/T, then [lo, hi] per row.
// p_own: the position word of the counter -- p, or with ragged prompts the row's OWN position p - start[b] (a draw must not depend on
// the prompt width the row's neighbours set).
// ROWS (SAMPLE only): rec is the record with a ROW PART (wipa.h: wipa_sample_rows_bytes) -- u32 seed_lo, seed_hi, B, 0, then per row
// [stream_lo, stream_hi, attempt, f32 1/T].  The key and the counter are built from the same words, so a row at (T, attempt) draws what
// the single-temperature record draws for it.  A row whose 1/T is 0 is a GREEDY row: the draw block is skipped and the row keeps the
// greedy answer computed above it.  That branch holds a __syncthreads(); it is uniform because ONE workgroup owns ONE row (b is
// blockIdx.x in every caller), so every thread of the workgroup reads the same 1/T.  ROWS = false compiles to what it was.
template <bool RULES, bool SAMPLE, bool ROWS = false>
__device__ __forceinline__ RowPick row_pick(const float* __restrict__ row, const float* __restrict__ mask, int V, const int32_t* __restrict__ tk,
                                            int p, int n_init, int eot, RulesDev r, float* s_v, int* s_i, float* s_sum,
                                            const uint32_t* __restrict__ rec, int b, int p_own) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = V >> 2;
    // the row's loads go out first; the history scan below hides under them
    f32x4 vals[GS_MAXQ];
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
        if (qi < nq) {
            vals[j] = *reinterpret_cast<const f32x4*>(row + 4 * qi) + *reinterpret_cast<const f32x4*>(mask + 4 * qi);
        } else {
            vals[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
    }
    const int ti = 4 * nq + tid;  // the (V mod 4) trailing elements: timestamp columns for every Whisper vocabulary, but not assumed
    const bool has_tail = tid < 4 && ti < V;
    float tailv = has_tail ? row[ti] + mask[ti] : -INFINITY;
    // history: seq = tk[n_init .. p].  Every WAVE scans all of it (at most n_ctx - n_init tokens, 7 per lane) and reduces with
    // shuffles: no LDS, no barrier, and every thread ends with the same t_idx
    int text_lo = 0, ts_lo = r.tb, ts_hi = V - 1;
    if constexpr (RULES) {
        const int len = p + 1 - n_init;
        int t_idx = -1;  // index in seq of its last timestamp token
        for (int i = lane; i < len; i += 64) t_idx = tk[n_init + i] >= r.tb ? i : t_idx;  // ascending per lane: the last match stays
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t_idx = max(t_idx, __shfl_xor(t_idx, o, 64));
        const bool first = len == 0;
        const bool last = t_idx >= 0 && t_idx == len - 1;
        const bool pen = len < 2 || tk[p - 1] >= r.tb;
        if (last && pen) ts_lo = V;         // a closed pair: text next
        if (last && !pen) text_lo = eot;    // a single timestamp: EOT or a timestamp next
        if (t_idx >= 0) ts_lo = max(ts_lo, tk[n_init + t_idx] + ((last && !pen) ? 0 : 1));
        if (first) {
            text_lo = r.tb;
            if (r.max_init >= 0) ts_hi = min(ts_hi, r.tb + r.max_init);
        }
    }
    auto alive = [&](int c) { return c < r.tb ? (c >= text_lo && c != r.nt) : (c >= ts_lo && c <= ts_hi); };
    MaxIdx mt{-INFINITY, 0x7fffffff}, ms{-INFINITY, 0x7fffffff};  // text side, timestamp side
    if (has_tail) {
        if (!alive(ti)) tailv = -INFINITY;
        if (ti < r.tb) mt = MaxIdx{tailv, ti};
        else ms = MaxIdx{tailv, ti};
    }
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * qi + e;
            if (qi < nq) {
                if (!alive(c)) vals[j][e] = -INFINITY;
                if (c < r.tb) mt = better(mt, MaxIdx{vals[j][e], c});
                else ms = better(ms, MaxIdx{vals[j][e], c});
            }
        }
    }
    // block_argmax / block_sum written out, two sides around ONE barrier each (and once more for the draw's keys below): routed through
    // the helpers the sampling kernels compiled to 350 - 400 bytes of scratch instead of 100 - 136, so this text stays as it is
    mt = wave_argmax(mt);
    ms = wave_argmax(ms);
    constexpr int NW = GS_WAVES;
    if (lane == 0) {
        s_v[wave] = mt.v; s_i[wave] = mt.i;
        s_v[NW + wave] = ms.v; s_i[NW + wave] = ms.i;
    }
    __syncthreads();
    MaxIdx bt{s_v[0], s_i[0]}, bs{s_v[NW], s_i[NW]};
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        bt = better(bt, MaxIdx{s_v[w], s_i[w]});
        bs = better(bs, MaxIdx{s_v[NW + w], s_i[NW + w]});
    }
    // sums of exponentials against each side's own max; a side with nothing alive has max -inf: base 0 keeps exp(-inf - base) = 0
    const float base_t = bt.v == -INFINITY ? 0.f : bt.v, base_s = bs.v == -INFINITY ? 0.f : bs.v;
    float se_t = 0.f, se_s = 0.f;
    if (has_tail) {
        if (ti < r.tb) se_t += __expf(tailv - base_t);
        else se_s += __expf(tailv - base_s);
    }
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool text = 4 * qi + e < r.tb;  // padding quads hold -inf: exp gives 0 on either side
            const float ex = __expf(vals[j][e] - (text ? base_t : base_s));
            se_t += text ? ex : 0.f;
            se_s += text ? 0.f : ex;
        }
    }
    se_t = wave_reduce_sum(se_t);
    se_s = wave_reduce_sum(se_s);
    if (lane == 0) {
        s_sum[wave] = se_t;
        s_sum[NW + wave] = se_s;
    }
    __syncthreads();
    float tot_t = 0.f, tot_s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        tot_t += s_sum[w];
        tot_s += s_sum[NW + w];
    }
    // timestamp mass against the best text token: the common normaliser cancels; false when no timestamp is alive
    const float ts_mass = bs.v == -INFINITY ? -INFINITY : bs.v + logf(tot_s);
    RowPick out;
    float top_v;  // l at the arg-max: logsumexp(l) = top_v - out.logprob
    if (ts_mass > bt.v) {  // text -inf: the row is its timestamp side
        out.next = bs.i;
        out.logprob = -logf(tot_s);
        top_v = bs.v;
    } else {
        const MaxIdx bm = better(bt, bs);
        out.next = bm.i;
        out.logprob = -logf(tot_t * __expf(base_t - bm.v) + (bs.v == -INFINITY ? 0.f : tot_s * __expf(base_s - bm.v)));
        top_v = bm.v;
    }
    if constexpr (SAMPLE) {
        const int dead_below = ts_mass > bt.v ? r.tb : 0;  // rule 5 killed the text side
        const float inv_t = __uint_as_float(ROWS ? rec[7 + 4 * b] : rec[3]);
        const uint32_t k0 = rec[0], k1 = rec[1], c1 = (uint32_t)p_own | ((ROWS ? rec[6 + 4 * b] : rec[2]) << 16),
                       c2 = ROWS ? rec[4 + 4 * b] : rec[4 + 2 * b], c3 = ROWS ? rec[5 + 4 * b] : rec[5 + 2 * b];
        if constexpr (ROWS) {
            if (inv_t == 0.f) return out;  // a greedy row; uniform over the workgroup (one row per workgroup): the barrier below is reached by all or none
        }
        MaxIdx mk{-INFINITY, 0x7fffffff};
        if (has_tail && ti >= dead_below && tailv > -INFINITY) {
            const Philox4 x = philox4x32_10((uint32_t)nq, c1, c2, c3, k0, k1);
            const uint32_t word = tid == 0 ? x.w[0] : tid == 1 ? x.w[1] : tid == 2 ? x.w[2] : x.w[3];  // has_tail: tid < 4
            mk = MaxIdx{fmaf(tailv, inv_t, gumbel_from_word(word)), ti};
        }
#pragma unroll
        for (int j = 0; j < GS_MAXQ; ++j) {
            const int qi = tid + j * GS_THREADS;
            bool any = false;  // padding quads and dead columns hold -inf
#pragma unroll
            for (int e = 0; e < 4; ++e) any = any || (4 * qi + e >= dead_below && vals[j][e] > -INFINITY);
            if (any) {
                const Philox4 x = philox4x32_10((uint32_t)qi, c1, c2, c3, k0, k1);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * qi + e >= dead_below && vals[j][e] > -INFINITY)
                        mk = better(mk, MaxIdx{fmaf(vals[j][e], inv_t, gumbel_from_word(x.w[e])), 4 * qi + e});
            }
        }
        mk = wave_argmax(mk);
        // s_v / s_i were last read before the barrier above the sums: every thread is past it
        if (lane == 0) {
            s_v[wave] = mk.v;
            s_i[wave] = mk.i;
        }
        __syncthreads();
        MaxIdx bk{s_v[0], s_i[0]};
#pragma unroll
        for (int w = 1; w < NW; ++w) bk = better(bk, MaxIdx{s_v[w], s_i[w]});
        if (bk.i != 0x7fffffff) {  // a row with nothing alive keeps the greedy answer
            out.logprob = ((row[bk.i] + mask[bk.i]) - top_v) + out.logprob;
            out.next = bk.i;
        }
    }
    return out;
}

// The step kernels with rules and / or the draw (no embedding): greedy_step_reg_kernel's walk test and thread-0 commit around row_pick.
// start: RAGGED && SAMPLE only -- the position word of the draw's counter is the row's own position (not looked at otherwise)
template <bool RULES, bool SAMPLE, bool RAGGED>
__device__ __forceinline__ void pick_step(const float* __restrict__ logits, int64_t ldl, int V, const float* __restrict__ mask_first,
                                          const float* __restrict__ mask_always, int32_t* __restrict__ tokens, int64_t ld_tok,
                                          const int32_t* __restrict__ pos_dev, int n_init, int eot, RulesDev r, const uint32_t* __restrict__ rec,
                                          float* __restrict__ sum_logprobs, int32_t* __restrict__ not_done, const int32_t* __restrict__ start,
                                          float* s_v, int* s_i, float* s_sum) {
    const int b = blockIdx.x;
    const int p = *pos_dev;
    if (in_prompt(p, n_init)) return;
    int32_t* tk = tokens + (int64_t)b * ld_tok;
    int p_own = p;
    if constexpr (SAMPLE && RAGGED) p_own = max(p - start[b], 0);
    const RowPick pick = row_pick<RULES, SAMPLE>(logits + (int64_t)b * ldl, step_mask(p, n_init, mask_first, mask_always), V, tk, p, n_init, eot, r,
                                                 s_v, s_i, s_sum, rec, b, p_own);
    commit_by_thread0(tk + p, eot, pick.next, pick.logprob, sum_logprobs + b, not_done);
}

// The tails with rules and / or the draw: greedy_tail_kernel with row_pick in the place of the plain row scan -- the same prompt walk,
// EOT latch, next embedding + LayerNorm (so the next step's input row has the bits the plain tail would give for the same token) and
// position advance
template <typename TO, bool RULES, bool SAMPLE, bool RAGGED>
__device__ __forceinline__ void pick_tail(const TailArgs<RAGGED>& q, RulesDev r, const uint32_t* __restrict__ rec, float* s_v, int* s_i,
                                          float* s_sum, float* s_red) {
    const int b = blockIdx.x;
    const int p = tail_pos(q.pos);
    int32_t* tk = q.tokens + (int64_t)b * q.ld_tok;
    int next;
    if (in_prompt(p, q.n_init)) {
        next = tk[p + 1];
    } else {
        int p_own = p;  // the position word of the draw's counter: the row's own position
        if constexpr (SAMPLE && RAGGED) p_own = max(p - q.start[b], 0);
        const RowPick pick = row_pick<RULES, SAMPLE>(q.logits + (int64_t)b * q.ldl, step_mask(p, q.n_init, q.mask_first, q.mask_always), q.V, tk, p,
                                                     q.n_init, q.eot, r, s_v, s_i, s_sum, rec, b, p_own);
        next = commit(tk + p, q.eot, pick.next, pick.logprob, q.sum_logprobs + b, q.not_done);
    }
    tail_finish<TO>(q, p, next, s_red);
}

// wipa_timestamp_step: wipa_greedy_step with the rules, no embedding
__global__ __launch_bounds__(GS_THREADS) void timestamp_step_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                                    const float* __restrict__ mask_first, const float* __restrict__ mask_always,
                                                                    int32_t* __restrict__ tokens, int64_t ld_tok, const int32_t* __restrict__ pos_dev,
                                                                    int n_init, int eot, RulesDev r, float* __restrict__ sum_logprobs,
                                                                    int32_t* __restrict__ not_done) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    pick_step<true, false, false>(logits, ldl, V, mask_first, mask_always, tokens, ld_tok, pos_dev, n_init, eot, r, nullptr, sum_logprobs, not_done,
                                  nullptr, s_v, s_i, s_sum);
}

// wipa_timestamp_step_embed: the step's tail with the rules
template <typename TO, bool RAGGED = false>
__global__ __launch_bounds__(GS_THREADS) void timestamp_tail_kernel(TailArgs<RAGGED> q, RulesDev r) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    __shared__ float s_red[4];
    pick_tail<TO, true, false>(q, r, nullptr, s_v, s_i, s_sum, s_red);
}

// wipa_sample_step: timestamp_step_kernel with the draw (RULES = false: wipa_greedy_step with the draw)
template <bool RULES, bool RAGGED = false>
__global__ __launch_bounds__(GS_THREADS) void sample_step_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                                 const float* __restrict__ mask_first, const float* __restrict__ mask_always,
                                                                 int32_t* __restrict__ tokens, int64_t ld_tok, const int32_t* __restrict__ pos_dev,
                                                                 int n_init, int eot, RulesDev r, const uint32_t* __restrict__ rec,
                                                                 float* __restrict__ sum_logprobs, int32_t* __restrict__ not_done,
                                                                 const int32_t* __restrict__ start) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    pick_step<RULES, true, RAGGED>(logits, ldl, V, mask_first, mask_always, tokens, ld_tok, pos_dev, n_init, eot, r, rec, sum_logprobs, not_done, start,
                                   s_v, s_i, s_sum);
}

// wipa_sample_step_embed: the tail of a decode step at a temperature above 0, with and without rules
template <typename TO, bool RULES, bool RAGGED = false>
__global__ __launch_bounds__(GS_THREADS) void sample_tail_kernel(TailArgs<RAGGED> q, RulesDev r, const uint32_t* __restrict__ rec) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    __shared__ float s_red[4];
    pick_tail<TO, RULES, true>(q, r, rec, s_v, s_i, s_sum, s_red);
}

// ------------------------------------------------------------------ continuous batching: the CONTINUOUS tails
// The RAGGED tails with a prompt end PER ROW (wipa_decode_call.continuous): the rows of a state are slots, and a slot's clip was admitted
// at its own column.  q.start is int32 [2][B]: start[b] is the row's first own column, start[B + b] the number of tokens it may generate.
// With own = start[b] + n_init (the row's first generated column), the step at column p
//   p + 1 <  own          the row is idle or in its prompt: the token of column p + 1 is taken as it stands, nothing is written, nothing
//                         is counted in not_done, sum_logprobs[b] is not touched;
//   p + 1 == own          the pick under mask_first;  own < p + 1 < own + limit: the pick under mask_always;
//   p + 1 >= own + limit  the row has generated what it may: column p + 1 takes eot without a log-probability, and the EOT latch of
//                         `commit` holds it from there on.
// The latch is read from the token of column p, so a slot leaves it when wipa_decoder_admit_rows writes the next clip's initial tokens
// over the finished row's last column: nothing is kept per row but the tokens, the two arrays and the log-probability sum.
// Position embedding (pos_row), the next step's input row and the position advance are the RAGGED ones (tail_finish<TO, true>); the draw's
// counter takes the row's own position p - start[b], as in the RAGGED sampling tail.  New kernels beside the RAGGED instantiations: those
// keep their code.  A step at the last column of the table (p + 1 >= n_ctx) does nothing at all, position advance included.
struct ContinuousRow {
    int own, limit;
};
__device__ __forceinline__ ContinuousRow continuous_row(const TailArgs<true>& q, int b) {
    return ContinuousRow{q.start[b] + q.n_init, q.start[(int)gridDim.x + b]};
}

template <typename TO>
__global__ __launch_bounds__(GS_THREADS) void greedy_tail_continuous_kernel(TailArgs<true> q) {
    __shared__ float s_v[GS_WAVES];
    __shared__ int s_i[GS_WAVES];
    __shared__ float s_sum[GS_WAVES];
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int p = tail_pos(q.pos);
    if (p + 1 >= q.n_ctx) return;  // uniform over the grid: no token column, no K / V row and no position row lies past the table
    const ContinuousRow r = continuous_row(q, b);
    int32_t* tk = q.tokens + (int64_t)b * q.ld_tok;
    int next;
    if (p + 1 < r.own) {  // uniform over the workgroup: one row per workgroup
        next = tk[p + 1];
    } else if (p + 1 >= r.own + r.limit) {
        next = q.eot;
        if (threadIdx.x == 0) tk[p + 1] = next;
    } else {
        const float* mask = (p + 1 == r.own) ? q.mask_first : q.mask_always;
        const RowScan sc = row_scan_reg(q.logits + (int64_t)b * q.ldl, mask, q.V, s_v, s_i, s_sum);
        next = commit(tk + p, q.eot, sc.top.i, -logf(sc.tot), q.sum_logprobs + b, q.not_done);
    }
    tail_finish<TO>(q, p, next, s_red);
}

template <typename TO>
__global__ __launch_bounds__(GS_THREADS) void sample_tail_continuous_kernel(TailArgs<true> q, const uint32_t* __restrict__ rec) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int p = tail_pos(q.pos);
    if (p + 1 >= q.n_ctx) return;
    const ContinuousRow r = continuous_row(q, b);
    int32_t* tk = q.tokens + (int64_t)b * q.ld_tok;
    int next;
    if (p + 1 < r.own) {
        next = tk[p + 1];
    } else if (p + 1 >= r.own + r.limit) {
        next = q.eot;
        if (threadIdx.x == 0) tk[p + 1] = next;
    } else {
        const float* mask = (p + 1 == r.own) ? q.mask_first : q.mask_always;
        const RulesDev none = {q.V, -1, -1};  // no rules: every column is on the text side
        const RowPick pick = row_pick<false, true>(q.logits + (int64_t)b * q.ldl, mask, q.V, tk, p, q.n_init, q.eot, none, s_v, s_i, s_sum, rec, b,
                                                   max(p - q.start[b], 0));
        next = commit(tk + p, q.eot, pick.next, pick.logprob, q.sum_logprobs + b, q.not_done);
    }
    tail_finish<TO>(q, p, next, s_red);
}

// The CONTINUOUS tails with the timestamp rules (wipa_decode_call.continuous and .rules).  The four cases above stay; the pick is
// row_pick<true, SAMPLE> on the row's OWN sequence tk[own .. p]: row_pick's n_init argument is nothing but the first column of the sequence
// it scans, so `own` in its place states the rule -- len = p + 1 - own, the pick is "first" (text dead, timestamps capped) when p + 1 == own,
// and no token below own is looked at: those belong to the slot's previous clip, which usually ended in timestamps, or to the prompt.  A
// column shift moves start and the tokens together, so own moves with the sequence and the pick cannot see it.
// The no-speech probability: at the step whose column is the row's <|startoftranscript|> (p == start[b], limit > 0) the logits row is
// upstream's logits[:, sot_index]; softmax(row)[no_speech_token] of the UNFILTERED row goes to no_speech[b] -- row_scan_reg's loads and
// reduction order without the mask, a plain store by thread 0.  With n_init == 1 the same step also picks: the scan's LDS slots are free
// again once every thread has left block_sum's barrier, and row_pick writes s_sum only behind a barrier of its own.
__device__ __forceinline__ void row_no_speech(const float* __restrict__ row, int V, int token, float* __restrict__ out, float* s_v, int* s_i,
                                              float* s_sum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = V >> 2;
    f32x4 vals[GS_MAXQ];
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
        vals[j] = qi < nq ? *reinterpret_cast<const f32x4*>(row + 4 * qi) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }
    const int ti = 4 * nq + tid;  // the (V mod 4) trailing elements
    const bool has_tail = tid < 4 && ti < V;
    const float tailv = has_tail ? row[ti] : -INFINITY;
    MaxIdx m{tailv, has_tail ? ti : 0x7fffffff};
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
#pragma unroll
        for (int e = 0; e < 4; ++e) m = better(m, MaxIdx{vals[j][e], qi < nq ? 4 * qi + e : 0x7fffffff});
    }
    const MaxIdx bm = block_argmax(m, lane, wave, s_v, s_i);
    float se = __expf(tailv - bm.v);
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) se += __expf(vals[j][e] - bm.v);
    const float tot = block_sum(se, lane, wave, s_sum);
    if (tid == 0) *out = __expf(row[token] - bm.v) / tot;
}

template <typename TO, bool SAMPLE>
__global__ __launch_bounds__(GS_THREADS) void rules_tail_continuous_kernel(TailArgs<true> q, RulesDev rules, const uint32_t* __restrict__ rec,
                                                                           float* __restrict__ no_speech, int no_speech_token) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int p = tail_pos(q.pos);
    if (p + 1 >= q.n_ctx) return;
    const ContinuousRow r = continuous_row(q, b);
    int32_t* tk = q.tokens + (int64_t)b * q.ld_tok;
    const float* row = q.logits + (int64_t)b * q.ldl;
    if (no_speech && r.limit > 0 && p + q.n_init == r.own) {  // p == start[b]; uniform over the workgroup
        row_no_speech(row, q.V, no_speech_token, no_speech + b, s_v, s_i, s_sum);
        __syncthreads();
    }
    int next;
    if (p + 1 < r.own) {
        next = tk[p + 1];
    } else if (p + 1 >= r.own + r.limit) {
        next = q.eot;
        if (threadIdx.x == 0) tk[p + 1] = next;
    } else {
        const float* mask = (p + 1 == r.own) ? q.mask_first : q.mask_always;
        const RowPick pick = row_pick<true, SAMPLE>(row, mask, q.V, tk, p, r.own, q.eot, rules, s_v, s_i, s_sum, rec, b, max(p - q.start[b], 0));
        next = commit(tk + p, q.eot, pick.next, pick.logprob, q.sum_logprobs + b, q.not_done);
    }
    tail_finish<TO>(q, p, next, s_red);
}

// The CONTINUOUS tails with a TEMPERATURE PER ROW (wipa_decode_call.sample_rows): rules_tail_continuous_kernel<TO, true> (RULES) and
// sample_tail_continuous_kernel (no rules) with the row's 1/T, attempt and stream read from the row's entry of the record with a row part
// (row_pick<RULES, true, true>).  The four cases, the no-speech store at p == start[b], `commit` and `tail_finish` are those kernels'.  A
// greedy row (1/T == 0) leaves row_pick with the greedy answer before the draw: the branch is uniform over the workgroup because one
// workgroup owns one row, so a retried window sits beside greedy first attempts and beside retries at other temperatures in ONE launch.
template <typename TO, bool RULES>
__global__ __launch_bounds__(GS_THREADS) void rows_tail_continuous_kernel(TailArgs<true> q, RulesDev rules, const uint32_t* __restrict__ rec,
                                                                          float* __restrict__ no_speech, int no_speech_token) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int p = tail_pos(q.pos);
    if (p + 1 >= q.n_ctx) return;
    const ContinuousRow r = continuous_row(q, b);
    int32_t* tk = q.tokens + (int64_t)b * q.ld_tok;
    const float* row = q.logits + (int64_t)b * q.ldl;
    if constexpr (RULES) {
        if (no_speech && r.limit > 0 && p + q.n_init == r.own) {  // p == start[b]; uniform over the workgroup
            row_no_speech(row, q.V, no_speech_token, no_speech + b, s_v, s_i, s_sum);
            __syncthreads();
        }
    }
    int next;
    if (p + 1 < r.own) {
        next = tk[p + 1];
    } else if (p + 1 >= r.own + r.limit) {
        next = q.eot;
        if (threadIdx.x == 0) tk[p + 1] = next;
    } else {
        const float* mask = (p + 1 == r.own) ? q.mask_first : q.mask_always;
        // RULES: the row's own sequence tk[own .. p]; without rules row_pick does not look at its n_init argument
        const RowPick pick = row_pick<RULES, true, true>(row, mask, q.V, tk, p, RULES ? r.own : q.n_init, q.eot, rules, s_v, s_i, s_sum, rec, b,
                                                         max(p - q.start[b], 0));
        next = commit(tk + p, q.eot, pick.next, pick.logprob, q.sum_logprobs + b, q.not_done);
    }
    tail_finish<TO>(q, p, next, s_red);
}

// The PROMPTED tails (wipa_decode_call.prompted): the CONTINUOUS tails for rows that carry a PROMPT in front of their
// admission column.  q.start is int32 [3][B]: start[b] is the row's window start (its first prompt column: what the RAGGED attention,
// the position rows and tail_finish read, as they read it in every continuous step), start[B + b] the tokens it may generate and
// start[2 B + b] its prompt columns L (0: no prompt).  The row's sot sequence stands at [start + L, start + L + n_init), so
//   own = start + L + n_init;   the no-speech store fires at p == start + L, i.e. p + n_init == own;   the rules scan tk[own .. p];
//   the draw's counter stays p - start[b], the row's position in its own unpadded sequence [sot_prev] + history + sot sequence + ...
// Everything else is the CONTINUOUS tails' four cases, on the same device functions (row_scan_reg / row_pick, row_no_speech, commit,
// tail_finish).  ONE body for the six (rules, draw) cases, as NEW kernels: the CONTINUOUS kernels above keep their symbols and their code.
enum TailDraw { DRAW_NONE = 0, DRAW_RECORD = 1, DRAW_ROWS = 2 };  // greedy | the single-temperature record | a temperature per row

template <typename TO, bool RULES, int DRAW>
__global__ __launch_bounds__(GS_THREADS) void tail_prompted_kernel(TailArgs<true> q, RulesDev rules, const uint32_t* __restrict__ rec,
                                                                   float* __restrict__ no_speech, int no_speech_token) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    __shared__ float s_red[4];
    const int b = blockIdx.x, B = (int)gridDim.x;
    const int p = tail_pos(q.pos);
    if (p + 1 >= q.n_ctx) return;  // uniform over the grid, as in the CONTINUOUS tails
    const int start = q.start[b], limit = q.start[B + b], own = start + q.start[2 * B + b] + q.n_init;
    int32_t* tk = q.tokens + (int64_t)b * q.ld_tok;
    const float* row = q.logits + (int64_t)b * q.ldl;
    if constexpr (RULES) {
        if (no_speech && limit > 0 && p + q.n_init == own) {  // p is the row's <|startoftranscript|> column; uniform over the workgroup
            row_no_speech(row, q.V, no_speech_token, no_speech + b, s_v, s_i, s_sum);
            __syncthreads();
        }
    }
    int next;
    if (p + 1 < own) {  // idle, in its prompt or in its sot sequence: the token is taken as it stands
        next = tk[p + 1];
    } else if (p + 1 >= own + limit) {
        next = q.eot;
        if (threadIdx.x == 0) tk[p + 1] = next;
    } else {
        const float* mask = (p + 1 == own) ? q.mask_first : q.mask_always;
        if constexpr (!RULES && DRAW == DRAW_NONE) {
            const RowScan sc = row_scan_reg(row, mask, q.V, s_v, s_i, s_sum);
            next = commit(tk + p, q.eot, sc.top.i, -logf(sc.tot), q.sum_logprobs + b, q.not_done);
        } else {
            // RULES: the row's own sequence tk[own .. p]; without rules row_pick does not look at its n_init argument
            const RowPick pick = row_pick<RULES, DRAW != DRAW_NONE, DRAW == DRAW_ROWS>(row, mask, q.V, tk, p, RULES ? own : q.n_init, q.eot, rules, s_v,
                                                                                        s_i, s_sum, rec, b, max(p - start, 0));
            next = commit(tk + p, q.eot, pick.next, pick.logprob, q.sum_logprobs + b, q.not_done);
        }
    }
    tail_finish<TO>(q, p, next, s_red);
}

// wipa_sample_rows_set: one row's entry of the record with a row part.  One thread; a slot outside the record's rows (its header holds
// B) is not written.
__global__ void sample_rows_set_kernel(uint32_t* rec, int slot, uint32_t stream_lo, uint32_t stream_hi, uint32_t attempt, float inv_t) {
    if (slot < 0 || (uint32_t)slot >= rec[2]) return;
    uint32_t* e = rec + 4 + 4 * slot;
    e[0] = stream_lo;
    e[1] = stream_hi;
    e[2] = attempt;
    e[3] = __float_as_uint(inv_t);
}

// wipa_sample_noise: g_c of one (row, position), c < V -- the numbers the sampling tails add, for measurement
__global__ __launch_bounds__(256) void sample_noise_kernel(const uint32_t* __restrict__ rec, int row, int p, int V, float* __restrict__ out) {
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (4 * qi >= V) return;
    const Philox4 x = philox4x32_10((uint32_t)qi, (uint32_t)p | (rec[2] << 16), rec[4 + 2 * row], rec[5 + 2 * row], rec[0], rec[1]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * qi + e < V) out[4 * qi + e] = gumbel_from_word(x.w[e]);
}

__global__ void add_i32_kernel(int32_t* p, int32_t v) { *p += v; }

// ------------------------------------------------------------------ masked cross entropy
constexpr int CE_THREADS = 512;
__global__ __launch_bounds__(CE_THREADS) void masked_ce_rows_kernel(const float* __restrict__ logits, int64_t ldl,
                                                                    const int32_t* __restrict__ tokens, int64_t ld_tok,
                                                                    int T, int V, int eot, float* __restrict__ row_buf,
                                                                    int rows) {
    __shared__ float s_red[CE_THREADS / 64];
    const int r = blockIdx.x;
    const int b = r / T, t = r - b * T;
    const int32_t* tk = tokens + (int64_t)b * ld_tok;
    const int tgt = tk[t + 1];
    const float* row = logits + (int64_t)r * ldl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mx = -INFINITY;
    for (int i = tid; i < V; i += CE_THREADS) mx = fmaxf(mx, row[i]);
    mx = wave_reduce_max(mx);
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int w = 1; w < CE_THREADS / 64; ++w) mx = fmaxf(mx, s_red[w]);
    __syncthreads();
    float se = 0.f;
    for (int i = tid; i < V; i += CE_THREADS) se += __expf(row[i] - mx);
    se = wave_reduce_sum(se);
    if (lane == 0) s_red[wave] = se;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < CE_THREADS / 64; ++w) tot += s_red[w];
        const float ce = logf(tot) + mx - row[tgt];
        // mask = (tgt != eot) | (cumsum(tgt == eot) == 1)      (train_whisper_ipa.py:242-247)
        bool keep = true;
        if (tgt == eot) {
            int c = 0;
            for (int u = 0; u <= t; ++u) c += (tk[u + 1] == eot);
            keep = (c == 1);
        }
        row_buf[r] = keep ? ce : 0.f;
        row_buf[rows + r] = keep ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void sum2_kernel(const float* __restrict__ row_buf, int rows, float* __restrict__ out2) {
    // deterministic: fixed-order tree over a single workgroup
    __shared__ float s_a[256], s_b[256];
    float a = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < rows; i += 256) {
        a += row_buf[i];
        c += row_buf[rows + i];
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_a[threadIdx.x] += s_a[threadIdx.x + o];
            s_b[threadIdx.x] += s_b[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out2[0] = s_a[0];
        out2[1] = s_b[0];
    }
}

// ------------------------------------------------------------------ mel pad + cast
template <typename TO>
__global__ __launch_bounds__(256) void mel_pad_cast_kernel(const float* __restrict__ mel, int n_mels, TO* __restrict__ out,
                                                           int64_t total) {
    // out [B, 3002, n_mels]; row 0 and 3001 zero, row t+1 = mel[b][t]
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t per = (int64_t)(WIPA_N_FRAMES + 2) * n_mels;
    const int64_t b = i / per;
    const int64_t r = i - b * per;
    const int row = (int)(r / n_mels);
    float v = 0.f;
    if (row >= 1 && row <= WIPA_N_FRAMES) v = mel[b * (int64_t)WIPA_N_FRAMES * n_mels + (r - n_mels)];
    out[i] = from_f32<TO>(v);
}

// the same for the first n_frames frames of every clip (short audio context: an encoder on n_frames / 2 positions)
template <typename TO>
__global__ __launch_bounds__(256) void mel_pad_cast_frames_kernel(const float* __restrict__ mel, int64_t clip_stride, int n_mels,
                                                                  int n_frames, TO* __restrict__ out, int64_t total) {
    // out [B, n_frames + 2, n_mels]; row 0 and n_frames + 1 zero, row t+1 = mel[b][t]
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t per = (int64_t)(n_frames + 2) * n_mels;
    const int64_t b = i / per;
    const int64_t r = i - b * per;
    const int row = (int)(r / n_mels);
    float v = 0.f;
    if (row >= 1 && row <= n_frames) v = mel[b * clip_stride + (r - n_mels)];
    out[i] = from_f32<TO>(v);
}

}  // namespace

extern "C" int wipa_layernorm(const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy, const float* w,
                              const float* b, int rows, int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(x && y && w && b, "wipa_layernorm: null pointer");
    WIPA_REQUIRE(D % 4 == 0 && D <= LN_MAXV * 256 && D > 0, "wipa_layernorm: D=%d must be a multiple of 4 and <= %d", D,
                 LN_MAXV * 256);
    WIPA_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0, "wipa_layernorm: ldx/ldy must be multiples of 4");
    if (rows <= 0) return WIPA_OK;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((rows + 3) / 4), block(256);
    const int nv = (D + 255) / 256;
#define LN_LAUNCH_NV(TI, TO, NV) \
    hipLaunchKernelGGL((layernorm_kernel<TI, TO, NV>), grid, block, 0, s, (const TI*)x, ldx, (TO*)y, ldy, w, b, rows, D, eps)
#define LN_LAUNCH(TI, TO)                      \
    do {                                       \
        if (nv <= 1) LN_LAUNCH_NV(TI, TO, 1);      \
        else if (nv <= 2) LN_LAUNCH_NV(TI, TO, 2); \
        else if (nv <= 3) LN_LAUNCH_NV(TI, TO, 3); \
        else if (nv <= 4) LN_LAUNCH_NV(TI, TO, 4); \
        else if (nv <= 5) LN_LAUNCH_NV(TI, TO, 5); \
        else LN_LAUNCH_NV(TI, TO, 8);              \
    } while (0)
    if (x_dtype == WIPA_F32 && y_dtype == WIPA_F32) LN_LAUNCH(float, float);
    else if (x_dtype == WIPA_F32 && y_dtype == WIPA_BF16) LN_LAUNCH(float, __bf16);
    else if (x_dtype == WIPA_BF16 && y_dtype == WIPA_BF16) LN_LAUNCH(__bf16, __bf16);
    else if (x_dtype == WIPA_BF16 && y_dtype == WIPA_F32) LN_LAUNCH(__bf16, float);
    else WIPA_REQUIRE(false, "wipa_layernorm: bad dtypes %d %d", x_dtype, y_dtype);
#undef LN_LAUNCH
#undef LN_LAUNCH_NV
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_add_slabs_layernorm(float* x, int64_t ldx, const float* slabs, int n_slabs, int64_t slab_stride, void* y,
                                        int y_dtype, int64_t ldy, const float* w, const float* b, int rows, int D, float eps,
                                        wipa_stream_t stream) {
    WIPA_REQUIRE(x && y && w && b && (slabs || n_slabs == 0), "wipa_add_slabs_layernorm: null pointer");
    WIPA_REQUIRE(n_slabs >= 0 && n_slabs <= LN_MAX_SLABS, "wipa_add_slabs_layernorm: n_slabs=%d (max %d)", n_slabs, LN_MAX_SLABS);
    WIPA_REQUIRE(D % 4 == 0 && D > 0 && D <= 2048, "wipa_add_slabs_layernorm: D=%d must be a multiple of 4 and <= 2048", D);
    WIPA_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && slab_stride % 4 == 0, "wipa_add_slabs_layernorm: strides must be multiples of 4");
    if (rows <= 0) return WIPA_OK;
    hipStream_t s = (hipStream_t)stream;
    WIPA_REQUIRE(y_dtype == WIPA_F32 || y_dtype == WIPA_BF16, "wipa_add_slabs_layernorm: bad dtype %d", y_dtype);
#define LN_SLABS(TO, NS)                                                                                                          \
    hipLaunchKernelGGL((add_slabs_layernorm_kernel<TO, NS>), dim3(rows), dim3(256), 0, s, x, ldx, slabs, n_slabs, slab_stride, (TO*)y, \
                       ldy, w, b, D, eps)
    if (y_dtype == WIPA_F32) {
        if (n_slabs <= 4) LN_SLABS(float, 4);
        else LN_SLABS(float, 16);
    } else {
        if (n_slabs <= 4) LN_SLABS(__bf16, 4);
        else LN_SLABS(__bf16, 16);
    }
#undef LN_SLABS
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_embed_tokens(const int32_t* tokens, int64_t ld_tok, int B, int T, int t_start, const int32_t* pos_dev,
                                 const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, float* x, int D,
                                 wipa_stream_t stream) {
    WIPA_REQUIRE(tokens && tok_emb && pos_emb && x, "wipa_embed_tokens: null pointer");
    WIPA_REQUIRE(emb_dtype != WIPA_FP8_E4M3 || emb_scale, "wipa_embed_tokens: fp8 embedding needs emb_scale");
    WIPA_REQUIRE(D % 4 == 0, "wipa_embed_tokens: D must be a multiple of 4");
    if (B * T <= 0) return WIPA_OK;
    hipStream_t s = (hipStream_t)stream;
    if (emb_dtype == WIPA_F32)
        hipLaunchKernelGGL((embed_kernel<float>), dim3(B * T), dim3(256), 0, s, tokens, ld_tok, T, t_start, pos_dev,
                           (const float*)tok_emb, pos_emb, x, D, (const int32_t*)nullptr);
    else if (emb_dtype == WIPA_BF16)
        hipLaunchKernelGGL((embed_kernel<__bf16>), dim3(B * T), dim3(256), 0, s, tokens, ld_tok, T, t_start, pos_dev,
                           (const __bf16*)tok_emb, pos_emb, x, D, (const int32_t*)nullptr);
    else if (emb_dtype == WIPA_FP8_E4M3)
        hipLaunchKernelGGL(embed_fp8_kernel, dim3(B * T), dim3(256), 0, s, tokens, ld_tok, T, t_start, pos_dev,
                           (const unsigned char*)tok_emb, emb_scale, pos_emb, x, D);
    else
        WIPA_REQUIRE(false, "wipa_embed_tokens: bad dtype %d", emb_dtype);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_embed_tokens_ragged(const int32_t* tokens, int64_t ld_tok, int B, int T, const int32_t* starts_dev, const void* tok_emb,
                                        int emb_dtype, const float* pos_emb, float* x, int D, wipa_stream_t stream) {
    WIPA_REQUIRE(tokens && starts_dev && tok_emb && pos_emb && x, "wipa_embed_tokens_ragged: null pointer (starts_dev is required)");
    WIPA_REQUIRE(emb_dtype == WIPA_F32 || emb_dtype == WIPA_BF16, "wipa_embed_tokens_ragged: f32 or bf16 embedding (got %d)", emb_dtype);
    WIPA_REQUIRE(D % 4 == 0 && B > 0 && T > 0, "wipa_embed_tokens_ragged: D must be a multiple of 4, B and T positive");
    hipStream_t s = (hipStream_t)stream;
    if (emb_dtype == WIPA_F32)
        hipLaunchKernelGGL((embed_kernel<float, true>), dim3(B * T), dim3(256), 0, s, tokens, ld_tok, T, 0, (const int32_t*)nullptr,
                           (const float*)tok_emb, pos_emb, x, D, starts_dev);
    else
        hipLaunchKernelGGL((embed_kernel<__bf16, true>), dim3(B * T), dim3(256), 0, s, tokens, ld_tok, T, 0, (const int32_t*)nullptr,
                           (const __bf16*)tok_emb, pos_emb, x, D, starts_dev);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// the register-resident row scan (row_scan_reg, row_pick) can serve this row layout: 16 quads per thread, 16-byte loads
static bool reg_scan_ok(const float* logits, int V, int64_t ldl, const float* mask_first, const float* mask_always) {
    return V <= 4 * GS_MAXQ * GS_THREADS && ldl % 4 == 0 && ((uintptr_t)logits % 16) == 0 && ((uintptr_t)mask_first % 16) == 0 &&
           ((uintptr_t)mask_always % 16) == 0;
}

extern "C" int wipa_greedy_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first,
                                const float* mask_always, int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev,
                                int n_init, int eot, float* sum_logprobs, int32_t* not_done, wipa_stream_t stream) {
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && sum_logprobs && not_done,
                 "wipa_greedy_step: null pointer");
    if (reg_scan_ok(logits, V, ldl, mask_first, mask_always))
        hipLaunchKernelGGL(greedy_step_reg_kernel, dim3(B), dim3(GS_THREADS), 0, (hipStream_t)stream, logits, ldl, V, mask_first,
                           mask_always, tokens, ld_tok, pos_dev, n_init, eot, sum_logprobs, not_done);
    else
        hipLaunchKernelGGL(greedy_step_kernel, dim3(B), dim3(GS_THREADS), 0, (hipStream_t)stream, logits, ldl, V, mask_first,
                           mask_always, tokens, ld_tok, pos_dev, n_init, eot, sum_logprobs, not_done);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

static int rules_check(const char* who, const wipa_decode_rules* rules, const float* logits, int V, int64_t ldl, const float* mask_first,
                       const float* mask_always, int eot, RulesDev* out) {
    WIPA_REQUIRE(rules, "%s: null rules", who);
    WIPA_REQUIRE(rules->timestamp_begin > 0 && rules->timestamp_begin < V && eot < rules->timestamp_begin && rules->no_timestamps >= 0 &&
                     rules->no_timestamps < rules->timestamp_begin,
                 "%s: need eot < timestamp_begin < V and no_timestamps below timestamp_begin (eot=%d timestamp_begin=%d no_timestamps=%d V=%d)", who,
                 eot, rules->timestamp_begin, rules->no_timestamps, V);
    // the rules live in the register-resident row scan only
    WIPA_REQUIRE(reg_scan_ok(logits, V, ldl, mask_first, mask_always), "%s: vocabulary of %d / unaligned logits or masks", who, V);
    out->tb = rules->timestamp_begin;
    out->nt = rules->no_timestamps;
    out->max_init = rules->max_initial_timestamp_index;
    return WIPA_OK;
}

// rules may be NULL: the plain filtered row, every column on the text side
static int sample_check(const char* who, const wipa_decode_rules* rules, const void* sample, const float* logits, int V, int64_t ldl,
                        const float* mask_first, const float* mask_always, int eot, int n_ctx, RulesDev* out) {
    WIPA_REQUIRE(sample && ((uintptr_t)sample % 4) == 0, "%s: null / unaligned sampling record", who);
    WIPA_REQUIRE(n_ctx <= 65536, "%s: positions above 65535 do not fit the draw's counter", who);
    if (rules) return rules_check(who, rules, logits, V, ldl, mask_first, mask_always, eot, out);
    WIPA_REQUIRE(V > 0 && reg_scan_ok(logits, V, ldl, mask_first, mask_always), "%s: vocabulary of %d / unaligned logits or masks", who, V);
    out->tb = V;
    out->nt = -1;
    out->max_init = -1;
    return WIPA_OK;
}

extern "C" int wipa_timestamp_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                   int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot,
                                   const wipa_decode_rules* rules, float* sum_logprobs, int32_t* not_done, wipa_stream_t stream) {
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && sum_logprobs && not_done && B > 0 && n_init >= 1,
                 "wipa_timestamp_step: bad arguments");
    RulesDev r;
    const int rc = rules_check("wipa_timestamp_step", rules, logits, V, ldl, mask_first, mask_always, eot, &r);
    if (rc != WIPA_OK) return rc;
    hipLaunchKernelGGL(timestamp_step_kernel, dim3(B), dim3(GS_THREADS), 0, (hipStream_t)stream, logits, ldl, V, mask_first, mask_always, tokens,
                       ld_tok, pos_dev, n_init, eot, r, sum_logprobs, not_done);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// ------------------------------------------------------------------ temperature sampling
// the sampling record: 16 bytes of header (u32 seed_lo, seed_hi, attempt; f32 1 / temperature) and one (lo, hi) u32 pair per row
extern "C" size_t wipa_sample_record_bytes(int B) { return B > 0 ? 16 + (size_t)B * 8 : 0; }

extern "C" int wipa_sample_record_fill(void* host_record, size_t record_bytes, uint64_t seed, int attempt, float temperature,
                                       const uint32_t* streams, int B) {
    WIPA_REQUIRE(host_record && B > 0 && record_bytes >= wipa_sample_record_bytes(B), "wipa_sample_record_fill: null record / %zu bytes for %d rows",
                 record_bytes, B);
    WIPA_REQUIRE(temperature > 0.f && temperature < INFINITY, "wipa_sample_record_fill: temperature %g (sampling needs a temperature above 0)",
                 (double)temperature);
    WIPA_REQUIRE(attempt >= 0 && attempt < 65536, "wipa_sample_record_fill: attempt %d outside 0..65535", attempt);
    uint32_t* r = (uint32_t*)host_record;
    const float inv_t = 1.0f / temperature;
    r[0] = (uint32_t)seed;
    r[1] = (uint32_t)(seed >> 32);
    r[2] = (uint32_t)attempt;
    memcpy(r + 3, &inv_t, 4);
    for (int b = 0; b < B; ++b) {
        r[4 + 2 * b] = streams ? streams[2 * b] : (uint32_t)b;
        r[5 + 2 * b] = streams ? streams[2 * b + 1] : 0u;
    }
    return WIPA_OK;
}

// the sampling record with a ROW PART: 16 bytes of header (u32 seed_lo, seed_hi, B, 0) and 16 bytes per row (u32 stream_lo, stream_hi,
// attempt; f32 1 / temperature, 0 for a greedy row)
extern "C" size_t wipa_sample_rows_bytes(int B) { return B > 0 ? 16 + (size_t)B * 16 : 0; }

extern "C" int wipa_sample_rows_fill(void* host_image, size_t bytes, uint64_t seed, int B) {
    WIPA_REQUIRE(host_image && B > 0 && bytes >= wipa_sample_rows_bytes(B), "wipa_sample_rows_fill: null image / %zu bytes for %d rows", bytes, B);
    uint32_t* r = (uint32_t*)host_image;
    r[0] = (uint32_t)seed;
    r[1] = (uint32_t)(seed >> 32);
    r[2] = (uint32_t)B;
    r[3] = 0u;
    for (int b = 0; b < B; ++b) {  // every row greedy, on stream (b, 0), attempt 0
        r[4 + 4 * b] = (uint32_t)b;
        r[5 + 4 * b] = 0u;
        r[6 + 4 * b] = 0u;
        r[7 + 4 * b] = 0u;  // 1 / T = 0.0f
    }
    return WIPA_OK;
}

// what one row entry may hold, refused by the argument's name; *inv_t: 1 / temperature, 0 for temperature 0 (a greedy row)
static int sample_rows_entry(const char* who, int B, int i, int slot, int attempt, float temperature, float* inv_t) {
    WIPA_REQUIRE(slot >= 0 && slot < B, "%s: slot[%d]=%d outside 0..%d", who, i, slot, B - 1);
    WIPA_REQUIRE(attempt >= 0 && attempt < 65536, "%s: attempt[%d]=%d outside 0..65535", who, i, attempt);
    WIPA_REQUIRE(temperature >= 0.f && temperature < INFINITY, "%s: temperature[%d]=%g is negative or not finite (0 is a greedy row)", who, i,
                 (double)temperature);
    *inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
    return WIPA_OK;
}

extern "C" int wipa_sample_rows_fill_row(void* host_image, size_t bytes, int B, int slot, uint32_t stream_lo, uint32_t stream_hi, int attempt,
                                         float temperature) {
    WIPA_REQUIRE(host_image && B > 0 && bytes >= wipa_sample_rows_bytes(B), "wipa_sample_rows_fill_row: null image / %zu bytes for %d rows", bytes, B);
    float inv_t;
    const int rc = sample_rows_entry("wipa_sample_rows_fill_row", B, 0, slot, attempt, temperature, &inv_t);
    if (rc != WIPA_OK) return rc;
    uint32_t* e = (uint32_t*)host_image + 4 + 4 * slot;
    e[0] = stream_lo;
    e[1] = stream_hi;
    e[2] = (uint32_t)attempt;
    memcpy(e + 3, &inv_t, 4);
    return WIPA_OK;
}

extern "C" int wipa_sample_rows_set(void* rows_dev, int B, int n_rows, const int32_t* slots_host, const uint32_t* streams_host,
                                    const int32_t* attempts_host, const float* temperatures_host, wipa_stream_t stream) {
    const char* who = "wipa_sample_rows_set";
    WIPA_REQUIRE(rows_dev && ((uintptr_t)rows_dev % 16) == 0, "%s: null / unaligned record (rows_dev: 16-byte aligned)", who);
    WIPA_REQUIRE(B > 0 && n_rows >= 0 && (n_rows == 0 || (slots_host && streams_host && attempts_host && temperatures_host)),
                 "%s: null pointer / bad row count", who);
    float inv_t = 0.f;  // every entry is checked before the first launch
    for (int i = 0; i < n_rows; ++i) {
        const int rc = sample_rows_entry(who, B, i, slots_host[i], attempts_host[i], temperatures_host[i], &inv_t);
        if (rc != WIPA_OK) return rc;
    }
    // the values travel as kernel arguments, like those of wipa_decoder_admit_rows: the host arrays are free when the call returns
    for (int i = 0; i < n_rows; ++i) {
        sample_rows_entry(who, B, i, slots_host[i], attempts_host[i], temperatures_host[i], &inv_t);
        hipLaunchKernelGGL(sample_rows_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (uint32_t*)rows_dev, slots_host[i], streams_host[2 * i],
                           streams_host[2 * i + 1], (uint32_t)attempts_host[i], inv_t);
        WIPA_LAUNCH_CHECK();
    }
    return WIPA_OK;
}

// wipa_sample_step and, with starts_dev (left-padded prompt rows: the draw's counter takes the row's own position *pos_dev - starts_dev[b]),
// wipa_sample_step_ragged
static int sample_step(const char* who, const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                       int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules,
                       const void* sample, const int32_t* starts_dev, float* sum_logprobs, int32_t* not_done, wipa_stream_t stream) {
    RulesDev r;
    const int rc = sample_check(who, rules, sample, logits, V, ldl, mask_first, mask_always, eot, 0, &r);
    if (rc != WIPA_OK) return rc;
#define SAMPLE_STEP(RULES, RAGGED)                                                                                                         \
    hipLaunchKernelGGL((sample_step_kernel<RULES, RAGGED>), dim3(B), dim3(GS_THREADS), 0, (hipStream_t)stream, logits, ldl, V, mask_first, \
                       mask_always, tokens, ld_tok, pos_dev, n_init, eot, r, (const uint32_t*)sample, sum_logprobs, not_done, starts_dev)
    if (starts_dev) {
        if (rules) SAMPLE_STEP(true, true);
        else SAMPLE_STEP(false, true);
    } else {
        if (rules) SAMPLE_STEP(true, false);
        else SAMPLE_STEP(false, false);
    }
#undef SAMPLE_STEP
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_sample_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules,
                                const void* sample, float* sum_logprobs, int32_t* not_done, wipa_stream_t stream) {
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && sum_logprobs && not_done && B > 0 && n_init >= 1,
                 "wipa_sample_step: bad arguments");
    return sample_step("wipa_sample_step", logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, n_init, eot, rules, sample, nullptr,
                       sum_logprobs, not_done, stream);
}

extern "C" int wipa_sample_step_ragged(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                       int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules,
                                       const void* sample, const int32_t* starts_dev, float* sum_logprobs, int32_t* not_done, wipa_stream_t stream) {
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && starts_dev && sum_logprobs && not_done && B > 0 && n_init >= 1,
                 "wipa_sample_step_ragged: bad arguments (starts_dev is required)");
    return sample_step("wipa_sample_step_ragged", logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, n_init, eot, rules, sample,
                       starts_dev, sum_logprobs, not_done, stream);
}

// ------------------------------------------------------------------ the step's tail and head: one fill, one check, one launcher
// the logits group stays unset for the head and the partials tail, the step-state group for the head
static TailParams tail_params(const float* logits, int64_t ldl, int V, const float* mask_first, const float* mask_always, int32_t* tokens,
                              int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init, int eot, float* sum_logprobs,
                              int32_t* not_done, const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx,
                              float* x, const float* ln_w, const float* ln_b, void* y, int D, float eps) {
    TailParams q = {};
    q.logits = logits; q.ldl = ldl; q.V = V; q.mask_first = mask_first; q.mask_always = mask_always;
    q.tokens = tokens; q.ld_tok = ld_tok; q.pos = pos_dev; q.posd = posd_dev; q.done_counter = done_counter;
    q.n_init = n_init; q.eot = eot; q.n_ctx = n_ctx; q.sum_logprobs = sum_logprobs; q.not_done = not_done;
    q.emb = tok_emb; q.emb_dtype = emb_dtype; q.emb_scale = emb_scale; q.pos_emb = pos_emb;
    q.x = x; q.ln_w = ln_w; q.ln_b = ln_b; q.y = y; q.D = D; q.eps = eps;
    return q;
}

enum TailKind { TAIL_HEAD, TAIL_STEP };  // embed_layernorm_kernel alone | a step's last launch

template <typename TO, bool RAGGED>
static void launch_tail_as(TailKind kind, const TailParams& tp, int B, bool rules, RulesDev r, const uint32_t* rec, const int32_t* starts,
                           hipStream_t s) {
    TailArgs<RAGGED> q = {};
    static_cast<TailParams&>(q) = tp;
    if constexpr (RAGGED) q.start = starts;
    const dim3 grid(B), block(GS_THREADS);
    if (kind == TAIL_HEAD) hipLaunchKernelGGL((embed_layernorm_kernel<TO, RAGGED>), grid, dim3(256), 0, s, q);
    else if (rec && rules) hipLaunchKernelGGL((sample_tail_kernel<TO, true, RAGGED>), grid, block, 0, s, q, r, rec);
    else if (rec) hipLaunchKernelGGL((sample_tail_kernel<TO, false, RAGGED>), grid, block, 0, s, q, r, rec);
    else if (rules) hipLaunchKernelGGL((timestamp_tail_kernel<TO, RAGGED>), grid, block, 0, s, q, r);
    else hipLaunchKernelGGL((greedy_tail_kernel<TO, RAGGED>), grid, block, 0, s, q);
}

// The checks every tail / head entry point shares, then the launch of the instantiation that (y_dtype, rules, sample, starts_dev) name.
// The callers have checked their own pointers; rules, sample and starts_dev may each be NULL.
static int launch_tail(const char* who, TailKind kind, const TailParams& tp, int B, int y_dtype, const wipa_decode_rules* rules, const void* sample,
                       const int32_t* starts_dev, wipa_stream_t stream) {
    WIPA_REQUIRE(tp.D % 4 == 0 && tp.D > 0 && tp.D <= 2048, "%s: D=%d must be a multiple of 4 and <= 2048", who, tp.D);
    WIPA_REQUIRE(tp.emb_dtype == WIPA_F32 || tp.emb_dtype == WIPA_BF16 || (tp.emb_dtype == WIPA_FP8_E4M3 && tp.emb_scale),
                 "%s: bad embedding dtype %d", who, tp.emb_dtype);
    if (tp.logits)
        WIPA_REQUIRE(reg_scan_ok(tp.logits, tp.V, tp.ldl, tp.mask_first, tp.mask_always), "%s: vocabulary of %d / unaligned logits or masks", who,
                     tp.V);
    RulesDev r = {tp.V, -1, -1};
    int rc = WIPA_OK;
    if (sample) rc = sample_check(who, rules, sample, tp.logits, tp.V, tp.ldl, tp.mask_first, tp.mask_always, tp.eot, tp.n_ctx, &r);
    else if (rules) rc = rules_check(who, rules, tp.logits, tp.V, tp.ldl, tp.mask_first, tp.mask_always, tp.eot, &r);
    if (rc != WIPA_OK) return rc;
    WIPA_REQUIRE(y_dtype == WIPA_F32 || y_dtype == WIPA_BF16, "%s: bad dtype %d", who, y_dtype);
    const uint32_t* rec = (const uint32_t*)sample;
    hipStream_t s = (hipStream_t)stream;
    const bool f32 = y_dtype == WIPA_F32;
    if (starts_dev) {
        if (f32) launch_tail_as<float, true>(kind, tp, B, rules != nullptr, r, rec, starts_dev, s);
        else launch_tail_as<__bf16, true>(kind, tp, B, rules != nullptr, r, rec, starts_dev, s);
    } else {
        if (f32) launch_tail_as<float, false>(kind, tp, B, rules != nullptr, r, rec, nullptr, s);
        else launch_tail_as<__bf16, false>(kind, tp, B, rules != nullptr, r, rec, nullptr, s);
    }
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// wipa_embed_layernorm and, with starts_dev, wipa_embed_layernorm_ragged
static int embed_layernorm(const char* who, const int32_t* tokens, int64_t ld_tok, int B, const int32_t* pos_dev, const int32_t* starts_dev,
                           const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w,
                           const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t stream) {
    const TailParams tp = tail_params(nullptr, 0, 0, nullptr, nullptr, const_cast<int32_t*>(tokens), ld_tok, const_cast<int32_t*>(pos_dev), nullptr,
                                      nullptr, 0, 0, nullptr, nullptr, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, D, eps);
    return launch_tail(who, TAIL_HEAD, tp, B, y_dtype, nullptr, nullptr, starts_dev, stream);
}

extern "C" int wipa_embed_layernorm(const int32_t* tokens, int64_t ld_tok, int B, const int32_t* pos_dev, const void* tok_emb,
                                    int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w,
                                    const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(tokens && pos_dev && tok_emb && pos_emb && x && ln_w && ln_b && y && B > 0 && n_ctx > 0, "wipa_embed_layernorm: bad arguments");
    return embed_layernorm("wipa_embed_layernorm", tokens, ld_tok, B, pos_dev, nullptr, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b,
                           y, y_dtype, D, eps, stream);
}

extern "C" int wipa_embed_layernorm_ragged(const int32_t* tokens, int64_t ld_tok, int B, const int32_t* pos_dev, const int32_t* starts_dev,
                                           const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x,
                                           const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(tokens && pos_dev && starts_dev && tok_emb && pos_emb && x && ln_w && ln_b && y && B > 0 && n_ctx > 0,
                 "wipa_embed_layernorm_ragged: bad arguments (starts_dev is required)");
    return embed_layernorm("wipa_embed_layernorm_ragged", tokens, ld_tok, B, pos_dev, starts_dev, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x,
                           ln_w, ln_b, y, y_dtype, D, eps, stream);
}

// The step's last launch on written logits (declared in wipa_common.h for the runtime; not exported): rules, sample and starts_dev
// may each be NULL, and name the exported entry point whose checks and error prefix apply
int wipa_step_tail(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always, int32_t* tokens,
                   int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init, int eot, const wipa_decode_rules* rules,
                   const void* sample, const int32_t* starts_dev, float* sum_logprobs, int32_t* not_done, const void* tok_emb, int emb_dtype,
                   const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b, void* y, int y_dtype,
                   int D, float eps, wipa_stream_t stream) {
    const char* who = starts_dev ? "wipa_step_embed_ragged" : sample ? "wipa_sample_step_embed" : rules ? "wipa_timestamp_step_embed"
                                                                                                   : "wipa_greedy_step_embed";
    const bool plain = !rules && !sample && !starts_dev;  // wipa_greedy_step_embed alone takes n_init below 1
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && posd_dev && done_counter && sum_logprobs && not_done && tok_emb &&
                     pos_emb && x && ln_w && ln_b && y && B > 0 && n_ctx > 0 && (plain || n_init >= 1),
                 "%s: bad arguments%s", who, starts_dev ? " (starts_dev is required)" : "");
    const TailParams tp = tail_params(logits, ldl, V, mask_first, mask_always, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot,
                                      sum_logprobs, not_done, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, D, eps);
    return launch_tail(who, TAIL_STEP, tp, B, y_dtype, rules, sample, starts_dev, stream);
}

extern "C" int wipa_greedy_step_embed(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                      int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter,
                                      int n_init, int eot, float* sum_logprobs, int32_t* not_done, const void* tok_emb, int emb_dtype,
                                      const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w,
                                      const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t stream) {
    return wipa_step_tail(logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot, nullptr, nullptr,
                          nullptr, sum_logprobs, not_done, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, y_dtype, D, eps, stream);
}

extern "C" int wipa_timestamp_step_embed(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                         int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter,
                                         int n_init, int eot, const wipa_decode_rules* rules, float* sum_logprobs, int32_t* not_done,
                                         const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x,
                                         const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(rules, "wipa_timestamp_step_embed: null rules");
    return wipa_step_tail(logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot, rules, nullptr,
                          nullptr, sum_logprobs, not_done, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, y_dtype, D, eps, stream);
}

extern "C" int wipa_sample_step_embed(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                      int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter,
                                      int n_init, int eot, const wipa_decode_rules* rules, const void* sample, float* sum_logprobs,
                                      int32_t* not_done, const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb,
                                      int n_ctx, float* x, const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps,
                                      wipa_stream_t stream) {
    WIPA_REQUIRE(sample, "wipa_sample_step_embed: null / unaligned sampling record");
    return wipa_step_tail(logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot, rules, sample,
                          nullptr, sum_logprobs, not_done, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, y_dtype, D, eps, stream);
}

// the RAGGED instantiations of the tails (left-padded prompt rows)
extern "C" int wipa_step_embed_ragged(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                                      int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter,
                                      int n_init, int eot, const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev,
                                      float* sum_logprobs, int32_t* not_done, const void* tok_emb, int emb_dtype, const float* emb_scale,
                                      const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b, void* y, int y_dtype,
                                      int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(starts_dev, "wipa_step_embed_ragged: bad arguments (starts_dev is required)");
    return wipa_step_tail(logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot, rules, sample,
                          starts_dev, sum_logprobs, not_done, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, y_dtype, D, eps, stream);
}

template <typename TO>
static void launch_tail_continuous_as(const TailArgs<true>& q, int B, bool rules, RulesDev r, const uint32_t* rec, const uint32_t* rows,
                                      float* no_speech_dev, int no_speech_token, hipStream_t s) {
    const dim3 grid(B), block(GS_THREADS);
    if (rows && rules) hipLaunchKernelGGL((rows_tail_continuous_kernel<TO, true>), grid, block, 0, s, q, r, rows, no_speech_dev, no_speech_token);
    else if (rows) hipLaunchKernelGGL((rows_tail_continuous_kernel<TO, false>), grid, block, 0, s, q, r, rows, nullptr, 0);
    else if (rules && rec) hipLaunchKernelGGL((rules_tail_continuous_kernel<TO, true>), grid, block, 0, s, q, r, rec, no_speech_dev, no_speech_token);
    else if (rules) hipLaunchKernelGGL((rules_tail_continuous_kernel<TO, false>), grid, block, 0, s, q, r, rec, no_speech_dev, no_speech_token);
    else if (rec) hipLaunchKernelGGL((sample_tail_continuous_kernel<TO>), grid, block, 0, s, q, rec);
    else hipLaunchKernelGGL((greedy_tail_continuous_kernel<TO>), grid, block, 0, s, q);
}

// the PROMPTED tails: the same selection among the instantiations of tail_prompted_kernel (starts_dev is int32 [3][B])
template <typename TO>
static void launch_tail_prompted_as(const TailArgs<true>& q, int B, bool rules, RulesDev r, const uint32_t* rec, const uint32_t* rows,
                                    float* no_speech_dev, int no_speech_token, hipStream_t s) {
    const dim3 grid(B), block(GS_THREADS);
#define TAIL_PROMPTED(RULES, DRAW, REC, NSP, NSP_TOKEN) \
    hipLaunchKernelGGL((tail_prompted_kernel<TO, RULES, DRAW>), grid, block, 0, s, q, r, REC, NSP, NSP_TOKEN)
    if (rows && rules) TAIL_PROMPTED(true, DRAW_ROWS, rows, no_speech_dev, no_speech_token);
    else if (rows) TAIL_PROMPTED(false, DRAW_ROWS, rows, nullptr, 0);
    else if (rules && rec) TAIL_PROMPTED(true, DRAW_RECORD, rec, no_speech_dev, no_speech_token);
    else if (rules) TAIL_PROMPTED(true, DRAW_NONE, rec, no_speech_dev, no_speech_token);
    else if (rec) TAIL_PROMPTED(false, DRAW_RECORD, rec, nullptr, 0);
    else TAIL_PROMPTED(false, DRAW_NONE, rec, nullptr, 0);
#undef TAIL_PROMPTED
}

// The CONTINUOUS tails (declared in wipa_common.h for the runtime; not exported): the checks of wipa_step_tail; starts_dev is int32 [2][B],
// the rows' first own columns and then the tokens each may generate.  rules, sample, sample_rows and no_speech_dev may each be NULL;
// the error prefix is that of wipa_decoder_run_ex, the one entry point that ends its steps here (prompted: starts_dev is int32 [3][B]
// with the rows' prompt columns last, and the tails are the PROMPTED ones).  With rules the tails are the rules_tail_continuous
// kernels, and no_speech_dev (float [B]) receives softmax(row)[no_speech_token] at a row's first column; sample_rows (the sampling record
// with a row part) takes the place of sample and selects the rows_tail_continuous kernels: a temperature per row.
int wipa_step_tail_continuous(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always, int32_t* tokens,
                              int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init, int eot,
                              const wipa_decode_rules* rules, const void* sample, const void* sample_rows, const int32_t* starts_dev,
                              int prompted, float* no_speech_dev, int no_speech_token, float* sum_logprobs, int32_t* not_done, const void* tok_emb,
                              int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b,
                              void* y, int y_dtype, int D, float eps, wipa_stream_t stream) {
    const char* who = "wipa_decoder_run_ex";
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && posd_dev && done_counter && sum_logprobs && not_done && tok_emb &&
                     pos_emb && x && ln_w && ln_b && y && starts_dev && B > 0 && n_ctx > 0 && n_init >= 1 && ld_tok >= n_ctx,
                 "%s: bad arguments of the step's tail (starts_dev is required)", who);
    const TailParams tp = tail_params(logits, ldl, V, mask_first, mask_always, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot,
                                      sum_logprobs, not_done, tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, D, eps);
    WIPA_REQUIRE(tp.D % 4 == 0 && tp.D > 0 && tp.D <= 2048, "%s: D=%d must be a multiple of 4 and <= 2048", who, tp.D);
    WIPA_REQUIRE(tp.emb_dtype == WIPA_F32 || tp.emb_dtype == WIPA_BF16, "%s: bad embedding dtype %d", who, tp.emb_dtype);
    WIPA_REQUIRE(reg_scan_ok(tp.logits, tp.V, tp.ldl, tp.mask_first, tp.mask_always), "%s: vocabulary of %d / unaligned logits or masks", who, tp.V);
    WIPA_REQUIRE(y_dtype == WIPA_F32 || y_dtype == WIPA_BF16, "%s: bad dtype %d", who, y_dtype);
    RulesDev r = {tp.V, -1, -1};
    int rc = WIPA_OK;
    WIPA_REQUIRE(!sample_rows || (!sample && ((uintptr_t)sample_rows % 16) == 0), "%s: sample_rows is 16-byte aligned and takes the place of sample", who);
    if (sample || sample_rows)
        rc = sample_check(who, rules, sample ? sample : sample_rows, tp.logits, tp.V, tp.ldl, tp.mask_first, tp.mask_always, tp.eot, tp.n_ctx, &r);
    else if (rules) rc = rules_check(who, rules, tp.logits, tp.V, tp.ldl, tp.mask_first, tp.mask_always, tp.eot, &r);
    if (rc != WIPA_OK) return rc;
    WIPA_REQUIRE(!no_speech_dev || (rules && no_speech_token >= 0 && no_speech_token < V), "%s: no_speech_token=%d outside the vocabulary of %d", who,
                 no_speech_token, V);
    TailArgs<true> q = {};
    static_cast<TailParams&>(q) = tp;
    q.start = starts_dev;
    hipStream_t s = (hipStream_t)stream;
    if (prompted) {
        if (y_dtype == WIPA_F32)
            launch_tail_prompted_as<float>(q, B, rules != nullptr, r, (const uint32_t*)sample, (const uint32_t*)sample_rows, no_speech_dev,
                                           no_speech_token, s);
        else
            launch_tail_prompted_as<__bf16>(q, B, rules != nullptr, r, (const uint32_t*)sample, (const uint32_t*)sample_rows, no_speech_dev,
                                            no_speech_token, s);
    } else if (y_dtype == WIPA_F32)
        launch_tail_continuous_as<float>(q, B, rules != nullptr, r, (const uint32_t*)sample, (const uint32_t*)sample_rows, no_speech_dev,
                                         no_speech_token, s);
    else
        launch_tail_continuous_as<__bf16>(q, B, rules != nullptr, r, (const uint32_t*)sample, (const uint32_t*)sample_rows, no_speech_dev,
                                          no_speech_token, s);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// the tail on wipa_logits_greedy's per-wave partials: no logits, so no rules, no draw and no ragged rows
extern "C" int wipa_greedy_step_embed_partials(const float* partials, int n_parts, int B, int32_t* tokens, int64_t ld_tok, int32_t* pos_dev,
                                               int64_t* posd_dev, int32_t* done_counter, int n_init, int eot, float* sum_logprobs,
                                               int32_t* not_done, const void* tok_emb, int emb_dtype, const float* emb_scale,
                                               const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b, void* y,
                                               int y_dtype, int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(partials && n_parts > 0 && tokens && pos_dev && posd_dev && done_counter && sum_logprobs && not_done && tok_emb && pos_emb && x &&
                     ln_w && ln_b && y && B > 0 && n_ctx > 0, "wipa_greedy_step_embed_partials: bad arguments");
    TailParams tp = tail_params(nullptr, 0, 0, nullptr, nullptr, tokens, ld_tok, pos_dev, posd_dev, done_counter, n_init, eot, sum_logprobs, not_done,
                                tok_emb, emb_dtype, emb_scale, pos_emb, n_ctx, x, ln_w, ln_b, y, D, eps);
    tp.part = partials; tp.n_part = n_parts;
    return launch_tail("wipa_greedy_step_embed_partials", TAIL_STEP, tp, B, y_dtype, nullptr, nullptr, nullptr, stream);
}

extern "C" int wipa_sample_noise(const void* sample, int row, int p, int V, float* out, wipa_stream_t stream) {
    WIPA_REQUIRE(sample && ((uintptr_t)sample % 4) == 0 && out && row >= 0 && p >= 0 && p < 65536 && V > 0, "wipa_sample_noise: bad arguments");
    hipLaunchKernelGGL(sample_noise_kernel, dim3(((V + 3) / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)sample, row, p, V, out);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_add_i32(int32_t* p, int32_t v, wipa_stream_t stream) {
    WIPA_REQUIRE(p, "wipa_add_i32: null pointer");
    hipLaunchKernelGGL(add_i32_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p, v);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_masked_ce(const float* logits, int64_t ldl, const int32_t* tokens, int64_t ld_tok, int B, int T, int V,
                              int eot, float* row_buf, float* out2, wipa_stream_t stream) {
    WIPA_REQUIRE(logits && tokens && row_buf && out2, "wipa_masked_ce: null pointer");
    const int rows = B * T;
    if (rows <= 0) return WIPA_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(masked_ce_rows_kernel, dim3(rows), dim3(CE_THREADS), 0, s, logits, ldl, tokens, ld_tok, T, V, eot,
                       row_buf, rows);
    hipLaunchKernelGGL(sum2_kernel, dim3(1), dim3(256), 0, s, row_buf, rows, out2);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_mel_pad_cast(const float* mel, int batch, int n_mels, void* mel_padded, int dtype,
                                 wipa_stream_t stream) {
    WIPA_REQUIRE(mel && mel_padded, "wipa_mel_pad_cast: null pointer");
    const int64_t total = (int64_t)batch * (WIPA_N_FRAMES + 2) * n_mels;
    if (total <= 0) return WIPA_OK;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == WIPA_F32)
        hipLaunchKernelGGL((mel_pad_cast_kernel<float>), grid, dim3(256), 0, s, mel, n_mels, (float*)mel_padded, total);
    else if (dtype == WIPA_BF16)
        hipLaunchKernelGGL((mel_pad_cast_kernel<__bf16>), grid, dim3(256), 0, s, mel, n_mels, (__bf16*)mel_padded, total);
    else
        WIPA_REQUIRE(false, "wipa_mel_pad_cast: bad dtype %d", dtype);
    WIPA_LAUNCH_CHECK();
    const size_t esz = wipa_dtype_size(dtype);
    WIPA_CHECK_HIP(hipMemsetAsync((char*)mel_padded + (size_t)total * esz, 0, 4 * (size_t)n_mels * esz, s));
    return WIPA_OK;
}

extern "C" int wipa_mel_pad_cast_frames(const float* mel, int64_t clip_stride, int batch, int n_mels, int n_frames, void* mel_padded,
                                        int dtype, wipa_stream_t stream) {
    WIPA_REQUIRE(mel && mel_padded, "wipa_mel_pad_cast_frames: null pointer");
    WIPA_REQUIRE(n_frames >= 1 && n_frames <= WIPA_N_FRAMES && n_mels > 0 && clip_stride >= (int64_t)n_frames * n_mels,
                 "wipa_mel_pad_cast_frames: n_frames=%d (1..%d), clip stride %lld", n_frames, WIPA_N_FRAMES, (long long)clip_stride);
    const int64_t total = (int64_t)batch * (n_frames + 2) * n_mels;
    if (total <= 0) return WIPA_OK;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == WIPA_F32)
        hipLaunchKernelGGL((mel_pad_cast_frames_kernel<float>), grid, dim3(256), 0, s, mel, clip_stride, n_mels, n_frames, (float*)mel_padded,
                           total);
    else if (dtype == WIPA_BF16)
        hipLaunchKernelGGL((mel_pad_cast_frames_kernel<__bf16>), grid, dim3(256), 0, s, mel, clip_stride, n_mels, n_frames,
                           (__bf16*)mel_padded, total);
    else
        WIPA_REQUIRE(false, "wipa_mel_pad_cast_frames: bad dtype %d", dtype);
    WIPA_LAUNCH_CHECK();
    const size_t esz = wipa_dtype_size(dtype);
    WIPA_CHECK_HIP(hipMemsetAsync((char*)mel_padded + (size_t)total * esz, 0, 4 * (size_t)n_mels * esz, s));
    return WIPA_OK;
}

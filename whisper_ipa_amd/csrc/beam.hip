// Beam search in the decode step's tail: BeamSearchDecoder.update / finalize and MaximumLikelihoodRanker.rank of openai-whisper's
// decoding.py, on the device.  The B rows of a call are B / G clips x G beams (candidate groups, cfg.dec_n_group = G = beam_size).
//   beam_topk_kernel    one workgroup per ROW: the filtered row of the greedy / rules tails (logits + mask, rules 1-5), its log-sum-exp
//                       with their summation order, then the row's G + 1 best columns as (logprob, column), sorted.
//   beam_select_kernel  one workgroup per CLIP: the G (G + 1) candidates (G + 1 on the first generated step, where the beams of a clip are
//                       the same sequence) in descending cumulative score; EOT candidates go to the clip's finished store, the first G
//                       others become the next beams: source row, token, sum.  It gathers the token rows and the ancestor table
//                       (attention.hip: decode_attn_kernel<.., BEAM>) by source, counts the clips whose store is not full, and -- as a
//                       step's last launch -- writes the next step's input rows and advances the position.
//   beam_finalize_kernel one wave per clip: fill the store with live beams + EOT up to G, rank, copy the winner.
// Nothing here goes back to the host within a step; the host reads not_done (4 bytes) when it looks whether to stop.
#include <string.h>

#include <algorithm>

#include "step_rows.h"

namespace {

constexpr int BEAM_MAX_G = 16;
constexpr int BEAM_MAX_CAND = 64;
constexpr int BEAM_MAX_N = BEAM_MAX_G * (BEAM_MAX_G + 1);  // candidates of one clip
constexpr int BS_THREADS = 256;

struct Cand {
    float logprob;
    int32_t col;
};

// the caller's beam buffer (wipa.h: wipa_beam_bytes): byte offsets of its parts
struct BeamLayout {
    size_t anc, cand, src, fin_tok, fin_score, fin_len, fin_count, counters, total;
    int cap;  // sequences a clip's store holds: max(G, max_candidates)
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
BeamLayout beam_layout(int B, int G, int maxc, int64_t ld_tok) {
    BeamLayout L;
    const size_t clips = (size_t)(B / G);
    L.cap = G > maxc ? G : maxc;
    size_t o = 0;
    L.anc = o;       o += up256((size_t)B * ld_tok);
    L.cand = o;      o += up256((size_t)B * (G + 1) * sizeof(Cand));
    L.src = o;       o += up256((size_t)B * 4);
    L.fin_tok = o;   o += up256(clips * L.cap * ld_tok * 4);
    L.fin_score = o; o += up256(clips * L.cap * 4);
    L.fin_len = o;   o += up256(clips * L.cap * 4);
    L.fin_count = o; o += up256(clips * 4);
    L.counters = o;  o += 256;  // int32 [0]: clips of this step whose store is not full; [1]: workgroups of beam_select that have arrived
    L.total = o;
    return L;
}

__global__ __launch_bounds__(256) void beam_begin_kernel(uint8_t* __restrict__ anc, int64_t anc_ld, int B, int G, int32_t* __restrict__ fin_count,
                                                         int clips, int32_t* __restrict__ counters) {
    const int64_t n = (int64_t)B * anc_ld;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        anc[i] = (uint8_t)((i / anc_ld) % G);  // the identity table: every column of row b lies in row b
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < clips; c += blockDim.x) fin_count[c] = 0;
        if (threadIdx.x < 2) counters[threadIdx.x] = 0;
    }
}

// The filtered row and its reductions are row_pick's text (elementwise.hip), copied and not shared: routed through a common helper the
// rules and sampling tails compiled to other instructions (more scratch), and those kernels keep theirs.  What differs comes after the
// log-sum-exp: rule 5's verdict is written into the registers, and the arg-max is taken n_top times.
template <bool RULES>
__global__ __launch_bounds__(GS_THREADS) void beam_topk_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                               const float* __restrict__ mask_first, const float* __restrict__ mask_always,
                                                               const int32_t* __restrict__ tokens, int64_t ld_tok,
                                                               const int32_t* __restrict__ pos_dev, int n_init, int eot, RulesDev r,
                                                               Cand* __restrict__ cand, int n_top) {
    __shared__ float s_v[2 * GS_WAVES];
    __shared__ int s_i[2 * GS_WAVES];
    __shared__ float s_sum[2 * GS_WAVES];
    const int b = blockIdx.x;
    const int p = *pos_dev;
    if (in_prompt(p, n_init)) return;
    const float* row = logits + (int64_t)b * ldl;
    const float* mask = step_mask(p, n_init, mask_first, mask_always);
    const int32_t* tk = tokens + (int64_t)b * ld_tok;
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
    float tailv = has_tail ? row[ti] + mask[ti] : -INFINITY;
    int text_lo = 0, ts_lo = r.tb, ts_hi = V - 1;
    if constexpr (RULES) {
        const int len = p + 1 - n_init;
        int t_idx = -1;  // index in seq of its last timestamp token
        for (int i = lane; i < len; i += 64) t_idx = tk[n_init + i] >= r.tb ? i : t_idx;
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
            const bool text = 4 * qi + e < r.tb;
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
    const float ts_mass = bs.v == -INFINITY ? -INFINITY : bs.v + logf(tot_s);
    const bool text_dead = ts_mass > bt.v;  // rule 5: the row is its timestamp side
    float top_v, top_logprob;  // l at the arg-max and its log-probability: logsumexp(l) = top_v - top_logprob
    if (text_dead) {
        top_logprob = -logf(tot_s);
        top_v = bs.v;
    } else {
        const MaxIdx bm = better(bt, bs);
        top_logprob = -logf(tot_t * __expf(base_t - bm.v) + (bs.v == -INFINITY ? 0.f : tot_s * __expf(base_s - bm.v)));
        top_v = bm.v;
    }
    // ---- the n_top best columns of the filtered row, lowest column on ties (a dead column is -inf and still a column) ----
    // A column that has been handed out, and the padding behind the row, become NaN: `better` never prefers a NaN.  The rounds' loop
    // then holds no test that does not change with k.
#pragma unroll
    for (int j = 0; j < GS_MAXQ; ++j) {
        const int qi = tid + j * GS_THREADS;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (text_dead && 4 * qi + e < r.tb) vals[j][e] = -INFINITY;
            if (qi >= nq) vals[j][e] = __builtin_nanf("");
        }
    }
    if (text_dead && ti < r.tb) tailv = -INFINITY;
    if (!has_tail) tailv = __builtin_nanf("");
    for (int k = 0; k < n_top; ++k) {
        MaxIdx m = better(MaxIdx{-INFINITY, 0x7fffffff}, MaxIdx{tailv, ti});
#pragma unroll
        for (int j = 0; j < GS_MAXQ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) m = better(m, MaxIdx{vals[j][e], 4 * (tid + j * GS_THREADS) + e});
        m = wave_argmax(m);
        // two sets of slots, by the parity of k: ONE barrier per round (a wave two rounds ahead has passed the barrier in between)
        const int slot = (k & 1) * NW;
        if (lane == 0) {
            s_v[slot + wave] = m.v;
            s_i[slot + wave] = m.i;
        }
        __syncthreads();
        MaxIdx bk{s_v[slot], s_i[slot]};
#pragma unroll
        for (int w = 1; w < NW; ++w) bk = better(bk, MaxIdx{s_v[slot + w], s_i[slot + w]});
        tailv = bk.i == ti ? __builtin_nanf("") : tailv;
#pragma unroll
        for (int j = 0; j < GS_MAXQ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) vals[j][e] = bk.i == 4 * (tid + j * GS_THREADS) + e ? __builtin_nanf("") : vals[j][e];
        if (tid == 0) {
            Cand c;
            c.logprob = bk.v == -INFINITY ? -INFINITY : (bk.v - top_v) + top_logprob;
            c.col = bk.i == 0x7fffffff ? -1 : bk.i;
            cand[(int64_t)b * n_top + k] = c;
        }
    }
}

struct BeamArgs {
    int32_t* tokens; int64_t ld_tok;
    int32_t* pos; int64_t* posd;
    int n_init, eot, n_ctx, G, maxc, cap;
    float* sum_logprobs; int32_t* not_done;
    const Cand* cand; uint8_t* anc; int32_t* src;
    int32_t* fin_tok; float* fin_score; int32_t* fin_len; int32_t* fin_count; int32_t* counters;
    const void* emb; int emb_dtype; const float* emb_scale; const float* pos_emb;
    float* x; const float* ln_w; const float* ln_b; void* y; int D; float eps;
};

// EMBED: a step's last launch (the next step's input rows, the position advance); without it the selection alone (wipa_beam_step).
// Every decision below is computed by every thread from LDS values all of them see after a barrier: candidate i finds its own place
// in the order by counting the candidates that precede it -- no thread walks the list for the others.
template <typename TO, bool EMBED>
__global__ __launch_bounds__(BS_THREADS) void beam_select_kernel(BeamArgs q) {
    __shared__ float s_score[BEAM_MAX_N];
    __shared__ int s_col[BEAM_MAX_N];
    __shared__ int s_bsrc[BEAM_MAX_G], s_btok[BEAM_MAX_G];
    __shared__ float s_bsum[BEAM_MAX_G];
    __shared__ int s_fsrc[BEAM_MAX_G];
    __shared__ float s_fscore[BEAM_MAX_G];
    __shared__ int s_nfin;
    __shared__ float s_red[4];
    __shared__ int32_t s_tok[BEAM_MAX_G][BS_THREADS];  // the gather's stage: a column of G rows per thread
    __shared__ uint8_t s_anc[BEAM_MAX_G][BS_THREADS];
    const int clip = blockIdx.x, tid = threadIdx.x, G = q.G;
    const int row0 = clip * G;
    const int p = tail_pos(q.pos);
    const bool walk = in_prompt(p, q.n_init);  // uniform: the token of column p + 1 is in place, nothing is selected
    if (!walk) {
        const int nb = (p + 1 == q.n_init) ? 1 : G;  // first generated step: the beams of a clip are one sequence, beam 0 offers alone
        const int N = nb * (G + 1);
        if (tid == 0) s_nfin = 0;
        for (int i = tid; i < N; i += BS_THREADS) {
            const int beam = i / (G + 1);
            const Cand c = q.cand[(int64_t)(row0 + beam) * (G + 1) + i % (G + 1)];
            s_score[i] = q.sum_logprobs[row0 + beam] + c.logprob;  // the cumulative score: one f32 add
            s_col[i] = c.col;
        }
        __syncthreads();
        for (int i = tid; i < N; i += BS_THREADS) {
            const float si = s_score[i];
            int before = 0, beams_before = 0;  // candidates ahead of i in the walk, and those of them that are no EOT
            for (int j = 0; j < N; ++j) {
                const float sj = s_score[j];
                const bool ahead = sj > si || (sj == si && j < i);  // descending score; ties: lower beam, then lower rank
                before += ahead ? 1 : 0;
                beams_before += (ahead && s_col[j] != q.eot) ? 1 : 0;
            }
            if (beams_before < G) {  // the walk reaches i: it stops once G beams are saved
                if (s_col[i] != q.eot) {
                    s_bsrc[beams_before] = i / (G + 1);
                    s_btok[beams_before] = s_col[i];
                    s_bsum[beams_before] = si;
                } else {
                    const int f = before - beams_before;  // EOT candidates ahead of it: at most one per beam, so f < G
                    s_fsrc[f] = i / (G + 1);
                    s_fscore[f] = si;
                    atomicAdd(&s_nfin, 1);
                }
            }
        }
        // the store's count is read by every thread BEFORE the barrier: thread 0 rewrites it at the end of this block
        const int cnt_old = q.fin_count[clip];
        __syncthreads();
        // newly finished sequences, in descending score, while the clip's store holds fewer than maxc
        const int room = q.maxc - cnt_old;
        const int n_acc = min(s_nfin, room > 0 ? room : 0);
        for (int f = 0; f < n_acc; ++f) {
            const int64_t slot = (int64_t)clip * q.cap + cnt_old + f;
            int32_t* dst = q.fin_tok + slot * q.ld_tok;
            const int32_t* from = q.tokens + (int64_t)(row0 + s_fsrc[f]) * q.ld_tok;
            for (int t = tid; t <= p; t += BS_THREADS) dst[t] = from[t];
            if (tid == 0) {
                dst[p + 1] = q.eot;
                q.fin_score[slot] = s_fscore[f];
                q.fin_len[slot] = p + 1 - q.n_init;
            }
        }
        // The clip completes at this step with fewer than G sequences (max_candidates < G, patience below 1): upstream leaves its loop
        // here and finalize fills the store with THIS step's new beams + EOT in descending sum -- the order the walk saved them in.  Done
        // now, because the decode may run on for some steps before the host looks at not_done, and the live beams then are others.
        int cnt_new = cnt_old + n_acc;
        if (room > 0 && cnt_new >= q.maxc && cnt_new < G) {
            for (int j = 0; cnt_new + j < G; ++j) {
                const int64_t slot = (int64_t)clip * q.cap + cnt_new + j;
                int32_t* dst = q.fin_tok + slot * q.ld_tok;
                const int32_t* from = q.tokens + (int64_t)(row0 + s_bsrc[j]) * q.ld_tok;
                for (int t = tid; t <= p; t += BS_THREADS) dst[t] = from[t];
                if (tid == 0) {
                    dst[p + 1] = s_btok[j];
                    dst[p + 2] = q.eot;
                    q.fin_score[slot] = s_bsum[j];
                    q.fin_len[slot] = p + 2 - q.n_init;
                }
            }
            cnt_new = G;
        }
        // the token rows and the ancestor table by source.  A thread owns its columns and its column of the LDS stage: it reads all G rows
        // of a column, then writes them (and the store copy above read the same columns in the same thread), so nothing is read after
        // another thread wrote it, and no barrier is needed
        for (int t = tid; t <= p; t += BS_THREADS) {
            for (int g = 0; g < G; ++g) {
                s_tok[g][tid] = q.tokens[(int64_t)(row0 + g) * q.ld_tok + t];
                s_anc[g][tid] = q.anc[(int64_t)(row0 + g) * q.ld_tok + t];
            }
            for (int j = 0; j < G; ++j) {
                const int sj = s_bsrc[j];
                q.tokens[(int64_t)(row0 + j) * q.ld_tok + t] = s_tok[sj][tid];
                q.anc[(int64_t)(row0 + j) * q.ld_tok + t] = s_anc[sj][tid];  // column p holds the source itself: the table was the identity there
            }
        }
        if (tid < G) {
            q.tokens[(int64_t)(row0 + tid) * q.ld_tok + p + 1] = s_btok[tid];
            q.sum_logprobs[row0 + tid] = s_bsum[tid];
            q.src[row0 + tid] = s_bsrc[tid];
        }
        if (tid == 0) {
            q.fin_count[clip] = cnt_new;
            if (cnt_new < q.maxc) atomicAdd(q.counters, 1);
        }
    }
    if constexpr (EMBED) {
        const int pp = min(p + 1, q.n_ctx - 1);
        for (int j = 0; j < G; ++j) {
            const int b = row0 + j;
            const int tok = walk ? q.tokens[(int64_t)b * q.ld_tok + p + 1] : s_btok[j];
            row_embed_layernorm<TO>(tid, tok, pp, q.emb, q.emb_dtype, q.emb_scale, q.pos_emb, q.x + (int64_t)b * q.D, q.ln_w, q.ln_b,
                                    (TO*)q.y + (int64_t)b * q.D, q.D, q.eps, s_red);
            __syncthreads();  // s_red is written again by the next row
        }
    }
    if (tid == 0) {
        __threadfence();
        const int arrived = atomicAdd(q.counters + 1, 1);
        if (arrived == (int)gridDim.x - 1) {  // the last workgroup: this step's count of clips still collecting, and the position
            __threadfence();
            q.counters[1] = 0;
            if (!walk) *q.not_done = atomicExch(q.counters, 0);
            if constexpr (EMBED) {
                *q.pos = p + 1;
                *q.posd = (int64_t)(p + 1) * q.D;
            }
        }
    }
}

// One wave per clip.  Every lane computes the same decisions from the same memory; the lanes share the copies.
__global__ __launch_bounds__(64) void beam_finalize_kernel(const int32_t* __restrict__ tokens, int64_t ld_tok, int G, int cap, int sample_begin,
                                                           int n, int eot, const float* __restrict__ sum_logprobs,
                                                           const double* __restrict__ penalty, int32_t* __restrict__ fin_tok,
                                                           float* __restrict__ fin_score, int32_t* __restrict__ fin_len,
                                                           int32_t* __restrict__ fin_count, int32_t* __restrict__ best_tokens, int64_t ld_out,
                                                           float* __restrict__ best_sum, int32_t* __restrict__ best_len) {
    const int clip = blockIdx.x, lane = threadIdx.x, row0 = clip * G;
    // wipa_rank_groups' arithmetic: (double)sum / penalty[length], the first maximum wins; length 0 scores -inf.  The store's sequences
    // are scored first, in their order, then the ones filled in below as they are made: their values are still in registers
    int best_len_v = 0;
    float best_sum_v = 0.f;
    double best_score = 0.0;
    const int32_t* best_from = nullptr;
    auto consider = [&](float sum, int len, const int32_t* from) {
        const double score = len > 0 ? (double)sum / penalty[len] : -__builtin_huge_val();
        if (!best_from || score > best_score) {
            best_score = score;
            best_sum_v = sum;
            best_len_v = len;
            best_from = from;
        }
    };
    int cnt = fin_count[clip];
    for (int k = 0; k < cnt; ++k) {
        const int64_t slot = (int64_t)clip * cap + k;
        consider(fin_score[slot], fin_len[slot], fin_tok + slot * ld_tok);
    }
    unsigned used = 0u;
    while (cnt < G) {  // fewer than G finished: live beams + EOT in descending sum (the lower beam on ties)
        int pick = -1;
        float pick_v = 0.f;
        for (int g = 0; g < G; ++g) {
            const float v = sum_logprobs[row0 + g];
            if (!((used >> g) & 1u) && (pick < 0 || v > pick_v)) {
                pick = g;
                pick_v = v;
            }
        }
        used |= 1u << pick;
        const int64_t slot = (int64_t)clip * cap + cnt;
        int32_t* dst = fin_tok + slot * ld_tok;
        const int32_t* from = tokens + (int64_t)(row0 + pick) * ld_tok;
        for (int t = lane; t < sample_begin + n; t += 64) dst[t] = from[t];
        if (lane == 0) {
            dst[sample_begin + n] = eot;
            fin_score[slot] = pick_v;
            fin_len[slot] = n;
        }
        consider(pick_v, n, from);  // the live row holds the same columns below sample_begin + n
        ++cnt;
    }
    if (lane == 0) fin_count[clip] = cnt;
    int32_t* dst = best_tokens + (int64_t)clip * ld_out;
    for (int t = lane; t < sample_begin + n + 1; t += 64) dst[t] = t < sample_begin + best_len_v ? best_from[t] : eot;
    if (lane == 0) {
        best_sum[clip] = best_sum_v;
        best_len[clip] = best_len_v;
    }
}

int beam_shape_check(const char* who, int B, int n_group, int max_candidates) {
    WIPA_REQUIRE(n_group >= 1 && n_group <= BEAM_MAX_G, "%s: n_group=%d outside 1..%d (2..%d beams, or 1: one row per clip)", who, n_group,
                 BEAM_MAX_G, BEAM_MAX_G);
    WIPA_REQUIRE(B > 0 && B % n_group == 0, "%s: B=%d rows are no multiple of n_group=%d (rows = clips x beams)", who, B, n_group);
    WIPA_REQUIRE(max_candidates >= 1 && max_candidates <= BEAM_MAX_CAND, "%s: max_candidates=%d outside 1..%d", who, max_candidates, BEAM_MAX_CAND);
    return WIPA_OK;
}

}  // namespace

extern "C" size_t wipa_beam_bytes(int B, int n_group, int max_candidates, int64_t ld_tok) {
    if (B <= 0 || n_group < 1 || n_group > BEAM_MAX_G || B % n_group != 0 || max_candidates < 1 || max_candidates > BEAM_MAX_CAND || ld_tok < 1)
        return 0;
    return beam_layout(B, n_group, max_candidates, ld_tok).total;
}

extern "C" int wipa_beam_begin(void* beam, size_t beam_bytes, int B, int n_group, int max_candidates, int64_t ld_tok, wipa_stream_t stream) {
    WIPA_REQUIRE(beam && ((uintptr_t)beam % 16) == 0 && ld_tok >= 1, "wipa_beam_begin: null / unaligned beam buffer");
    const int rc = beam_shape_check("wipa_beam_begin", B, n_group, max_candidates);
    if (rc != WIPA_OK) return rc;
    const BeamLayout L = beam_layout(B, n_group, max_candidates, ld_tok);
    WIPA_REQUIRE(beam_bytes >= L.total, "wipa_beam_begin: the beam buffer holds %zu bytes, this shape needs %zu (wipa_beam_bytes)", beam_bytes, L.total);
    char* bb = (char*)beam;
    const int64_t n = (int64_t)B * ld_tok;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(beam_begin_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint8_t*)(bb + L.anc), ld_tok, B, n_group,
                       (int32_t*)(bb + L.fin_count), B / n_group, (int32_t*)(bb + L.counters));
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// The beam tail on written logits: beam_topk + beam_select.  tok_emb == NULL: the selection alone (wipa_beam_step); else a decode step's
// last two launches (declared in wipa_common.h for the runtime; not exported).
int wipa_beam_tail(const char* who, const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                   int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int n_init, int eot, const wipa_decode_rules* rules,
                   void* beam, int n_group, int max_candidates, float* sum_logprobs, int32_t* not_done, const void* tok_emb, int emb_dtype,
                   const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b, void* y, int y_dtype,
                   int D, float eps, wipa_stream_t stream) {
    WIPA_REQUIRE(logits && mask_first && mask_always && tokens && pos_dev && sum_logprobs && not_done && n_init >= 1, "%s: bad arguments", who);
    WIPA_REQUIRE(beam && ((uintptr_t)beam % 16) == 0, "%s: null / unaligned beam buffer", who);
    const int rc = beam_shape_check(who, B, n_group, max_candidates);
    if (rc != WIPA_OK) return rc;
    WIPA_REQUIRE(V > n_group + 1 && V <= 4 * GS_MAXQ * GS_THREADS && ldl % 4 == 0 && ldl >= V && ((uintptr_t)logits % 16) == 0 &&
                     ((uintptr_t)mask_first % 16) == 0 && ((uintptr_t)mask_always % 16) == 0,
                 "%s: vocabulary of %d / unaligned logits or masks", who, V);
    WIPA_REQUIRE(eot >= 0 && eot < V && ld_tok >= 2, "%s: eot=%d outside the vocabulary of %d", who, eot, V);
    RulesDev r = {V, -1, -1};
    if (rules) {
        WIPA_REQUIRE(rules->timestamp_begin > 0 && rules->timestamp_begin < V && eot < rules->timestamp_begin && rules->no_timestamps >= 0 &&
                         rules->no_timestamps < rules->timestamp_begin,
                     "%s: need eot < timestamp_begin < V and no_timestamps below timestamp_begin (eot=%d timestamp_begin=%d no_timestamps=%d V=%d)",
                     who, eot, rules->timestamp_begin, rules->no_timestamps, V);
        r.tb = rules->timestamp_begin;
        r.nt = rules->no_timestamps;
        r.max_init = rules->max_initial_timestamp_index;
    }
    if (tok_emb) {
        WIPA_REQUIRE(posd_dev && pos_emb && x && ln_w && ln_b && y && n_ctx > 0 && ld_tok >= n_ctx + 2, "%s: bad arguments", who);
        WIPA_REQUIRE(D % 4 == 0 && D > 0 && D <= 2048, "%s: D=%d must be a multiple of 4 and <= 2048", who, D);
        WIPA_REQUIRE(emb_dtype == WIPA_F32 || emb_dtype == WIPA_BF16, "%s: bad embedding dtype %d", who, emb_dtype);
        WIPA_REQUIRE(y_dtype == WIPA_F32 || y_dtype == WIPA_BF16, "%s: bad dtype %d", who, y_dtype);
    }
    const BeamLayout L = beam_layout(B, n_group, max_candidates, ld_tok);
    char* bb = (char*)beam;
    hipStream_t s = (hipStream_t)stream;
    Cand* cand = (Cand*)(bb + L.cand);
    if (rules)
        hipLaunchKernelGGL((beam_topk_kernel<true>), dim3(B), dim3(GS_THREADS), 0, s, logits, ldl, V, mask_first, mask_always, tokens, ld_tok, pos_dev,
                           n_init, eot, r, cand, n_group + 1);
    else
        hipLaunchKernelGGL((beam_topk_kernel<false>), dim3(B), dim3(GS_THREADS), 0, s, logits, ldl, V, mask_first, mask_always, tokens, ld_tok, pos_dev,
                           n_init, eot, r, cand, n_group + 1);
    WIPA_LAUNCH_CHECK();
    BeamArgs q = {};
    q.tokens = tokens; q.ld_tok = ld_tok; q.pos = pos_dev; q.posd = posd_dev;
    q.n_init = n_init; q.eot = eot; q.n_ctx = n_ctx; q.G = n_group; q.maxc = max_candidates; q.cap = L.cap;
    q.sum_logprobs = sum_logprobs; q.not_done = not_done;
    q.cand = cand; q.anc = (uint8_t*)(bb + L.anc); q.src = (int32_t*)(bb + L.src);
    q.fin_tok = (int32_t*)(bb + L.fin_tok); q.fin_score = (float*)(bb + L.fin_score); q.fin_len = (int32_t*)(bb + L.fin_len);
    q.fin_count = (int32_t*)(bb + L.fin_count); q.counters = (int32_t*)(bb + L.counters);
    q.emb = tok_emb; q.emb_dtype = emb_dtype; q.emb_scale = emb_scale; q.pos_emb = pos_emb;
    q.x = x; q.ln_w = ln_w; q.ln_b = ln_b; q.y = y; q.D = D; q.eps = eps;
    const dim3 grid(B / n_group), block(BS_THREADS);
    if (!tok_emb) hipLaunchKernelGGL((beam_select_kernel<float, false>), grid, block, 0, s, q);
    else if (y_dtype == WIPA_F32) hipLaunchKernelGGL((beam_select_kernel<float, true>), grid, block, 0, s, q);
    else hipLaunchKernelGGL((beam_select_kernel<__bf16, true>), grid, block, 0, s, q);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_beam_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always, int32_t* tokens,
                              int64_t ld_tok, int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules, void* beam, int n_group,
                              int max_candidates, float* sum_logprobs, int32_t* not_done, wipa_stream_t stream) {
    return wipa_beam_tail("wipa_beam_step", logits, ldl, B, V, mask_first, mask_always, tokens, ld_tok, pos_dev, nullptr, n_init, eot, rules, beam,
                          n_group, max_candidates, sum_logprobs, not_done, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0.f,
                          stream);
}

extern "C" int wipa_beam_finalize(void* beam, const int32_t* tokens, int64_t ld_tok, int B, int n_group, int max_candidates, int sample_begin, int n,
                                  int eot, const float* sum_logprobs, const double* penalty, int32_t* best_tokens, int64_t ld_out, float* best_sum,
                                  int32_t* best_len, wipa_stream_t stream) {
    WIPA_REQUIRE(beam && tokens && sum_logprobs && penalty && best_tokens && best_sum && best_len, "wipa_beam_finalize: null pointer");
    const int rc = beam_shape_check("wipa_beam_finalize", B, n_group, max_candidates);
    if (rc != WIPA_OK) return rc;
    WIPA_REQUIRE(sample_begin >= 0 && n >= 1 && (int64_t)sample_begin + n + 1 <= ld_tok && (int64_t)sample_begin + n + 1 <= ld_out,
                 "wipa_beam_finalize: columns [%d, %d + %d] outside ld_tok=%lld / ld_out=%lld", sample_begin, sample_begin, n, (long long)ld_tok,
                 (long long)ld_out);
    const BeamLayout L = beam_layout(B, n_group, max_candidates, ld_tok);
    char* bb = (char*)beam;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(B / n_group), dim3(64), 0, (hipStream_t)stream, tokens, ld_tok, n_group, L.cap, sample_begin, n, eot,
                       sum_logprobs, penalty, (int32_t*)(bb + L.fin_tok), (float*)(bb + L.fin_score), (int32_t*)(bb + L.fin_len),
                       (int32_t*)(bb + L.fin_count), best_tokens, ld_out, best_sum, best_len);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// Best-of-N ranking of candidate groups on the device (wipa_rank_groups): MaximumLikelihoodRanker.rank of openai-whisper's decoding.py,
// which mlx_whisper ports -- the sampling path of DecodingTask.run draws n_group = best_of candidates per window and keeps the one with
// the highest length-normalised log-probability (the reference reaches it through mlx_whisper.transcribe's temperature fallback).
// One wave per clip: the lanes look for a candidate's first EOT together, lane 0 scores the candidates in order, all lanes copy
// the winner's row.  The host then reads clips x columns instead of rows x columns.
#include "wipa_common.h"

namespace {

// score = (double)sum_logprobs / penalty[length] in IEEE double division on operands that are exactly upstream's (the f32 sum widened,
// the penalty as the host's Python floats computed it), so the device ranks as the Python arithmetic does, bit for bit.  length 0 (EOT
// in the first generated column; suppress_blank=False only) scores -inf where upstream divides by zero.
__global__ __launch_bounds__(64) void rank_groups_kernel(const int32_t* __restrict__ tokens, int64_t ld_tok, int n_group, int sample_begin,
                                                         int n, int eot, const float* __restrict__ sum_logprobs,
                                                         const double* __restrict__ penalty, int32_t* __restrict__ winner,
                                                         int32_t* __restrict__ length, int32_t* __restrict__ best_tokens, int64_t ld_out,
                                                         float* __restrict__ best_sum) {
    const int clip = blockIdx.x, lane = threadIdx.x;
    int best = 0;
    double best_score = 0.0;
    for (int k = 0; k < n_group; ++k) {
        const int b = clip * n_group + k;
        const int32_t* row = tokens + (int64_t)b * ld_tok + sample_begin;
        int first = n;  // generated tokens before the first EOT; n when there is none
        for (int i = lane; i < n; i += 64)
            if (row[i] == eot) {
                first = i;
                break;
            }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
        const double score = first > 0 ? (double)sum_logprobs[b] / penalty[first] : -__builtin_huge_val();
        if (lane == 0) length[b] = first;
        if (k == 0 || score > best_score) {  // strictly greater: the first maximum wins (np.argmax)
            best = k;
            best_score = score;
        }
    }
    const int bw = clip * n_group + best;
    if (lane == 0) {
        winner[clip] = best;
        best_sum[clip] = sum_logprobs[bw];
    }
    const int32_t* src = tokens + (int64_t)bw * ld_tok;
    int32_t* dst = best_tokens + (int64_t)clip * ld_out;
    for (int i = lane; i < sample_begin + n; i += 64) dst[i] = src[i];
}

}  // namespace

extern "C" int wipa_rank_groups(const int32_t* tokens, int64_t ld_tok, int B, int n_group, int sample_begin, int n, int eot,
                                const float* sum_logprobs, const double* penalty, int32_t* winner, int32_t* length, int32_t* best_tokens,
                                int64_t ld_out, float* best_sum, wipa_stream_t stream) {
    WIPA_REQUIRE(tokens && sum_logprobs && penalty && winner && length && best_tokens && best_sum, "wipa_rank_groups: null pointer");
    WIPA_REQUIRE(B > 0 && n_group >= 1 && n_group <= 64 && B % n_group == 0, "wipa_rank_groups: B=%d rows, n_group=%d (1..64, dividing B)", B, n_group);
    WIPA_REQUIRE(sample_begin >= 0 && n >= 1 && (int64_t)sample_begin + n <= ld_tok && (int64_t)sample_begin + n <= ld_out,
                 "wipa_rank_groups: columns [%d, %d + %d) outside ld_tok=%lld / ld_out=%lld", sample_begin, sample_begin, n, (long long)ld_tok,
                 (long long)ld_out);
    hipLaunchKernelGGL(rank_groups_kernel, dim3(B / n_group), dim3(64), 0, (hipStream_t)stream, tokens, ld_tok, n_group, sample_begin, n, eot,
                       sum_logprobs, penalty, winner, length, best_tokens, ld_out, best_sum);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

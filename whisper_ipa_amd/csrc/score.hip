// K14: batched edit distances for PER / PFER scoring.  Replaces the dynamic programs of scripts/evaluate_ipa.py -- edit_distance
// behind phone_error_rate (reference evaluate_ipa.py:80-105) and PFERCalculator.phone_feature_error_rate (:139-213) -- for a whole
// batch of (reference, hypothesis) phone sequences in ONE launch.  The host keeps the Unicode work (tokenisation, one feature lookup
// per distinct phone); every DP cell is computed here.
//
//   per[i][j]  = min(per[i-1][j] + 1,   per[i][j-1] + 1,   per[i-1][j-1] + (ref_id[i] != hyp_id[j]))
//   pf24[i][j] = min(pf24[i-1][j] + 24, pf24[i][j-1] + 24, pf24[i-1][j-1] + d(ref[i], hyp[j]))
//   d(a, b) = number of the 24 features that differ = popcount((x | x >> 1) & 0x5555...), x = code[a] ^ code[b]  (2 bits a feature)
//
// pf24 is the reference's float DP times 24 in exact integers (insertion = deletion = 1 -> 24, substitution k/24 -> k).  Equal ids
// have equal codes, so the reference's "same string costs 0" shortcut needs no branch; two different phones the table does not know
// both carry the zero code and cost 0, as in the reference.  Integers only: nothing here depends on the order of anything.
//
// MI355X mapping: one wave (64 lanes) per pair, four independent waves per workgroup (no barrier anywhere), pairs taken in the
// host's m*n-descending `order` so that the long pairs start first.  The hypothesis runs along the lanes in chunks of 64 columns;
// inside a chunk the reference is walked by ANTI-DIAGONALS: at step t lane l computes cell (i = t - l + 1, j = 64 c + l + 1).
// Its upper neighbour is its own previous value, its left neighbour the previous value of lane l - 1 (one __shfl_up per DP) and its
// diagonal neighbour the left value of the step before (kept in a register), so a step costs two shuffles for the two DPs and three
// to move the reference phone (id + 64-bit code) one lane up.  The alternative, row by row with dp[i][j] = 24 j + prefixmin_k<=j(a_k
// - 24 k), needs a 6-step wave scan per DP and row -- twelve dependent shuffles per 64 cells against five here -- and wins only the
// 63 fill / drain steps per chunk, which at the typical 20-110 phones is less than the scans cost.  Lane 0 takes its left / diagonal
// neighbours from the last column of the previous chunk, which lane 63 leaves in LDS (one int2 per reference row and wave, 8 KB a
// wave); that column and the reference phones are fetched 64 rows at a time (lane k holds row t0 + k) and handed to lane 0 with a
// v_readlane per step, so no step waits on a dependent memory load.  A 1024 x 1024 pair is 16 chunks x 1087 steps.
#include "wipa_common.h"

namespace {

constexpr int WAVES = 4;
constexpr int MAX_LEN = WIPA_SCORE_MAX_LEN;
constexpr int FEATURE_COST = 24;  // insertion / deletion in units of 1/24

__device__ __forceinline__ int lane_value(int v, int src_lane) { return __builtin_amdgcn_readlane(v, src_lane); }
__device__ __forceinline__ unsigned long long lane_value(unsigned long long v, int src_lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src_lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src_lane);
    return ((unsigned long long)hi << 32) | lo;
}

template <bool FEATURES>
__global__ __launch_bounds__(WAVES * 64) void edit_distance_kernel(const int32_t* __restrict__ ref_ids, const int32_t* __restrict__ ref_off,
                                                                   const int32_t* __restrict__ hyp_ids, const int32_t* __restrict__ hyp_off,
                                                                   const int32_t* __restrict__ order, int n_pairs,
                                                                   const unsigned long long* __restrict__ codes, int n_phones,
                                                                   int32_t* __restrict__ per_dist, int32_t* __restrict__ pfer24) {
    __shared__ int2 edge_all[WAVES][MAX_LEN + 1];  // [row i] = (per, pf24) of the previous chunk's last column
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // the pair's lengths stay scalar
    const int slot = blockIdx.x * WAVES + wave;
    if (slot >= n_pairs) return;
    const int p = order[slot];
    if ((unsigned)p >= (unsigned)n_pairs) return;  // not a permutation: the Python layer never builds one
    const int r0 = ref_off[p], h0 = hyp_off[p];
    const int m = ref_off[p + 1] - r0, n = hyp_off[p + 1] - h0;
    if (m < 0 || n < 0 || m > MAX_LEN || n > MAX_LEN) {  // the entry point has checked the host copy of the offsets
        if (lane == 0) per_dist[p] = pfer24[p] = -1;
        return;
    }
    if (n == 0) {  // m deletions
        if (lane == 0) {
            per_dist[p] = m;
            pfer24[p] = FEATURE_COST * m;
        }
        return;
    }
    int2* edge = edge_all[wave];
    const int32_t* ref = ref_ids + r0;
    const int32_t* hyp = hyp_ids + h0;
    auto code_of = [&](int id) -> unsigned long long { return FEATURES && (unsigned)id < (unsigned)n_phones ? codes[id] : 0ull; };

    int cur_per = 0, cur_pf = 0;
    const int n_chunks = (n + 63) >> 6;
    for (int c = 0; c < n_chunks; ++c) {
        const int j = 64 * c + lane + 1;  // this lane's column, 1-based
        const int width = min(64, n - 64 * c);
        const int hid = j <= n ? hyp[j - 1] : -1;
        const unsigned long long hcode = code_of(hid);
        cur_per = j;  // row 0
        cur_pf = FEATURE_COST * j;
        int diag_per = j - 1, diag_pf = FEATURE_COST * (j - 1);
        int rid = -2, blk_rid = -2, blk_per = 0, blk_pf = 0;
        unsigned long long rcode = 0, blk_rcode = 0;
        const int steps = m + width - 1;  // the chunk's last live lane reaches row m at step m + width - 2
        for (int t = 0; t < steps; ++t) {
            if ((t & 63) == 0) {  // rows t + 1 .. t + 64: reference phones and the column left of lane 0, one row per lane
                const int row = t + lane + 1;
                blk_rid = row <= m ? ref[row - 1] : -2;
                blk_rcode = code_of(blk_rid);
                if (c == 0) {
                    blk_per = row;
                    blk_pf = FEATURE_COST * row;
                } else if (row <= m) {  // rows >= t + 1 are rewritten from step t + 63 on: still the previous chunk's
                    const int2 e = edge[row];
                    blk_per = e.x;
                    blk_pf = e.y;
                }
            }
            const int src = t & 63;
            int left_per = __shfl_up(cur_per, 1, 64), left_pf = __shfl_up(cur_pf, 1, 64);
            int up_rid = __shfl_up(rid, 1, 64);
            unsigned long long up_rcode = FEATURES ? __shfl_up(rcode, 1, 64) : 0ull;
            const int in_per = lane_value(blk_per, src), in_pf = lane_value(blk_pf, src), in_rid = lane_value(blk_rid, src);
            const unsigned long long in_rcode = FEATURES ? lane_value(blk_rcode, src) : 0ull;
            if (lane == 0) {
                left_per = in_per;
                left_pf = in_pf;
                up_rid = in_rid;
                up_rcode = in_rcode;
            }
            rid = up_rid;  // the phone of row i = t - lane + 1
            rcode = up_rcode;
            const int i = t - lane + 1;
            if (i >= 1 && i <= m && j <= n) {
                const unsigned long long x = rcode ^ hcode;
                const int d = FEATURES ? __popcll((x | (x >> 1)) & 0x5555555555555555ull) : 0;
                cur_per = min(min(cur_per, left_per) + 1, diag_per + (rid != hid ? 1 : 0));
                cur_pf = min(min(cur_pf, left_pf) + FEATURE_COST, diag_pf + d);
                diag_per = left_per;
                diag_pf = left_pf;
                if (lane == 63) edge[i] = make_int2(cur_per, cur_pf);
            }
        }
        // lane 0 of the next chunk reads what lane 63 of this one wrote: same wave, so program order is all it takes
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (lane == ((n - 1) & 63)) {
        per_dist[p] = cur_per;
        pfer24[p] = FEATURES ? cur_pf : FEATURE_COST * cur_per;
    }
}

}  // namespace

extern "C" int wipa_edit_distance_batch(const int32_t* ref_ids, const int32_t* ref_off, const int32_t* hyp_ids, const int32_t* hyp_off,
                                        const int32_t* order, int n_pairs, const uint64_t* feat_codes, int n_phones,
                                        const int32_t* ref_off_host, const int32_t* hyp_off_host, int32_t* per_dist, int32_t* pfer24,
                                        wipa_stream_t s) {
    WIPA_REQUIRE(n_pairs >= 0, "wipa_edit_distance_batch: n_pairs %d is negative", n_pairs);
    WIPA_REQUIRE(n_phones >= 1, "wipa_edit_distance_batch: n_phones %d, need at least 1", n_phones);
    WIPA_REQUIRE(n_pairs == 0 || (ref_off_host && hyp_off_host), "wipa_edit_distance_batch: null host offsets");
    if (n_pairs > 0) {
        WIPA_REQUIRE(ref_off_host[0] == 0 && hyp_off_host[0] == 0, "wipa_edit_distance_batch: pair 0: offsets start at %d / %d, not 0",
                     ref_off_host[0], hyp_off_host[0]);
    }
    for (int p = 0; p < n_pairs; ++p) {
        const long long m = (long long)ref_off_host[p + 1] - ref_off_host[p], n = (long long)hyp_off_host[p + 1] - hyp_off_host[p];
        WIPA_REQUIRE(m >= 0 && n >= 0, "wipa_edit_distance_batch: pair %d: decreasing offsets (lengths %lld / %lld)", p, m, n);
        WIPA_REQUIRE(m <= WIPA_SCORE_MAX_LEN && n <= WIPA_SCORE_MAX_LEN, "wipa_edit_distance_batch: pair %d: lengths %lld / %lld exceed %d",
                     p, m, n, WIPA_SCORE_MAX_LEN);
    }
    if (n_pairs == 0) return WIPA_OK;
    WIPA_REQUIRE(ref_ids && ref_off && hyp_ids && hyp_off && order && per_dist && pfer24, "wipa_edit_distance_batch: null pointer");
    const dim3 grid((n_pairs + WAVES - 1) / WAVES), block(WAVES * 64);
    const auto* codes = reinterpret_cast<const unsigned long long*>(feat_codes);
    if (feat_codes)
        hipLaunchKernelGGL(edit_distance_kernel<true>, grid, block, 0, (hipStream_t)s, ref_ids, ref_off, hyp_ids, hyp_off, order, n_pairs,
                           codes, n_phones, per_dist, pfer24);
    else
        hipLaunchKernelGGL(edit_distance_kernel<false>, grid, block, 0, (hipStream_t)s, ref_ids, ref_off, hyp_ids, hyp_off, order, n_pairs,
                           codes, n_phones, per_dist, pfer24);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

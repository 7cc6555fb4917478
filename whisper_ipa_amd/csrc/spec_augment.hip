// SpecAugment on the device (include/wipa.h "SpecAugment"): time and mel-bin masks stored into an f32 mel, in place.
//   The draw is stated in integers -- Philox words, a Q16 rate, __umulhi for the span starts -- and lives in ONE function,
//   spec_draw(), that the host (wipa_spec_augment_plan) and the kernel compile from the same text, so a clip's plan and the mask
//   the device writes are the same numbers by construction.
//   The kernel never reads the mel: a workgroup owns (clip, chunk of CHUNK frames), derives the clip's two span sets into LDS
//   (2 x 65 Philox calls by the first 130 lanes), turns them into a frame flag per chunk row and a flag per mel bin, and stores
//   `fill` to masked elements only: a time-masked frame goes out as 16-byte stores over the whole row, any other frame gets its
//   masked bins (a whole 16-byte group when all four bins are masked, single dwords at the edges of a bin span).
//   Every masked element is written by exactly one thread of exactly one workgroup and its value depends on (seed, stream, lengths)
//   only: no atomics, no dependence on B, on the clip's row or on the grid.
#include "wipa_common.h"

#include "philox.h"

namespace {

constexpr int SPANS = WIPA_SPEC_AUGMENT_MAX_SPANS;  // 64
constexpr int CHUNK = 128;                          // frames per workgroup
constexpr int MAX_BINS = 512;                       // flags held in LDS
constexpr int THREADS = 256;

struct SpecAxis {
    uint32_t L, w, n;
};

// axis geometry and span count of (stream, axis): L the axis length, w = min(length, L), n spans (0 when L == 0)
WIPA_HD SpecAxis spec_axis(const wipa_spec_augment_cfg& cfg, int a, uint32_t L, uint32_t s_lo, uint32_t s_hi, uint32_t k0, uint32_t k1) {
    SpecAxis ax;
    ax.L = L;
    ax.w = (uint32_t)cfg.length[a] < L ? (uint32_t)cfg.length[a] : L;
    if (L == 0) {
        ax.n = 0;
        return ax;
    }
    const uint64_t x = (uint64_t)cfg.rate_q16[a] * L;
    const uint32_t word = philox4x32_10(0xffffffffu, (uint32_t)a, s_lo, s_hi, k0, k1).w[0];
    uint64_t n = (x >> 16) + (((uint64_t)(word >> 16) < (x & 0xffffu)) ? 1u : 0u);
    if (n < (uint64_t)cfg.min_masks[a]) n = (uint64_t)cfg.min_masks[a];
    ax.n = n > SPANS ? SPANS : (uint32_t)n;
    return ax;
}

// start of span k of (stream, axis): a multiply-high onto [0, L - w]
WIPA_HD uint32_t spec_start(int a, uint32_t k, uint32_t L, uint32_t w, uint32_t s_lo, uint32_t s_hi, uint32_t k0, uint32_t k1) {
    return philox_mulhi(philox4x32_10(k, (uint32_t)a, s_lo, s_hi, k0, k1).w[0], L - w + 1u);
}

WIPA_HD uint32_t spec_time_length(const int32_t* n_frames, int b, int frames) {
    if (!n_frames) return (uint32_t)frames;
    const int32_t v = n_frames[b];
    return (uint32_t)(v < 0 ? 0 : (v > frames ? frames : v));
}

// VEC: rows are 16-byte aligned and n_mels is a multiple of 4 (every layout the package makes); else one dword per thread
template <bool VEC>
__global__ __launch_bounds__(THREADS) void spec_augment_kernel(float* __restrict__ mel, int64_t ld_clip, int64_t ld_frame, int frames,
                                                               int n_mels, wipa_spec_augment_cfg cfg, const uint32_t* __restrict__ streams,
                                                               const int32_t* __restrict__ n_frames, uint32_t k0, uint32_t k1) {
    __shared__ uint32_t s_start[2][SPANS];
    __shared__ uint32_t s_n[2], s_w[2];
    __shared__ uint32_t s_any;  // does this workgroup store anything
    __shared__ uint8_t s_frame[CHUNK];
    __shared__ __attribute__((aligned(4))) uint8_t s_bin[MAX_BINS];  // read four flags at a time

    const int b = blockIdx.y, tid = threadIdx.x;
    const int f0 = blockIdx.x * CHUNK;
    const uint32_t s_lo = streams[2 * b], s_hi = streams[2 * b + 1];
    const uint32_t L0 = spec_time_length(n_frames, b, frames);
    if (tid == 0) s_any = 0;
    if (tid < 2 * (SPANS + 1)) {
        const int a = tid / (SPANS + 1), j = tid - a * (SPANS + 1);
        const uint32_t L = a == 0 ? L0 : (uint32_t)n_mels;
        if (j == SPANS) {
            const SpecAxis ax = spec_axis(cfg, a, L, s_lo, s_hi, k0, k1);
            s_n[a] = ax.n;
            s_w[a] = ax.w;
        } else if (L > 0) {  // all 64 candidate starts: which of them count is known after the barrier
            const uint32_t w = (uint32_t)cfg.length[a] < L ? (uint32_t)cfg.length[a] : L;
            s_start[a][j] = spec_start(a, (uint32_t)j, L, w, s_lo, s_hi, k0, k1);
        }
    }
    __syncthreads();
    const int rows = min(CHUNK, frames - f0);  // > 0 by the grid
    for (int i = tid; i < rows + n_mels; i += THREADS) {
        const int a = i < rows ? 0 : 1;
        const uint32_t p = a == 0 ? (uint32_t)(f0 + i) : (uint32_t)(i - rows);
        const uint32_t n = s_n[a], w = s_w[a];
        bool hit = false;
        for (uint32_t k = 0; k < n; ++k) hit |= (p - s_start[a][k]) < w;  // unsigned: start <= p < start + w
        if (a == 0) s_frame[i] = hit; else s_bin[i - rows] = hit;
        if (hit) s_any = 1;  // same value from every writer
    }
    __syncthreads();
    if (!s_any) return;
    const float fill = cfg.fill;
    float* base = mel + (int64_t)b * ld_clip + (int64_t)f0 * ld_frame;
    if (VEC) {
        const int G = n_mels >> 2;
        const f32x4 fill4 = {fill, fill, fill, fill};
        for (int i = tid; i < rows * G; i += THREADS) {
            const int r = i / G, g = i - r * G;
            float* p = base + (int64_t)r * ld_frame + 4 * g;
            const uint32_t bins = *reinterpret_cast<const uint32_t*>(&s_bin[4 * g]);  // four byte flags
            if (s_frame[r] || bins == 0x01010101u) {
                *reinterpret_cast<f32x4*>(p) = fill4;
            } else if (bins) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((bins >> (8 * e)) & 1u) p[e] = fill;
            }
        }
    } else {
        for (int i = tid; i < rows * n_mels; i += THREADS) {
            const int r = i / n_mels, m = i - r * n_mels;
            if (s_frame[r] || s_bin[m]) base[(int64_t)r * ld_frame + m] = fill;
        }
    }
}

// what both entry points refuse, by name
int spec_check_cfg(const char* who, const wipa_spec_augment_cfg* cfg, int B, int frames, int n_mels) {
    WIPA_REQUIRE(cfg, "%s: null cfg", who);
    WIPA_REQUIRE(B > 0 && frames > 0 && n_mels > 0 && frames < (1 << 24) && n_mels <= MAX_BINS,
                 "%s: bad shape (B=%d frames=%d n_mels=%d; n_mels <= %d)", who, B, frames, n_mels, MAX_BINS);
    static const char* axis[2] = {"time", "feature"};
    for (int a = 0; a < 2; ++a) {
        WIPA_REQUIRE(cfg->length[a] >= 1, "%s: mask_%s_length = %d, must be >= 1", who, axis[a], cfg->length[a]);
        WIPA_REQUIRE(cfg->min_masks[a] >= 0 && cfg->min_masks[a] <= SPANS, "%s: mask_%s_min_masks = %d, outside 0..%d", who, axis[a],
                     cfg->min_masks[a], SPANS);
        WIPA_REQUIRE(cfg->rate_q16[a] <= 65536u, "%s: mask_%s rate_q16 = %u, above 65536 (a probability above 1)", who, axis[a],
                     cfg->rate_q16[a]);
        const uint64_t L_max = a == 0 ? (uint64_t)frames : (uint64_t)n_mels;
        const uint64_t most = (((uint64_t)cfg->rate_q16[a] * L_max) >> 16) + 1;
        WIPA_REQUIRE(most <= SPANS, "%s: too many spans: mask_%s settings can need %llu spans over %llu positions, at most %d are drawn", who,
                     axis[a], (unsigned long long)most, (unsigned long long)L_max, SPANS);
    }
    return WIPA_OK;
}

}  // namespace

extern "C" int wipa_spec_augment_plan(const wipa_spec_augment_cfg* cfg, const uint32_t* streams_host, const int32_t* n_frames_host, int B,
                                      int frames, int n_mels, uint64_t seed, int32_t* spans_out) {
    const int rc = spec_check_cfg("wipa_spec_augment_plan", cfg, B, frames, n_mels);
    if (rc != WIPA_OK) return rc;
    WIPA_REQUIRE(streams_host && spans_out, "wipa_spec_augment_plan: null pointer");
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
    for (int b = 0; b < B; ++b) {
        const uint32_t s_lo = streams_host[2 * b], s_hi = streams_host[2 * b + 1];
        for (int a = 0; a < 2; ++a) {
            int32_t* row = spans_out + ((int64_t)b * 2 + a) * (SPANS + 1);
            const uint32_t L = a == 0 ? spec_time_length(n_frames_host, b, frames) : (uint32_t)n_mels;
            const SpecAxis ax = spec_axis(*cfg, a, L, s_lo, s_hi, k0, k1);
            row[0] = (int32_t)ax.n;
            for (uint32_t k = 0; k < (uint32_t)SPANS; ++k)
                row[1 + k] = k < ax.n ? (int32_t)spec_start(a, k, ax.L, ax.w, s_lo, s_hi, k0, k1) : -1;
        }
    }
    return WIPA_OK;
}

extern "C" int wipa_spec_augment(float* mel, int64_t ld_clip, int64_t ld_frame, int B, int frames, int n_mels, const wipa_spec_augment_cfg* cfg,
                                 const uint32_t* streams_dev, const int32_t* n_frames_dev, uint64_t seed, wipa_stream_t stream) {
    const int rc = spec_check_cfg("wipa_spec_augment", cfg, B, frames, n_mels);
    if (rc != WIPA_OK) return rc;
    WIPA_REQUIRE(mel && streams_dev && ((uintptr_t)mel % 4) == 0, "wipa_spec_augment: null or misaligned pointer");
    WIPA_REQUIRE(ld_frame >= n_mels && ld_clip >= (int64_t)(frames - 1) * ld_frame + n_mels,
                 "wipa_spec_augment: ld_frame = %lld < n_mels = %d, or ld_clip = %lld shorter than a clip's %d frames", (long long)ld_frame, n_mels,
                 (long long)ld_clip, frames);
    WIPA_REQUIRE(B <= 65535, "wipa_spec_augment: B = %d, at most 65535 clips per call", B);
    const bool vec = ((uintptr_t)mel % 16) == 0 && ld_clip % 4 == 0 && ld_frame % 4 == 0 && n_mels % 4 == 0;
    const dim3 grid((unsigned)((frames + CHUNK - 1) / CHUNK), (unsigned)B);
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
    if (vec)
        hipLaunchKernelGGL(spec_augment_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, mel, ld_clip, ld_frame, frames, n_mels, *cfg,
                           streams_dev, n_frames_dev, k0, k1);
    else
        hipLaunchKernelGGL(spec_augment_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, mel, ld_clip, ld_frame, frames, n_mels, *cfg,
                           streams_dev, n_frames_dev, k0, k1);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

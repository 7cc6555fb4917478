// K0: audio ingest -- raw interleaved PCM -> mono f32 at 16 kHz, zero-padded / cut to 30 s.  Replaces the host side of
// load_audio -> pad_or_trim (scripts/ipa_data_loader.py:44,80, scripts/transcribe_single.py:43-44, scripts/evaluate_model.py:63).
//
//   y[m] = sum_{k=-K..K} T[p][k+K] * x[q+k],   q = (m S) div D,  p = (m S) mod D,   x = 0 outside [0, n_frames)
//
// T is the windowed-sinc polyphase table of audio.resample_table (D phases x 2K+1 taps, f32), x the channel mean of the clip's
// samples scaled as load_audio scales them.  The same rate is S = D = 1, K = 0, T = [1]: one fma by 1.0, bit-exact.
//
// MI355X mapping: ONE launch for the batch, grid (ceil(480000 / TILE), B).  A workgroup owns TILE consecutive outputs of one
// clip: its input window -- at most ceil(TILE S / D) + 2K + 1 samples -- is converted and mixed down into LDS once (positions
// outside the clip as zeros, so the tap loop has no bounds test and never sees a neighbour's bytes), then every thread
// accumulates its outputs (lane = consecutive m, coalesced stores) from LDS and its phase's table row (a 58 KB table at
// 44.1 kHz: L2 hits) in f32, taps in order.  TILE = 512 keeps the window at the steepest supported ratio (192 kHz: 12 input
// samples per output, K = 192) at 26 KB, so LDS never limits a CU below six workgroups.  Every element of [B, 480000] is
// written here, the zero tail included.  m S reaches 2.1e10 (479 999 x 44 099): the tile's first position is taken in 64 bits,
// positions inside the tile (< D + TILE S <= 16 000 + 512 x 192 000) in 32.
#include "wipa_common.h"

namespace {

constexpr int TILE = WIPA_RESAMPLE_TILE;
constexpr int THREADS = 256;
constexpr int DST_RATE = 16000;
constexpr int MIN_RATE = 4000, MAX_RATE = 192000;
constexpr int MAX_K = 16 * (MAX_RATE / DST_RATE);                   // 192
constexpr int WIN_MAX = TILE * (MAX_RATE / DST_RATE) + 2 * MAX_K + 1;  // 6529 floats
constexpr int MAX_CHANNELS = 8;

// one sample as load_audio scales it: (u - 128) / 128, / 32768, / 2147483648 (all exact but the int32 -> f32 rounding)
__device__ __forceinline__ float pcm_value(const uint8_t* p, int format) {
    if (format == WIPA_PCM_S16) return (float)*reinterpret_cast<const int16_t*>(p) * (1.0f / 32768.0f);
    if (format == WIPA_PCM_S32) return (float)*reinterpret_cast<const int32_t*>(p) * (1.0f / 2147483648.0f);
    return ((float)*p - 128.0f) * (1.0f / 128.0f);
}

__global__ __launch_bounds__(THREADS) void resample_pad_kernel(const uint8_t* __restrict__ pcm, const wipa_pcm_clip* __restrict__ descs,
                                                               const float* __restrict__ tables, float* __restrict__ out) {
    __shared__ float win[WIN_MAX];
    const wipa_pcm_clip c = descs[blockIdx.y];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * TILE;
    float* y = out + (size_t)blockIdx.y * WIPA_N_SAMPLES + m0;
    const int n_tile = min(TILE, WIPA_N_SAMPLES - m0);
    const int n_live = min(n_tile, c.n_out - m0);  // outputs of this tile that lie inside the resampled clip
    const unsigned S = (unsigned)c.S, D = (unsigned)c.D;
    const int taps = 2 * c.K + 1;
    const unsigned long long first = (unsigned long long)m0 * S;  // position of output m0 in units of 1/D input samples
    const long long q0 = (long long)(first / D);
    const unsigned p0 = (unsigned)(first % D);
    // window: input samples q0 - K .. q0 + span + K, span = q of the tile's last live output relative to q0
    const int W = n_live > 0 ? (int)((p0 + (unsigned)(n_live - 1) * S) / D) + taps : 0;
    if (n_live <= 0 || W > WIN_MAX) {  // past the clip's end (pad_or_trim's zeros); W > WIN_MAX: a descriptor the host check refuses
        for (int j = tid; j < n_tile; j += THREADS) y[j] = 0.0f;
        return;
    }
    const long long w0 = q0 - c.K;
    const int frame_bytes = c.n_channels * c.format;
    const uint8_t* src = pcm + c.byte_offset;
    const float n_ch = (float)c.n_channels;
    for (int i = tid; i < W; i += THREADS) {
        const long long idx = w0 + i;
        float v = 0.0f;
        if (idx >= 0 && idx < c.n_frames) {
            const uint8_t* f = src + idx * frame_bytes;
            v = pcm_value(f, c.format);
            if (c.n_channels > 1) {  // numpy's mean over the channel axis: f32 sum in channel order, one f32 division
                for (int ch = 1; ch < c.n_channels; ++ch) v += pcm_value(f + ch * c.format, c.format);
                v = v / n_ch;
            }
        }
        win[i] = v;
    }
    __syncthreads();
    const float* tab = tables + c.table_offset;
    for (int j = tid; j < n_tile; j += THREADS) {
        float acc = 0.0f;
        if (j < n_live) {
            const unsigned t = p0 + (unsigned)j * S;
            const unsigned dq = t / D;
            const float* w = tab + (size_t)(t - dq * D) * taps;
            const float* x = win + dq;  // x[k + K] = input sample q + k
            for (int k = 0; k < taps; ++k) acc = fmaf(w[k], x[k], acc);
        }
        y[j] = acc;
    }
}

int gcd_int(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

extern "C" int wipa_resample_pad(const void* pcm, size_t pcm_bytes, const wipa_pcm_clip* descs, const wipa_pcm_clip* descs_host,
                                 int batch, const float* tables, size_t tables_floats, float* audio_out, wipa_stream_t s) {
    WIPA_REQUIRE(pcm && descs && descs_host && tables && audio_out, "wipa_resample_pad: null pointer");
    WIPA_REQUIRE(batch >= 1 && batch <= 65535, "wipa_resample_pad: batch %d outside 1..65535", batch);
    for (int b = 0; b < batch; ++b) {
        const wipa_pcm_clip& c = descs_host[b];
        WIPA_REQUIRE(c.rate >= MIN_RATE && c.rate <= MAX_RATE, "wipa_resample_pad: clip %d: source rate %d Hz outside %d..%d Hz", b,
                     c.rate, MIN_RATE, MAX_RATE);
        const int g = gcd_int(c.rate, DST_RATE);
        WIPA_REQUIRE(c.S == c.rate / g && c.D == DST_RATE / g, "wipa_resample_pad: clip %d: S/D = %d/%d is not %d Hz -> %d Hz in lowest terms",
                     b, c.S, c.D, c.rate, DST_RATE);
        WIPA_REQUIRE(c.S == c.D ? c.K == 0 : (c.K >= 1 && c.K <= MAX_K), "wipa_resample_pad: clip %d: K = %d outside the supported range", b,
                     c.K);
        const long long window = ((long long)TILE * c.S + c.D - 1) / c.D + 2 * c.K + 1;
        WIPA_REQUIRE(window <= WIN_MAX, "wipa_resample_pad: clip %d: window of %lld samples exceeds the kernel's %d", b, window, WIN_MAX);
        WIPA_REQUIRE(c.format == WIPA_PCM_U8 || c.format == WIPA_PCM_S16 || c.format == WIPA_PCM_S32,
                     "wipa_resample_pad: clip %d: sample format %d (u8 = 1, s16 = 2, s32 = 4)", b, c.format);
        WIPA_REQUIRE(c.n_channels >= 1 && c.n_channels <= MAX_CHANNELS, "wipa_resample_pad: clip %d: %d channels outside 1..%d", b,
                     c.n_channels, MAX_CHANNELS);
        WIPA_REQUIRE(c.n_frames >= 0 && c.n_out >= 0 && c.n_out <= WIPA_N_SAMPLES, "wipa_resample_pad: clip %d: n_frames %d / n_out %d", b,
                     c.n_frames, c.n_out);
        const long long bytes = (long long)c.n_frames * c.n_channels * c.format;
        WIPA_REQUIRE(c.byte_offset >= 0 && c.byte_offset % c.format == 0 && (unsigned long long)(c.byte_offset + bytes) <= pcm_bytes,
                     "wipa_resample_pad: clip %d: bytes [%lld, %lld) misaligned or outside the %zu-byte buffer", b, (long long)c.byte_offset,
                     (long long)c.byte_offset + bytes, pcm_bytes);
        const long long table = (long long)c.D * (2 * c.K + 1);
        WIPA_REQUIRE(c.table_offset >= 0 && (unsigned long long)(c.table_offset + table) <= tables_floats,
                     "wipa_resample_pad: clip %d: table [%lld, %lld) outside the %zu-float buffer", b, (long long)c.table_offset,
                     (long long)c.table_offset + table, tables_floats);
    }
    const dim3 grid((WIPA_N_SAMPLES + TILE - 1) / TILE, batch);
    hipLaunchKernelGGL(resample_pad_kernel, grid, dim3(THREADS), 0, (hipStream_t)s, (const uint8_t*)pcm, descs, tables, audio_out);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// Model runtime: sequences the kernels of libwipa for a whole encoder pass, the cross-KV
// projection, the KV-cached greedy decode loop (replayed from a hipGraph: every per-step
// quantity -- token position, KV write offset, visible keys -- lives in device memory, so
// one captured step is valid for all steps) and the teacher-forced decoder.
//
// Replaces mlx_whisper.whisper.{AudioEncoder,TextDecoder}.__call__ and
// mlx_whisper.decoding.DecodingTask._main_loop (call sites scripts/train_whisper_ipa.py:223,232,356;
// scripts/transcribe_single.py:54-55; scripts/evaluate_model.py:197-200).
#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "wipa_common.h"

// ------------------------------------------------------------------ errors / version
static thread_local char g_err[512] = "";
void wipa_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* wipa_last_error(void) { return g_err; }
extern "C" int wipa_version(void) { return 101; }

extern "C" int wipa_stream_create_cu_limited(int n_cus, wipa_stream_t* out) {
    int dev = 0, total = 0;
    WIPA_CHECK_HIP(hipGetDevice(&dev));
    WIPA_CHECK_HIP(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, dev));
    WIPA_REQUIRE(out && n_cus >= 8 && n_cus <= total && n_cus % 8 == 0, "wipa_stream_create_cu_limited: n_cus=%d must be a multiple of 8 in [8, %d]",
                 n_cus, total);
    uint32_t mask[32] = {0};
    WIPA_REQUIRE(total <= 32 * 32, "wipa_stream_create_cu_limited: %d CUs", total);
    for (int i = 0; i < n_cus; ++i) mask[i / 32] |= 1u << (i % 32);
    hipStream_t s = nullptr;
    WIPA_CHECK_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)((total + 31) / 32), mask));
    *out = (wipa_stream_t)s;
    return WIPA_OK;
}
extern "C" int wipa_stream_create(wipa_stream_t* out) {
    WIPA_REQUIRE(out, "wipa_stream_create: null out");
    hipStream_t s = nullptr;
    WIPA_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = (wipa_stream_t)s;
    return WIPA_OK;
}
extern "C" int wipa_stream_destroy(wipa_stream_t s) {
    WIPA_REQUIRE(s, "wipa_stream_destroy: null stream");
    WIPA_CHECK_HIP(hipStreamDestroy((hipStream_t)s));
    return WIPA_OK;
}

namespace {

constexpr float QK_SCALE = 0.35355339059327379f;  // 64 ** -0.25
constexpr int ENC_KEY_TILE = 64;                    // keys per tile of wipa_flash_attn_enc_bf16 (its V^T rows are whole tiles)

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline int k_multiple(int dtype) { return dtype == WIPA_BF16 ? 64 : 32; }
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// The encoder runs on T = cfg.n_audio_ctx positions, i.e. on the first 2T mel frames (wipa_model_cfg).  Per clip: 2T + 2 padded
// frames (3002 at T = 1500) and a V^T row of ceil64(T) keys (1536 at T = 1500).
inline int enc_rows_in(int T) { return 2 * T + 2; }
inline int enc_vt_pad(int T) { return round_up(T, ENC_KEY_TILE); }
inline bool audio_ctx_ok(const wipa_model_cfg* c) { return c->n_audio_ctx >= 1 && c->n_audio_ctx <= WIPA_N_FRAMES / 2; }

#define RT_CALL(expr)                 \
    do {                              \
        int _rc = (expr);             \
        if (_rc != WIPA_OK) return _rc; \
    } while (0)

int cfg_check(const wipa_model_cfg* c) {
    WIPA_REQUIRE(c, "null cfg");
    WIPA_REQUIRE(c->dtype == WIPA_F32 || c->dtype == WIPA_BF16, "cfg.dtype %d", c->dtype);
    WIPA_REQUIRE(c->n_audio_state == c->n_audio_head * WIPA_HEAD_DIM && c->n_text_state == c->n_text_head * WIPA_HEAD_DIM,
                 "head_dim must be 64 (state %d heads %d)", c->n_audio_state, c->n_audio_head);
    WIPA_REQUIRE(audio_ctx_ok(c), "n_audio_ctx %d: must be 1..%d", c->n_audio_ctx, WIPA_N_FRAMES / 2);
    WIPA_REQUIRE(c->n_audio_state % 64 == 0 && c->n_text_state % 64 == 0, "state must be a multiple of 64");
    WIPA_REQUIRE(c->dec_w_dtype == 0 || (c->dec_w_dtype == WIPA_FP8_E4M3 && c->dtype == WIPA_BF16),
                 "cfg.dec_w_dtype %d: fp8 (e4m3) decoder weights need a bf16 model", c->dec_w_dtype);
    WIPA_REQUIRE(c->dec_cross_absorbed == 0 ||
                     (c->dec_cross_absorbed == 1 && c->dtype == WIPA_BF16 && c->dec_w_dtype == 0 && c->n_text_head <= 16 &&
                      (c->n_text_state == 384 || c->n_text_state == 512 || c->n_text_state == 768 || c->n_text_state == 1024)),
                 "cfg.dec_cross_absorbed %d: absorbed cross-attention needs a bf16 model without fp8 decoder tables, <= 16 heads, d in "
                 "{384, 512, 768, 1024}", c->dec_cross_absorbed);
    WIPA_REQUIRE(c->dec_cross_splits >= 0 && c->dec_cross_splits <= 4 && (c->dec_cross_splits == 0 || c->dec_cross_absorbed == 1),
                 "cfg.dec_cross_splits %d: 0 (default) or 1..4 frame splits, with dec_cross_absorbed = 1 only", c->dec_cross_splits);
    WIPA_REQUIRE(c->dec_n_group >= 0 && c->dec_n_group <= 64, "cfg.dec_n_group %d: 0 / 1 (one clip per row) or 2..64 candidates per clip", c->dec_n_group);
    WIPA_REQUIRE(c->enc_act_fp8 == 0 || (c->enc_act_fp8 == 1 && c->dtype == WIPA_BF16 && c->n_audio_state % 128 == 0),
                 "cfg.enc_act_fp8 %d: fp8 encoder activations need a bf16 model whose width is a multiple of 128", c->enc_act_fp8);
    return WIPA_OK;
}

// ---- stage profiler (wipa_profile_begin / wipa_profile_end): HIP events around every launch of the encoder forward and
// the cross-K/V projection, summed per kernel class.  Host-thread local; inactive (one pointer test) otherwise.
enum { PROF_GEMM = 0, PROF_ATTN = 1, PROF_NORM = 2, PROF_OTHER = 3, PROF_CLASSES = 4 };
struct Profiler {
    hipStream_t stream;
    std::vector<std::tuple<int, hipEvent_t, hipEvent_t>> spans;
};
thread_local Profiler* t_prof = nullptr;
struct ProfSpan {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int cls;
    explicit ProfSpan(int c) : cls(c) {
        if (!t_prof) return;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { e0 = e1 = nullptr; return; }
        hipEventRecord(e0, t_prof->stream);
    }
    ~ProfSpan() {
        if (!t_prof || !e0) return;
        hipEventRecord(e1, t_prof->stream);
        t_prof->spans.emplace_back(cls, e0, e1);
    }
};
#define PROF(cls, call)        \
    do {                       \
        ProfSpan _span(cls);   \
        RT_CALL(call);         \
    } while (0)

// wipa_model_cfg.f32_split of the runtime call in progress on this host thread (set by the entry points below)
thread_local int t_f32_split = 0;
struct SplitScope {
    int prev;
    explicit SplitScope(const wipa_model_cfg* c) : prev(t_f32_split) { t_f32_split = (c && c->dtype == WIPA_F32 && c->f32_split) ? 1 : 0; }
    ~SplitScope() { t_f32_split = prev; }
};

// fp8 decoder weights (wipa_model_cfg.dec_w_dtype = WIPA_FP8_E4M3): matrix pointer -> per-row scale, built from the weight
// table by the decode entry points for the duration of the call (host-thread local, enqueue-time only).
typedef std::map<const void*, const float*> W8Map;
thread_local const W8Map* t_w8 = nullptr;
struct W8Scope {
    W8Map map;
    const W8Map* prev;
    W8Scope(const wipa_model_cfg* c, const void* const* w) : prev(t_w8) {
        if (c && w && c->dec_w_dtype == WIPA_FP8_E4M3) {
            const int base = WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * c->n_text_layer;
            map[w[0]] = (const float*)w[base];
            static const int slots[WIPA_DEC_FP8_PER_LAYER] = {2, 4, 8, 12, 16, 18};
            for (int l = 0; l < c->n_text_layer; ++l)
                for (int j = 0; j < WIPA_DEC_FP8_PER_LAYER; ++j)
                    map[w[WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l + slots[j]]] = (const float*)w[base + 1 + WIPA_DEC_FP8_PER_LAYER * l + j];
            t_w8 = &map;
        }
    }
    ~W8Scope() { t_w8 = prev; }
};
inline int emb_dtype(const wipa_model_cfg* c) { return c->dec_w_dtype == WIPA_FP8_E4M3 ? WIPA_FP8_E4M3 : c->dtype; }
inline const float* emb_scale(const wipa_model_cfg* c, const void* const* w) {
    return c->dec_w_dtype == WIPA_FP8_E4M3 ? (const float*)w[WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * c->n_text_layer] : nullptr;
}

int gemm(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K, int in_dt,
         int out_dt, const float* bias, int act, const void* residual, wipa_stream_t s, wipa_gemm_desc* extra = nullptr) {
    wipa_gemm_desc g;
    if (extra) g = *extra; else memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.in_dtype = in_dt; g.out_dtype = out_dt;
    g.bias = bias; g.act = act; g.residual = residual;
    g.f32_split = t_f32_split;
    if (t_w8) {  // fp8 decoder weights: matrices are recognised by their table pointer
        auto it = t_w8->find(W);
        if (it != t_w8->end()) {
            g.w_dtype = WIPA_FP8_E4M3;
            g.w_scale = it->second;
        }
    }
    return wipa_gemm(&g, s);
}

// fp8 x fp8 GEMM (cfg.enc_act_fp8): A codes [M, K] + a_scale[M], W codes [N, K] + w_scale[N]
int gemm_f8(const void* A, int64_t lda, const float* a_scale, const void* W, int64_t ldw, const float* w_scale, void* C, int64_t ldc,
            int M, int N, int K, int out_dt, const float* bias, int act, const void* residual, wipa_stream_t s,
            wipa_gemm_desc* extra = nullptr) {
    wipa_gemm_desc g;
    if (extra) g = *extra; else memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.in_dtype = WIPA_FP8_E4M3; g.out_dtype = out_dt;
    g.bias = bias; g.act = act; g.residual = residual;
    g.a_scale = a_scale; g.w_scale = w_scale;
    return wipa_gemm(&g, s);
}

// ------------------------------------------------------------------ encoder
struct EncWs {
    size_t c1, x, ln, qk, v, ao, h, total;
};
EncWs enc_ws(const wipa_model_cfg* c, int B) {
    const size_t e = wipa_dtype_size(c->dtype), d = c->n_audio_state, M = (size_t)B * c->n_audio_ctx;
    const size_t ROWS_IN = enc_rows_in(c->n_audio_ctx), T_ENC_PAD = enc_vt_pad(c->n_audio_ctx);
    EncWs w;
    size_t o = 0;
    w.c1 = o; o += align256(((size_t)B * ROWS_IN + 4) * d * e);
    w.x = o;  o += align256(M * d * 4);
    w.ln = o; o += align256(M * d * e);
    w.qk = o; o += align256(M * 2 * d * e);
    w.v = o;  o += align256(c->dtype == WIPA_BF16 ? (size_t)B * d * T_ENC_PAD * e + 256 : M * d * e);
    w.ao = o; o += align256(M * d * e);
    w.h = o;  o += align256(M * 4 * d * e);
    w.total = o;
    return w;
}

// V [B*T][d] (row-major, bf16) -> V^T [B][d][ldvt] for wipa_flash_attn_enc_bf16; columns >= T are left as the memset wrote them.
// grid (d / 64, ceil(T / 64), B); the tile goes through LDS so that both the reads and the writes run along rows.
__global__ __launch_bounds__(256) void vt_from_rows_kernel(const __bf16* __restrict__ v, __bf16* __restrict__ vt, int T, int d, int64_t ldvt) {
    __shared__ __bf16 tile[64][66];
    const int c0 = blockIdx.x * 64, t0 = blockIdx.y * 64, b = blockIdx.z;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int t = t0 + i;
        tile[i][tx] = t < T ? v[((int64_t)b * T + t) * d + c0 + tx] : (__bf16)0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int t = t0 + tx;
        if (t < T) vt[((int64_t)b * d + c0 + i) * ldvt + t] = tile[tx][i];
    }
}

}  // namespace

extern "C" size_t wipa_encoder_workspace_bytes(const wipa_model_cfg* cfg, int B) {
    if (!cfg || B <= 0 || !audio_ctx_ok(cfg)) return 0;
    return enc_ws(cfg, B).total;
}

extern "C" int wipa_encoder_forward(const wipa_model_cfg* cfg, const void* const* w, const void* mel_padded, void* out,
                                    void* workspace, size_t workspace_bytes, int B, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(w && mel_padded && out && workspace && B > 0, "wipa_encoder_forward: null pointer / bad batch");
    const EncWs L = enc_ws(cfg, B);
    WIPA_REQUIRE(workspace_bytes >= L.total, "wipa_encoder_forward: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    const int dt = cfg->dtype;
    const size_t e = wipa_dtype_size(dt);
    const int d = cfg->n_audio_state, H = cfg->n_audio_head, T = cfg->n_audio_ctx, M = B * T;
    const int ROWS_IN = enc_rows_in(T), T_ENC_PAD = enc_vt_pad(T);
    char* ws = (char*)workspace;
    void* c1 = ws + L.c1;
    float* x = (float*)(ws + L.x);
    void* ln = ws + L.ln;
    void* qk = ws + L.qk;
    void* vb = ws + L.v;
    void* ao = ws + L.ao;
    void* hb = ws + L.h;
    const int K1 = round_up(3 * cfg->n_mels, k_multiple(dt));

    // conv1 (k3,p1) + GELU as a GEMM with overlapping rows; output row g lands at c1 row g+1,
    // dead rows (t >= 2T; 3000 at T = 1500) write the zero halos of conv2.
    WIPA_CHECK_HIP(hipMemsetAsync(c1, 0, (size_t)d * e, s));
    {
        wipa_gemm_desc g;
        memset(&g, 0, sizeof(g));
        g.rg_in = ROWS_IN; g.rg_valid = 2 * T; g.rg_stride = (int64_t)ROWS_IN * d; g.zero_invalid_rows = 1;
        g.c_offset = d;
        PROF(PROF_GEMM, gemm(mel_padded, cfg->n_mels, w[0], K1, c1, d, B * ROWS_IN, d, K1, dt, dt, (const float*)w[1], 1, nullptr,
                     stream, &g));
    }
    // conv2 (k3,s2,p1) + GELU + positional embedding -> residual stream x (f32)
    {
        wipa_gemm_desc g;
        memset(&g, 0, sizeof(g));
        g.rg_in = T + 1; g.rg_valid = T; g.rg_stride = (int64_t)T * d;
        g.pos = (const float*)w[4]; g.ldpos = d;
        PROF(PROF_GEMM, gemm(c1, 2 * d, w[2], 3 * d, x, d, B * (T + 1), d, 3 * d, dt, WIPA_F32, (const float*)w[3], 1, nullptr,
                     stream, &g));
    }
    if (dt == WIPA_BF16) WIPA_CHECK_HIP(hipMemsetAsync(vb, 0, (size_t)B * d * T_ENC_PAD * e, s));
    // fp8 activations (cfg.enc_act_fp8, BASELINE.json configs[4]): the LayerNorm outputs and the GELU output are quantised per
    // row to e4m3 and q|k, value, mlp1, mlp2 multiply fp8 x fp8 on the block-scaled fp8 MFMA.  Buffers are the bf16 path's:
    // `ln` holds the codes [M, d] followed by their M row scales, the (idle) q|k buffer takes the codes of the GELU output
    // [M, 4d] and the (idle) attention-output buffer their row scales.
    const bool f8 = cfg->enc_act_fp8 != 0;
    float* ln_scale = (float*)((char*)ln + (size_t)M * d);  // M*d bytes of codes, then M floats (M*d*2 bytes available)
    const void* const* w8 = w + WIPA_ENC_GLOBAL + WIPA_ENC_PER_LAYER * cfg->n_audio_layer;
    for (int l = 0; l < cfg->n_audio_layer; ++l) {
        const void* const* lw = w + WIPA_ENC_GLOBAL + WIPA_ENC_PER_LAYER * l;
        const void* const* l8 = w8 + WIPA_ENC_FP8_PER_LAYER * l;
        if (f8) PROF(PROF_NORM, wipa_layernorm_fp8(x, d, ln, d, ln_scale, (const float*)lw[0], (const float*)lw[1], M, d, 1e-5f, stream));
        else PROF(PROF_NORM, wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)lw[0], (const float*)lw[1], M, d, 1e-5f, stream));
        {
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.col_scale_n = 2 * d; g.col_scale = QK_SCALE;
            if (f8) PROF(PROF_GEMM, gemm_f8(ln, d, ln_scale, l8[0], d, (const float*)l8[1], qk, 2 * d, M, 2 * d, d, dt, (const float*)lw[3], 0,
                                            nullptr, stream, &g));
            else PROF(PROF_GEMM, gemm(ln, d, lw[2], d, qk, 2 * d, M, 2 * d, d, dt, dt, (const float*)lw[3], 0, nullptr, stream, &g));
        }
        if (dt == WIPA_BF16) {
            // V^T per clip: swap the operand roles so the GEMM writes [d][t] directly
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.bias_along_m = 1;
            if (T % 4 == 0) {  // one launch: the columns (tokens) are remapped per clip
                g.cg_in = T; g.cg_stride = (int64_t)d * T_ENC_PAD;
                if (f8) PROF(PROF_GEMM, gemm_f8(l8[2], d, (const float*)l8[3], ln, d, ln_scale, vb, T_ENC_PAD, d, M, d, dt, (const float*)lw[5], 0,
                                                nullptr, stream, &g));
                else PROF(PROF_GEMM, gemm(lw[4], d, ln, d, vb, T_ENC_PAD, d, M, d, dt, dt, (const float*)lw[5], 0, nullptr, stream, &g));
            } else {
                // the epilogue remaps columns in groups of 4 (wipa_gemm_desc.cg_in): a clip of T % 4 != 0 tokens (short audio
                // context only) would share a group with its neighbour.  V is projected row-major into the (idle) mlp buffer
                // and transposed per clip by one launch.
                if (f8) PROF(PROF_GEMM, gemm_f8(ln, d, ln_scale, l8[2], d, (const float*)l8[3], hb, d, M, d, d, dt, (const float*)lw[5], 0, nullptr,
                                                stream));
                else PROF(PROF_GEMM, gemm(ln, d, lw[4], d, hb, d, M, d, d, dt, dt, (const float*)lw[5], 0, nullptr, stream));
                {
                    ProfSpan span(PROF_OTHER);
                    hipLaunchKernelGGL(vt_from_rows_kernel, dim3(d / 64, (T + 63) / 64, B), dim3(256), 0, s, (const __bf16*)hb, (__bf16*)vb, T, d,
                                       (int64_t)T_ENC_PAD);
                    WIPA_LAUNCH_CHECK();
                }
            }
            PROF(PROF_ATTN, wipa_flash_attn_enc_bf16(qk, 2 * d, vb, T_ENC_PAD, ao, d, B, H, T, stream));
        } else {
            PROF(PROF_GEMM, gemm(ln, d, lw[4], d, vb, d, M, d, d, dt, dt, (const float*)lw[5], 0, nullptr, stream));
            PROF(PROF_ATTN, wipa_flash_attn_enc_f32((const float*)qk, 2 * d, (const float*)qk + d, 2 * d, (const float*)vb, d, (float*)ao, d,
                                            B, H, T, t_f32_split, stream));
        }
        PROF(PROF_GEMM, gemm(ao, d, lw[6], d, x, d, M, d, d, dt, WIPA_F32, (const float*)lw[7], 0, x, stream));
        if (f8) {
            PROF(PROF_NORM, wipa_layernorm_fp8(x, d, ln, d, ln_scale, (const float*)lw[8], (const float*)lw[9], M, d, 1e-5f, stream));
            PROF(PROF_GEMM, gemm_f8(ln, d, ln_scale, l8[4], d, (const float*)l8[5], hb, 4 * d, M, 4 * d, d, dt, (const float*)lw[11], 1, nullptr,
                                    stream));
            void* h8 = qk;                 // [M, 4d] codes in the q|k buffer (M * 2d * 2 bytes)
            float* h_scale = (float*)ao;   // M floats in the attention-output buffer
            PROF(PROF_NORM, wipa_rowquant_fp8(hb, dt, 4 * d, h8, 4 * d, h_scale, M, 4 * d, stream));
            PROF(PROF_GEMM, gemm_f8(h8, 4 * d, h_scale, l8[6], 4 * d, (const float*)l8[7], x, d, M, d, 4 * d, WIPA_F32, (const float*)lw[13], 0,
                                    x, stream));
        } else {
            PROF(PROF_NORM, wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)lw[8], (const float*)lw[9], M, d, 1e-5f, stream));
            PROF(PROF_GEMM, gemm(ln, d, lw[10], d, hb, 4 * d, M, 4 * d, d, dt, dt, (const float*)lw[11], 1, nullptr, stream));
            PROF(PROF_GEMM, gemm(hb, 4 * d, lw[12], 4 * d, x, d, M, d, 4 * d, dt, WIPA_F32, (const float*)lw[13], 0, x, stream));
        }
    }
    PROF(PROF_NORM, wipa_layernorm(x, WIPA_F32, d, out, dt, d, (const float*)w[5], (const float*)w[6], M, d, 1e-5f, stream));
    return WIPA_OK;
}

// ------------------------------------------------------------------ decoder state
namespace {

constexpr int MAX_SLABS = 4;
// Candidate groups (cfg.dec_n_group = G > 1; best-of-N sampling): the B rows of a decode call are B / G clips x G candidates, and what
// is per CLIP -- the cross_kv region and every read of it -- is sized and indexed by clip: row b reads clip b / G.
inline int group_of(const wipa_model_cfg* c) { return c->dec_n_group > 1 ? c->dec_n_group : 1; }
inline int clips_of(const wipa_model_cfg* c, int B) { return B / group_of(c); }
struct DecScratch {
    size_t x, x2, ln, q, ao, h, slabs, posd, absorbed, greedy_part, total;
};
// split-K factor of a decode-step residual GEMM: keep >= 3 fragment steps per wave (4 waves)
inline int k_slices_for(int K, int dtype) {
    const int ksteps = K * (int)wipa_dtype_size(dtype) / 64;
    int s = ksteps / 12;
    return s < 1 ? 1 : (s > MAX_SLABS ? MAX_SLABS : s);
}
int decode_mode(const wipa_model_cfg* cfg, int B);  // 0 unfused, 1 fused blocks, 2 unfused + fused cross block (defined below)
constexpr int MAX_PROMPT = 4;  // prompt positions handled by one prefill pass (wipa_decoder_begin takes 1..4 tokens)
DecScratch dec_scratch(const wipa_model_cfg* c, int B) {
    const size_t e = wipa_dtype_size(c->dtype), d = c->n_text_state;
    const size_t R = (size_t)B * MAX_PROMPT;  // rows: one per clip in a decode step, up to four per clip in the prefill
    DecScratch s;
    size_t o = 0;
    s.x = o;    o += align256(R * d * 4);
    s.x2 = o;   o += align256((size_t)B * d * 4);  // fused step: the residual stream ping-pongs between x and x2
    s.ln = o;   o += align256(R * d * e);
    s.q = o;    o += align256(R * d * e);
    s.ao = o;   o += align256(R * d * e);
    s.h = o;    o += align256(R * 4 * d * e);
    // split-K slabs of the unfused residual GEMMs, or one slab per head from the fused self block
    s.slabs = o; o += align256(std::max((size_t)MAX_SLABS * R, (size_t)c->n_text_head * B) * d * 4);
    s.posd = o; o += 256;
    s.absorbed = o;  // Qp + split partials of the absorbed cross-attention (cfg.dec_cross_absorbed)
    if (c->dec_cross_absorbed) o += align256(wipa_cross_absorbed_scratch_bytes(B, (int)d, c->n_audio_ctx));
    s.greedy_part = o;  // arg-max / log-sum-exp partials of the logits projection (wipa_logits_greedy)
    if (wipa_logits_greedy_supported(B, c->n_vocab, (int)d, c->dtype)) o += align256(wipa_logits_greedy_partials_bytes(B));
    s.total = o;
    return s;
}

wipa_dec_layout dec_layout(const wipa_model_cfg* c, int B) {
    const size_t e = wipa_dtype_size(c->dtype);
    const size_t d = c->n_text_state, H = c->n_text_head;
    wipa_dec_layout L;
    size_t o = 0;
    L.ld_tok = c->n_text_ctx + 8;
    L.tokens = o; o += align256((size_t)B * L.ld_tok * 4);
    L.pos = o; o += 256;
    L.not_done = o; o += 256;
    L.sum_logprobs = o; o += align256((size_t)B * 4);
    L.ld_logits = round_up(c->n_vocab, 8);
    L.logits = o; o += align256((size_t)B * L.ld_logits * 4);
    // cached cross K / V of every layer -- or, with absorbed projections, ONE copy of the encoder output [B, n_audio_ctx, d]
    const size_t Bc = clips_of(c, B);  // the audio is held once per clip
    L.cross_kv = o; o += align256(c->dec_cross_absorbed ? Bc * c->n_audio_ctx * d * e
                                                        : (size_t)c->n_text_layer * Bc * 2 * H * c->n_audio_ctx * 64 * e);
    L.self_kv = o; o += align256((size_t)c->n_text_layer * 3 * B * c->n_text_ctx * d * e);
    L.scratch = o; o += dec_scratch(c, B).total;
    L.total_bytes = o;
    return L;
}

__global__ void advance_pos_kernel(int32_t* pos, int64_t* posd, int d) {
    const int p = *pos + 1;
    *pos = p;
    *posd = (int64_t)p * d;
}

__global__ void fill_tokens_kernel(int32_t* tokens, int64_t ld_tok, int B, int n_init, int i0, int i1, int i2, int i3) {
    // every row gets the same prompt of up to four tokens; per-row prompts of any length come through wipa_decoder_begin_ragged
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int first4[4] = {i0, i1, i2, i3};
    for (int t = 0; t < n_init; ++t) tokens[(int64_t)b * ld_tok + t] = first4[t & 3];
}

// one decoder step (all layers + logits + greedy update + position advance)
// WIPA_ABS_FUSED_PROLOGUE=0 keeps the separate LayerNorm / query GEMM / absorb launches of the absorbed cross block (A/B runs)
bool absorbed_block_fused() {
    const char* e = getenv("WIPA_ABS_FUSED_PROLOGUE");
    return !(e && atoi(e) == 0);
}

// WIPA_ABS_MERGE_OUT=1 folds the cross-attention out projection of the absorbed block into its merge launch (one slab per head,
// wipa_decode_cross_absorbed_block_out).  Built, parity-tested and NOT the default: measured r04 (whisper-small, 64 clips, MI355X)
// the fused launch takes 17.0 us where merge 10.5 + out-projection GEMM 4.9 take 15.4 -- its 192 workgroups pull the head's
// Wo slice (98 KB) on top of the Wv slice through the same per-CU load path and write 12 slabs instead of 2 -- decode step
// 1.338 vs 1.306 ms, pipelined pass 78.2 vs 75.0 ms.  A launch in a replayed graph costs ~1.6 us; 98 KB more per workgroup costs 2.
bool absorbed_merge_out() {
    const char* e = getenv("WIPA_ABS_MERGE_OUT");
    return e && atoi(e) == 1;
}
// WIPA_DECODE_TAIL=0 keeps the separate greedy_step / advance_pos / embed / first-LayerNorm launches (A/B runs, part of the graph
// key); default: ONE launch, wipa_greedy_step_embed, ends a step and prepares the next one's input rows
bool tail_fused() {
    const char* e = getenv("WIPA_DECODE_TAIL");
    return !(e && atoi(e) == 0);
}
// What one decode call asks of its steps: the caller's wipa_decode_call (include/wipa.h documents every field: which tail, which
// attention instantiation, what `starts` holds) plus `lean`.  step_ctx() builds it, and it goes down by const reference to everything
// that enqueues a step or keys a graph: nothing about a call is ambient, and nothing below reads the public struct.
struct StepCtx {
    const wipa_decode_rules* rules;
    const void* sample;
    const int32_t* starts;
    int n_init, eot;
    const float *mask_first, *mask_always;
    // a step whose logits nobody reads (every step of a run call but the last) does not write them at all
    bool lean;
    bool continuous;
    float* no_speech;
    int no_speech_token;
    const void* sample_rows;
    bool prompted;
    void* beam;
    size_t beam_bytes;
    int beam_max_candidates;
    const wipa_adapter_bank* bank;
};
StepCtx step_ctx(const wipa_decode_call& k) {
    return StepCtx{k.rules, k.sample, k.starts_dev, k.n_init, k.eot, k.mask_first, k.mask_always, false, k.continuous != 0, k.no_speech_dev,
                   k.no_speech_token, k.sample_rows, k.prompted != 0, k.beam, k.beam_bytes, k.beam ? k.beam_max_candidates : 0, k.bank};
}
// The logits projection with the greedy partials in its epilogue + a tail that merges them (round 4; WIPA_LOGITS_FUSED=0 restores
// the plain GEMM + the row-scanning tail): bf16 models without fp8 decoder tables, <= 64 rows, tail-fused steps.  Measured on
// whisper-small, 64 clips: the logits' 64-byte stores were 8 of the GEMM's 32 us, the tail's read-back of the 13 MB another ~10.
bool logits_fused(const wipa_model_cfg* cfg, int B, const StepCtx& c) {
    const char* e = getenv("WIPA_LOGITS_FUSED");  // read per call like the other step variants: part of the graph key
    const bool on = !(e && atoi(e) == 0);
    return on && !c.rules && !c.sample && !c.starts && !c.beam && tail_fused() && cfg->dec_w_dtype == 0 && wipa_logits_greedy_supported(B, cfg->n_vocab, cfg->n_text_state, cfg->dtype);
}
int32_t* done_counter_of(char* st, const wipa_dec_layout& L) { return (int32_t*)(st + L.pos + 64); }  // zeroed with pos by wipa_decoder_begin

// x = embedding of the token at the current position, ln = first block's LayerNorm of it: what a tail-fused step expects to find
int enqueue_step_head(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, const StepCtx& ctx,
                      wipa_stream_t stream) {
    const DecScratch S = dec_scratch(cfg, B);
    char* sc = st + L.scratch;
    const void* const* lw0 = w + WIPA_DEC_GLOBAL;
    if (ctx.starts)
        return wipa_embed_layernorm_ragged((const int32_t*)(st + L.tokens), L.ld_tok, B, (const int32_t*)(st + L.pos), ctx.starts, w[0], emb_dtype(cfg),
                                           emb_scale(cfg, w), (const float*)w[1], cfg->n_text_ctx, (float*)(sc + S.x), (const float*)lw0[0],
                                           (const float*)lw0[1], sc + S.ln, cfg->dtype, cfg->n_text_state, 1e-5f, stream);
    return wipa_embed_layernorm((const int32_t*)(st + L.tokens), L.ld_tok, B, (const int32_t*)(st + L.pos), w[0], emb_dtype(cfg), emb_scale(cfg, w),
                                (const float*)w[1], cfg->n_text_ctx, (float*)(sc + S.x), (const float*)lw0[0], (const float*)lw0[1], sc + S.ln,
                                cfg->dtype, cfg->n_text_state, 1e-5f, stream);
}

// The f32 residual stream of a decode step and of the four-row prompt pass.  Residual GEMMs (out, cross.out, mlp2) are split along K
// over workgroups; each slice writes a partial slab and the NEXT LayerNorm kernel adds the slabs to x in a fixed order first
// (deterministic split-K, no atomics).  `pend` = slabs waiting to be folded into x.
struct SlabStream {
    float* x;
    float* slabs;
    void* ln;
    int rows, d, dt;
    int split_rows_max;  // split-K lives in the weight-streaming kernel: up to this many rows
    int stream_weights;
    wipa_stream_t stream;
    int64_t slab_stride = (int64_t)rows * d;
    int pend = 0;
    int ln_step(const void* lw_w, const void* lw_b) {
        const int rc = wipa_add_slabs_layernorm(x, d, slabs, pend, slab_stride, ln, dt, d, (const float*)lw_w, (const float*)lw_b,
                                                rows, d, 1e-5f, stream);
        pend = 0;
        return rc;
    }
    int residual_gemm(const void* A, int K, const void* W, const void* bias) {
        wipa_gemm_desc g;
        memset(&g, 0, sizeof(g));
        g.stream_weights = stream_weights;
        g.k_slices = rows <= split_rows_max ? k_slices_for(K, dt) : 1;
        g.slab_stride = slab_stride;
        pend = g.k_slices;
        return gemm(A, K, W, K, slabs, d, rows, d, K, dt, WIPA_F32, (const float*)bias, 0, nullptr, stream, &g);
    }
};

// Sites of a decoder block in a wipa_adapter_bank (include/wipa.h)
enum { SITE_Q = 0, SITE_K, SITE_V, SITE_O, SITE_CQ, SITE_CK, SITE_CV, SITE_CO, SITE_MLP1, SITE_MLP2 };
inline bool bank_on(const wipa_adapter_bank* bk, int site) { return bk && (bk->site_mask >> site & 1u); }
// One wipa_lora_bank_apply behind the GEMM of `n_seg` consecutive sites from `site0` that share the input x [M, K] (x_dt): the adapters'
// terms land in y (y_dt) where the GEMM wrote -- `addr` is that GEMM's descriptor (row / column groups and the device offset), NULL for
// plain rows of ld elements.  scales: the sites' column scales.  Nothing is enqueued when none of the sites is targeted and act is 0.
int bank_apply(const wipa_adapter_bank* bk, int layer, int site0, int n_seg, const float* scales, const void* x, int64_t ldx, int x_dt, void* y,
               int y_dt, int64_t ld, const wipa_gemm_desc* addr, int M, int K, int N, int rows_per_id, int ids_stride, const int32_t* ids, int act,
               wipa_stream_t stream) {
    wipa_lora_bank_desc b;
    memset(&b, 0, sizeof(b));
    bool any = false;
    for (int s = 0; s < n_seg; ++s) {
        b.col_scale[s] = scales[s];
        if (!bank_on(bk, site0 + s)) continue;
        b.A[s] = bk->A[(size_t)layer * WIPA_BANK_SITES + site0 + s];
        b.B[s] = bk->B[(size_t)layer * WIPA_BANK_SITES + site0 + s];
        WIPA_REQUIRE(b.A[s] && b.B[s], "call.bank: layer %d site %d is in site_mask but has no A / B", layer, site0 + s);
        any = true;
    }
    if (!any && !act) return WIPA_OK;
    b.x = x; b.y = y; b.out = y; b.gain = bk->gain; b.ids = ids; b.ldx = ldx; b.ld = ld;
    b.M = M; b.K = K; b.N = N; b.r = bk->rank; b.n = bk->n; b.rows_per_id = rows_per_id; b.n_seg = n_seg; b.ids_stride = ids_stride;
    b.x_dtype = x_dt; b.y_dtype = y_dt; b.act = act;
    if (addr) {
        b.rg_in = addr->rg_in; b.rg_stride = addr->rg_stride; b.cg_in = addr->cg_in; b.cg_stride = addr->cg_stride;
        b.c_offset = addr->c_offset; b.c_offset_dev = addr->c_offset_dev;
    }
    return wipa_lora_bank_apply(&b, stream);
}
const float SCALES_QKV[3] = {QK_SCALE, QK_SCALE, 1.f};
const float SCALE_ONE[1] = {1.f};

int enqueue_step(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, const StepCtx& ctx,
                 wipa_stream_t stream) {
    const int dt = cfg->dtype;
    const bool tail = tail_fused();
    const size_t e = wipa_dtype_size(dt);
    const int d = cfg->n_text_state, H = cfg->n_text_head, nctx = cfg->n_text_ctx, Ta = cfg->n_audio_ctx;
    const DecScratch S = dec_scratch(cfg, B);
    char* sc = st + L.scratch;
    float* x_other = (float*)(sc + S.x2);
    const bool absorbed = cfg->dec_cross_absorbed != 0;
    const wipa_adapter_bank* bk = ctx.bank;
    // with a bank the cross block takes its separate launches: the fused prologues compute the cross query inside a launch
    const bool cross_fused = !bk && !absorbed && decode_mode(cfg, B) == 2;
    const int G = group_of(cfg), Bc = clips_of(cfg, B);
    void* ln = sc + S.ln;
    void* q = sc + S.q;
    void* ao = sc + S.ao;
    void* hb = sc + S.h;
    int64_t* posd = (int64_t*)(sc + S.posd);
    int32_t* tokens = (int32_t*)(st + L.tokens);
    int32_t* pos = (int32_t*)(st + L.pos);
    float* slabs = (float*)(sc + S.slabs);
    SlabStream r{(float*)(sc + S.x), slabs, ln, B, d, dt, 256, 0, stream};  // r.x moves to x_other and back with every fused cross block
    const int64_t slab_stride = r.slab_stride;
    // tail-fused steps find x (this position's embedding) and ln (the first block's LayerNorm of it) in place: written by the
    // previous step's last launch, or by enqueue_step_head before the first step of a wipa_decoder_run call
    float* const x_first = r.x;
    if (!tail) RT_CALL(wipa_embed_tokens(tokens, L.ld_tok, B, 1, 0, pos, w[0], emb_dtype(cfg), emb_scale(cfg, w), (const float*)w[1], r.x, d, stream));
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        const void* const* lw = w + WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l;
        char* skv = st + L.self_kv + (size_t)l * 3 * B * nctx * d * e;  // [3][B][nctx][d]
        char* ckv = st + L.cross_kv + (size_t)l * Bc * 2 * H * Ta * 64 * e;
        bool cross_out_done = false;
        if (!(tail && l == 0)) RT_CALL(r.ln_step(lw[0], lw[1]));
        {
            // q|k|v of this position -> slot[n / d][b][pos][n % d]
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.col_scale_n = 2 * d; g.col_scale = QK_SCALE;
            g.rg_in = 1; g.rg_valid = 1; g.rg_stride = (int64_t)nctx * d;
            g.cg_in = d; g.cg_stride = (int64_t)B * nctx * d;
            g.c_offset_dev = posd;
            RT_CALL(gemm(ln, d, lw[2], d, skv, d, B, 3 * d, d, dt, dt, (const float*)lw[3], 0, nullptr, stream, &g));
            if (bk) RT_CALL(bank_apply(bk, l, SITE_Q, 3, SCALES_QKV, ln, d, dt, skv, dt, d, &g, B, d, 3 * d, 1, 1, bk->ids_dev, 0, stream));
        }
        {
            wipa_attn_desc a;
            memset(&a, 0, sizeof(a));
            const size_t slot = (size_t)B * nctx * d * e;
            a.q = skv; a.k = skv + slot; a.v = skv + 2 * slot; a.out = ao;
            a.q_row_dev = pos; a.tk_dev = pos;
            a.q_bs = (int64_t)nctx * d; a.q_rs = d; a.q_hs = 64;
            a.k_bs = a.q_bs; a.k_rs = d; a.k_hs = 64;
            a.v_bs = a.q_bs; a.v_rs = d; a.v_hs = 64;
            a.o_bs = d; a.o_rs = d; a.o_hs = 64;
            a.B = B; a.H = H; a.Tq = 1; a.Tk = 1; a.causal = 0; a.dtype = dt;
            if (ctx.starts) RT_CALL(wipa_decode_attn_ragged(&a, ctx.starts, stream));  // row b sees keys starts[b] .. pos
            else if (ctx.beam) RT_CALL(wipa_decode_attn_beam(&a, (const uint8_t*)ctx.beam, L.ld_tok, G, stream));  // the table heads the buffer
            else RT_CALL(wipa_decode_attn(&a, stream));
        }
        RT_CALL(r.residual_gemm(ao, d, lw[4], lw[5]));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_O, 1, SCALE_ONE, ao, d, dt, slabs, WIPA_F32, d, nullptr, B, d, d, 1, 1, bk->ids_dev, 0, stream));
        if (cross_fused) {
            // one launch for [slab sum + residual + cross_attn_ln + cross query + cross-attention]; the residual row moves to
            // the other buffer (H workgroups read the row that one of them writes)
            wipa_cross_block_desc c;
            memset(&c, 0, sizeof(c));
            c.x_in = r.x; c.x_out = x_other; c.slabs = slabs; c.bias_o = nullptr;  // slab 0 carries the out-projection bias
            c.ln_w = (const float*)lw[6]; c.ln_b = (const float*)lw[7]; c.wq = lw[8]; c.bq = (const float*)lw[9];
            c.kv = ckv; c.out = ao; c.slab_stride = slab_stride;
            c.n_slabs = r.pend; c.B = B; c.d = d; c.H = H; c.Tk = Ta; c.dtype = dt; c.eps = 1e-5f; c.qk_scale = QK_SCALE;
            c.n_group = cfg->dec_n_group;
            RT_CALL(wipa_decode_cross_block(&c, stream));
            r.pend = 0;
            std::swap(r.x, x_other);
        } else if (!bk && absorbed && absorbed_block_fused() && r.pend <= 4) {
            // three launches: [slab sum + residual + cross_attn_ln + cross query + absorbed query] -> stream over the encoder output
            // -> [merge + value projection]; the residual row moves to the other buffer like in the fused cross block
            const void* wkT = w[WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * cfg->n_text_layer + WIPA_DEC_ABSORBED_PER_LAYER * l];
            wipa_cross_block_desc c;
            memset(&c, 0, sizeof(c));
            c.x_in = r.x; c.x_out = x_other; c.slabs = slabs; c.bias_o = nullptr;
            c.ln_w = (const float*)lw[6]; c.ln_b = (const float*)lw[7]; c.wq = lw[8]; c.bq = (const float*)lw[9];
            c.kv = st + L.cross_kv; c.out = ao; c.slab_stride = slab_stride;
            c.n_slabs = r.pend; c.B = B; c.d = d; c.H = H; c.Tk = Ta; c.dtype = dt; c.eps = 1e-5f; c.qk_scale = QK_SCALE;
            c.cross_splits = cfg->dec_cross_splits;
            c.n_group = cfg->dec_n_group;
            if (absorbed_merge_out()) {
                // ... and the cross-attention OUT projection rides in the third launch: one slab per head, summed by the mlp LayerNorm
                RT_CALL(wipa_decode_cross_absorbed_block_out(&c, wkT, (const char*)lw[10] + (size_t)d * d * e, (const float*)lw[11] + d,
                                                             lw[12], (const float*)lw[13], slabs, slab_stride, sc + S.absorbed,
                                                             S.greedy_part - S.absorbed, stream));
                r.pend = H;
                std::swap(r.x, x_other);
                cross_out_done = true;
            } else {
                RT_CALL(wipa_decode_cross_absorbed_block(&c, wkT, (const char*)lw[10] + (size_t)d * d * e, (const float*)lw[11] + d,
                                                         sc + S.absorbed, S.greedy_part - S.absorbed, stream));
                r.pend = 0;
                std::swap(r.x, x_other);
            }
        } else {
            RT_CALL(r.ln_step(lw[6], lw[7]));
            {
                wipa_gemm_desc g;
                memset(&g, 0, sizeof(g));
                g.col_scale_n = d; g.col_scale = QK_SCALE;
                RT_CALL(gemm(ln, d, lw[8], d, q, d, B, d, d, dt, dt, (const float*)lw[9], 0, nullptr, stream, &g));
                if (bk) RT_CALL(bank_apply(bk, l, SITE_CQ, 1, SCALES_QKV, ln, d, dt, q, dt, d, nullptr, B, d, d, 1, 1, bk->ids_dev, 0, stream));
            }
            if (absorbed) {
                // scores and values from ONE pass over the encoder output: Wk absorbed into the query, Wv into the output
                const void* wkT = w[WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * cfg->n_text_layer + WIPA_DEC_ABSORBED_PER_LAYER * l];
                // (G = 1 is wipa_cross_absorbed_attention)
                RT_CALL(wipa_cross_absorbed_attention_grouped(q, d, wkT, st + L.cross_kv, (const char*)lw[10] + (size_t)d * d * e,
                                                              (const float*)lw[11] + d, ao, d, sc + S.absorbed, S.greedy_part - S.absorbed, B, H,
                                                              d, Ta, QK_SCALE, cfg->dec_cross_splits, G, stream));
            } else if (G > 1) {
                RT_CALL(wipa_decode_cross_attn_grouped(q, ckv, ao, B, H, Ta, 1, G, dt, stream));
            } else {
                RT_CALL(wipa_decode_cross_attn(q, ckv, ao, B, H, Ta, dt, stream));
            }
        }
        if (!cross_out_done) RT_CALL(r.residual_gemm(ao, d, lw[12], lw[13]));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_CO, 1, SCALE_ONE, ao, d, dt, slabs, WIPA_F32, d, nullptr, B, d, d, 1, 1, bk->ids_dev, 0, stream));
        RT_CALL(r.ln_step(lw[14], lw[15]));
        // mlp1 with adapters: the GEMM without its GELU, which the apply call performs behind the adapters' term
        const bool mlp1_bank = bank_on(bk, SITE_MLP1);
        RT_CALL(gemm(ln, d, lw[16], d, hb, 4 * d, B, 4 * d, d, dt, dt, (const float*)lw[17], mlp1_bank ? 0 : 1, nullptr, stream));
        if (mlp1_bank) RT_CALL(bank_apply(bk, l, SITE_MLP1, 1, SCALE_ONE, ln, d, dt, hb, dt, 4 * d, nullptr, B, d, 4 * d, 1, 1, bk->ids_dev, 1, stream));
        RT_CALL(r.residual_gemm(hb, 4 * d, lw[18], lw[19]));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_MLP2, 1, SCALE_ONE, hb, 4 * d, dt, slabs, WIPA_F32, d, nullptr, B, 4 * d, d, 1, 1, bk->ids_dev, 0, stream));
    }
    RT_CALL(r.ln_step(w[2], w[3]));
    float* logits = (float*)(st + L.logits);
    if (logits_fused(cfg, B, ctx)) {
        const void* const* lw0 = w + WIPA_DEC_GLOBAL;
        float* part = (float*)(sc + S.greedy_part);
        RT_CALL(wipa_logits_greedy(ln, d, w[0], d, ctx.lean ? nullptr : logits, L.ld_logits, B, cfg->n_vocab, d, ctx.mask_first, ctx.mask_always, pos,
                                   ctx.n_init, part, wipa_logits_greedy_partials_bytes(B), stream));
        RT_CALL(wipa_greedy_step_embed_partials(part, WIPA_GREEDY_PARTS, B, tokens, L.ld_tok, pos, posd, done_counter_of(st, L), ctx.n_init, ctx.eot,
                                                (float*)(st + L.sum_logprobs), (int32_t*)(st + L.not_done), w[0], emb_dtype(cfg), emb_scale(cfg, w),
                                                (const float*)w[1], nctx, x_first, (const float*)lw0[0], (const float*)lw0[1], ln, dt, d, 1e-5f,
                                                stream));
        return WIPA_OK;
    }
    RT_CALL(gemm(ln, d, w[0], d, logits, L.ld_logits, B, cfg->n_vocab, d, dt, WIPA_F32, nullptr, 0, nullptr, stream));
    if (tail) {
        // greedy update + embedding of the chosen token + first LayerNorm of the NEXT position + position advance: one launch
        // (with ctx.rules the timestamp rules, with ctx.sample the draw, with ctx.starts the RAGGED tails: position embedding and sampling
        // counter at the row's own position)
        const void* const* lw0 = w + WIPA_DEC_GLOBAL;
        if (ctx.beam)  // top G + 1 per row, then per clip: selection, gather, finished store, the next input rows, the position advance
            return wipa_beam_tail("wipa_decoder_run_ex", logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos,
                                  posd, ctx.n_init, ctx.eot, ctx.rules, ctx.beam, G, ctx.beam_max_candidates, (float*)(st + L.sum_logprobs),
                                  (int32_t*)(st + L.not_done), w[0], emb_dtype(cfg), emb_scale(cfg, w), (const float*)w[1], nctx, x_first,
                                  (const float*)lw0[0], (const float*)lw0[1], ln, dt, d, 1e-5f, stream);
        if (ctx.continuous)
            return wipa_step_tail_continuous(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, posd,
                                             done_counter_of(st, L), ctx.n_init, ctx.eot, ctx.rules, ctx.sample, ctx.sample_rows, ctx.starts,
                                             (int)ctx.prompted, ctx.no_speech, ctx.no_speech_token, (float*)(st + L.sum_logprobs), (int32_t*)(st + L.not_done), w[0],
                                             emb_dtype(cfg), emb_scale(cfg, w), (const float*)w[1], nctx, x_first, (const float*)lw0[0],
                                             (const float*)lw0[1], ln, dt, d, 1e-5f, stream);
        RT_CALL(wipa_step_tail(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, posd,
                               done_counter_of(st, L), ctx.n_init, ctx.eot, ctx.rules, ctx.sample, ctx.starts, (float*)(st + L.sum_logprobs), (int32_t*)(st + L.not_done), w[0],
                               emb_dtype(cfg), emb_scale(cfg, w), (const float*)w[1], nctx, x_first, (const float*)lw0[0], (const float*)lw0[1], ln,
                               dt, d, 1e-5f, stream));
        return WIPA_OK;
    }
    WIPA_REQUIRE(!ctx.rules && !ctx.sample && !ctx.starts, "decode step: the timestamp rules, sampling and ragged prompts need the fused tail (WIPA_DECODE_TAIL=0 is set)");
    RT_CALL(wipa_greedy_step(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, ctx.n_init,
                             ctx.eot, (float*)(st + L.sum_logprobs), (int32_t*)(st + L.not_done), stream));
    hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, pos, posd, d);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// One decoder step with the fused blocks of decode_fused.hip: embed + 5 launches per layer + final LayerNorm + logits +
// greedy update + position advance (65 launches for whisper-small instead of 137).  Same state transitions as enqueue_step.
int enqueue_step_fused(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, const StepCtx& ctx,
                       wipa_stream_t stream) {
    const int dt = cfg->dtype;
    const size_t e = wipa_dtype_size(dt);
    const int d = cfg->n_text_state, H = cfg->n_text_head, nctx = cfg->n_text_ctx, Ta = cfg->n_audio_ctx;
    WIPA_REQUIRE(!ctx.rules && !ctx.sample && !ctx.starts, "decode step: the timestamp rules, sampling and ragged prompts need the fused tail (WIPA_DECODE_FUSED=1 is set)");
    const DecScratch S = dec_scratch(cfg, B);
    char* sc = st + L.scratch;
    float* xa = (float*)(sc + S.x);
    float* xb = (float*)(sc + S.x2);
    void* ln = sc + S.ln;
    void* ao = sc + S.ao;
    void* hb = sc + S.h;
    float* slabs = (float*)(sc + S.slabs);
    int64_t* posd = (int64_t*)(sc + S.posd);
    int32_t* tokens = (int32_t*)(st + L.tokens);
    int32_t* pos = (int32_t*)(st + L.pos);
    RT_CALL(wipa_embed_tokens(tokens, L.ld_tok, B, 1, 0, pos, w[0], emb_dtype(cfg), emb_scale(cfg, w), (const float*)w[1], xa, d, stream));
    float* cur = xa;
    float* other = xb;
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        const void* const* lw = w + WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l;
        char* skv = st + L.self_kv + (size_t)l * 3 * B * nctx * d * e;  // [3][B][nctx][d]: slot 0 unused here, 1 K, 2 V
        char* ckv = st + L.cross_kv + (size_t)l * B * 2 * H * Ta * 64 * e;
        const size_t slot = (size_t)B * nctx * d * e;
        {
            wipa_self_block_desc a;
            memset(&a, 0, sizeof(a));
            a.x = cur; a.ln_w = (const float*)lw[0]; a.ln_b = (const float*)lw[1];
            a.wqkv = lw[2]; a.bqkv = (const float*)lw[3]; a.wo = lw[4];
            a.kcache = skv + slot; a.vcache = skv + 2 * slot; a.pos = pos; a.slabs = slabs;
            a.kv_batch_stride = (int64_t)nctx * d; a.slab_stride = (int64_t)B * d;
            a.B = B; a.d = d; a.H = H; a.dtype = dt; a.eps = 1e-5f; a.qk_scale = QK_SCALE;
            RT_CALL(wipa_decode_self_block(&a, stream));
        }
        {
            wipa_cross_block_desc c;
            memset(&c, 0, sizeof(c));
            c.x_in = cur; c.x_out = other; c.slabs = slabs; c.bias_o = (const float*)lw[5];
            c.ln_w = (const float*)lw[6]; c.ln_b = (const float*)lw[7]; c.wq = lw[8]; c.bq = (const float*)lw[9];
            c.kv = ckv; c.out = ao; c.slab_stride = (int64_t)B * d;
            c.n_slabs = H; c.B = B; c.d = d; c.H = H; c.Tk = Ta; c.dtype = dt; c.eps = 1e-5f; c.qk_scale = QK_SCALE;
            RT_CALL(wipa_decode_cross_block(&c, stream));
        }
        std::swap(cur, other);
        // cross out projection and the MLP update the residual rows in place (no split-K: one launch each)
        RT_CALL(gemm(ao, d, lw[12], d, cur, d, B, d, d, dt, WIPA_F32, (const float*)lw[13], 0, cur, stream));
        {
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.ln_x = cur; g.ln_ldx = d; g.ln_w = (const float*)lw[14]; g.ln_b = (const float*)lw[15]; g.ln_eps = 1e-5f;
            RT_CALL(gemm(nullptr, d, lw[16], d, hb, 4 * d, B, 4 * d, d, dt, dt, (const float*)lw[17], 1, nullptr, stream, &g));
        }
        RT_CALL(gemm(hb, 4 * d, lw[18], 4 * d, cur, d, B, d, 4 * d, dt, WIPA_F32, (const float*)lw[19], 0, cur, stream));
    }
    RT_CALL(wipa_add_slabs_layernorm(cur, d, nullptr, 0, 0, ln, dt, d, (const float*)w[2], (const float*)w[3], B, d, 1e-5f, stream));
    float* logits = (float*)(st + L.logits);
    RT_CALL(gemm(ln, d, w[0], d, logits, L.ld_logits, B, cfg->n_vocab, d, dt, WIPA_F32, nullptr, 0, nullptr, stream));
    RT_CALL(wipa_greedy_step(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, ctx.n_init,
                             ctx.eot, (float*)(st + L.sum_logprobs), (int32_t*)(st + L.not_done), stream));
    hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, pos, posd, d);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// Decode-step variants, WIPA_DECODE_FUSED (read at enqueue / capture time, part of the graph key):
//   2 (default)  the unfused step with ONE fusion: [split-K slab sum + residual + cross_attn_ln + cross query + cross-attention]
//                in a single launch (wipa_decode_cross_block, query weights prefetched under the prologue): 9 launches per
//                layer, 1.311 ms per step against 1.352 ms (whisper-small bf16, 64 rows, MI355X, r02);
//   0            the unfused step, 11 launches per layer;
//   1            every fused block (5 launches per layer).  NOT the default: it measured 2.05 ms per step
//                (profiles/r02_fused_step_by_kernel.txt) -- a fused block is a chain of dependent memory round trips (LayerNorm
//                rows -> weight fragments -> cache rows -> weight fragments) that costs more than the ~4.5 us launch gaps it
//                removes: self block 34.9 us vs 23.4 us for the four launches it replaces, LayerNorm-prologue mlp1 37.2 us vs
//                12 us, and without split-K the mlp2 projection has 48 workgroups to stream 4.7 MB (19.7 us vs 7.4 us).
int decode_mode(const wipa_model_cfg* cfg, int B) {
    const char* e = getenv("WIPA_DECODE_FUSED");
    const int m = e ? atoi(e) : 2;
    // the fused blocks read their weights as T: fp8 tables stay on the unfused step
    if (m == 0 || cfg->dec_w_dtype != 0 || cfg->n_text_state > 1280 || cfg->n_text_head > 20 || B > 65535) return 0;
    return m == 1 ? 1 : 2;
}
bool use_fused_step(const wipa_model_cfg* cfg, int B) { return !cfg->dec_cross_absorbed && decode_mode(cfg, B) == 1; }
// whether the steps of this configuration end with the fused tail (and therefore need enqueue_step_head before the first one)
bool step_needs_head(const wipa_model_cfg* cfg, int B) { return !use_fused_step(cfg, B) && tail_fused(); }

int enqueue_decode_step(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, const StepCtx& ctx,
                        wipa_stream_t stream) {
    if (use_fused_step(cfg, B)) return enqueue_step_fused(cfg, w, st, L, B, ctx, stream);
    return enqueue_step(cfg, w, st, L, B, ctx, stream);
}

__global__ void set_pos_kernel(int32_t* pos, int64_t* posd, int value, int d) {
    *pos = value;
    *posd = (int64_t)value * d;
}

// The first new token after a batched prompt pass over P = ctx.n_init columns, from the last column's logits in the state: the
// position is set to P - 1, the update writes token P (a draw with a sampling record -- at the row's own position with starts --,
// rule 4 under rules: timestamps only, capped at max_initial_timestamp_index), the position advances.
int enqueue_first_token(const wipa_model_cfg* cfg, char* st, const wipa_dec_layout& L, int B, const StepCtx& ctx, wipa_stream_t stream) {
    const int P = ctx.n_init, d = cfg->n_text_state;
    float* logits = (float*)(st + L.logits);
    int64_t* posd = (int64_t*)(st + L.scratch + dec_scratch(cfg, B).posd);
    int32_t* tokens = (int32_t*)(st + L.tokens);
    int32_t* pos = (int32_t*)(st + L.pos);
    float* sums = (float*)(st + L.sum_logprobs);
    int32_t* not_done = (int32_t*)(st + L.not_done);
    hipLaunchKernelGGL(set_pos_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, pos, posd, P - 1, d);
    if (ctx.beam)
        RT_CALL(wipa_beam_step(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, P, ctx.eot, ctx.rules,
                               ctx.beam, group_of(cfg), ctx.beam_max_candidates, sums, not_done, stream));
    else if (ctx.sample && ctx.starts)
        RT_CALL(wipa_sample_step_ragged(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, P, ctx.eot,
                                        ctx.rules, ctx.sample, ctx.starts, sums, not_done, stream));
    else if (ctx.sample)
        RT_CALL(wipa_sample_step(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, P, ctx.eot, ctx.rules,
                                 ctx.sample, sums, not_done, stream));
    else if (ctx.rules)
        RT_CALL(wipa_timestamp_step(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, P, ctx.eot, ctx.rules,
                                    sums, not_done, stream));
    else
        RT_CALL(wipa_greedy_step(logits, L.ld_logits, B, cfg->n_vocab, ctx.mask_first, ctx.mask_always, tokens, L.ld_tok, pos, P, ctx.eot, sums,
                                 not_done, stream));
    hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, pos, posd, d);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// The first n_init decoder steps as ONE batched pass over the prompt (rows (b, t), t < n_init): mlx_whisper runs the
// prompt through the decoder in one forward too.  Self-K/V of positions 0..n_init-1 land in the cache, the cross K/V are
// streamed once for all prompt positions (decode_attn_multi_kernel), logits are computed for the last position only, and
// the greedy update writes token n_init.  Afterwards the state equals that after n_init calls of enqueue_step.
int enqueue_prefill(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, const StepCtx& ctx,
                    wipa_stream_t stream) {
    const int dt = cfg->dtype;
    const size_t e = wipa_dtype_size(dt);
    const int d = cfg->n_text_state, H = cfg->n_text_head, nctx = cfg->n_text_ctx, Ta = cfg->n_audio_ctx;
    const int P = ctx.n_init, M = B * P;
    const int G = group_of(cfg), Bc = clips_of(cfg, B);
    const DecScratch S = dec_scratch(cfg, B);
    char* sc = st + L.scratch;
    char* ln = sc + S.ln;
    void* q = sc + S.q;
    void* ao = sc + S.ao;
    void* hb = sc + S.h;
    SlabStream r{(float*)(sc + S.x), (float*)(sc + S.slabs), ln, M, d, dt, 1024, 1, stream};
    const wipa_adapter_bank* bk = ctx.bank;  // rows (b, t): P rows per id
    float* slabs = r.slabs;
    RT_CALL(wipa_embed_tokens((const int32_t*)(st + L.tokens), L.ld_tok, B, P, 0, nullptr, w[0], emb_dtype(cfg), emb_scale(cfg, w), (const float*)w[1],
                              r.x, d, stream));
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        const void* const* lw = w + WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l;
        char* skv = st + L.self_kv + (size_t)l * 3 * B * nctx * d * e;  // [3][B][nctx][d]
        char* ckv = st + L.cross_kv + (size_t)l * Bc * 2 * H * Ta * 64 * e;
        RT_CALL(r.ln_step(lw[0], lw[1]));
        {
            // q|k|v of positions 0..P-1 -> slot[n / d][b][t][n % d]
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.stream_weights = 1;
            g.col_scale_n = 2 * d; g.col_scale = QK_SCALE;
            g.rg_in = P; g.rg_valid = P; g.rg_stride = (int64_t)nctx * d;
            g.cg_in = d; g.cg_stride = (int64_t)B * nctx * d;
            RT_CALL(gemm(ln, d, lw[2], d, skv, d, M, 3 * d, d, dt, dt, (const float*)lw[3], 0, nullptr, stream, &g));
            if (bk) RT_CALL(bank_apply(bk, l, SITE_Q, 3, SCALES_QKV, ln, d, dt, skv, dt, d, &g, M, d, 3 * d, P, 1, bk->ids_dev, 0, stream));
        }
        {
            wipa_attn_desc a;
            memset(&a, 0, sizeof(a));
            const size_t slot = (size_t)B * nctx * d * e;
            a.q = skv; a.k = skv + slot; a.v = skv + 2 * slot; a.out = ao;
            a.q_bs = (int64_t)nctx * d; a.q_rs = d; a.q_hs = 64;
            a.k_bs = a.q_bs; a.k_rs = d; a.k_hs = 64;
            a.v_bs = a.q_bs; a.v_rs = d; a.v_hs = 64;
            a.o_bs = (int64_t)P * d; a.o_rs = d; a.o_hs = 64;
            a.B = B; a.H = H; a.Tq = P; a.Tk = P; a.causal = 1; a.dtype = dt;
            RT_CALL(wipa_attention(&a, stream));
        }
        RT_CALL(r.residual_gemm(ao, d, lw[4], lw[5]));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_O, 1, SCALE_ONE, ao, d, dt, slabs, WIPA_F32, d, nullptr, M, d, d, P, 1, bk->ids_dev, 0, stream));
        RT_CALL(r.ln_step(lw[6], lw[7]));
        {
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.stream_weights = 1;
            g.col_scale_n = d; g.col_scale = QK_SCALE;
            RT_CALL(gemm(ln, d, lw[8], d, q, d, M, d, d, dt, dt, (const float*)lw[9], 0, nullptr, stream, &g));
            if (bk) RT_CALL(bank_apply(bk, l, SITE_CQ, 1, SCALES_QKV, ln, d, dt, q, dt, d, nullptr, M, d, d, P, 1, bk->ids_dev, 0, stream));
        }
        if (cfg->dec_cross_absorbed) {
            // one absorbed pass per prompt position: rows (b, t) of q / ao with row stride P * d
            const void* wkT = w[WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * cfg->n_text_layer + WIPA_DEC_ABSORBED_PER_LAYER * l];
            for (int t = 0; t < P; ++t)
                RT_CALL(wipa_cross_absorbed_attention_grouped((const char*)q + (size_t)t * d * e, (int64_t)P * d, wkT, st + L.cross_kv,
                                                              (const char*)lw[10] + (size_t)d * d * e, (const float*)lw[11] + d,
                                                              (char*)ao + (size_t)t * d * e, (int64_t)P * d, sc + S.absorbed,
                                                              S.greedy_part - S.absorbed, B, H, d, Ta, QK_SCALE, cfg->dec_cross_splits, G, stream));
        } else if (G > 1) {  // candidate groups: the prompt rows of every candidate against the K / V of its clip
            RT_CALL(wipa_decode_cross_attn_grouped(q, ckv, ao, B, H, Ta, P, G, dt, stream));
        } else {
            RT_CALL(wipa_decode_cross_attn_multi(q, ckv, ao, B, H, Ta, P, dt, stream));
        }
        RT_CALL(r.residual_gemm(ao, d, lw[12], lw[13]));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_CO, 1, SCALE_ONE, ao, d, dt, slabs, WIPA_F32, d, nullptr, M, d, d, P, 1, bk->ids_dev, 0, stream));
        RT_CALL(r.ln_step(lw[14], lw[15]));
        {
            const bool mlp1_bank = bank_on(bk, SITE_MLP1);  // as in enqueue_step: the apply call performs the GELU
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.stream_weights = 1;
            RT_CALL(gemm(ln, d, lw[16], d, hb, 4 * d, M, 4 * d, d, dt, dt, (const float*)lw[17], mlp1_bank ? 0 : 1, nullptr, stream, &g));
            if (mlp1_bank) RT_CALL(bank_apply(bk, l, SITE_MLP1, 1, SCALE_ONE, ln, d, dt, hb, dt, 4 * d, nullptr, M, d, 4 * d, P, 1, bk->ids_dev, 1, stream));
        }
        RT_CALL(r.residual_gemm(hb, 4 * d, lw[18], lw[19]));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_MLP2, 1, SCALE_ONE, hb, 4 * d, dt, slabs, WIPA_F32, d, nullptr, M, 4 * d, d, P, 1, bk->ids_dev, 0, stream));
    }
    RT_CALL(r.ln_step(w[2], w[3]));
    // logits of the LAST prompt position only: rows (b, P-1) of ln, i.e. row stride P*d
    RT_CALL(gemm(ln + (size_t)(P - 1) * d * e, (int64_t)P * d, w[0], d, st + L.logits, L.ld_logits, B, cfg->n_vocab, d, dt, WIPA_F32, nullptr, 0,
                 nullptr, stream));
    return enqueue_first_token(cfg, st, L, B, ctx, stream);
}

// Hardware-counter collection (rocprofv3 --pmc sets ROCPROF_COUNTER_COLLECTION) serialises every dispatch and intercepts the
// queues; a captured step replayed under it hung once in round 1 and no artefact of that run survives.  CANDIDATE cause (the only
// one the code ever offered, not a confirmed one): before round 2 the once-only hipFuncSetAttribute pass ran inside the first
// wipa_gemm call, i.e. INSIDE the relaxed capture whenever a decode step was the first GEMM of the process -- exactly the shape
// of a counter micro-target.  Since round 2 every attribute call sits behind wipa_gemm_init / wipa_decode_fused_init /
// wipa_cross_absorbed_init (each a once-per-process pass), which the decode entry points call BEFORE they begin a capture, so
// nothing but kernel launches is issued between hipStreamBeginCapture and hipStreamEndCapture; with that change the one bounded
// confirmation run (WIPA_DECODE_GRAPH=force under --pmc, tools/pmc_graph_confirm.py, profiles/r03_graph_replay_under_counters.txt)
// captured and replayed a step with counters attached and reproduced the eager ids.  The eager-under-counters DEFAULT stays for a
// different reason: a per-kernel counter run wants the dispatches separate anyway, and graphs_allowed() prints one line when it
// takes that path so that PMC numbers are not mistaken for graph-replay numbers.  WIPA_DECODE_GRAPH=0 asks for the eager path
// explicitly (any other queue-intercepting tool), =force keeps the graphs under counters.  Kernel tracing alone keeps the graphs.
bool counters_attached() {
    const char* e = getenv("ROCPROF_COUNTER_COLLECTION");
    return e && *e && strcmp(e, "0") != 0 && strcasecmp(e, "false") != 0;
}
bool graphs_allowed() {
    const char* g = getenv("WIPA_DECODE_GRAPH");
    if (g && (strcmp(g, "0") == 0 || strcasecmp(g, "off") == 0)) return false;
    if (g && strcasecmp(g, "force") == 0) return true;
    if (counters_attached()) {
        // say so once: numbers collected under --pmc are those of the EAGER step (same kernels, host-enqueued), not of graph replay
        static std::once_flag once;
        std::call_once(once, [] {
            fprintf(stderr, "libwipa: hardware counters attached (ROCPROF_COUNTER_COLLECTION): decode steps are enqueued eagerly, not "
                            "replayed from the captured graph (WIPA_DECODE_GRAPH=force keeps the graphs)\n");
        });
        return false;
    }
    return true;
}
// every kernel attribute the step needs, set outside any capture
int init_before_capture(const wipa_model_cfg* cfg) {
    RT_CALL(wipa_decode_fused_init());
    RT_CALL(wipa_gemm_init());
    if (cfg && cfg->dec_cross_absorbed) RT_CALL(wipa_cross_absorbed_init(cfg->n_text_state));
    return WIPA_OK;
}

// The blob layout depends on the configuration (dtype, absorbed / cached cross-attention, fp8 tables): a blob allocated for one
// cfg and handed in with another would be written far past its end.  Every entry point checks the caller's size.
int state_fits(const char* who, const wipa_dec_layout& L, size_t state_bytes) {
    WIPA_REQUIRE((int64_t)state_bytes >= L.total_bytes,
                 "%s: the state blob holds %zu bytes, this configuration needs %lld (wipa_decoder_layout); re-allocate it after a "
                 "change of dtype / cross-attention form / weight format", who, state_bytes, (long long)L.total_bytes);
    return WIPA_OK;
}

// graph cache: one captured step per (state blob, weights, masks, shape)
// The key carries cfg->weights_generation: the host address of a weight table can be reused by a NEW table after the old
// one was freed, so the address alone does not identify the device pointers baked into a captured graph.
// The timestamp rules are baked into the captured tail's arguments: three more terms (timestamp_begin = 0: no rules).
// The sampling record enters with its ADDRESS (NULL: temperature 0): seed, attempt, temperature and streams are read from it by
// the replayed tail, so a new seed or temperature replays the same graph.
// The starts array of a ragged call enters with its ADDRESS too (NULL: no prompts): the replayed kernels read the rows' starts from it.
// The ragged prompt pass (kind 3 + 16 * (sot_col + 1)) bakes its workspace in as well (NULL otherwise).
// A continuous step with rules bakes in the no-speech array's address and its vocabulary column: the last two terms (NULL and 0 otherwise).
// A continuous step with a temperature per row has its own variant bit, and its record's address stands in the sampling record's term.
// A PROMPTED continuous step is the continuous key plus a variant bit of its own (candidate groups, which share that range of the word,
// are not served by a continuous call).
// A BEAM step bakes in the beam buffer's address and max_candidates: the last two terms, of their own (NULL and 0 without beams).
// An ADAPTER BANK bakes in its address, its ids array's address and (n, rank, site_mask): the last three terms (NULL, NULL and 0 without
// a bank).  The ids themselves are read by the replayed kernels.
typedef std::tuple<const void*, const void*, const void*, const void*, int, int, int, int, int, int, int, int, int, const void*, const void*, const void*, const void*, int, const void*, int, const void*, const void*, int64_t> GraphKey;  // ..., generation, kind: 0 step, 1 prefill, 2 lean step (no logit stores), rules, sampling record, starts, workspace, no-speech array, no-speech column
// sampling lives in the fused step tail, like the rules: refused before anything is enqueued where the step cannot carry it
int sample_servable(const char* who, const wipa_model_cfg* cfg, int B, const void* sample) {
    if (!sample) return WIPA_OK;
    WIPA_REQUIRE(tail_fused() && !use_fused_step(cfg, B),
                 "%s: sampling lives in the fused step tail; WIPA_DECODE_TAIL=0 / WIPA_DECODE_FUSED=1 cannot serve it", who);
    WIPA_REQUIRE(cfg->n_vocab <= 65536 && cfg->n_text_ctx <= 65536, "%s: need n_vocab and n_text_ctx <= 65536 (n_vocab=%d)", who, cfg->n_vocab);
    return WIPA_OK;
}
// candidate groups are served where a sampling decode is served (what sampling refuses is refused in sampling's words), on rows that
// divide into whole groups; refused before anything is enqueued
int group_servable(const char* who, const wipa_model_cfg* cfg, int B) {
    const int G = group_of(cfg);
    WIPA_REQUIRE(B % G == 0, "%s: B=%d rows are no multiple of cfg.dec_n_group=%d (rows = clips x candidates)", who, B, G);
    if (G == 1) return WIPA_OK;
    WIPA_REQUIRE(tail_fused() && !use_fused_step(cfg, B),
                 "%s: sampling lives in the fused step tail; WIPA_DECODE_TAIL=0 / WIPA_DECODE_FUSED=1 cannot serve it", who);
    return WIPA_OK;
}
// ragged prompts live in the RAGGED instantiations of the unfused step's self-attention and tail: refused before anything is enqueued
// where the step is another one, and on fp8 decoder tables (as wipa_decoder_logits refuses them)
int starts_servable(const char* who, const wipa_model_cfg* cfg, int B, int n_init, const int32_t* starts_dev) {
    if (!starts_dev) return WIPA_OK;
    WIPA_REQUIRE(tail_fused() && !use_fused_step(cfg, B),
                 "%s: starts_dev (ragged prompts) needs the unfused step with the fused tail; WIPA_DECODE_TAIL=0 / WIPA_DECODE_FUSED=1 cannot serve it", who);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "%s: starts_dev (ragged prompts) is not served on fp8 decoder tables (cfg.dec_w_dtype)", who);
    WIPA_REQUIRE(n_init >= 1 && n_init <= cfg->n_text_ctx, "%s: prompt width P=%d outside 1..n_text_ctx=%d", who, n_init, cfg->n_text_ctx);
    return WIPA_OK;
}
// a configuration whose steps cannot carry the rules is refused before anything is enqueued: never decoded without them
int rules_servable(const char* who, const wipa_model_cfg* cfg, int B, int eot, const wipa_decode_rules* r) {
    if (!r) return WIPA_OK;
    WIPA_REQUIRE(tail_fused() && !use_fused_step(cfg, B),
                 "%s: the timestamp rules live in the fused step tail; WIPA_DECODE_TAIL=0 / WIPA_DECODE_FUSED=1 cannot serve them", who);
    WIPA_REQUIRE(r->timestamp_begin > 0 && r->timestamp_begin < cfg->n_vocab && eot < r->timestamp_begin && r->no_timestamps >= 0 &&
                     r->no_timestamps < r->timestamp_begin && cfg->n_vocab <= 65536,
                 "%s: need eot < timestamp_begin < n_vocab <= 65536 and no_timestamps below timestamp_begin (eot=%d timestamp_begin=%d "
                 "no_timestamps=%d n_vocab=%d)", who, eot, r->timestamp_begin, r->no_timestamps, cfg->n_vocab);
    return WIPA_OK;
}
// what a continuous decode serves, in the words of its entry points: bf16 / f32 decoder tables, one row per clip
int continuous_servable(const char* who, const wipa_model_cfg* cfg, int B, const int32_t* starts_dev) {
    WIPA_REQUIRE(starts_dev, "%s: starts_dev (int32 [2][B]: first own columns, then token limits) is required", who);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "%s: fp8 decoder tables are not served (cfg.dec_w_dtype)", who);
    WIPA_REQUIRE(group_of(cfg) == 1, "%s: candidate groups are not served (cfg.dec_n_group=%d)", who, cfg->dec_n_group);
    WIPA_REQUIRE(B > 0, "%s: bad batch", who);
    return WIPA_OK;
}
// what a beam call serves, in the words of its entry point; refused before anything is enqueued
int beam_servable(const char* who, const wipa_model_cfg* cfg, int B, const StepCtx& c) {
    if (!c.beam) return WIPA_OK;
    const int G = group_of(cfg);
    WIPA_REQUIRE(!c.sample && !c.sample_rows, "%s: call.beam and call.sample / call.sample_rows cannot be given together (beams run at temperature 0)", who);
    WIPA_REQUIRE(!c.starts && !c.continuous, "%s: call.beam is not served with call.starts_dev / call.continuous (the beams of a clip share one prompt)", who);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "%s: call.beam is not served on fp8 decoder tables (cfg.dec_w_dtype)", who);
    WIPA_REQUIRE(tail_fused() && !use_fused_step(cfg, B), "%s: call.beam needs the unfused step with the fused tail; WIPA_DECODE_TAIL=0 / WIPA_DECODE_FUSED=1 cannot serve it", who);
    WIPA_REQUIRE(G >= 1 && G <= 16, "%s: cfg.dec_n_group=%d (n_group) outside 1..16", who, G);
    WIPA_REQUIRE(B % G == 0, "%s: B=%d rows are no multiple of cfg.dec_n_group=%d (n_group)", who, B, G);
    WIPA_REQUIRE(c.beam_max_candidates >= 1 && c.beam_max_candidates <= 64, "%s: call.beam_max_candidates=%d outside 1..64", who, c.beam_max_candidates);
    WIPA_REQUIRE(cfg->n_vocab <= 65536, "%s: need n_vocab <= 65536 (n_vocab=%d)", who, cfg->n_vocab);
    const size_t need = wipa_beam_bytes(B, G, c.beam_max_candidates, dec_layout(cfg, B).ld_tok);
    WIPA_REQUIRE(c.beam_bytes >= need, "%s: call.beam_bytes: the beam buffer holds %zu bytes, this shape needs %zu (wipa_beam_bytes)", who, c.beam_bytes, need);
    return WIPA_OK;
}
// what the steps of a call with rules, a sampling record, starts or candidate groups must be able to serve
// what an adapter bank needs of its struct and of the configuration; `who` may be an entry point that takes the bank itself
int bank_servable(const char* who, const wipa_model_cfg* cfg, const wipa_adapter_bank* bk) {
    if (!bk) return WIPA_OK;
    WIPA_REQUIRE(bk->n >= 1 && bk->n <= WIPA_LORA_BANK_MAX_ADAPTERS, "%s: call.bank: n = %d: a bank holds 1..%d adapters", who, bk->n,
                 WIPA_LORA_BANK_MAX_ADAPTERS);
    WIPA_REQUIRE(bk->rank >= 4 && bk->rank <= 64 && bk->rank % 4 == 0, "%s: call.bank: rank = %d: a multiple of 4 in 4..64", who, bk->rank);
    WIPA_REQUIRE(bk->site_mask != 0 && bk->site_mask < (1u << WIPA_BANK_SITES), "%s: call.bank: site_mask = 0x%x: 1..%d sites of a block", who,
                 bk->site_mask, WIPA_BANK_SITES);
    WIPA_REQUIRE(bk->A && bk->B && bk->gain && bk->ids_dev, "%s: call.bank: A, B, gain and ids_dev are required", who);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "%s: call.bank is not served on fp8 decoder tables (cfg.dec_w_dtype)", who);
    WIPA_REQUIRE(!cfg->dec_cross_absorbed || !(bank_on(bk, SITE_CK) || bank_on(bk, SITE_CV)),
                 "%s: call.bank targets cross_attn.key / cross_attn.value, which the absorbed cross-attention form (cfg.dec_cross_absorbed) "
                 "does not serve: the cached form adds their terms to the cached K / V (wipa_decoder_adapt_cross)", who);
    return WIPA_OK;
}
int bank_call_servable(const char* who, const wipa_model_cfg* cfg, int B, const StepCtx& c) {
    if (!c.bank) return WIPA_OK;
    WIPA_REQUIRE(!c.beam, "%s: call.bank is not served with call.beam (beam search decodes one adapter at a time: Whisper.set_adapter)", who);
    // rows with their own first column: the steps carry a bank as any step does; the ragged prompt pass and the prompted admission take
    // it themselves (wipa_decoder_prefill_ragged_bank, wipa_decoder_admit_rows_prompted_bank), an unprompted admission is followed by the
    // slot's id and wipa_decoder_adapt_cross
    WIPA_REQUIRE(tail_fused() && !use_fused_step(cfg, B),
                 "%s: call.bank needs the unfused step with the fused tail; WIPA_DECODE_TAIL=0 / WIPA_DECODE_FUSED=1 cannot serve it", who);
    return bank_servable(who, cfg, c.bank);
}
int step_servable(const char* who, const wipa_model_cfg* cfg, int B, const StepCtx& c) {
    RT_CALL(bank_call_servable(who, cfg, B, c));
    RT_CALL(rules_servable(who, cfg, B, c.eot, c.rules));
    RT_CALL(sample_servable(who, cfg, B, c.sample ? c.sample : c.sample_rows));
    RT_CALL(starts_servable(who, cfg, B, c.n_init, c.starts));
    return group_servable(who, cfg, B);
}
// Every refusal of wipa_decoder_run_ex (prefill = false) and wipa_decoder_prefill_ex (n_steps = 1), in order: null pointers and ranges,
// fields that exclude or need each other, then what the configuration's step cannot serve.  Nothing is enqueued before it returns.
int decode_call_checks(const char* who, const wipa_model_cfg* cfg, const void* const* w, const void* state, int B, const StepCtx& c, int n_steps,
                       bool prefill) {
    WIPA_REQUIRE(w && state && c.mask_first && c.mask_always && B > 0 && n_steps >= 0,
                 "%s: bad arguments (weights, state, call.mask_first and call.mask_always are required; B > 0, n_steps >= 0)", who);
    WIPA_REQUIRE(!c.sample || !c.sample_rows, "%s: call.sample_rows takes the place of call.sample: pass one of them", who);
    WIPA_REQUIRE(!prefill || (!c.starts && !c.continuous && !c.prompted && !c.sample_rows && !c.no_speech),
                 "%s: call.starts_dev, call.continuous, call.prompted, call.sample_rows and call.no_speech_dev are not served by the prompt pass "
                 "(rows with their own prompts: wipa_decoder_prefill_ragged; an admitted clip's prompt: wipa_decoder_admit_rows_prompted)", who);
    WIPA_REQUIRE(c.continuous || (!c.sample_rows && !c.no_speech && !c.prompted),
                 "%s: call.sample_rows, call.no_speech_dev and call.prompted need call.continuous", who);
    WIPA_REQUIRE(!c.continuous || c.starts, "%s: call.continuous needs call.starts_dev (int32 [2][B]: first own columns, then token limits; "
                 "[3][B] with call.prompted: window starts, token limits, prompt columns)", who);
    WIPA_REQUIRE(!c.no_speech || c.rules, "%s: call.no_speech_dev needs call.rules", who);
    WIPA_REQUIRE(((uintptr_t)c.sample_rows % 16) == 0, "%s: call.sample_rows (wipa_sample_rows_bytes) must be 16-byte aligned", who);
    if (c.continuous) {
        RT_CALL(continuous_servable(who, cfg, B, c.starts));
        WIPA_REQUIRE(c.n_init >= 1 && c.n_init <= 4, "%s: call.n_init: 1..4 initial tokens per clip (got %d)", who, c.n_init);
    }
    WIPA_REQUIRE(!c.no_speech || (c.no_speech_token >= 0 && c.no_speech_token < cfg->n_vocab),
                 "%s: call.no_speech_token=%d outside the vocabulary of %d", who, c.no_speech_token, cfg->n_vocab);
    RT_CALL(beam_servable(who, cfg, B, c));
    RT_CALL(step_servable(who, cfg, B, c));
    WIPA_REQUIRE(!prefill || (c.n_init >= 1 && c.n_init <= MAX_PROMPT), "%s: call.n_init: 1..%d prompt tokens (got %d)", who, MAX_PROMPT, c.n_init);
    // the position lives on the device: a call may carry the prompt walk (P - 1 steps) besides the new tokens, so what can be
    // refused here is a step count that no position admits
    WIPA_REQUIRE(!c.starts || n_steps <= cfg->n_text_ctx - 1, "%s: n_steps=%d with call.starts_dev and P=%d runs past n_text_ctx=%d", who, n_steps,
                 c.n_init, cfg->n_text_ctx);
    return WIPA_OK;
}
std::mutex g_graph_mu;
std::map<GraphKey, hipGraphExec_t> g_graphs;

// the variant word of a step or prefill key: every switch that changes what enqueue_decode_step / enqueue_prefill enqueue for (cfg, B).
// (The streaming launch's resident_groups argument is baked into the captured step too, but needs no term here: it is a function
// of B, the width, the frame count and dec_cross_splits -- all in the key -- and of a budget that is constant per process.)
// The call's context decides with the switches: logits_fused() looks at its rules, its sampling record and its starts.
bool lean_steps(const wipa_model_cfg* cfg, int B, const StepCtx& c) { return !use_fused_step(cfg, B) && logits_fused(cfg, B, c); }
int step_variant(const wipa_model_cfg* cfg, int B, const StepCtx& c) {
    return cfg->dtype * 2 + t_f32_split + 4 * decode_mode(cfg, B) + 16 * cfg->dec_w_dtype +
           64 * cfg->dec_cross_absorbed * (absorbed_block_fused() ? 2 : 1) + 256 * (int)tail_fused() + 512 * (int)absorbed_merge_out() +
           1024 * cfg->dec_cross_splits + 8192 * (int)lean_steps(cfg, B, c) +
           16384 * (cfg->dec_cross_absorbed ? wipa_cross_absorbed_loop_variant() : 0) + 65536 * (group_of(cfg) > 1 ? group_of(cfg) : 0) +
           (1 << 27) * (int)(c.continuous && c.prompted) + (1 << 28) * (int)c.continuous + (1 << 29) * (int)(c.continuous && c.rules) + (1 << 30) * (int)(c.continuous && c.sample_rows);
}
// a key from the context of a decode call; the three rule terms are 0 without rules
GraphKey graph_key(const wipa_model_cfg* cfg, const void* const* w, const void* state, int B, const StepCtx& c, int variant, int kind,
                   const void* workspace) {
    return GraphKey(state, (const void*)w, (const void*)c.mask_first, (const void*)c.mask_always, B, c.n_init, c.eot, variant,
                    cfg->weights_generation, kind, c.rules ? c.rules->timestamp_begin : 0, c.rules ? c.rules->no_timestamps : 0,
                    c.rules ? c.rules->max_initial_timestamp_index : 0, c.sample ? c.sample : c.sample_rows, (const void*)c.starts, workspace,
                    (const void*)c.no_speech, c.no_speech ? c.no_speech_token : 0, (const void*)c.beam, c.beam ? c.beam_max_candidates : 0,
                    (const void*)c.bank, c.bank ? (const void*)c.bank->ids_dev : nullptr,
                    c.bank ? ((int64_t)c.bank->site_mask | (int64_t)c.bank->n << 16 | (int64_t)c.bank->rank << 24) : 0);
}
// The executable graph cached under `key`.  When there is none, `enqueue` is captured on s (relaxed mode, nothing but kernel launches
// between begin and end), instantiated and inserted; an enqueue that fails ends the capture, destroys the graph and hands its code back.
template <typename Enqueue>
int cached_graph(const GraphKey& key, hipStream_t s, Enqueue&& enqueue, hipGraphExec_t* out) {
    hipGraphExec_t exec = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_graph_mu);
        auto it = g_graphs.find(key);
        if (it != g_graphs.end()) exec = it->second;
    }
    if (!exec) {
        hipGraph_t graph = nullptr;
        WIPA_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
        const int rc = enqueue();
        const hipError_t ee = hipStreamEndCapture(s, &graph);
        if (rc != WIPA_OK) {
            if (graph) hipGraphDestroy(graph);
            return rc;
        }
        WIPA_CHECK_HIP(ee);
        WIPA_CHECK_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        WIPA_CHECK_HIP(hipGraphDestroy(graph));
        std::lock_guard<std::mutex> lk(g_graph_mu);
        g_graphs[key] = exec;
    }
    *out = exec;
    return WIPA_OK;
}
// A prompt pass: replayed from the graph cached under `key`, or enqueued as it is -- without use_graph, where graphs are off, and
// quietly on the default stream, which cannot be captured.
template <typename Enqueue>
int replay_or_enqueue(bool use_graph, hipStream_t s, const GraphKey& key, Enqueue&& enqueue) {
    if (!use_graph || s == nullptr || !graphs_allowed()) return enqueue();
    hipGraphExec_t exec = nullptr;
    RT_CALL(cached_graph(key, s, enqueue, &exec));
    WIPA_CHECK_HIP(hipGraphLaunch(exec, s));
    return WIPA_OK;
}

// What wipa_decoder_run_ex, wipa_decoder_prefill_ex and wipa_decoder_prefill_ragged do between their argument checks and their first
// launch, in this order: the entry point's `checks` refuse what it cannot serve, then a state blob too small for the layout (*L); every
// kernel attribute is set outside any capture; a call that will enqueue steps (n_steps > 0) starts the greedy tail's arrival counter
// at zero (4 bytes, outside the step graph).
template <typename Checks>
int decode_prologue(const char* who, const wipa_model_cfg* cfg, int B, char* st, size_t state_bytes, int n_steps, hipStream_t s,
                    wipa_dec_layout* L, Checks&& checks) {
    RT_CALL(checks());
    *L = dec_layout(cfg, B);
    RT_CALL(state_fits(who, *L, state_bytes));
    RT_CALL(init_before_capture(cfg));
    if (n_steps > 0) WIPA_CHECK_HIP(hipMemsetAsync(done_counter_of(st, *L), 0, sizeof(int32_t), s));
    return WIPA_OK;
}

// One layer's cached cross K / V of `n_clips` clips (lw: the layer's weights): features x [Wk | Wv] with the key half scaled, written to
// ckv as [clip][K | V][H][Ta][64].  wipa_decoder_set_audio projects all clips of a call, wipa_decoder_admit_rows one clip into its slot.
int cross_kv_gemm(const wipa_model_cfg* cfg, const void* const* lw, const void* features, void* ckv, int n_clips, wipa_stream_t stream) {
    const int d = cfg->n_text_state, H = cfg->n_text_head, Ta = cfg->n_audio_ctx, dt = cfg->dtype;
    wipa_gemm_desc g;
    memset(&g, 0, sizeof(g));
    g.col_scale_n = d; g.col_scale = QK_SCALE;  // the key half; values stay unscaled
    g.rg_in = Ta; g.rg_valid = Ta; g.rg_stride = (int64_t)2 * H * Ta * 64;
    g.cg_in = 64; g.cg_stride = (int64_t)Ta * 64;
    return gemm(features, d, lw[10], d, ckv, 64, n_clips * Ta, 2 * d, d, dt, dt, (const float*)lw[11], 0, nullptr, stream, &g);
}

// What wipa_decoder_begin and wipa_decoder_begin_ragged reset before they write their tokens: every token column (padding columns hold
// token 0), the position, the per-row results and the step's position offset
int begin_reset(const wipa_model_cfg* cfg, char* st, const wipa_dec_layout& L, int B, hipStream_t s) {
    RT_CALL(wipa_decode_fused_init());  // kernel attributes are set here, outside the stream capture of the step
    RT_CALL(wipa_gemm_init());
    WIPA_CHECK_HIP(hipMemsetAsync(st + L.tokens, 0, (size_t)B * L.ld_tok * 4, s));
    WIPA_CHECK_HIP(hipMemsetAsync(st + L.pos, 0, 512, s));  // pos and not_done
    WIPA_CHECK_HIP(hipMemsetAsync(st + L.sum_logprobs, 0, (size_t)B * 4, s));
    WIPA_CHECK_HIP(hipMemsetAsync(st + L.scratch + dec_scratch(cfg, B).posd, 0, 8, s));
    return WIPA_OK;
}

}  // namespace

extern "C" int wipa_profile_begin(wipa_stream_t stream) {
    WIPA_REQUIRE(!t_prof, "wipa_profile_begin: a profile is already open on this thread");
    t_prof = new Profiler{(hipStream_t)stream, {}};
    return WIPA_OK;
}

extern "C" int wipa_profile_end(float* ms_by_class, int* launches_by_class) {
    WIPA_REQUIRE(t_prof, "wipa_profile_end: no open profile");
    Profiler* p = t_prof;
    t_prof = nullptr;
    const hipError_t se = hipStreamSynchronize(p->stream);
    for (int c = 0; c < PROF_CLASSES; ++c) {
        if (ms_by_class) ms_by_class[c] = 0.f;
        if (launches_by_class) launches_by_class[c] = 0;
    }
    for (auto& sp : p->spans) {
        float ms = 0.f;
        if (se == hipSuccess && hipEventElapsedTime(&ms, std::get<1>(sp), std::get<2>(sp)) == hipSuccess) {
            if (ms_by_class) ms_by_class[std::get<0>(sp)] += ms;
            if (launches_by_class) launches_by_class[std::get<0>(sp)] += 1;
        }
        hipEventDestroy(std::get<1>(sp));
        hipEventDestroy(std::get<2>(sp));
    }
    delete p;
    WIPA_CHECK_HIP(se);
    return WIPA_OK;
}

extern "C" int wipa_decoder_layout(const wipa_model_cfg* cfg, int B, wipa_dec_layout* out) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(out && B > 0, "wipa_decoder_layout: bad arguments");
    WIPA_REQUIRE(B % group_of(cfg) == 0, "wipa_decoder_layout: B=%d rows are no multiple of cfg.dec_n_group=%d", B, cfg->dec_n_group);
    *out = dec_layout(cfg, B);
    return WIPA_OK;
}

extern "C" int wipa_decoder_set_audio(const wipa_model_cfg* cfg, const void* const* w, const void* features, void* state,
                                      size_t state_bytes, int B, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(w && features && state && B > 0, "wipa_decoder_set_audio: null pointer / bad batch");
    WIPA_REQUIRE(B % group_of(cfg) == 0, "wipa_decoder_set_audio: B=%d rows are no multiple of cfg.dec_n_group=%d", B, cfg->dec_n_group);
    const int Bc = clips_of(cfg, B);  // features hold B / dec_n_group clips: copied / projected once per clip
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits("wipa_decoder_set_audio", L, state_bytes));
    const size_t e = wipa_dtype_size(cfg->dtype);
    const int d = cfg->n_text_state, H = cfg->n_text_head, Ta = cfg->n_audio_ctx;
    WIPA_REQUIRE(cfg->n_audio_state == d, "encoder/decoder widths differ");
    if (cfg->dec_cross_absorbed) {
        // no key / value projection and no cache: the decode steps stream the encoder output itself (csrc/cross_absorbed.hip)
        WIPA_CHECK_HIP(hipMemcpyAsync((char*)state + L.cross_kv, features, (size_t)Bc * Ta * d * e, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return WIPA_OK;
    }
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        const void* const* lw = w + WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l;
        PROF(PROF_GEMM, cross_kv_gemm(cfg, lw, features, (char*)state + L.cross_kv + (size_t)l * Bc * 2 * H * Ta * 64 * e, Bc, stream));
    }
    return WIPA_OK;
}

extern "C" int wipa_decoder_begin(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B,
                                  const int32_t* initial_tokens_host, int n_init, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(state && initial_tokens_host && n_init >= 1 && n_init <= 4 && B > 0,
                 "wipa_decoder_begin: need 1..4 prompt tokens (got %d)", n_init);
    WIPA_REQUIRE(B % group_of(cfg) == 0, "wipa_decoder_begin: B=%d rows are no multiple of cfg.dec_n_group=%d", B, cfg->dec_n_group);
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits("wipa_decoder_begin", L, state_bytes));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    RT_CALL(begin_reset(cfg, st, L, B, s));
    int t4[4] = {0, 0, 0, 0};
    for (int i = 0; i < n_init; ++i) t4[i] = initial_tokens_host[i];
    hipLaunchKernelGGL(fill_tokens_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (int32_t*)(st + L.tokens), L.ld_tok, B, n_init,
                       t4[0], t4[1], t4[2], t4[3]);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" int wipa_decoder_begin_ragged(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, const int32_t* tokens_host,
                                         const int32_t* starts_host, int P, int32_t* starts_dev, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(state && tokens_host && starts_host && starts_dev && B > 0, "wipa_decoder_begin_ragged: null pointer / bad batch");
    WIPA_REQUIRE(P >= 1 && P <= cfg->n_text_ctx, "wipa_decoder_begin_ragged: prompt width P=%d outside 1..n_text_ctx=%d", P, cfg->n_text_ctx);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "wipa_decoder_begin_ragged: ragged prompts are not served on fp8 decoder tables (cfg.dec_w_dtype)");
    WIPA_REQUIRE(B % group_of(cfg) == 0, "wipa_decoder_begin_ragged: B=%d rows are no multiple of cfg.dec_n_group=%d", B, cfg->dec_n_group);
    for (int b = 0; b < B; ++b)
        WIPA_REQUIRE(starts_host[b] >= 0 && P - starts_host[b] >= 1, "wipa_decoder_begin_ragged: start[%d]=%d outside 0..P-1 (P=%d): a row holds 1..P tokens",
                     b, starts_host[b], P);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < P; ++t)
            WIPA_REQUIRE(tokens_host[(size_t)b * P + t] >= 0 && tokens_host[(size_t)b * P + t] < cfg->n_vocab,
                         "wipa_decoder_begin_ragged: tokens[%d][%d]=%d outside the vocabulary of %d", b, t, tokens_host[(size_t)b * P + t], cfg->n_vocab);
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits("wipa_decoder_begin_ragged", L, state_bytes));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    RT_CALL(begin_reset(cfg, st, L, B, s));
    // the rows as the caller packed them (row b's own tokens in columns [start[b], P)), and the starts the step's kernels read
    WIPA_CHECK_HIP(hipMemcpy2DAsync(st + L.tokens, (size_t)L.ld_tok * 4, tokens_host, (size_t)P * 4, (size_t)P * 4, (size_t)B, hipMemcpyHostToDevice, s));
    WIPA_CHECK_HIP(hipMemcpyAsync(starts_dev, starts_host, (size_t)B * 4, hipMemcpyHostToDevice, s));
    return WIPA_OK;
}

// `full` is the call's context as its last step sees it (lean = false); `who` names the entry point in the refusals.
static int decoder_run(const char* who, const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                       const StepCtx& full, int n_steps, int use_graph, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    // every step of the call but the LAST is "lean" when the logits projection carries the greedy partials: its logits are not
    // written (state.logits holds those of the last step of a call, which is what callers read)
    StepCtx lean = full;
    lean.lean = true;
    char* st = (char*)state;
    hipStream_t s = (hipStream_t)stream;
    wipa_dec_layout L;
    RT_CALL(decode_prologue(who, cfg, B, st, state_bytes, n_steps, s, &L, [&]() -> int { return decode_call_checks(who, cfg, w, state, B, full, n_steps, false); }));
    if (n_steps == 0) return WIPA_OK;
    W8Scope w8_scope(cfg, w);
    // the first step's input rows (embedding + first LayerNorm of the token at the current position): every later step gets
    // them from the previous step's last launch.  Outside the graph: once per call, whatever wrote the token (the greedy
    // update, the prompt, a forced history)
    if (step_needs_head(cfg, B)) RT_CALL(enqueue_step_head(cfg, w, st, L, B, full, stream));
    const bool lean_ok = lean_steps(cfg, B, full);
    if (!use_graph || !graphs_allowed()) {
        for (int i = 0; i < n_steps; ++i) RT_CALL(enqueue_decode_step(cfg, w, st, L, B, (lean_ok && i + 1 < n_steps) ? lean : full, stream));
        return WIPA_OK;
    }
    WIPA_REQUIRE(s != nullptr, "%s: graph capture needs a non-default stream", who);
    const int variant = step_variant(cfg, B, full);
    auto step_graph = [&](const StepCtx& c, hipGraphExec_t* out) -> int {  // kind 0: the full step, 2: the lean one
        return cached_graph(graph_key(cfg, w, state, B, c, variant, c.lean ? 2 : 0, nullptr), s,
                            [&]() -> int { return enqueue_decode_step(cfg, w, st, L, B, c, stream); }, out);
    };
    hipGraphExec_t full_exec = nullptr, lean_exec = nullptr;
    RT_CALL(step_graph(full, &full_exec));
    if (lean_ok && n_steps > 1) RT_CALL(step_graph(lean, &lean_exec));
    for (int i = 0; i < n_steps; ++i) WIPA_CHECK_HIP(hipGraphLaunch((lean_exec && i + 1 < n_steps) ? lean_exec : full_exec, s));
    return WIPA_OK;
}

extern "C" int wipa_decoder_run_ex(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                                   const wipa_decode_call* call, int n_steps, int use_graph, wipa_stream_t stream) {
    WIPA_REQUIRE(call, "wipa_decoder_run_ex: call is required");
    return decoder_run("wipa_decoder_run_ex", cfg, w, state, state_bytes, B, step_ctx(*call), n_steps, use_graph, stream);
}

extern "C" int wipa_decoder_run(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int n_init,
                                int eot, const float* mask_first, const float* mask_always, int n_steps, int use_graph,
                                wipa_stream_t stream) {
    const wipa_decode_call call = {n_init, eot, mask_first, mask_always};
    return wipa_decoder_run_ex(cfg, w, state, state_bytes, B, &call, n_steps, use_graph, stream);
}

extern "C" int wipa_decoder_prefill_ex(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                                       const wipa_decode_call* call, int use_graph, wipa_stream_t stream) {
    const char* who = "wipa_decoder_prefill_ex";
    WIPA_REQUIRE(call, "%s: call is required", who);
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    const StepCtx ctx = step_ctx(*call);
    char* st = (char*)state;
    hipStream_t s = (hipStream_t)stream;
    wipa_dec_layout L;
    RT_CALL(decode_prologue(who, cfg, B, st, state_bytes, 1, s, &L, [&]() -> int { return decode_call_checks(who, cfg, w, state, B, ctx, 1, true); }));
    W8Scope w8_scope(cfg, w);
    return replay_or_enqueue(use_graph, s, graph_key(cfg, w, state, B, ctx, step_variant(cfg, B, ctx), 1, nullptr), [&]() -> int {
        if (ctx.n_init == 1) {  // a bare [sot] prompt: one ordinary step at position 0 (with its head when the step is tail-fused)
            if (step_needs_head(cfg, B)) RT_CALL(enqueue_step_head(cfg, w, st, L, B, ctx, stream));
            return enqueue_decode_step(cfg, w, st, L, B, ctx, stream);
        }
        return enqueue_prefill(cfg, w, st, L, B, ctx, stream);
    });
}

extern "C" int wipa_decoder_prefill(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                                    int n_init, int eot, const float* mask_first, const float* mask_always, int use_graph,
                                    wipa_stream_t stream) {
    const wipa_decode_call call = {n_init, eot, mask_first, mask_always};
    return wipa_decoder_prefill_ex(cfg, w, state, state_bytes, B, &call, use_graph, stream);
}

extern "C" int wipa_decoder_graph_count(void) {
    std::lock_guard<std::mutex> lk(g_graph_mu);
    return (int)g_graphs.size();
}

extern "C" int wipa_decoder_adapt_cross(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                                        const void* features, int n_rows, const int32_t* slots_host, const wipa_adapter_bank* bank,
                                        wipa_stream_t stream) {
    const char* who = "wipa_decoder_adapt_cross";
    RT_CALL(cfg_check(cfg));
    WIPA_REQUIRE(w && state && features && bank && B > 0, "%s: weights, state, features and bank are required; B > 0", who);
    WIPA_REQUIRE(B % group_of(cfg) == 0, "%s: B=%d rows are no multiple of cfg.dec_n_group=%d", who, B, cfg->dec_n_group);
    RT_CALL(bank_servable(who, cfg, bank));
    const int G = group_of(cfg), Bc = clips_of(cfg, B);
    WIPA_REQUIRE(slots_host ? (n_rows >= 1 && n_rows <= Bc) : n_rows == Bc, "%s: n_rows=%d: %s", who, n_rows,
                 slots_host ? "1..B / cfg.dec_n_group listed slots" : "without slots_host every clip is adapted: B / cfg.dec_n_group");
    for (int i = 0; slots_host && i < n_rows; ++i)
        WIPA_REQUIRE(slots_host[i] >= 0 && slots_host[i] < Bc, "%s: slots_host[%d]=%d outside 0..%d", who, i, slots_host[i], Bc - 1);
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits(who, L, state_bytes));
    if (!bank_on(bank, SITE_CK) && !bank_on(bank, SITE_CV)) return WIPA_OK;
    const size_t e = wipa_dtype_size(cfg->dtype);
    const int d = cfg->n_text_state, H = cfg->n_text_head, Ta = cfg->n_audio_ctx, dt = cfg->dtype;
    const float scales[2] = {QK_SCALE, 1.f};  // the key half is scaled like cross_kv_gemm's
    wipa_gemm_desc g;  // cross_kv_gemm's addressing: [clip][K | V][H][Ta][64]
    memset(&g, 0, sizeof(g));
    g.rg_in = Ta; g.rg_stride = (int64_t)2 * H * Ta * 64;
    g.cg_in = 64; g.cg_stride = (int64_t)Ta * 64;
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        char* ckv = (char*)state + L.cross_kv + (size_t)l * Bc * 2 * H * Ta * 64 * e;
        if (!slots_host) {
            RT_CALL(bank_apply(bank, l, SITE_CK, 2, scales, features, d, dt, ckv, dt, 64, &g, Bc * Ta, d, 2 * d, Ta, G, bank->ids_dev, 0, stream));
            continue;
        }
        for (int i = 0; i < n_rows; ++i) {
            g.c_offset = (int64_t)slots_host[i] * g.rg_stride;
            RT_CALL(bank_apply(bank, l, SITE_CK, 2, scales, (const char*)features + (size_t)i * Ta * d * e, d, dt, ckv, dt, 64, &g, Ta, d, 2 * d, Ta,
                               1, bank->ids_dev + (size_t)slots_host[i] * G, 0, stream));
        }
    }
    return WIPA_OK;
}

// ------------------------------------------------------------------ continuous batching: slots, admission, column shift
namespace {

// one admitted clip: its initial tokens into columns [*pos, *pos + n_init) of the slot's row, the slot's start, limit and log-probability
// sum, and (with a sampling record) the Philox stream of its draws.  One thread; a column range that does not fit the table is not written.
__global__ void admit_row_kernel(int32_t* tokens, int64_t ld_tok, const int32_t* pos, int n_ctx, int slot, int B, int n_init, int t0, int t1,
                                 int t2, int t3, int limit, int32_t* starts, float* sum_logprobs, uint32_t* rec, uint32_t stream_lo,
                                 uint32_t stream_hi) {
    const int c = *pos;
    if (c < 0 || c + n_init >= n_ctx) return;
    const int first4[4] = {t0, t1, t2, t3};
    for (int t = 0; t < n_init; ++t) tokens[(int64_t)slot * ld_tok + c + t] = first4[t];
    starts[slot] = c;
    starts[B + slot] = limit;
    sum_logprobs[slot] = 0.f;
    if (rec) {
        rec[4 + 2 * slot] = stream_lo;
        rec[5 + 2 * slot] = stream_hi;
    }
}

// wipa_decoder_shift_columns, part 1: the bytes [shift * row_bytes, (*pos + 1) * row_bytes) of every strip move down by shift * row_bytes.
// Source and destination overlap; the ORDER makes it safe, no scratch: ONE workgroup owns a strip and walks it in ascending chunks of
// 256 x 16 bytes, every thread loads its 16 bytes of the chunk, the workgroup meets at a barrier, then every thread stores.  The
// destination lies below the source (shift > 0), so a chunk's stores end below the first byte of the next chunk's loads, and within a
// chunk every load precedes every store.  strip s of the grid starts at base + s * strip_bytes; row_bytes is a multiple of 16.
__global__ __launch_bounds__(256) void shift_rows_kernel(char* base, int64_t strip_bytes, int64_t row_bytes, const int32_t* pos, int n_ctx, int shift) {
    const int p = *pos;
    if (shift <= 0 || shift > p || p >= n_ctx) return;  // uniform; nothing is read or written outside the strip's n_ctx rows
    char* strip = base + (int64_t)blockIdx.x * strip_bytes;
    const int64_t n = (int64_t)(p + 1 - shift) * row_bytes, off = (int64_t)shift * row_bytes;
    for (int64_t c0 = 0; c0 < n; c0 += 256 * 16) {  // uniform trip count: the barrier is reached by all
        const int64_t i = c0 + (int64_t)threadIdx.x * 16;
        uint4 v = {0u, 0u, 0u, 0u};
        if (i < n) v = *reinterpret_cast<const uint4*>(strip + off + i);
        __syncthreads();
        if (i < n) *reinterpret_cast<uint4*>(strip + i) = v;
        __syncthreads();  // the next chunk's loads stay behind this chunk's stores (they touch disjoint bytes; kept for a plain proof)
    }
}
// part 2, the token columns (4-byte elements: a shift need not keep 16-byte alignment): one workgroup per row, the same order
__global__ __launch_bounds__(256) void shift_tokens_kernel(int32_t* tokens, int64_t ld_tok, const int32_t* pos, int n_ctx, int shift) {
    const int p = *pos;
    if (shift <= 0 || shift > p || p >= n_ctx) return;
    int32_t* row = tokens + (int64_t)blockIdx.x * ld_tok;
    const int n = p + 1 - shift;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + (int)threadIdx.x;
        int32_t v = 0;
        if (i < n) v = row[shift + i];
        __syncthreads();
        if (i < n) row[i] = v;
        __syncthreads();
    }
}
// part 3, after both: the position and the rows' starts.  A row whose start lies below the shift has left the table's window -- it was
// finished, or never admitted: start 0, limit 0 (it takes eot at every column).
__global__ void shift_finish_kernel(int32_t* pos, int64_t* posd, int d, int32_t* starts, int B, int n_ctx, int shift) {
    const int p = *pos;
    if (shift <= 0 || shift > p || p >= n_ctx) return;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int s0 = starts[b];
        starts[b] = max(s0 - shift, 0);
        if (s0 < shift) starts[B + b] = 0;
    }
    if (threadIdx.x == 0) {
        *pos = p - shift;
        *posd = (int64_t)(p - shift) * d;
    }
}

// what wipa_decoder_admit_rows and wipa_decoder_admit_rows_prompted refuse alike, before anything is enqueued
int admit_checks(const char* who, const wipa_model_cfg* cfg, const void* const* w, const void* state, int B, int n_rows, const int32_t* slots_host,
                 const void* const* features_host, const int32_t* initial_tokens_host, int n_init, const int32_t* limits_host,
                 const int32_t* starts_dev, const void* sample, const uint32_t* streams_host) {
    RT_CALL(continuous_servable(who, cfg, B, starts_dev));
    WIPA_REQUIRE(w && state && n_rows >= 0 && (n_rows == 0 || (slots_host && features_host && initial_tokens_host && limits_host)),
                 "%s: null pointer / bad row count", who);
    WIPA_REQUIRE(n_init >= 1 && n_init <= 4, "%s: 1..4 initial tokens per clip (got %d)", who, n_init);
    WIPA_REQUIRE(!sample || (streams_host && ((uintptr_t)sample % 4) == 0), "%s: a sampling record needs streams_host (uint32 [n_rows][2])", who);
    for (int i = 0; i < n_rows; ++i) {
        WIPA_REQUIRE(slots_host[i] >= 0 && slots_host[i] < B, "%s: slot[%d]=%d outside 0..%d", who, i, slots_host[i], B - 1);
        for (int j = 0; j < i; ++j) WIPA_REQUIRE(slots_host[j] != slots_host[i], "%s: slot %d is listed twice", who, slots_host[i]);
        WIPA_REQUIRE(features_host[i], "%s: features[%d] is null", who, i);
        WIPA_REQUIRE(limits_host[i] >= 0 && limits_host[i] <= cfg->n_text_ctx, "%s: limit[%d]=%d outside 0..n_text_ctx", who, i, limits_host[i]);
        for (int t = 0; t < n_init; ++t)
            WIPA_REQUIRE(initial_tokens_host[i * n_init + t] >= 0 && initial_tokens_host[i * n_init + t] < cfg->n_vocab,
                         "%s: initial token [%d][%d]=%d outside the vocabulary of %d", who, i, t, initial_tokens_host[i * n_init + t], cfg->n_vocab);
    }
    WIPA_REQUIRE(cfg->n_audio_state == cfg->n_text_state, "encoder/decoder widths differ");
    return WIPA_OK;
}

// one admitted clip's cross-attention input into its slot of the blob
int admit_cross(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, int slot, const void* features,
                wipa_stream_t stream) {
    const size_t e = wipa_dtype_size(cfg->dtype);
    const int d = cfg->n_text_state, H = cfg->n_text_head, Ta = cfg->n_audio_ctx;
    const size_t clip_bytes = (size_t)Ta * d * e;
    if (cfg->dec_cross_absorbed) {  // the steps stream the encoder output itself: an admission is a copy
        WIPA_CHECK_HIP(hipMemcpyAsync(st + L.cross_kv + (size_t)slot * clip_bytes, features, clip_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return WIPA_OK;
    }
    // the cached form: wipa_decoder_set_audio's projection for this clip alone, into the slot's K / V of every layer
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        const void* const* lw = w + WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l;
        RT_CALL(cross_kv_gemm(cfg, lw, features, st + L.cross_kv + ((size_t)l * B + slot) * 2 * H * Ta * 64 * e, 1, stream));
    }
    return WIPA_OK;
}

// wipa_decoder_seek: the position of an idle state, and the element offset (column * d) the q|k|v GEMM of a step scatters at
__global__ void seek_kernel(int32_t* pos, int64_t* posd, int d, int column) {
    *pos = column;
    *posd = (int64_t)column * d;
}

// wipa_decoder_admit_rows_prompted.  meta is int32 [n_rows][ADMIT_META]: slot, prompt columns L, limit, the four initial tokens, the
// Philox stream (lo, hi); ptok int32 [n_rows][W] holds the prompts right-aligned.  With c = *pos, row i's prompt goes to columns
// [c - L, c) of its slot, its initial tokens to [c, c + n_init), and starts[slot], starts[B + slot], starts[2 B + slot] take c - L, the
// limit and L.  One workgroup per admitted row.  An admission without room -- c - W < 0, or no column left to generate -- is not carried
// out: the same test stands in scatter_prompt_kv_kernel, so a row is admitted with its K / V or not at all.
constexpr int ADMIT_META = 12;
__device__ __forceinline__ bool admission_fits(int c, int W, int n_init, int n_ctx) { return c - W >= 0 && c + n_init < n_ctx; }

__global__ __launch_bounds__(256) void admit_rows_prompted_kernel(int32_t* tokens, int64_t ld_tok, const int32_t* pos, int n_ctx, int B, int n_init,
                                                                  int W, const int32_t* __restrict__ meta, const int32_t* __restrict__ ptok,
                                                                  int32_t* starts, float* sum_logprobs, uint32_t* rec) {
    const int c = *pos;
    if (!admission_fits(c, W, n_init, n_ctx)) return;
    const int32_t* m = meta + (int64_t)blockIdx.x * ADMIT_META;
    const int slot = m[0], L = m[1];
    int32_t* tk = tokens + (int64_t)slot * ld_tok;
    for (int j = threadIdx.x; j < L; j += blockDim.x) tk[c - L + j] = ptok[(int64_t)blockIdx.x * W + (W - L) + j];
    if (threadIdx.x == 0) {
        for (int t = 0; t < n_init; ++t) tk[c + t] = m[3 + t];
        starts[slot] = c - L;
        starts[B + slot] = m[2];
        starts[2 * B + slot] = L;
        sum_logprobs[slot] = 0.f;
        if (rec) {
            rec[4 + 2 * slot] = (uint32_t)m[7];
            rec[5 + 2 * slot] = (uint32_t)m[8];
        }
    }
}

// The prompt pass left a layer's q|k|v in packed rows [n_rows * W][3 d]; the K and V rows j >= W - L_i of row i go to columns
// [c - L_i, c) of the slot's K and V strips of that layer, skv [3][B][n_ctx][d] (c = *pos).  Workgroup (i, K | V) owns one strip;
// 16-byte plain loads and stores, row_bytes = d * element size is a multiple of 16.
__global__ __launch_bounds__(256) void scatter_prompt_kv_kernel(const char* __restrict__ qkv, char* __restrict__ skv, const int32_t* __restrict__ meta,
                                                                const int32_t* pos, int n_ctx, int n_init, int W, int B, int64_t row_bytes) {
    const int c = *pos;
    if (!admission_fits(c, W, n_init, n_ctx)) return;
    const int i = blockIdx.x, part = 1 + (int)blockIdx.y;  // 1: K, 2: V
    const int slot = meta[(int64_t)i * ADMIT_META], L = meta[(int64_t)i * ADMIT_META + 1];
    const char* src = qkv + ((int64_t)i * W + (W - L)) * 3 * row_bytes + part * row_bytes;
    char* dst = skv + (((int64_t)part * B + slot) * n_ctx + (c - L)) * row_bytes;
    const int per_row = (int)(row_bytes / 16), total = L * per_row;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int r = idx / per_row, o = idx - r * per_row;
        *reinterpret_cast<uint4*>(dst + (int64_t)r * row_bytes + o * 16) = *reinterpret_cast<const uint4*>(src + (int64_t)r * 3 * row_bytes + o * 16);
    }
}

}  // namespace

extern "C" int wipa_decoder_admit_rows(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int n_rows,
                                       const int32_t* slots_host,
                                       const void* const* features_host, const int32_t* initial_tokens_host, int n_init,
                                       const int32_t* limits_host, int32_t* starts_dev, void* sample, const uint32_t* streams_host,
                                       wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    const char* who = "wipa_decoder_admit_rows";
    RT_CALL(admit_checks(who, cfg, w, state, B, n_rows, slots_host, features_host, initial_tokens_host, n_init, limits_host, starts_dev, sample,
                         streams_host));
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits(who, L, state_bytes));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    for (int i = 0; i < n_rows; ++i) {
        const int slot = slots_host[i];
        RT_CALL(admit_cross(cfg, w, st, L, B, slot, features_host[i], stream));
        int t4[4] = {0, 0, 0, 0};
        for (int t = 0; t < n_init; ++t) t4[t] = initial_tokens_host[i * n_init + t];
        hipLaunchKernelGGL(admit_row_kernel, dim3(1), dim3(1), 0, s, (int32_t*)(st + L.tokens), L.ld_tok, (const int32_t*)(st + L.pos),
                           cfg->n_text_ctx, slot, B, n_init, t4[0], t4[1], t4[2], t4[3], limits_host[i], starts_dev, (float*)(st + L.sum_logprobs),
                           (uint32_t*)sample, sample ? streams_host[2 * i] : 0u, sample ? streams_host[2 * i + 1] : 0u);
        WIPA_LAUNCH_CHECK();
    }
    return WIPA_OK;
}

extern "C" int wipa_decoder_shift_columns(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, int32_t* starts_dev, int shift,
                                          wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    const char* who = "wipa_decoder_shift_columns";
    RT_CALL(continuous_servable(who, cfg, B, starts_dev));
    WIPA_REQUIRE(state && shift >= 1 && shift < cfg->n_text_ctx, "%s: shift=%d outside 1..n_text_ctx-1", who, shift);
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits(who, L, state_bytes));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    const size_t e = wipa_dtype_size(cfg->dtype);
    const int d = cfg->n_text_state, nctx = cfg->n_text_ctx;
    const int64_t row_bytes = (int64_t)d * e, strip_bytes = (int64_t)nctx * row_bytes, slot = (int64_t)B * strip_bytes;
    WIPA_REQUIRE(row_bytes % 16 == 0, "%s: a K / V row of %lld bytes is no multiple of 16", who, (long long)row_bytes);
    const int32_t* pos = (const int32_t*)(st + L.pos);
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        char* skv = st + L.self_kv + (size_t)l * 3 * slot;  // [3][B][nctx][d]: the query slot holds nothing a later step reads
        hipLaunchKernelGGL(shift_rows_kernel, dim3(2 * B), dim3(256), 0, s, skv + slot, strip_bytes, row_bytes, pos, nctx, shift);  // K then V: 2 B strips
    }
    hipLaunchKernelGGL(shift_tokens_kernel, dim3(B), dim3(256), 0, s, (int32_t*)(st + L.tokens), L.ld_tok, pos, nctx, shift);
    hipLaunchKernelGGL(shift_finish_kernel, dim3(1), dim3(256), 0, s, (int32_t*)(st + L.pos), (int64_t*)(st + L.scratch + dec_scratch(cfg, B).posd), d,
                       starts_dev, B, nctx, shift);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

// ------------------------------------------------------------------ ragged prompt pass
// The whole prompt of every row (up to n_text_ctx columns, rows left-padded to the common width P) in ONE batched pass: the existing
// prefill is sized for four rows per clip and runs one absorbed cross-attention launch per prompt position, neither of which scales
// to P = 227.  This pass and the teacher-forced one (tf_layers) are ONE layer walk, batched_layers: batched GEMMs over B * P rows,
// wipa_attention for both attentions.  Here it runs with what a decode state needs: the q|k|v GEMM scatters into the blob's self-K/V
// cache at columns 0 .. P-1 (as enqueue_prefill does), embedding and self-attention take the rows' starts, the cross K/V come from the
// blob (cached form) or are projected per layer from the blob's copy of the encoder output (absorbed form), and logits exist for two
// columns per clip only.
namespace {
struct PromptWs {
    size_t sot_logits, x, ln, q, ao, h, ckv, total;
};
PromptWs prompt_ws(const wipa_model_cfg* c, int B, int P) {
    const size_t e = wipa_dtype_size(c->dtype), d = c->n_text_state, M = (size_t)B * P;
    PromptWs w;
    size_t o = 0;
    w.sot_logits = o; o += align256((size_t)B * round_up(c->n_vocab, 8) * 4);  // first: the caller reads it at offset 0
    w.x = o;   o += align256(M * d * 4);
    w.ln = o;  o += align256(M * d * e);
    w.q = o;   o += align256(M * d * e);
    w.ao = o;  o += align256(M * d * e);
    w.h = o;   o += align256(M * 4 * d * e);
    w.ckv = o; o += c->dec_cross_absorbed ? align256((size_t)clips_of(c, B) * 2 * c->n_text_head * c->n_audio_ctx * 64 * e) : 0;  // per clip
    w.total = o;
    return w;
}

// what wipa_decoder_align does between a layer's cross-attention projections and its cross-attention
struct TfHook {
    virtual int after_cross_projections(int layer, const void* q, const void* ckv, int64_t k_bs, int64_t k_hs) const = 0;
    virtual ~TfHook() {}
};

// what wipa_decoder_admit_rows_prompted does behind a layer's q|k|v GEMM (qkv: where the layer's q|k|v went)
struct QkvHook {
    virtual int after_qkv(int layer, const char* qkv) const = 0;
    virtual ~QkvHook() {}
};

// The batched decoder-layer walk over B * T rows (T columns per row): embedding, then per layer LayerNorm, q|k|v GEMM, causal
// self-attention, out GEMM with residual, LayerNorm, query GEMM, cross K / V projection, cross-attention, out GEMM, LayerNorm and the
// two MLP GEMMs.  Leaves the residual stream in x.  Its callers, the teacher-forced pass (tf_layers) and the ragged prompt pass
// (enqueue_prefill_ragged), differ in the first five numbered places; the prompt pass of an admission (wipa_decoder_admit_rows_prompted) adds the sixth.
struct BatchedWalk {
    int B, T;
    const int32_t* tokens;  // [B, ld_tok]
    int64_t ld_tok;
    float* x;               // workspace: x f32 [B * T, d]; ln, q, ao [B * T, d] and hb [B * T, 4 d] in the model dtype
    char* ln;
    void *q, *ao, *hb;
    char* qkv;              // 1. q|k|v land in packed rows [B * T, 3 d] of the workspace, or (NULL) are scattered into the blob's
    char* self_kv;          //    self-K/V cache [layer][3][B][nctx][d] at columns 0 .. T-1, as enqueue_prefill does
    const int32_t* starts;  // 2. NULL, or the rows' first own columns: embedding and self-attention are the `starts`-aware ones
    const void* features;   // 3. the cross K / V are projected per layer from features [clips, n_audio_ctx, d] into ckv_ws, or (NULL)
    char* ckv_ws;           //    read from the blob's cached K / V, [layer][clips][2][H][n_audio_ctx][64]
    const char* ckv_cache;
    int n_group;            // 4. candidate groups: rows = clips x n_group; the cross-attention takes a clip's candidates together
    const TfHook* hook;     // 5. NULL, or what runs between the cross projections and the cross-attention
    const QkvHook* qkv_hook;  // 6. NULL, or what runs behind a layer's q|k|v GEMM; with kv_only the walk is wanted for the K / V of its
    bool kv_only;             //    columns alone, and the last layer stops there (nothing reads what lies behind)
    const wipa_adapter_bank* bank;  // 7. NULL, or an adapter bank: one wipa_lora_bank_apply behind every targeted GEMM, row b of the walk
    const int32_t* ids;             //    (all its T columns) under the adapter ids[b * ids_stride]; residual sites add into x itself
    int ids_stride;
};
int batched_layers(const wipa_model_cfg* cfg, const void* const* w, const BatchedWalk& k, wipa_stream_t stream) {
    const int dt = cfg->dtype;
    const size_t e = wipa_dtype_size(dt);
    const int d = cfg->n_text_state, H = cfg->n_text_head, nctx = cfg->n_text_ctx, Ta = cfg->n_audio_ctx;
    const int B = k.B, T = k.T, M = B * T, G = k.n_group, Bc = B / G;
    float* x = k.x;
    char* ln = k.ln;
    void *q = k.q, *ao = k.ao, *hb = k.hb;
    const wipa_adapter_bank* bk = k.bank;
    if (k.starts) RT_CALL(wipa_embed_tokens_ragged(k.tokens, k.ld_tok, B, T, k.starts, w[0], dt, (const float*)w[1], x, d, stream));
    else RT_CALL(wipa_embed_tokens(k.tokens, k.ld_tok, B, T, 0, nullptr, w[0], dt, nullptr, (const float*)w[1], x, d, stream));
    for (int l = 0; l < cfg->n_text_layer; ++l) {
        const void* const* lw = w + WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * l;
        // q, k and v of a row lie `part` bytes apart: side by side in a packed row, or a cache slot [B][nctx][d] apart
        char* qkv = k.qkv ? k.qkv : k.self_kv + (size_t)l * 3 * B * nctx * d * e;
        const size_t part = k.qkv ? (size_t)d * e : (size_t)B * nctx * d * e;
        const int64_t qkv_rs = k.qkv ? 3 * d : d, qkv_bs = k.qkv ? (int64_t)T * 3 * d : (int64_t)nctx * d;
        RT_CALL(wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)lw[0], (const float*)lw[1], M, d, 1e-5f, stream));
        {
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.col_scale_n = 2 * d; g.col_scale = QK_SCALE;
            if (!k.qkv) {  // columns 0..T-1 -> slot[n / d][b][t][n % d] of the blob's cache
                g.rg_in = T; g.rg_valid = T; g.rg_stride = (int64_t)nctx * d;
                g.cg_in = d; g.cg_stride = (int64_t)B * nctx * d;
            }
            RT_CALL(gemm(ln, d, lw[2], d, qkv, qkv_rs, M, 3 * d, d, dt, dt, (const float*)lw[3], 0, nullptr, stream, &g));
            if (bk) RT_CALL(bank_apply(bk, l, SITE_Q, 3, SCALES_QKV, ln, d, dt, qkv, dt, qkv_rs, k.qkv ? nullptr : &g, M, d, 3 * d, T, k.ids_stride, k.ids, 0, stream));
        }
        if (k.qkv_hook) RT_CALL(k.qkv_hook->after_qkv(l, qkv));
        if (k.kv_only && l + 1 == cfg->n_text_layer) break;
        {
            wipa_attn_desc a;
            memset(&a, 0, sizeof(a));
            a.q = qkv; a.k = qkv + part; a.v = qkv + 2 * part; a.out = ao;
            a.q_bs = qkv_bs; a.q_rs = qkv_rs; a.q_hs = 64;
            a.k_bs = a.q_bs; a.k_rs = qkv_rs; a.k_hs = 64;
            a.v_bs = a.q_bs; a.v_rs = qkv_rs; a.v_hs = 64;
            a.o_bs = (int64_t)T * d; a.o_rs = d; a.o_hs = 64;
            a.B = B; a.H = H; a.Tq = T; a.Tk = T; a.causal = 1; a.dtype = dt;
            if (k.starts) RT_CALL(wipa_attention_ragged(&a, k.starts, stream));  // row b: column i sees columns starts[b] .. i
            else RT_CALL(wipa_attention(&a, stream));
        }
        RT_CALL(gemm(ao, d, lw[4], d, x, d, M, d, d, dt, WIPA_F32, (const float*)lw[5], 0, x, stream));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_O, 1, SCALE_ONE, ao, d, dt, x, WIPA_F32, d, nullptr, M, d, d, T, k.ids_stride, k.ids, 0, stream));
        RT_CALL(wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)lw[6], (const float*)lw[7], M, d, 1e-5f, stream));
        {
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.col_scale_n = d; g.col_scale = QK_SCALE;
            RT_CALL(gemm(ln, d, lw[8], d, q, d, M, d, d, dt, dt, (const float*)lw[9], 0, nullptr, stream, &g));
            if (bk) RT_CALL(bank_apply(bk, l, SITE_CQ, 1, SCALES_QKV, ln, d, dt, q, dt, d, nullptr, M, d, d, T, k.ids_stride, k.ids, 0, stream));
        }
        const int64_t ckv_bs = (int64_t)2 * H * Ta * 64, ckv_hs = (int64_t)Ta * 64;
        const char* ckv = k.ckv_ws;
        if (k.features) {
            wipa_gemm_desc g;
            memset(&g, 0, sizeof(g));
            g.col_scale_n = d; g.col_scale = QK_SCALE;  // the key half; values stay unscaled
            g.rg_in = Ta; g.rg_valid = Ta; g.rg_stride = ckv_bs;
            g.cg_in = 64; g.cg_stride = ckv_hs;
            RT_CALL(gemm(k.features, d, lw[10], d, k.ckv_ws, 64, Bc * Ta, 2 * d, d, dt, dt, (const float*)lw[11], 0, nullptr, stream, &g));
            // a clip's id is that of its first row (a cached K / V of the blob carries its terms already: wipa_decoder_adapt_cross)
            if (bk) RT_CALL(bank_apply(bk, l, SITE_CK, 2, SCALES_QKV + 1, k.features, d, dt, k.ckv_ws, dt, 64, &g, Bc * Ta, d, 2 * d, Ta, k.ids_stride * G, k.ids, 0, stream));
        } else {
            ckv = k.ckv_cache + (size_t)l * Bc * ckv_bs * e;
        }
        if (k.hook) RT_CALL(k.hook->after_cross_projections(l, q, ckv, ckv_bs, ckv_hs));
        {
            wipa_attn_desc a;
            memset(&a, 0, sizeof(a));
            a.q = q; a.k = ckv; a.v = ckv + (size_t)H * Ta * 64 * e; a.out = ao;
            a.q_bs = (int64_t)T * d; a.q_rs = d; a.q_hs = 64;
            a.k_bs = ckv_bs; a.k_rs = 64; a.k_hs = ckv_hs;
            a.v_bs = a.k_bs; a.v_rs = 64; a.v_hs = a.k_hs;
            a.o_bs = (int64_t)T * d; a.o_rs = d; a.o_hs = 64;
            a.B = B; a.H = H; a.Tq = T; a.Tk = Ta; a.causal = 0; a.dtype = dt;
            if (G > 1) {
                // candidate groups: the G x T query rows of a clip's candidates are contiguous -- one batch entry per CLIP holds them
                // all against the clip's K / V, on the kernel T rows take (every query row's arithmetic is its own)
                a.B = Bc; a.Tq = G * T;
                a.q_bs = (int64_t)G * T * d; a.o_bs = a.q_bs;
                RT_CALL(wipa_attention_as(&a, T, stream));
            } else {
                RT_CALL(wipa_attention(&a, stream));
            }
        }
        RT_CALL(gemm(ao, d, lw[12], d, x, d, M, d, d, dt, WIPA_F32, (const float*)lw[13], 0, x, stream));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_CO, 1, SCALE_ONE, ao, d, dt, x, WIPA_F32, d, nullptr, M, d, d, T, k.ids_stride, k.ids, 0, stream));
        RT_CALL(wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)lw[14], (const float*)lw[15], M, d, 1e-5f, stream));
        const bool mlp1_bank = bank_on(bk, SITE_MLP1);  // as in enqueue_step: the apply call performs the GELU
        RT_CALL(gemm(ln, d, lw[16], d, hb, 4 * d, M, 4 * d, d, dt, dt, (const float*)lw[17], mlp1_bank ? 0 : 1, nullptr, stream));
        if (mlp1_bank) RT_CALL(bank_apply(bk, l, SITE_MLP1, 1, SCALE_ONE, ln, d, dt, hb, dt, 4 * d, nullptr, M, d, 4 * d, T, k.ids_stride, k.ids, 1, stream));
        RT_CALL(gemm(hb, 4 * d, lw[18], 4 * d, x, d, M, d, 4 * d, dt, WIPA_F32, (const float*)lw[19], 0, x, stream));
        if (bk) RT_CALL(bank_apply(bk, l, SITE_MLP2, 1, SCALE_ONE, hb, 4 * d, dt, x, WIPA_F32, d, nullptr, M, 4 * d, d, T, k.ids_stride, k.ids, 0, stream));
    }
    return WIPA_OK;
}

int enqueue_prefill_ragged(const wipa_model_cfg* cfg, const void* const* w, char* st, const wipa_dec_layout& L, int B, int sot_col,
                           const StepCtx& ctx, char* ws, const PromptWs& W, wipa_stream_t stream) {
    const int dt = cfg->dtype;
    const size_t e = wipa_dtype_size(dt);
    const int d = cfg->n_text_state, P = ctx.n_init, M = B * P;
    BatchedWalk k = {};
    k.B = B; k.T = P;
    k.tokens = (const int32_t*)(st + L.tokens); k.ld_tok = L.ld_tok;
    k.x = (float*)(ws + W.x); k.ln = ws + W.ln; k.q = ws + W.q; k.ao = ws + W.ao; k.hb = ws + W.h;
    k.self_kv = st + L.self_kv;
    k.starts = ctx.starts;
    // absorbed form: the blob holds the encoder output itself (per clip); every layer's K / V are projected from it into the workspace
    if (cfg->dec_cross_absorbed) { k.features = st + L.cross_kv; k.ckv_ws = ws + W.ckv; }
    else k.ckv_cache = st + L.cross_kv;
    k.n_group = group_of(cfg);
    if (ctx.bank) { k.bank = ctx.bank; k.ids = ctx.bank->ids_dev; k.ids_stride = 1; }
    RT_CALL(batched_layers(cfg, w, k, stream));
    RT_CALL(wipa_layernorm(k.x, WIPA_F32, d, k.ln, dt, d, (const float*)w[2], (const float*)w[3], M, d, 1e-5f, stream));
    // logits of two columns per clip: the last prompt column (rows (b, P-1) of ln, row stride P * d) into the state, and the
    // <|startoftranscript|> column into the workspace (upstream's logits[:, sot_index], for no_speech_prob)
    RT_CALL(gemm(k.ln + (size_t)(P - 1) * d * e, (int64_t)P * d, w[0], d, st + L.logits, L.ld_logits, B, cfg->n_vocab, d, dt, WIPA_F32, nullptr, 0,
                 nullptr, stream));
    if (sot_col >= 0)
        RT_CALL(gemm(k.ln + (size_t)sot_col * d * e, (int64_t)P * d, w[0], d, ws + W.sot_logits, L.ld_logits, B, cfg->n_vocab, d, dt, WIPA_F32,
                     nullptr, 0, nullptr, stream));
    return enqueue_first_token(cfg, st, L, B, ctx, stream);
}
}  // namespace

extern "C" size_t wipa_decoder_prompt_workspace_bytes(const wipa_model_cfg* cfg, int B, int P) {
    if (!cfg || !audio_ctx_ok(cfg) || B <= 0 || P <= 0) return 0;
    return prompt_ws(cfg, B, P).total;
}

static int prefill_ragged(const char* who, const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int P,
                          int sot_col, int eot, const float* mask_first, const float* mask_always, int use_graph,
                          const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev, void* workspace,
                          size_t workspace_bytes, const wipa_adapter_bank* bank, wipa_stream_t stream);
extern "C" int wipa_decoder_prefill_ragged(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int P,
                                           int sot_col, int eot, const float* mask_first, const float* mask_always, int use_graph,
                                           const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev, void* workspace,
                                           size_t workspace_bytes, wipa_stream_t stream) {
    return prefill_ragged("wipa_decoder_prefill_ragged", cfg, w, state, state_bytes, B, P, sot_col, eot, mask_first, mask_always, use_graph, rules,
                          sample, starts_dev, workspace, workspace_bytes, nullptr, stream);
}
extern "C" int wipa_decoder_prefill_ragged_bank(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int P,
                                                int sot_col, int eot, const float* mask_first, const float* mask_always, int use_graph,
                                                const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev,
                                                void* workspace, size_t workspace_bytes, const wipa_adapter_bank* bank, wipa_stream_t stream) {
    return prefill_ragged("wipa_decoder_prefill_ragged_bank", cfg, w, state, state_bytes, B, P, sot_col, eot, mask_first, mask_always, use_graph,
                          rules, sample, starts_dev, workspace, workspace_bytes, bank, stream);
}
static int prefill_ragged(const char* who, const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int P,
                          int sot_col, int eot, const float* mask_first, const float* mask_always, int use_graph,
                          const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev, void* workspace,
                          size_t workspace_bytes, const wipa_adapter_bank* bank, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(w && state && mask_first && mask_always && B > 0, "wipa_decoder_prefill_ragged: bad arguments");
    WIPA_REQUIRE(starts_dev && workspace, "wipa_decoder_prefill_ragged: starts_dev and workspace are required");
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "wipa_decoder_prefill_ragged: the prompt pass runs on a bf16 / f32 weight table (cfg.dec_w_dtype: fp8 tables "
                                        "serve the decode step)");
    StepCtx ctx{rules, sample, starts_dev, P, eot, mask_first, mask_always, false};
    ctx.bank = bank;
    char* st = (char*)state;
    hipStream_t s = (hipStream_t)stream;
    wipa_dec_layout L;
    const PromptWs W = prompt_ws(cfg, B, P);  // offsets only: nothing is touched before the checks
    RT_CALL(decode_prologue(who, cfg, B, st, state_bytes, 1, s, &L, [&]() -> int {
        RT_CALL(step_servable(who, cfg, B, ctx));
        WIPA_REQUIRE(P + 1 <= cfg->n_text_ctx, "wipa_decoder_prefill_ragged: P=%d leaves no column to generate in n_text_ctx=%d", P, cfg->n_text_ctx);
        WIPA_REQUIRE(sot_col >= -1 && sot_col < P, "wipa_decoder_prefill_ragged: sot_col=%d outside -1..P-1 (P=%d)", sot_col, P);
        WIPA_REQUIRE(workspace_bytes >= W.total, "wipa_decoder_prefill_ragged: workspace too small (%zu < %zu: wipa_decoder_prompt_workspace_bytes)",
                     workspace_bytes, W.total);
        return WIPA_OK;
    }));
    // the prompt pass has its own, shorter variant word
    const int variant = cfg->dtype * 2 + t_f32_split + 64 * cfg->dec_cross_absorbed + 256 * (group_of(cfg) > 1 ? group_of(cfg) : 0);
    return replay_or_enqueue(use_graph, s, graph_key(cfg, w, state, B, ctx, variant, 3 + 16 * (sot_col + 1), workspace), [&]() -> int {
        return enqueue_prefill_ragged(cfg, w, st, L, B, sot_col, ctx, (char*)workspace, W, stream);
    });
}

// ------------------------------------------------------------------ continuous batching with a prompt per row
namespace {
struct AdmitWs {
    size_t meta, tokens, starts, feat, x, ln, qkv, q, ao, h, ckv, total;
};
AdmitWs admit_ws(const wipa_model_cfg* c, int n_rows, int W) {
    const size_t e = wipa_dtype_size(c->dtype), d = c->n_text_state, M = (size_t)n_rows * W;
    AdmitWs w;
    size_t o = 0;
    w.meta = o;   o += align256((size_t)n_rows * ADMIT_META * 4);
    w.tokens = o; o += align256(M * 4);
    w.starts = o; o += align256((size_t)n_rows * 4);
    w.feat = w.x = w.ln = w.qkv = w.q = w.ao = w.h = w.ckv = o;
    if (W > 0) {  // the prompt pass
        w.feat = o; o += align256((size_t)n_rows * c->n_audio_ctx * d * e);
        w.x = o;    o += align256(M * d * 4);
        w.ln = o;   o += align256(M * d * e);
        w.qkv = o;  o += align256(M * 3 * d * e);
        w.q = o;    o += align256(M * d * e);
        w.ao = o;   o += align256(M * d * e);
        w.h = o;    o += align256(M * 4 * d * e);
        w.ckv = o;  o += align256((size_t)n_rows * 2 * c->n_text_head * c->n_audio_ctx * 64 * e);
    }
    w.total = o;
    return w;
}
struct ScatterHook : QkvHook {
    const wipa_model_cfg* cfg;
    char* self_kv;
    const int32_t *meta, *pos;
    int n_rows, W, B, n_init;
    hipStream_t s;
    int after_qkv(int layer, const char* qkv) const override {
        const int64_t row_bytes = (int64_t)cfg->n_text_state * wipa_dtype_size(cfg->dtype);
        char* skv = self_kv + (size_t)layer * 3 * B * cfg->n_text_ctx * row_bytes;
        hipLaunchKernelGGL(scatter_prompt_kv_kernel, dim3(n_rows, 2), dim3(256), 0, s, qkv, skv, meta, pos, cfg->n_text_ctx, n_init, W, B, row_bytes);
        WIPA_LAUNCH_CHECK();
        return WIPA_OK;
    }
};
}  // namespace

extern "C" int wipa_decoder_seek(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, int column, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    const char* who = "wipa_decoder_seek";
    WIPA_REQUIRE(state && B > 0, "%s: null pointer / bad batch", who);
    WIPA_REQUIRE(column >= 0 && column < cfg->n_text_ctx - 1, "%s: column=%d outside 0..n_text_ctx-2", who, column);
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits(who, L, state_bytes));
    char* st = (char*)state;
    hipLaunchKernelGGL(seek_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int32_t*)(st + L.pos), (int64_t*)(st + L.scratch + dec_scratch(cfg, B).posd),
                       cfg->n_text_state, column);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

extern "C" size_t wipa_decoder_admit_prompted_workspace_bytes(const wipa_model_cfg* cfg, int n_rows, int W) {
    if (!cfg || !audio_ctx_ok(cfg) || n_rows <= 0 || W < 0) return 0;
    return admit_ws(cfg, n_rows, W).total;
}

static int admit_rows_prompted(const char* who, const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                               int n_rows, const int32_t* slots_host, const void* const* features_host, const int32_t* initial_tokens_host,
                               int n_init, const int32_t* limits_host, const int32_t* prompt_lens_host, const int32_t* prompt_tokens_host,
                               int W, int32_t* starts_dev, void* sample, const uint32_t* streams_host, void* workspace,
                               size_t workspace_bytes, const wipa_adapter_bank* bank, const int32_t* ids_host, wipa_stream_t stream);
extern "C" int wipa_decoder_admit_rows_prompted(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int n_rows,
                                                const int32_t* slots_host, const void* const* features_host,
                                                const int32_t* initial_tokens_host, int n_init, const int32_t* limits_host,
                                                const int32_t* prompt_lens_host, const int32_t* prompt_tokens_host, int W, int32_t* starts_dev,
                                                void* sample, const uint32_t* streams_host, void* workspace, size_t workspace_bytes,
                                                wipa_stream_t stream) {
    return admit_rows_prompted("wipa_decoder_admit_rows_prompted", cfg, w, state, state_bytes, B, n_rows, slots_host, features_host,
                               initial_tokens_host, n_init, limits_host, prompt_lens_host, prompt_tokens_host, W, starts_dev, sample, streams_host,
                               workspace, workspace_bytes, nullptr, nullptr, stream);
}
extern "C" int wipa_decoder_admit_rows_prompted_bank(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                                                     int n_rows, const int32_t* slots_host, const void* const* features_host,
                                                     const int32_t* initial_tokens_host, int n_init, const int32_t* limits_host,
                                                     const int32_t* prompt_lens_host, const int32_t* prompt_tokens_host, int W,
                                                     int32_t* starts_dev, void* sample, const uint32_t* streams_host, void* workspace,
                                                     size_t workspace_bytes, const wipa_adapter_bank* bank, const int32_t* ids_host,
                                                     wipa_stream_t stream) {
    const char* who = "wipa_decoder_admit_rows_prompted_bank";
    WIPA_REQUIRE(bank && (ids_host || n_rows == 0), "%s: bank and ids_host (int32 [n_rows]: the admitted clips' adapters, -1 for none) are required", who);
    return admit_rows_prompted(who, cfg, w, state, state_bytes, B, n_rows, slots_host, features_host, initial_tokens_host, n_init, limits_host,
                               prompt_lens_host, prompt_tokens_host, W, starts_dev, sample, streams_host, workspace, workspace_bytes, bank,
                               ids_host, stream);
}
static int admit_rows_prompted(const char* who, const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                               int n_rows, const int32_t* slots_host, const void* const* features_host, const int32_t* initial_tokens_host,
                               int n_init, const int32_t* limits_host, const int32_t* prompt_lens_host, const int32_t* prompt_tokens_host,
                               int W, int32_t* starts_dev, void* sample, const uint32_t* streams_host, void* workspace,
                               size_t workspace_bytes, const wipa_adapter_bank* bank, const int32_t* ids_host, wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    RT_CALL(bank_servable(who, cfg, bank));
    WIPA_REQUIRE(starts_dev, "%s: starts_dev (int32 [3][B]: window starts, token limits, prompt columns) is required", who);
    RT_CALL(admit_checks(who, cfg, w, state, B, n_rows, slots_host, features_host, initial_tokens_host, n_init, limits_host, starts_dev, sample,
                         streams_host));
    const int L_max = cfg->n_text_ctx - n_init - 1;
    WIPA_REQUIRE(W >= 0 && W <= L_max && (n_rows == 0 || prompt_lens_host) && (W == 0 || n_rows == 0 || prompt_tokens_host),
                 "%s: prompt width W=%d outside 0..%d (n_text_ctx - n_init - 1), or null prompt arrays", who, W, L_max);
    for (int i = 0; i < n_rows; ++i) {
        const int Li = prompt_lens_host[i];
        WIPA_REQUIRE(Li >= 0 && Li <= L_max, "%s: prompt length L[%d]=%d outside 0..%d (n_text_ctx - n_init - 1)", who, i, Li, L_max);
        WIPA_REQUIRE(Li <= W, "%s: prompt length L[%d]=%d exceeds the width W=%d of the prompt array", who, i, Li, W);
        for (int j = W - Li; j < W; ++j)
            WIPA_REQUIRE(prompt_tokens_host[(size_t)i * W + j] >= 0 && prompt_tokens_host[(size_t)i * W + j] < cfg->n_vocab,
                         "%s: prompt token [%d][%d]=%d outside the vocabulary of %d", who, i, j, prompt_tokens_host[(size_t)i * W + j], cfg->n_vocab);
    }
    for (int i = 0; bank && i < n_rows; ++i)
        WIPA_REQUIRE(ids_host[i] >= -1 && ids_host[i] < bank->n, "%s: ids_host[%d]=%d: -1 or an adapter of the bank (n = %d)", who, i, ids_host[i],
                     bank->n);
    if (n_rows == 0) return WIPA_OK;
    const AdmitWs A = admit_ws(cfg, n_rows, W);
    WIPA_REQUIRE(workspace && workspace_bytes >= A.total, "%s: workspace too small (%zu < %zu: wipa_decoder_admit_prompted_workspace_bytes)", who,
                 workspace ? workspace_bytes : (size_t)0, A.total);
    const size_t e = wipa_dtype_size(cfg->dtype);
    const int d = cfg->n_text_state, Ta = cfg->n_audio_ctx;
    WIPA_REQUIRE(((size_t)d * e) % 16 == 0, "%s: a K / V row of %zu bytes is no multiple of 16", who, (size_t)d * e);
    const wipa_dec_layout L = dec_layout(cfg, B);
    RT_CALL(state_fits(who, L, state_bytes));
    hipStream_t s = (hipStream_t)stream;
    char* st = (char*)state;
    char* ws = (char*)workspace;
    // meta, the right-aligned prompts (padding columns hold token 0) and the local starts W - L_i: one host image, one copy.  The image is
    // pageable memory, which the copy has left when the call returns (as wipa_decoder_begin_ragged's arrays)
    std::vector<int32_t> image((A.feat - A.meta) / 4, 0);
    for (int i = 0; i < n_rows; ++i) {
        int32_t* m = image.data() + (size_t)i * ADMIT_META;
        m[0] = slots_host[i]; m[1] = prompt_lens_host[i]; m[2] = limits_host[i];
        for (int t = 0; t < n_init; ++t) m[3 + t] = initial_tokens_host[i * n_init + t];
        m[7] = sample ? (int32_t)streams_host[2 * i] : 0;
        m[8] = sample ? (int32_t)streams_host[2 * i + 1] : 0;
        m[9] = bank ? ids_host[i] : -1;  // the admitted clip's adapter: what the prompt pass below reads, row by row
        for (int j = W - prompt_lens_host[i]; j < W; ++j) image[A.tokens / 4 + (size_t)i * W + j] = prompt_tokens_host[(size_t)i * W + j];
        image[A.starts / 4 + i] = W - prompt_lens_host[i];
    }
    WIPA_CHECK_HIP(hipMemcpyAsync(ws + A.meta, image.data(), image.size() * 4, hipMemcpyHostToDevice, s));
    const int32_t* meta = (const int32_t*)(ws + A.meta);
    const int32_t* pos = (const int32_t*)(st + L.pos);
    for (int i = 0; i < n_rows; ++i) RT_CALL(admit_cross(cfg, w, st, L, B, slots_host[i], features_host[i], stream));
    for (int i = 0; bank && i < n_rows; ++i) {
        // the slot's id for the steps (a plain copy, before the slot's first step), then the clip's cross K / V terms behind admit_cross
        WIPA_CHECK_HIP(hipMemcpyAsync((void*)(bank->ids_dev + slots_host[i]), ids_host + i, sizeof(int32_t), hipMemcpyHostToDevice, s));
        RT_CALL(wipa_decoder_adapt_cross(cfg, w, state, state_bytes, B, features_host[i], 1, slots_host + i, bank, stream));
    }
    hipLaunchKernelGGL(admit_rows_prompted_kernel, dim3(n_rows), dim3(256), 0, s, (int32_t*)(st + L.tokens), L.ld_tok, pos, cfg->n_text_ctx, B, n_init,
                       W, meta, (const int32_t*)(ws + A.tokens), starts_dev, (float*)(st + L.sum_logprobs), (uint32_t*)sample);
    WIPA_LAUNCH_CHECK();
    if (W == 0) return WIPA_OK;
    // the prompt pass: ONE batched walk over the admitted rows only, packed [n_rows * W], local starts W - L_i; it is wanted for the K / V
    // of the prompt columns alone, which ScatterHook moves into the slots' self-attention cache behind every layer's q|k|v GEMM
    const size_t clip_bytes = (size_t)Ta * d * e;
    for (int i = 0; i < n_rows; ++i)
        WIPA_CHECK_HIP(hipMemcpyAsync(ws + A.feat + (size_t)i * clip_bytes, features_host[i], clip_bytes, hipMemcpyDeviceToDevice, s));
    ScatterHook hook;
    hook.cfg = cfg; hook.self_kv = st + L.self_kv; hook.meta = meta; hook.pos = pos;
    hook.n_rows = n_rows; hook.W = W; hook.B = B; hook.n_init = n_init; hook.s = s;
    BatchedWalk k = {};
    k.B = n_rows; k.T = W;
    k.tokens = (const int32_t*)(ws + A.tokens); k.ld_tok = W;
    k.x = (float*)(ws + A.x); k.ln = ws + A.ln; k.q = ws + A.q; k.ao = ws + A.ao; k.hb = ws + A.h;
    k.qkv = ws + A.qkv;
    k.starts = (const int32_t*)(ws + A.starts);
    k.features = ws + A.feat; k.ckv_ws = ws + A.ckv;  // projected per layer from the admitted clips' features, in both cross forms
    k.n_group = 1;
    if (bank) { k.bank = bank; k.ids = meta + 9; k.ids_stride = ADMIT_META; }
    k.qkv_hook = &hook; k.kv_only = true;
    return batched_layers(cfg, w, k, stream);
}

extern "C" int wipa_decoder_release(void* state) {
    std::lock_guard<std::mutex> lk(g_graph_mu);
    for (auto it = g_graphs.begin(); it != g_graphs.end();) {
        if (std::get<0>(it->first) == state) {
            hipGraphExecDestroy(it->second);
            it = g_graphs.erase(it);
        } else {
            ++it;
        }
    }
    return WIPA_OK;
}

// ------------------------------------------------------------------ teacher-forced decoder
namespace {
struct TfWs {
    size_t x, ln, qkv, q, ao, h, ckv, total;
};
TfWs tf_ws(const wipa_model_cfg* c, int B, int T) {
    const size_t e = wipa_dtype_size(c->dtype), d = c->n_text_state, M = (size_t)B * T;
    TfWs w;
    size_t o = 0;
    w.x = o;   o += align256(M * d * 4);
    w.ln = o;  o += align256(M * d * e);
    w.qkv = o; o += align256(M * 3 * d * e);
    w.q = o;   o += align256(M * d * e);
    w.ao = o;  o += align256(M * d * e);
    w.h = o;   o += align256(M * 4 * d * e);
    w.ckv = o; o += align256((size_t)B * 2 * c->n_text_head * c->n_audio_ctx * 64 * e);
    w.total = o;
    return w;
}
}  // namespace

namespace {
// embedding + every decoder layer of the teacher-forced pass; leaves the residual stream in ws.x (f32 [B*T, d])
int tf_layers(const wipa_model_cfg* cfg, const void* const* w, const int32_t* tokens, const void* features, char* ws, const TfWs& L, int B,
              int T, const TfHook* hook, wipa_stream_t stream) {
    BatchedWalk k = {};
    k.B = B; k.T = T;
    k.tokens = tokens; k.ld_tok = T;
    k.x = (float*)(ws + L.x); k.ln = ws + L.ln; k.q = ws + L.q; k.ao = ws + L.ao; k.hb = ws + L.h;
    k.qkv = ws + L.qkv;
    k.features = features; k.ckv_ws = ws + L.ckv;  // one clip per row
    k.n_group = 1;
    k.hook = hook;
    return batched_layers(cfg, w, k, stream);
}
}  // namespace

extern "C" size_t wipa_decoder_logits_workspace_bytes(const wipa_model_cfg* cfg, int B, int T) {
    if (!cfg || !audio_ctx_ok(cfg) || B <= 0 || T <= 0) return 0;
    return tf_ws(cfg, B, T).total;
}

extern "C" int wipa_decoder_logits(const wipa_model_cfg* cfg, const void* const* w, const int32_t* tokens, const void* features,
                                   float* logits, int64_t ld_logits, void* workspace, size_t workspace_bytes, int B, int T,
                                   wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(w && tokens && features && logits && workspace && B > 0 && T > 0, "wipa_decoder_logits: bad arguments");
    WIPA_REQUIRE(T <= cfg->n_text_ctx, "wipa_decoder_logits: T=%d exceeds n_text_ctx=%d", T, cfg->n_text_ctx);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "wipa_decoder_logits: the teacher-forced decoder runs on a bf16 / f32 weight table (fp8 tables serve the decode step)");
    const TfWs L = tf_ws(cfg, B, T);
    WIPA_REQUIRE(workspace_bytes >= L.total, "wipa_decoder_logits: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    RT_CALL(tf_layers(cfg, w, tokens, features, (char*)workspace, L, B, T, nullptr, stream));
    const int dt = cfg->dtype, d = cfg->n_text_state, M = B * T;
    float* x = (float*)((char*)workspace + L.x);
    void* ln = (char*)workspace + L.ln;
    RT_CALL(wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)w[2], (const float*)w[3], M, d, 1e-5f, stream));
    RT_CALL(gemm(ln, d, w[0], d, logits, ld_logits, M, cfg->n_vocab, d, dt, WIPA_F32, nullptr, 0, nullptr, stream));
    return WIPA_OK;
}

// ------------------------------------------------------------------ word-timestamp alignment on the teacher-forced pass
namespace {
constexpr size_t ALIGN_LOGITS_BYTES = (size_t)1 << 30;  // the most f32 logits that exist at once
struct AlignWs {
    TfWs tf;
    size_t stats, stats_bytes, logits, trace, trace_bytes, total;
    int block_rows;
};
AlignWs align_ws(const wipa_model_cfg* c, int B, int T, int n_heads, int logits_rows) {
    AlignWs a;
    a.tf = tf_ws(c, B, T);
    size_t o = a.tf.total;
    const int per_layer = std::min(std::max(n_heads, 1), (int)c->n_text_head);  // a layer holds each of its heads once
    a.stats_bytes = wipa_align_weights_scratch_bytes(B, T, per_layer, c->n_audio_ctx);
    a.stats = o; o += align256(a.stats_bytes);
    const size_t row_bytes = (size_t)round_up(c->n_vocab, 8) * 4;  // the row stride Whisper.logits uses
    size_t rows = std::max<size_t>(1, ALIGN_LOGITS_BYTES / row_bytes);
    if (logits_rows > 0) rows = std::min<size_t>(rows, (size_t)logits_rows);
    a.block_rows = (int)std::min<size_t>(rows, (size_t)B * T);
    a.logits = o; o += align256((size_t)a.block_rows * row_bytes);
    a.trace_bytes = wipa_dtw_scratch_bytes(B, T);
    a.trace = o; o += align256(a.trace_bytes);
    a.total = o;
    return a;
}
struct AlignHook : TfHook {
    const wipa_model_cfg* cfg;
    std::vector<std::vector<int32_t>> by_layer;  // head indices in list order
    int last_layer = -1, n_heads = 0, B = 0, T = 0;
    const int32_t *n_tokens = nullptr, *n_frames = nullptr;
    void* stats = nullptr;
    size_t stats_bytes = 0;
    float* matrix = nullptr;
    wipa_stream_t stream = nullptr;
    int after_cross_projections(int layer, const void* q, const void* ckv, int64_t k_bs, int64_t k_hs) const override {
        const std::vector<int32_t>& hs = by_layer[layer];
        if (hs.empty()) return WIPA_OK;
        return wipa_align_weights(q, ckv, k_bs, k_hs, cfg->dtype, B, T, cfg->n_text_state, cfg->n_audio_ctx, hs.data(), (int)hs.size(), n_tokens,
                                  n_frames, stats, stats_bytes, matrix, cfg->n_audio_ctx, layer == last_layer ? (float)n_heads : 0.f, stream);
    }
};
}  // namespace

extern "C" size_t wipa_decoder_align_workspace_bytes(const wipa_model_cfg* cfg, int B, int T, int n_heads, int logits_rows) {
    if (!cfg || !audio_ctx_ok(cfg) || B <= 0 || T <= 0 || n_heads <= 0 || logits_rows < 0) return 0;
    return align_ws(cfg, B, T, n_heads, logits_rows).total;
}

extern "C" int wipa_decoder_align(const wipa_model_cfg* cfg, const void* const* w, const int32_t* tokens, const void* features,
                                  const int32_t* heads_host, int n_heads, const int32_t* n_tokens, const int32_t* n_frames,
                                  const int32_t* n_rows, const int32_t* n_tokens_host, const int32_t* n_frames_host, const int32_t* n_rows_host,
                                  int first_row, int eot, float* matrix, int32_t* text_idx, int32_t* time_idx, int64_t ld_path, int32_t* path_len,
                                  float* token_probs, int logits_rows, void* workspace, size_t workspace_bytes, int B, int T,
                                  wipa_stream_t stream) {
    RT_CALL(cfg_check(cfg));
    SplitScope split_scope(cfg);
    WIPA_REQUIRE(w && tokens && features && heads_host && n_tokens && n_frames && n_rows && n_tokens_host && n_frames_host && n_rows_host &&
                     matrix && text_idx && time_idx && path_len && token_probs && workspace && B > 0 && T > 0,
                 "wipa_decoder_align: bad arguments");
    WIPA_REQUIRE(T <= cfg->n_text_ctx && T <= WIPA_ALIGN_MAX_TOKENS, "wipa_decoder_align: T=%d exceeds n_text_ctx=%d", T, cfg->n_text_ctx);
    WIPA_REQUIRE(cfg->dec_w_dtype == 0, "wipa_decoder_align: the teacher-forced decoder runs on a bf16 / f32 weight table (fp8 tables serve the decode step)");
    WIPA_REQUIRE(n_heads >= 1 && n_heads <= cfg->n_text_layer * cfg->n_text_head && cfg->n_text_head <= WIPA_ALIGN_MAX_HEADS,
                 "wipa_decoder_align: %d alignment heads (1..%d)", n_heads, cfg->n_text_layer * cfg->n_text_head);
    WIPA_REQUIRE(logits_rows >= 0 && eot >= 1 && eot <= cfg->n_vocab && first_row >= 0, "wipa_decoder_align: logits_rows=%d eot=%d first_row=%d",
                 logits_rows, eot, first_row);
    for (int b = 0; b < B; ++b) {
        WIPA_REQUIRE(n_tokens_host[b] >= 1 && n_tokens_host[b] <= T, "wipa_decoder_align: clip %d: %d tokens (1..%d)", b, n_tokens_host[b], T);
        WIPA_REQUIRE(n_frames_host[b] >= 1 && n_frames_host[b] <= cfg->n_audio_ctx, "wipa_decoder_align: clip %d: %d frames (1..%d)", b,
                     n_frames_host[b], cfg->n_audio_ctx);
        WIPA_REQUIRE(n_rows_host[b] >= 0 && first_row + n_rows_host[b] <= n_tokens_host[b], "wipa_decoder_align: clip %d: rows [%d, %d + %d) of %d tokens",
                     b, first_row, first_row, n_rows_host[b], n_tokens_host[b]);
    }
    AlignHook hook;
    hook.cfg = cfg;
    hook.by_layer.resize(cfg->n_text_layer);
    for (int i = 0; i < n_heads; ++i) {
        const int l = heads_host[2 * i], h = heads_host[2 * i + 1];
        WIPA_REQUIRE(l >= 0 && l < cfg->n_text_layer && h >= 0 && h < cfg->n_text_head, "wipa_decoder_align: alignment head (%d, %d) of %d x %d", l, h,
                     cfg->n_text_layer, cfg->n_text_head);
        std::vector<int32_t>& hs = hook.by_layer[l];
        WIPA_REQUIRE(std::find(hs.begin(), hs.end(), h) == hs.end(), "wipa_decoder_align: alignment head (%d, %d) listed twice", l, h);
        hs.push_back(h);
        hook.last_layer = std::max(hook.last_layer, l);
    }
    const AlignWs L = align_ws(cfg, B, T, n_heads, logits_rows);
    WIPA_REQUIRE(workspace_bytes >= L.total, "wipa_decoder_align: workspace too small (%zu < %zu)", workspace_bytes, L.total);
    char* ws = (char*)workspace;
    const int dt = cfg->dtype, d = cfg->n_text_state, Ta = cfg->n_audio_ctx, M = B * T, V = cfg->n_vocab, ldl = round_up(V, 8);
    hook.n_heads = n_heads; hook.B = B; hook.T = T;
    hook.n_tokens = n_tokens; hook.n_frames = n_frames;
    hook.stats = ws + L.stats; hook.stats_bytes = L.stats_bytes;
    hook.matrix = matrix; hook.stream = stream;
    WIPA_CHECK_HIP(hipMemsetAsync(matrix, 0, (size_t)M * Ta * sizeof(float), (hipStream_t)stream));
    RT_CALL(tf_layers(cfg, w, tokens, features, ws, L.tf, B, T, &hook, stream));
    RT_CALL(wipa_dtw_batch(matrix, (int64_t)T * Ta, Ta, first_row, T, n_rows, n_frames, n_rows_host, n_frames_host, B, ws + L.trace, L.trace_bytes,
                           text_idx, time_idx, ld_path, path_len, stream));
    float* x = (float*)(ws + L.tf.x);
    char* ln = ws + L.tf.ln;
    float* lg = (float*)(ws + L.logits);
    RT_CALL(wipa_layernorm(x, WIPA_F32, d, ln, dt, d, (const float*)w[2], (const float*)w[3], M, d, 1e-5f, stream));
    for (int r0 = 0; r0 < M; r0 += L.block_rows) {
        const int rows = std::min(L.block_rows, M - r0);
        RT_CALL(gemm(ln + (size_t)r0 * d * wipa_dtype_size(dt), d, w[0], d, lg, ldl, rows, V, d, dt, WIPA_F32, nullptr, 0, nullptr, stream));
        RT_CALL(wipa_token_probs(lg, ldl, r0, rows, tokens, n_tokens, B, T, eot, token_probs, stream));
    }
    return WIPA_OK;
}

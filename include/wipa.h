/* wipa.h -- C ABI of libwipa.so: the MI355X (gfx950) Whisper -> IPA hot path.
 *
 * The reference (barathanaslan/whisper-ipa) has no FFI of its own: its hot path
 * sits behind Python calls into mlx_whisper / mlx.  Each entry
 * point below names the reference call site it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller unless it says "host";
 *     the library never allocates or frees caller-visible memory -- scratch comes in
 *     as (workspace, bytes) with a *_bytes() query;
 *   - row-major, contiguous unless a leading dimension is given (in ELEMENTS);
 *   - asynchronous on the given hipStream_t, no hidden synchronisation;
 *   - returns 0 or a negative error code; wipa_last_error() has the text;
 *   - no torch / C++ types cross this boundary.
 * dtype: "T" below is the matrix/activation type of the call (f32 or bf16);
 * biases, LayerNorm parameters, positional tables, the residual stream and the
 * logits are always f32; all accumulation is f32.
 */
#ifndef WIPA_H
#define WIPA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* wipa_stream_t; /* hipStream_t */

enum { WIPA_F32 = 0, WIPA_BF16 = 1, WIPA_FP8_E4M3 = 2 /* weights only: OCP e4m3fn codes, one byte per element */ };
enum { WIPA_OK = 0, WIPA_ERR_ARG = -1, WIPA_ERR_HIP = -2, WIPA_ERR_STATE = -3 };

#define WIPA_N_SAMPLES 480000 /* 30 s at 16 kHz (mlx_whisper.audio.N_SAMPLES) */
#define WIPA_N_FRAMES 3000
#define WIPA_N_FFT 400
#define WIPA_HOP 160
#define WIPA_HEAD_DIM 64

int wipa_version(void);
const char* wipa_last_error(void);

/* A HIP stream whose kernels may only run on the first n_cus compute units of the device's CU-mask order (on MI355X mask bit
 * i is CU i/8 of XCD i%8, so every XCD keeps n_cus/8 of its 32 CUs; n_cus a multiple of 8).  Serving keeps several passes in
 * flight; giving the MFMA-bound encoder of one pass fewer than all CUs leaves the rest to the HBM-/latency-bound decode loop of
 * another (bench.py --encoder-cus).  The caller destroys the stream after synchronising it. */
/* A plain non-blocking HIP stream created by the library, in the order the host asks for them.  ROCm hands hardware queues to
 * streams in creation order (GPU_MAX_HW_QUEUES of them, then shared), so a host that keeps several passes in flight
 * (whisper_ipa_amd/pipeline.py; reference: the batch loops of scripts/evaluate_model.py:181-212) creates its pass streams -- and,
 * before them, any idle padding streams -- itself instead of taking them from a framework's pool. */
int wipa_stream_create(wipa_stream_t* out);
int wipa_stream_create_cu_limited(int n_cus, wipa_stream_t* out);
int wipa_stream_destroy(wipa_stream_t s);

/* ------------------------------------------------------------------ K0 audio ingest
 * replaces the host side of load_audio -> pad_or_trim at scripts/ipa_data_loader.py:44,80, scripts/transcribe_single.py:43-44,
 * scripts/evaluate_model.py:63: raw interleaved PCM (the bytes of a WAV data chunk, as read) -> mono f32 at 16 kHz, zero-padded or
 * cut to 30 s, one launch for a batch whose clips may differ in rate, sample format and channel count.
 *   x[i]  = mean over the channels (f32, channel order) of the samples of frame i, scaled (u - 128) / 128 | / 32768 | / 2147483648;
 *   y[m]  = sum_{k=-K..K} T[p][k+K] * x[q+k],  q = (m S) div D,  p = (m S) mod D,  x = 0 outside [0, n_frames),  for m < n_out;
 *   y[m]  = 0 for n_out <= m < 480000 (every element of audio_out [batch, 480000] f32 is written).
 * S / D = rate / 16000 in lowest terms; T = the clip's table, D x (2K+1) f32 at tables + table_offset: the Hann-windowed sinc
 * cutoff sinc(cutoff dt) (0.5 + 0.5 cos(pi clip(dt / half, -1, 1))), dt = p / D - k, cutoff = min(1, D / S), half = 16 / cutoff,
 * K = ceil(half) (whisper_ipa_amd.audio.resample_table builds it); rate = 16000 is S = D = 1, K = 0, T = [1], bit-exact.
 * n_frames: the frames present at byte_offset -- a caller need not upload more than ceil(480000 S / D) + K + 1 of a long clip;
 * n_out = min(480000, ceil(frames of the whole clip * D / S)).  byte_offset is a multiple of the sample size.
 * Supported: 4000 <= rate <= 192000 Hz, 1..8 channels.  pcm (pcm_bytes long), descs, tables (tables_floats long) and audio_out are
 * device pointers; descs_host is the same descriptor array in HOST memory: every clip is checked against the limits and the two
 * buffer sizes before the launch, and a clip outside them is an error (WIPA_ERR_ARG, wipa_last_error names the clip). */
enum { WIPA_PCM_U8 = 1, WIPA_PCM_S16 = 2, WIPA_PCM_S32 = 4 }; /* = bytes per sample */
#define WIPA_RESAMPLE_TILE 512 /* consecutive outputs per workgroup */
typedef struct wipa_pcm_clip {
    int64_t byte_offset;  /* of the clip's first frame, from pcm */
    int64_t table_offset; /* of the clip's table, in floats from tables */
    int32_t n_frames;     /* frames uploaded */
    int32_t n_out;        /* outputs before the zero tail */
    int32_t n_channels;
    int32_t format;       /* WIPA_PCM_* */
    int32_t rate;         /* source rate, Hz */
    int32_t S, D, K;
} wipa_pcm_clip;
int wipa_resample_pad(const void* pcm, size_t pcm_bytes, const wipa_pcm_clip* descs, const wipa_pcm_clip* descs_host, int batch,
                      const float* tables, size_t tables_floats, float* audio_out, wipa_stream_t s);

/* ------------------------------------------------------------------ K1 log-mel
 * replaces mlx_whisper.audio.log_mel_spectrogram (+ pad_or_trim) at
 * scripts/ipa_data_loader.py:80-82, scripts/transcribe_single.py:44-45,
 * scripts/evaluate_model.py:188-189.
 * tables: DFT(window folded in) + mel filterbank, built once by wipa_logmel_init.
 * audio  [B, 480000] f32 (already pad_or_trim'ed);
 * mel    [B*3002 + 4, n_mels] T ("padded mel"): frame t of clip b at row b*3002 + t + 1,
 *        rows b*3002 and b*3002+3001 (the conv1 halo) and the 4 tail rows written as zero,
 *        values = (max(log10(max(mel,1e-10)), gmax-8)+4)/4. */
#define WIPA_MEL_ROWS(B) ((int64_t)(B) * 3002 + 4)
size_t wipa_logmel_tables_bytes(int n_mels);
int wipa_logmel_init(void* tables, int n_mels, wipa_stream_t s);
size_t wipa_logmel_workspace_bytes(int batch, int n_mels);
int wipa_logmel(const float* audio, int batch, int n_mels, const void* tables, void* mel, int mel_dtype,
                void* workspace, size_t workspace_bytes, wipa_stream_t s);
/* [B,3000,n_mels] f32 (any producer) -> padded mel [B*3002 + 4, n_mels] T for the encoder. */
int wipa_mel_pad_cast(const float* mel, int batch, int n_mels, void* mel_padded, int dtype, wipa_stream_t s);
/* Short audio context (wipa_model_cfg.n_audio_ctx = T < 1500): the encoder consumes the first n_frames = 2T frames in the layout
 *   [B*(n_frames + 2) + 4, n_mels] T: frame t of clip b at row b*(n_frames + 2) + t + 1, rows b*(n_frames + 2) and
 *   b*(n_frames + 2) + n_frames + 1 and the 4 tail rows zero.
 * The 3002-row layout cannot be read in place: its row n_frames + 1 is the real frame n_frames, where conv1 at frame n_frames - 1
 * must see its zero padding.  The front end is unchanged -- 30 s of audio, the clamp at the clip's maximum - 8 taken over all 3000
 * frames -- so rows 1..n_frames carry the bits wipa_logmel writes there.  1 <= n_frames <= 3000; n_frames = 3000 is the layout above.
 * wipa_logmel_frames: wipa_logmel into the workspace (wipa_logmel_frames_workspace_bytes), then one copy of the rows.
 * wipa_mel_pad_cast_frames: mel f32, frame t of clip b at mel + b*clip_stride + t*n_mels (clip_stride in elements, >= n_frames *
 * n_mels: 3000 * n_mels takes the first n_frames of a full mel without a copy). */
#define WIPA_MEL_ROWS_FRAMES(B, n_frames) ((int64_t)(B) * ((n_frames) + 2) + 4)
size_t wipa_logmel_frames_workspace_bytes(int batch, int n_mels, int n_frames);
int wipa_logmel_frames(const float* audio, int batch, int n_mels, const void* tables, void* mel, int mel_dtype, int n_frames,
                       void* workspace, size_t workspace_bytes, wipa_stream_t s);
int wipa_mel_pad_cast_frames(const float* mel, int64_t clip_stride, int batch, int n_mels, int n_frames, void* mel_padded, int dtype,
                             wipa_stream_t s);

/* ------------------------------------------------------------------ SpecAugment (fine-tuning; no counterpart in the reference)
 * Time and mel-bin masks (Park et al. 2019; transformers' apply_spec_augment / mask_time_prob / mask_feature_prob) stored into an f32
 * mel in place.  The draw is stated in integers, so the host plan, the kernel and a numpy restatement agree bit for bit.
 * Per clip b and axis a (0 = time, 1 = mel bins):
 *   L = min(max(n_frames[b], 0), frames) for time (frames when n_frames is NULL), n_mels for bins;  w = min(length[a], L);
 *   word(k) = word 0 of philox4x32_10(counter (k, a, stream_lo[b], stream_hi[b]), key (seed & 0xffffffff, seed >> 32));
 *   x = rate_q16[a] * L;  n = min(64, max(min_masks[a], (x >> 16) + ((word(0xffffffff) >> 16) < (x & 0xffff) ? 1 : 0)));  n = 0 if L == 0;
 *   span k in 0..n-1 covers w consecutive indices from umulhi(word(k), L - w + 1).  Spans may overlap; the mask is their union.
 * Element (b, t, m) becomes fill when t is in a time span or m in a bin span; every other element is neither read nor written.
 * rate_q16 = min(65536, round(prob / length * 65536)) is the caller's: the expected number of spans per position in Q16.
 * Refused (WIPA_ERR_ARG, wipa_last_error names the setting): length < 1, min_masks outside 0..64, rate_q16 > 65536, and "too many
 * spans": ((rate_q16 * L_max) >> 16) + 1 > 64 with L_max = frames (time) or n_mels (bins); n_mels <= 512.
 * wipa_spec_augment_plan: HOST only, touches no GPU; streams_host uint32 [B][2] (lo, hi), n_frames_host int32 [B] or NULL;
 *   spans_out int32 [B][2][65]: the count, then the starts (-1 in the unused places).
 * wipa_spec_augment: element (b, t, m) at mel + b*ld_clip + t*ld_frame + m (elements), t < frames: [B, 3000, n_mels] dense, the first
 *   2N frames of such a mel (ld_clip = 3000*n_mels, frames = 2N), or the padded layout (mel = padded + n_mels, ld_clip = (frames +
 *   2)*n_mels): halo rows and whatever lies beyond frames are left alone.  streams_dev / n_frames_dev as above, on the device.
 *   One launch, asynchronous; 16-byte stores when mel, ld_clip, ld_frame and n_mels allow them. */
#define WIPA_SPEC_AUGMENT_MAX_SPANS 64
typedef struct wipa_spec_augment_cfg {
    int32_t length[2];    /* span length: time, bins */
    int32_t min_masks[2]; /* lower bound of the span count */
    uint32_t rate_q16[2]; /* spans per position, Q16 */
    float fill;           /* the value masked elements take (transformers: 0) */
} wipa_spec_augment_cfg;
int wipa_spec_augment_plan(const wipa_spec_augment_cfg* cfg, const uint32_t* streams_host, const int32_t* n_frames_host, int B, int frames,
                           int n_mels, uint64_t seed, int32_t* spans_out);
int wipa_spec_augment(float* mel, int64_t ld_clip, int64_t ld_frame, int B, int frames, int n_mels, const wipa_spec_augment_cfg* cfg,
                      const uint32_t* streams_dev, const int32_t* n_frames_dev, uint64_t seed, wipa_stream_t s);

/* ------------------------------------------------------------------ K4 GEMM
 * C = epilogue(A * W^T): every nn.Linear / Conv1d of mlx_whisper.whisper
 * (AudioEncoder, TextDecoder, MultiHeadAttention, ResidualAttentionBlock).
 * A: row m starts at A + m*lda (rows may OVERLAP: conv-as-GEMM, STFT framing), K contiguous.
 * W: [N,K] row-major (nn.Linear layout [out,in]); K must be a multiple of 128/sizeof(T)
 *    bytes-wise (64 bf16 / 32 f32): pad W with zero columns, A must stay readable.
 * epilogue, in order: + bias, * col_scale (columns < col_scale_n), gelu(erf),
 *    + pos[(m % rg_in) * ldpos + n], + residual, cast, store.
 * output element (m,n) lives at
 *    C + c_offset + (*c_offset_dev) + (m / rg_in) * rg_stride + (m % rg_in) * ldc
 *      + (n / cg_in) * cg_stride + (n % cg_in)
 *    rows with (m % rg_in) >= rg_valid are skipped (or written as 0 if zero_invalid_rows).
 *    Defaults rg_in = M (rg_valid = M), cg_in = N give the plain C[m*ldc + n].
 * residual uses the same addressing and dtype as C and may alias it. */
typedef struct wipa_gemm_desc {
    const void* A;
    const void* W;
    void* C;
    const float* bias;
    const void* residual;
    const float* pos;
    const int64_t* c_offset_dev;
    int64_t lda, ldw, ldc, ldpos;
    int64_t rg_stride, cg_stride, c_offset;
    int64_t slab_stride; /* elements between the k_slices partial outputs */
    int32_t M, N, K;
    int32_t in_dtype, out_dtype;
    int32_t rg_in, rg_valid, cg_in;
    int32_t zero_invalid_rows;
    int32_t bias_along_m;
    int32_t act; /* 0 none, 1 gelu(erf) */
    int32_t col_scale_n;
    float col_scale;
    int32_t k_slices; /* 0/1: whole K.  >1: K is cut into k_slices contiguous slices
                       * computed by different workgroups; slice z writes its PARTIAL sums (bias in
                       * slice 0 only, no act/pos/residual) to C + z*slab_stride -- to be summed in a
                       * fixed order by wipa_add_slabs_layernorm or wipa_sum_slabs (deterministic split-K).  M <= 1024
                       * runs in the weight-streaming kernel, larger M in the 128x128 tile kernel. */
    int32_t f32_split; /* float32 inputs in the tile kernels (M > 256 rows).  0 (default): exact f32 products on the f32 MFMA.
                        * 1: every product a*w is taken as three bf16 MFMA terms on operands split into hi + lo
                        * (a_hi*w_lo + a_lo*w_hi + a_hi*w_hi, f32 accumulation): about twice the rate at ~5e-6 relative error
                        * of a K = 768 dot product (f32 MFMA: ~1.5e-6).  The weight-streaming kernel always multiplies exactly. */
    /* fp8 weights (BASELINE.json configs[4]: whisper-large-v3 fp8-weight inference).  w_dtype = WIPA_FP8_E4M3: W holds OCP
     * e4m3fn codes [N, K] (ldw in bytes = elements), the weight value is code * w_scale[n]; activations must be bf16.
     * Weight-streaming kernel only (M <= 1024): the decode step, where the weight stream is what a projection costs.
     * w_dtype = 0: W has the input dtype. */
    const float* w_scale;
    int32_t w_dtype;
    /* LayerNorm prologue (decode step: mlp_ln folded into mlp1).  ln_x != NULL: A is ignored and the A operand is
     * LayerNorm(ln_x[m, 0:K]; ln_w, ln_b, ln_eps) rounded to the input dtype, computed inside the kernel from the f32 rows
     * ln_x + m*ln_ldx.  Weight-streaming kernel only: M <= 1024, K a multiple of 64 and <= 1280, no k_slices. */
    const float* ln_x;
    const float* ln_w;
    const float* ln_b;
    int64_t ln_ldx;
    float ln_eps;
    int32_t stream_weights; /* 1: the rows are decode rows (one or a few per clip) and W is a weight matrix: use the
                             * weight-streaming kernel up to M = 1024 instead of 256, so that a prompt prefill of
                             * 4 rows per clip rounds exactly like the single-row steps (batch invariance) */
    /* K-major operands (float32 in and out, 128x128 tile kernel, k_slices allowed): a_trans: A is stored [K][M] (lda =
     * elements per k-row, M a multiple of 4); w_trans: W is stored [K][N] (ldw likewise, N a multiple of 4).  The staging
     * pass transposes into LDS, so the backward pass of a linear layer multiplies by W^T (input gradient) and by dy^T, x^T
     * (weight gradient) without a transposed copy: nn.value_and_grad at scripts/train_whisper_ipa.py:284. */
    int32_t a_trans;
    int32_t w_trans;
    /* fp8 ACTIVATIONS x fp8 weights on the block-scaled fp8 matrix instruction (BASELINE.json configs[4]: "CDNA4 fp8 MFMA").
     * in_dtype = WIPA_FP8_E4M3: A [M, K] and W [N, K] both hold OCP e4m3fn codes (lda / ldw in bytes = elements), the values
     * are code * a_scale[m] and code * w_scale[n] (power-of-two scales from wipa_layernorm_fp8 / wipa_rowquant_fp8 and the
     * weight quantiser); K a multiple of 128.  256 x 256 tile kernel, every epilogue option except k_slices. */
    const float* a_scale;
} wipa_gemm_desc;
int wipa_gemm(const wipa_gemm_desc* d, wipa_stream_t s);
/* Dispatch census (measurement / test aid, no reference counterpart): how many wipa_gemm calls of this process went to each
 * kernel family since the last reset.  out (HOST) receives the first n counters; reset != 0 clears all of them afterwards.
 * The parity tests of the fine-tune step (scripts/train_whisper_ipa.py:266-311) use it to prove that the shape-dependent
 * branches tuned for 32 clips x 64 tokens (split-K, 384 x 128 tiles, K-major operands) are the ones under test. */
enum {
    WIPA_GEMM_TILE128 = 0,   /* 128 x 128 register-staged tile kernel */
    WIPA_GEMM_TILE256 = 1,   /* 256 x 256 LDS-DMA tile kernel */
    WIPA_GEMM_TILE384 = 2,   /* 384 x 256 */
    WIPA_GEMM_TILE384N = 3,  /* 384 x 128 (float32, badly quantised wide grids) */
    WIPA_GEMM_TILE256P = 4,  /* phase-interleaved 256 x 256 (WIPA_GEMM_TILE=2568) */
    WIPA_GEMM_SKINNY = 5,    /* weight-streaming kernel (decode rows) */
    WIPA_GEMM_SKINNY_FP8 = 6,
    WIPA_GEMM_SKINNY_LN = 7, /* ... with the LayerNorm prologue */
    WIPA_GEMM_KMAJOR = 8,    /* a_trans / w_trans operands (128 x 128 kernel) */
    WIPA_GEMM_SPLIT_K = 9,   /* calls with k_slices > 1 (counted in addition to their kernel family) */
    WIPA_GEMM_TILE_FP8 = 10, /* fp8 x fp8 on v_mfma_scale_f32_16x16x128_f8f6f4 (in_dtype = WIPA_FP8_E4M3): every such call */
    WIPA_GEMM_TILE_FP8_384 = 11, /* ... those of them that took the 384 x 256 tile (counted in addition) */
    WIPA_GEMM_DISPATCH_CLASSES = 12
};
int wipa_gemm_dispatch_counts(int64_t* out, int n, int reset);

/* ------------------------------------------------------------------ K3 LayerNorm
 * nn.LayerNorm(eps=1e-5) rows of width D (attn_ln, cross_attn_ln, mlp_ln, ln_post, ln). */
int wipa_layernorm(const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy, const float* w,
                   const float* b, int rows, int D, float eps, wipa_stream_t s);

/* fp8 activations (cfg.enc_act_fp8): y = e4m3fn codes of LayerNorm(x) [rows, D] bytes (row stride ldy) with ONE power-of-two
 * scale per row, y_scale[r] = the smallest power of two with max|LN(x)[r,:]| / y_scale <= 448; value = code * y_scale[r].
 * x f32 rows; D a multiple of 4. */
int wipa_layernorm_fp8(const float* x, int64_t ldx, void* y, int64_t ldy, float* y_scale, const float* w, const float* b, int rows,
                       int D, float eps, wipa_stream_t s);
/* the same row quantisation of an existing activation matrix x [rows, D] (x_dtype WIPA_BF16 or WIPA_F32; D a multiple of 8). */
int wipa_rowquant_fp8(const void* x, int x_dtype, int64_t ldx, void* y, int64_t ldy, float* y_scale, int rows, int D, wipa_stream_t s);

/* Decode-step fusion: x[r,:] += sum_s slabs[s][r,:] (fixed order s = 0..n_slabs-1; x f32, in place),
 * then y = LayerNorm(x).  slabs are the k_slices partial outputs of the preceding residual GEMM. */
int wipa_add_slabs_layernorm(float* x, int64_t ldx, const float* slabs, int n_slabs, int64_t slab_stride, void* y,
                             int y_dtype, int64_t ldy, const float* w, const float* b, int rows, int D, float eps,
                             wipa_stream_t s);

/* ------------------------------------------------------------------ K8 embedding
 * TextDecoder: token_embedding[tokens] + positional_embedding[offset : offset+T].
 * tokens [B, ld_tok] int32; row (b,t) uses token tokens[b][p] and position p,
 * p = t_start + (pos_dev ? *pos_dev : 0) + t.  x [B*T, D] f32.  emb_dtype WIPA_FP8_E4M3: tok_emb holds e4m3 codes and
 * row v dequantises as bf16(code * emb_scale[v]) (emb_scale is ignored otherwise). */
int wipa_embed_tokens(const int32_t* tokens, int64_t ld_tok, int B, int T, int t_start, const int32_t* pos_dev,
                      const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, float* x, int D,
                      wipa_stream_t s);

/* ------------------------------------------------------------------ attention
 * MultiHeadAttention.qkv_attention with head_dim 64; q and k arrive already
 * scaled by 64**-0.25 (GEMM epilogue col_scale), softmax in f32.
 * decoder causal self-attention and teacher-forced cross-attention (mlx_whisper
 * TextDecoder blocks behind scripts/train_whisper_ipa.py:232), any Tq / Tk.  float32 with
 * Tq >= 16 and no device-side offsets runs on the f32 MFMA (exact f32 products, 64 queries
 * per workgroup); the few-row prompt prefill and bf16 use the f32-math VALU kernel.
 * Element (b, t, h, d) of X is at
 *   X + b*x_bs + t*x_rs + h*x_hs + d.
 * Tk = (tk_dev ? *tk_dev : 0) + Tk;  causal: query i sees keys <= i + (Tk - Tq). */
typedef struct wipa_attn_desc {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    const int32_t* tk_dev;
    const int32_t* q_row_dev; /* optional device int: first query row = *q_row_dev (decode step) */
    float* lse;               /* optional out (wipa_attention only): f32 [B,H,Tq] log-sum-exp of each score row */
    int64_t q_bs, q_rs, q_hs;
    int64_t k_bs, k_rs, k_hs;
    int64_t v_bs, v_rs, v_hs;
    int64_t o_bs, o_rs, o_hs;
    int32_t B, H, Tq, Tk;
    int32_t causal, dtype;
} wipa_attn_desc;
int wipa_attention(const wipa_attn_desc* d, wipa_stream_t s);

/* K5 encoder self-attention, bf16 MFMA flash kernel (non-causal, T keys).
 * qk  [B*T, ldqk] bf16: q of head h at column h*64, k at column D + h*64;
 * vt  [B][D][ldvt] bf16: V transposed per clip (row h*64+d, column t), ldvt >= ceil64(T),
 *     columns >= T must hold finite values;
 * out [B*T, ldo] bf16. */
int wipa_flash_attn_enc_bf16(const void* qk, int64_t ldqk, const void* vt, int64_t ldvt, void* out, int64_t ldo,
                             int B, int H, int T, wipa_stream_t s);
/* K5 in f32: the same encoder attention on the f32 MFMA (exact f32 products) for models kept in float32, as the
 * reference's scripts do (transcribe_single.py:13, train_whisper_ipa.py:505).  q, k, v: [B*T, ld*] f32 with head h at
 * column h*64 (q and k pre-scaled by 64^-0.25 each); out [B*T, ldo].  Row strides multiples of 4, pointers 16-byte aligned.
 * f32_split != 0: scores on a three-way and P*V on a two-way bf16 split of the operands (bf16 MFMA, error ~2^-24 of a
 * score) instead of exact f32 products -- the same opt-in as wipa_gemm_desc.f32_split. */
int wipa_flash_attn_enc_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                            int64_t ldo, int B, int H, int T, int f32_split, wipa_stream_t s);

/* K11/K12 decode-step attention (HBM-bound): ONE query row per (b,h) (Tq must be 1) against
 * cached K/V with the strides of wipa_attn_desc; 8 (bf16) / 16 (f32) lanes stream one 64-dim key
 * row with 16-byte loads, online softmax per lane group, merged across 4 waves.  Used for the
 * growing self-attention cache (tk_dev / q_row_dev = position) and, via the wrapper below,
 * for cross-attention. */
int wipa_decode_attn(const wipa_attn_desc* d, wipa_stream_t s);
/* cross-attention wrapper: q [B, H*64] T; kv [B][2H][Tk][64] T (K heads then V heads);
 * out [B, H*64] T. */
int wipa_decode_cross_attn(const void* q, const void* kv, void* out, int B, int H, int Tk, int dtype,
                           wipa_stream_t s);
/* n_q (1..4) query rows per clip against the same cache: q / out [B*n_q, H*64] rows (b, t); every K/V row is read once. */
int wipa_decode_cross_attn_multi(const void* q, const void* kv, void* out, int B, int H, int Tk, int n_q, int dtype,
                                 wipa_stream_t s);

/* candidate groups: q / out as above for B rows, kv holds B / n_group clips and row b reads the cache of clip b / n_group -- the
 * arithmetic of wipa_decode_cross_attn (n_q = 1) / wipa_decode_cross_attn_multi on the same bytes, in separate instantiations of their
 * kernels.  n_group >= 1 and B % n_group == 0; n_group = 1 launches exactly what the ungrouped entry points launch. */
int wipa_decode_cross_attn_grouped(const void* q, const void* kv, void* out, int B, int H, int Tk, int n_q, int n_group, int dtype,
                                   wipa_stream_t s);

/* ------------------------------------------------------------------ fused decode-step blocks (K11 / K12)
 * One decode step of mlx_whisper's ResidualAttentionBlock with a KV cache (DecodingTask._main_loop,
 * transcribe_single.py:55) in 5 launches per layer instead of 11: see csrc/decode_fused.hip.
 *
 * self block, one workgroup per (head, 16 token rows):
 *   y = LayerNorm(x[b]; ln_w, ln_b) -> (q|k|v)_h = y Wqkv[h]^T + b (q, k scaled by qk_scale, rounded to T) -> k, v appended to
 *   the caches at position *pos -> o_h = softmax(q_h K_h^T) V_h over positions 0..*pos -> slabs[h][b][:] = o_h Wo[:, h*64:(h+1)*64]^T.
 * x [B, d] f32; wqkv [3d, d] T (query | key | value rows), bqkv [3d]; wo [d, d] T; kcache / vcache T [B][n_ctx][d]
 * (kv_batch_stride = n_ctx * d elements); slabs f32 [H][B][d] with slab_stride >= B*d elements.  The residual update
 * x + bias_o + sum_h slabs[h] is left to wipa_decode_cross_block. */
typedef struct wipa_self_block_desc {
    const float* x;
    const float* ln_w;
    const float* ln_b;
    const void* wqkv;
    const float* bqkv;
    const void* wo;
    void* kcache;
    void* vcache;
    const int32_t* pos; /* device */
    float* slabs;
    int64_t kv_batch_stride, slab_stride;
    int32_t B, d, H, dtype;
    float eps, qk_scale;
} wipa_self_block_desc;
int wipa_decode_self_block(const wipa_self_block_desc* d, wipa_stream_t s);
/* cross block, one workgroup per (head, clip):
 *   r = x_in[b] + bias_o + slabs[0][b] + ... + slabs[n_slabs-1][b] (that order; bias_o may be NULL when slab 0 already carries
 *   the bias, as the split-K slabs of wipa_gemm do; the h = 0 workgroup stores r to x_out[b]) ->
 *   y = LayerNorm(r; ln_w, ln_b) -> q_h = (y Wq[h]^T + bq) * qk_scale (rounded to T) -> out[b][h*64:(h+1)*64] =
 *   softmax(q_h K^T) V over the cached cross keys/values kv [B][2H][Tk][64] T (K heads then V heads; every element read
 *   once, non-temporal).  x_out must not alias x_in.  n_slabs <= 20. */
typedef struct wipa_cross_block_desc {
    const float* x_in;
    float* x_out;
    const float* slabs;
    const float* bias_o;
    const float* ln_w;
    const float* ln_b;
    const void* wq;
    const float* bq;
    const void* kv;
    void* out;
    int64_t slab_stride;
    int32_t n_slabs, B, d, H, Tk, dtype;
    float eps, qk_scale;
    int32_t cross_splits; /* wipa_decode_cross_absorbed_block[_out] only: frame splits per clip of the streaming launch, 1..4; 0 = the
                           * default (4).  wipa_decode_cross_block ignores it. */
    int32_t n_group;      /* candidate groups (wipa_model_cfg.dec_n_group): G > 1: the B rows are B / G clips x G candidates, kv holds
                           * B / G clips and row b reads clip b / G (a separate instantiation of the kernels that read kv; B % G == 0).
                           * 0 / 1: one clip per row, the launches and kernels of a descriptor without the field. */
} wipa_cross_block_desc;
int wipa_decode_cross_block(const wipa_cross_block_desc* d, wipa_stream_t s);

/* ------------------------------------------------------------------ K11 with ABSORBED key / value projections
 * Decode-step cross-attention that streams the encoder output xa itself instead of cached K = xa Wk^T and V = xa Wv^T + bv
 * (mlx_whisper MultiHeadAttention with xa, behind DecodingTask._main_loop, transcribe_single.py:55):
 *     scores_h = (q_h Wk_h) xa^T,   out_h = (softmax(scores_h) xa) Wv_h^T + bv_h
 * -- one pass over xa [Tk, d] per clip, layer and step instead of one over K and one over V (half the bytes), no K/V cache and no
 * cross-K/V projection; the 12x larger contractions run on the matrix cores (csrc/cross_absorbed.hip).  bf16, H <= 16 heads of
 * 64, d in {384, 512, 768, 1024}.
 * q   [B rows, row stride q_row_stride] bf16: the cross query, already multiplied by 64^-0.25 (and with its bias);
 * wkT [d, d] bf16 = Wk^T ([in][out]);  xa [B, Tk, d] bf16;  wv [d, d] bf16 ([out][in]), bv [d] f32;
 * out [B rows, row stride out_row_stride] bf16;  k_scale = 64^-0.25 (the key side's share of the score scale);
 * scratch: wipa_cross_absorbed_scratch_bytes(B, d, Tk) bytes, 16-byte aligned (sized for the largest split count).
 * wipa_cross_absorbed_init(d) raises the kernel's LDS limit (call it once outside any stream capture).
 * Frame splits: the streaming launch has n_splits x B workgroups, each holding a CU for Tk / n_splits frames of one clip, and the
 * merge adds the split partials in split order -- so the count is part of the result's rounding and NEVER depends on B.  4 (the
 * default; want = 0) fills the 256 CUs at 64 clips and gives a lone decode step its shortest launch; 2 leaves half the chip to
 * the other passes in flight (round 4, whisper-small, 64 clips, 4 passes in flight: 72.3 against 75.3 ms per pass, a lone step
 * 1.35 against 1.25 ms; 3: 73.5 ms / 1.26 ms) -- the caller who pipelines passes chooses (wipa_model_cfg.dec_cross_splits).
 * wipa_cross_absorbed_splits(want, Tk) = the count a launch uses: want clamped to 1..4 and to >= two 32-frame tiles per split. */
int wipa_cross_absorbed_splits(int want, int Tk);
/* xa residency: the streaming launch loads the first wipa_cross_absorbed_resident_groups(B, d, Tk, n_splits) 16-frame groups of every
 * split with the default cache policy (they stay in the Infinity Cache for the next layer and step, which stream the same xa) and the
 * rest non-temporally.  A cache hint only: no result depends on it.  _for(..., budget_bytes) is the rule itself -- a byte budget per
 * pass (negative: every group), min(groups per split, budget / (B n_splits 16 d 2)); the four-argument form applies the process's
 * budget (a default per split count, or WIPA_XA_RESIDENT_MB in 10^6 bytes, read once: -1 every group default policy, 0 none). */
int wipa_cross_absorbed_resident_groups_for(int B, int d, int Tk, int n_splits, int64_t budget_bytes);
int wipa_cross_absorbed_resident_groups(int B, int d, int Tk, int n_splits);
size_t wipa_cross_absorbed_scratch_bytes(int B, int d, int Tk);
int wipa_cross_absorbed_init(int d);
int wipa_cross_absorbed_attention(const void* q, int64_t q_row_stride, const void* wkT, const void* xa, const void* wv, const float* bv,
                                  void* out, int64_t out_row_stride, void* scratch, size_t scratch_bytes, int B, int H, int d, int Tk,
                                  float k_scale, int n_splits, wipa_stream_t s);
/* candidate groups: B query rows, xa [B / n_group, Tk, d]; the streaming launch reads row b's frames at clip b / n_group (a separate
 * instantiation; the query prologue, the partials and the merge are per row and unchanged) and the residency rule counts the
 * B / n_group distinct clips.  n_group = 1 is wipa_cross_absorbed_attention. */
int wipa_cross_absorbed_attention_grouped(const void* q, int64_t q_row_stride, const void* wkT, const void* xa, const void* wv,
                                          const float* bv, void* out, int64_t out_row_stride, void* scratch, size_t scratch_bytes, int B,
                                          int H, int d, int Tk, float k_scale, int n_splits, int n_group, wipa_stream_t s);
/* The absorbed cross block of ONE decode step in three launches (the decode loop's form; wipa_cross_absorbed_attention with a
 * given query serves the prompt prefill and the tests): [split-K slab sum + residual + cross_attn_ln + cross query + absorbed query]
 * -> streaming kernel -> [merge + value projection].  The descriptor is wipa_decode_cross_block's with c->kv = the encoder output
 * xa [B][Tk][d] and c->out [B][d] bf16; bias_o must be NULL (slab 0 carries the out-projection bias), n_slabs <= 4;
 * wkT / wv / bv / scratch as above.  c->x_out must not alias c->x_in. */
int wipa_decode_cross_absorbed_block(const wipa_cross_block_desc* c, const void* wkT, const void* wv, const float* bv, void* scratch,
                                     size_t scratch_bytes, wipa_stream_t s);
/* The same block with the cross-attention OUT projection inside its third launch (round 4; what the decode step runs): instead of
 * c->out (may be NULL) the launch writes H split-K slabs slabs_out[h * slab_stride + b * d + n] = v_h[b] . Wo[n][h*64 .. h*64+63]
 * (f32; slab 0 carries bo) -- MultiHeadAttention.out of the cross-attention as a per-head K split -- which the next
 * wipa_add_slabs_layernorm(n_slabs = H <= 16) adds to the residual rows in head order.  wo [d, d] bf16 ([out][in]), bo [d] f32;
 * slabs_out may be the buffer c->slabs points to. */
int wipa_decode_cross_absorbed_block_out(const wipa_cross_block_desc* c, const void* wkT, const void* wv, const float* bv, const void* wo,
                                         const float* bo, float* slabs_out, int64_t slab_stride, void* scratch, size_t scratch_bytes,
                                         wipa_stream_t s);
/* measurement aid: the streaming kernel of wipa_cross_absorbed_attention alone, on a scratch a full call has filled */
int wipa_cross_absorbed_stream(const void* xa, void* scratch, size_t scratch_bytes, int B, int H, int d, int Tk, int n_splits,
                               wipa_stream_t s);

/* ------------------------------------------------------------------ K13 greedy step
 * GreedyDecoder.update + SuppressBlank + SuppressTokens of mlx_whisper.decoding
 * (transcribe_single.py:49-55).  p = *pos_dev is the position whose logits these are.
 * If p + 1 < n_init the next token is already given (prompt) and nothing is written.
 * Otherwise: logits += (p + 1 == n_init ? mask_first : mask_always) (0 / -inf, f32 [V]);
 * next = argmax (lowest index on ties); sum_logprobs += log_softmax[next] unless the
 * previous token was eot; next = eot if previous was eot; tokens[b][p+1] = next.
 * not_done is incremented by the number of rows whose next != eot. */
int wipa_greedy_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first,
                     const float* mask_always, int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init,
                     int eot, float* sum_logprobs, int32_t* not_done, wipa_stream_t s);
int wipa_add_i32(int32_t* p, int32_t v, wipa_stream_t s);
/* The decode step's tail in ONE launch (round 4; the step replayed by wipa_decoder_run ends with it): wipa_greedy_step as above
 * (at a prompt position, p + 1 < n_init, the given token is taken), THEN the next step's input row -- x[b] = tok_emb[next] +
 * pos_emb[min(p + 1, n_ctx - 1)] (f32) and y[b] = LayerNorm(x[b]; ln_w, ln_b) in y_dtype (the first block's attn_ln) -- and, by
 * the last workgroup to arrive on *done_counter (int32, zero between launches), *pos_dev = p + 1 and *posd_dev = (p + 1) * D.
 * tok_emb: emb_dtype WIPA_F32 / WIPA_BF16 / WIPA_FP8_E4M3 (codes, with emb_scale [V] f32).  TextDecoder's
 * token_embedding + positional_embedding + blocks[0].attn_ln of the NEXT position (mlx_whisper; transcribe_single.py:55). */
int wipa_greedy_step_embed(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                           int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init,
                           int eot, float* sum_logprobs, int32_t* not_done, const void* tok_emb, int emb_dtype,
                           const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b,
                           void* y, int y_dtype, int D, float eps, wipa_stream_t s);
/* The logits projection of a greedy decode step together with the arg-max / log-sum-exp PARTIALS of its filtered rows (round 4):
 * logits[b][v] = x[b] . W[v] (x [B, d] bf16, row stride ldx; W [V, d] bf16 -- TextDecoder's tied token_embedding, mlx_whisper;
 * transcribe_single.py:55) on the persistent wide kernel of wipa_gemm, whose waves also keep, per row, max / arg-max (lowest column
 * on ties) / sum of exponentials of logit + mask over the columns they compute (mask = mask_first when *pos_dev + 1 == n_init, else
 * mask_always; 0 / -inf, f32 [V]) and write one partial per (row, wave): partials [B][3][WIPA_GREEDY_PARTS] f32 (max | sum exp |
 * arg-max as int32).  logits may be NULL: then the 13 MB of logits are neither written nor read back (the steps of a greedy loop
 * whose logits nobody looks at).  bf16, B <= 64, V >= 8192, d in {384, 512, 768, 1024} (wipa_logits_greedy_supported).
 * wipa_greedy_step_embed_partials is wipa_greedy_step_embed on those partials instead of the logits: the same tokens; the
 * log-probability sum differs from the row scan's in the last bits (another summation order, fixed and batch-independent). */
#define WIPA_GREEDY_PARTS 2048
int wipa_logits_greedy_supported(int B, int V, int d, int dtype);
size_t wipa_logits_greedy_partials_bytes(int B);
int wipa_logits_greedy(const void* x, int64_t ldx, const void* w, int64_t ldw, float* logits, int64_t ldl, int B, int V, int d,
                       const float* mask_first, const float* mask_always, const int32_t* pos_dev, int n_init, float* partials,
                       size_t partials_bytes, wipa_stream_t s);
int wipa_greedy_step_embed_partials(const float* partials, int n_parts, int B, int32_t* tokens, int64_t ld_tok, int32_t* pos_dev,
                                    int64_t* posd_dev, int32_t* done_counter, int n_init, int eot, float* sum_logprobs,
                                    int32_t* not_done, const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb,
                                    int n_ctx, float* x, const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps,
                                    wipa_stream_t s);
/* Timestamp rules in the greedy update: ApplyTimestampRules of openai-whisper's decoding.py, which mlx_whisper.transcribe applies
 * on every step (scripts/evaluate_model.py:112-119 of the reference; transformers' WhisperTimeStampLogitsProcessor is the same
 * algorithm; mlx_whisper's port is [UPSTREAM-UNVERIFIED]).  With tb = timestamp_begin, nt = no_timestamps, seq = tokens[b][n_init .. p]:
 *   1. l = logits + (p + 1 == n_init ? mask_first : mask_always); l[nt] = -inf
 *   2. last = len(seq) >= 1 and seq[-1] >= tb; pen = len(seq) < 2 or seq[-2] >= tb;
 *      last and pen: l[tb:] = -inf;  last and not pen: l[:eot] = -inf
 *   3. t = the last token >= tb of seq IN ORDER (not the maximum), if any; t_last = t if last and not pen else t + 1; l[tb:t_last] = -inf
 *   4. p + 1 == n_init: l[:tb] = -inf and, if max_initial_timestamp_index >= 0, l[tb + index + 1:] = -inf
 *   5. logsumexp(l[tb:]) > max(l[:tb]) (false when no timestamp is left): l[:tb] = -inf
 *   6. next = argmax(l), lowest index on ties; sum_logprobs += l[next] - logsumexp(l) over the row after 5, unless the previous
 *      token was eot; EOT latch and not_done as wipa_greedy_step.
 * The kernel reads the row's own history; there is no per-row mask in memory.  V <= 65536, 16-byte aligned rows and masks,
 * eot < timestamp_begin < V. */
typedef struct wipa_decode_rules {
    int32_t timestamp_begin;             /* first timestamp token <|0.00|> */
    int32_t no_timestamps;               /* <|notimestamps|>: never sampled under the rules */
    int32_t max_initial_timestamp_index; /* round(max_initial_timestamp / 0.02); < 0: no cap */
} wipa_decode_rules;
/* wipa_greedy_step with the rules (no embedding): the rule arithmetic alone, on any rows */
int wipa_timestamp_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                        int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules,
                        float* sum_logprobs, int32_t* not_done, wipa_stream_t s);
/* wipa_greedy_step_embed with the rules: the tail of a decode step with wipa_decode_call.rules */
int wipa_timestamp_step_embed(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                              int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init,
                              int eot, const wipa_decode_rules* rules, float* sum_logprobs, int32_t* not_done, const void* tok_emb,
                              int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w,
                              const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t s);
/* Temperature sampling in the greedy update (upstream's GreedyDecoder.update with temperature > 0).  On the filtered row l -- the row
 * the greedy tails reduce: logits + mask, after rules 1-5 above when rules are given, rule 5 evaluated on the untempered row --
 *   next ~ Categorical(softmax(l / T)),   sum_logprobs += l[next] - logsumexp(l)   (the UNTEMPERED log-softmax at the drawn column);
 * EOT latch, not_done, prompt walk, next embedding + LayerNorm and position advance as in the greedy tails.
 * The draw is Gumbel-max: next = argmax_c (l[c] * (1 / T) + g_c) over the alive columns, lowest column on ties, with
 *   g_c = -log(-log(u_c)),  u_c = ((word >> 9) + 0.5) * 2^-23  (exact in f32; g in (-2.8, 16.7); logf for both logarithms),
 * and the bits from Philox4x32-10: key = (seed_lo, seed_hi), counter = (c >> 2, p | attempt << 16, stream_lo[b], stream_hi[b]),
 * word c & 3 of the output for column c; p = *pos_dev, the position whose logits these are, read on the device.  A row's noise
 * depends on (seed, stream[b], attempt, p, c) only -- never on B or on the row's index -- so a row draws the same tokens in
 * whichever batch it is decoded.  A row with no alive column keeps the greedy answer.
 *
 * The SAMPLING RECORD is one caller-owned DEVICE buffer of wipa_sample_record_bytes(B) bytes, 4-byte aligned:
 *   offset  0  uint32 seed_lo          offset  8  uint32 attempt (< 65536)
 *   offset  4  uint32 seed_hi          offset 12  float  1 / temperature
 *   offset 16 + 8 * b  uint32 stream_lo[b], uint32 stream_hi[b]          for every row b < B
 * The kernels read it when they RUN: the caller may rewrite it between calls (stream-ordered) and a captured step graph that
 * holds its address serves every seed, attempt, temperature and stream assignment.  wipa_sample_record_fill writes the HOST
 * image of a record (streams: [B][2] uint32, NULL: (b, 0)); the caller copies it to the device.  It returns WIPA_ERR_ARG for a
 * temperature that is not above 0 or an attempt outside 0..65535; every entry point below returns WIPA_ERR_ARG for a NULL record
 * where one is required.  V <= 65536 and positions below 65536. */
size_t wipa_sample_record_bytes(int B);
int wipa_sample_record_fill(void* host_record, size_t record_bytes, uint64_t seed, int attempt, float temperature,
                            const uint32_t* streams, int B);
/* The SAMPLING RECORD WITH A ROW PART: a second form, for a decode whose rows differ in temperature and attempt (continuous batching
 * with the temperature fallback: wipa_decode_call.sample_rows).  One caller-owned DEVICE buffer of wipa_sample_rows_bytes(B)
 * = 16 + 16 * B bytes, 16-byte aligned:
 *   offset  0  uint32 seed_lo          offset  8  uint32 B (the rows the buffer holds)
 *   offset  4  uint32 seed_hi          offset 12  uint32 0
 *   offset 16 + 16 * b  uint32 stream_lo[b], uint32 stream_hi[b], uint32 attempt[b] (< 65536), float 1 / temperature[b]   for b < B
 * 1 / temperature[b] == 0 marks a GREEDY row: its pick is the arg-max of the filtered row and nothing is drawn.  A sampled row's bits
 * are those of the record above: key = (seed_lo, seed_hi), counter = (c >> 2, p_own | attempt[b] << 16, stream_lo[b], stream_hi[b]), so a
 * row at temperature T and attempt a draws exactly the tokens the single-temperature tails draw for it.  The kernels read the record
 * when they RUN: admissions rewrite row entries in stream order and one captured step graph serves every assignment.
 * wipa_sample_rows_fill writes the HOST image: the header, and every row greedy on stream (b, 0) at attempt 0; the caller copies it to
 *   the device.
 * wipa_sample_rows_fill_row writes ONE row's entry into the host image, with the checks and the 1 / temperature of wipa_sample_rows_set.
 * wipa_sample_rows_set writes, in stream order, the entries of rows slots_host[i], i < n_rows: streams_host[i] = (lo, hi) (uint32
 *   [n_rows][2]), attempts_host[i], 1 / temperatures_host[i] (0 for temperature 0).  The values travel as kernel arguments (the host
 *   arrays may be freed when the call returns), as those of wipa_decoder_admit_rows do.  WIPA_ERR_ARG, with a message naming the
 *   argument and nothing enqueued: a temperature that is negative or not finite, an attempt outside 0..65535, a slot outside 0..B-1. */
size_t wipa_sample_rows_bytes(int B);
int wipa_sample_rows_fill(void* host_image, size_t bytes, uint64_t seed, int B);
int wipa_sample_rows_fill_row(void* host_image, size_t bytes, int B, int slot, uint32_t stream_lo, uint32_t stream_hi, int attempt,
                              float temperature);
int wipa_sample_rows_set(void* rows_dev, int B, int n_rows, const int32_t* slots_host, const uint32_t* streams_host,
                         const int32_t* attempts_host, const float* temperatures_host, wipa_stream_t s);
/* the draw alone on any rows (no embedding), like wipa_timestamp_step; rules may be NULL (the plain filtered row); sample: required */
int wipa_sample_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                     int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules,
                     const void* sample, float* sum_logprobs, int32_t* not_done, wipa_stream_t s);
/* wipa_timestamp_step_embed / wipa_greedy_step_embed (rules == NULL) with the draw: the tail of a sampling decode step */
int wipa_sample_step_embed(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                           int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init,
                           int eot, const wipa_decode_rules* rules, const void* sample, float* sum_logprobs, int32_t* not_done,
                           const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x,
                           const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t s);
/* a measurement aid: out[c] = g_c of row `row` of the record at position p, for c < V */
int wipa_sample_noise(const void* sample, int row, int p, int V, float* out, wipa_stream_t s);
/* Best-of-N ranking on the device: MaximumLikelihoodRanker.rank of upstream's decoding.py over candidate groups, one wave per clip.
 * tokens int32 [B, ld_tok], B = clips x n_group, rows c G .. c G + G - 1 the candidates of clip c; the generated columns are
 * [sample_begin, sample_begin + n).  Per candidate: length = generated tokens before the first eot, n when there is none (upstream's
 * t[sample_begin : first eot]); score = (double)sum_logprobs[b] / penalty[length] (IEEE division; penalty: DEVICE f64 [n + 1], built
 * by the host exactly as upstream computes it: length, or ((5 + length) / 6) ** length_penalty).  ONE deviation: length 0 scores
 * -inf where upstream divides by zero (reachable with suppress_blank=False only).  Per clip the winner is the FIRST maximum (the
 * lowest candidate on ties, np.argmax).  Outputs: winner int32 [clips], length int32 [B], best_tokens int32 [clips, ld_out] = the
 * winner's columns [0, sample_begin + n) (ld_out >= sample_begin + n), best_sum f32 [clips] = the winner's sum_logprobs.
 * 1 <= n_group <= 64, B % n_group == 0, n >= 1. */
int wipa_rank_groups(const int32_t* tokens, int64_t ld_tok, int B, int n_group, int sample_begin, int n, int eot, const float* sum_logprobs,
                     const double* penalty, int32_t* winner, int32_t* length, int32_t* best_tokens, int64_t ld_out, float* best_sum,
                     wipa_stream_t s);
/* The same row routine alone, for the token ALREADY at position p = *pos_dev: x[b] = tok_emb[tokens[b][p]] + pos_emb[p],
 * y[b] = LayerNorm(x[b]).  wipa_decoder_run launches it once before its first step. */
int wipa_embed_layernorm(const int32_t* tokens, int64_t ld_tok, int B, const int32_t* pos_dev, const void* tok_emb, int emb_dtype,
                         const float* emb_scale, const float* pos_emb, int n_ctx, float* x, const float* ln_w, const float* ln_b,
                         void* y, int y_dtype, int D, float eps, wipa_stream_t s);

/* Ragged prompts (prompt conditioning: wipa_decoder_begin_ragged / wipa_decode_call.starts_dev below).  The rows of a batch carry prompts
 * of different lengths RIGHT-ALIGNED to one common width P: row b's own tokens sit in columns [start[b], P) of tokens[b], columns below
 * start[b] are padding (token 0, never looked at), generation starts at column P for every row, and ONE position counter serves the
 * batch.  starts_dev: int32 [B] on the device, required by every *_ragged entry point.  Per row then:
 *   - the position-embedding index of column c is max(c - start[b], 0);
 *   - the Philox counter's position word of a draw is the row's own position p - start[b] (a row draws the same tokens in whichever
 *     batch, i.e. under whichever P, it is decoded);
 *   - the self-attention of column p reads keys start[b] .. p (wipa_decode_attn_ragged; a padding query reads its own key only).
 * These are separate instantiations of the step's kernels: the entry points without starts launch what they always launched.
 * wipa_embed_layernorm_ragged is wipa_embed_layernorm, wipa_step_embed_ragged is the step's tail -- wipa_sample_step_embed with a
 * sampling record, else wipa_timestamp_step_embed with rules, else wipa_greedy_step_embed -- and wipa_decode_attn_ragged is
 * wipa_decode_attn in its four-wave form for the self-attention cache (q_row_dev and tk_dev required). */
int wipa_embed_layernorm_ragged(const int32_t* tokens, int64_t ld_tok, int B, const int32_t* pos_dev, const int32_t* starts_dev,
                                const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx, float* x,
                                const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t s);
int wipa_step_embed_ragged(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                           int32_t* tokens, int64_t ld_tok, int32_t* pos_dev, int64_t* posd_dev, int32_t* done_counter, int n_init,
                           int eot, const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev, float* sum_logprobs,
                           int32_t* not_done, const void* tok_emb, int emb_dtype, const float* emb_scale, const float* pos_emb, int n_ctx,
                           float* x, const float* ln_w, const float* ln_b, void* y, int y_dtype, int D, float eps, wipa_stream_t s);
int wipa_decode_attn_ragged(const wipa_attn_desc* d, const int32_t* starts_dev, wipa_stream_t s);
/* wipa_decode_attn for the self-attention cache of beams (see wipa_beam_bytes below): the B rows are clips x n_group beams and key t of
 * row b is read from physical row b - b % n_group + anc[b][t] (anc uint8, row stride anc_ld, device).  With the identity table it is
 * wipa_decode_attn bit for bit; with any table it equals wipa_decode_attn on a cache gathered accordingly.  At most 512 keys.  Like
 * wipa_decode_attn_ragged it always takes the four-wave form: under WIPA_SELF_ATTN_WAVES=1, where wipa_decode_attn takes one wave per
 * head, the two agree to rounding only. */
int wipa_decode_attn_beam(const wipa_attn_desc* d, const uint8_t* anc, int64_t anc_ld, int n_group, wipa_stream_t s);
/* The same three sites for a whole prompt at once (wipa_decoder_prefill_ragged): wipa_embed_tokens for columns 0 .. T-1 (f32 / bf16
 * embedding), wipa_attention for the causal self-attention with Tq == Tk (always the f32-math VALU kernel: the f32 MFMA form declines
 * device-side offsets; a padding query sees the row's first own key), and wipa_sample_step with the row's own position in the counter. */
int wipa_embed_tokens_ragged(const int32_t* tokens, int64_t ld_tok, int B, int T, const int32_t* starts_dev, const void* tok_emb,
                             int emb_dtype, const float* pos_emb, float* x, int D, wipa_stream_t s);
int wipa_attention_ragged(const wipa_attn_desc* d, const int32_t* starts_dev, wipa_stream_t s);
int wipa_sample_step_ragged(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always,
                            int32_t* tokens, int64_t ld_tok, const int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules,
                            const void* sample, const int32_t* starts_dev, float* sum_logprobs, int32_t* not_done, wipa_stream_t s);

/* ------------------------------------------------------------------ K14 PER / PFER edit distances
 * replaces the dynamic programs behind phone_error_rate (scripts/evaluate_ipa.py:80-105: editdistance.eval on the two phone lists)
 * and PFERCalculator.phone_feature_error_rate (:139-213: the O(m n) Python loop with a feature comparison per cell), as
 * evaluate_batch (:346-378) runs them for every (reference, hypothesis) pair: n_pairs pairs in one launch, one wave per pair
 * (csrc/score.hip).  Phones are ids into a per-call vocabulary of n_phones entries.
 *   ref_ids / hyp_ids: the pairs' sequences back to back; pair p is ref_ids[ref_off[p] .. ref_off[p+1]) against hyp_ids[hyp_off[p] ..
 *   hyp_off[p+1]); ref_off / hyp_off int32 [n_pairs + 1];  order int32 [n_pairs]: a permutation of the pairs, the order in which
 *   the workgroups take them (the caller sorts by length product, longest first);
 *   feat_codes uint64 [n_phones]: 24 articulatory features at 2 bits each (bits 2f, 2f+1: 0 for 0, 1 for +1, 2 for -1), or NULL;
 *   per_dist[p]  = Levenshtein distance with unit costs (substitution: the ids differ);
 *   pfer24[p]    = the same recurrence with insertion = deletion = 24 and substitution = the number of features that differ
 *                  (24 x the reference's feature-weighted distance, exactly); 24 * per_dist[p] when feat_codes is NULL.
 * All of the above are device pointers.  ref_off_host / hyp_off_host are the two offset arrays in HOST memory: they are checked
 * before the launch -- first offset 0, non-decreasing, no sequence longer than WIPA_SCORE_MAX_LEN -- and a violation is an error
 * (WIPA_ERR_ARG, wipa_last_error names the pair) with nothing launched.  The ids are the caller's to keep inside [0, n_phones).
 * n_pairs = 0 succeeds without a launch. */
#define WIPA_SCORE_MAX_LEN 1024 /* phones per sequence */
int wipa_edit_distance_batch(const int32_t* ref_ids, const int32_t* ref_off, const int32_t* hyp_ids, const int32_t* hyp_off,
                             const int32_t* order, int n_pairs, const uint64_t* feat_codes, int n_phones,
                             const int32_t* ref_off_host, const int32_t* hyp_off_host,
                             int32_t* per_dist, int32_t* pfer24, wipa_stream_t s);

/* ------------------------------------------------------------------ K15 word-timestamp alignment (csrc/align.hip)
 * The numeric core of openai-whisper timing.py find_alignment, which mlx_whisper ports ([UPSTREAM-UNVERIFIED]: restated from
 * memory, pinned to the local transformers copy of the same chain): per alignment head softmax over a window's own frames,
 * z-score over the token axis (population std, no epsilon), width-7 median filter with reflect padding, mean over heads; then
 * dynamic time warping of the negated matrix.  All sizes per clip live in device memory; nothing of clip b depends on the
 * rest of the batch. */
#define WIPA_ALIGN_MAX_TOKENS 448  /* token rows per clip (n_text_ctx) */
#define WIPA_ALIGN_MAX_FRAMES 1500 /* encoder frames per clip (n_audio_ctx) */
#define WIPA_ALIGN_MAX_HEADS 32    /* alignment heads of one decoder layer */
/* One decoder layer's alignment heads, ADDED into out [B, T, ld_out] f32 (the caller zeroes it before the first layer):
 *   q [B, T, d] and keys k[b * k_bs + h * k_hs + frame * 64 + c] (elements), both of `dtype` and both carrying the 64^-0.25 scale, as
 *   wipa_decoder_logits leaves them in its workspace; heads_host: n_heads head indices of this layer (HOST), summed in this order;
 *   n_tokens / n_frames int32 [B] (device): clip b uses rows [0, n_tokens[b]) and frames [0, n_frames[b]) only, other cells of out
 *   are not touched; n_frames[b] <= 3 skips the median filter, as upstream does.
 *   divisor != 0: the cell is divided by it after the LAST head of this call (the mean over all heads of all layers).
 * Everything after the q.k products (f32 FMA chains, exact for f32 and bf16 operands) runs in f32.  No float atomics: one
 * thread owns an output cell for all heads of a call.  scratch: wipa_align_weights_scratch_bytes(B, T, n_heads, n_audio_ctx). */
size_t wipa_align_weights_scratch_bytes(int B, int T, int n_heads, int n_audio_ctx);
int wipa_align_weights(const void* q, const void* k, int64_t k_bs, int64_t k_hs, int dtype, int B, int T, int d, int n_audio_ctx,
                       const int32_t* heads_host, int n_heads, const int32_t* n_tokens, const int32_t* n_frames, void* scratch,
                       size_t scratch_bytes, float* out, int64_t ld_out, float divisor, wipa_stream_t s);
/* probs[m] for the rows m = row0 .. row0 + rows - 1 of a [B * T] grid (m = b T + t): softmax over columns [0, eot) of logits row
 * m - row0, taken at tokens[m + 1]; 0 where t + 1 >= n_tokens[b] or that token is not below eot. */
int wipa_token_probs(const float* logits, int64_t ldl, int row0, int rows, const int32_t* tokens, const int32_t* n_tokens, int B, int T,
                     int eot, float* probs, wipa_stream_t s);
/* Batched DTW, one wave per clip.  Clip b aligns rows [first_row, first_row + n_rows[b]) and columns [0, n_cols[b]) of
 * matrix[b * batch_stride + row * ld + col]; the kernel negates the matrix itself.  cost is f32 [N+1, M+1], +inf except
 * cost[0][0] = 0; cost[i][j] = -x[i-1][j-1] + c with (c, t) = (c0, 0) if c0 < c1 and c0 < c2, else (c1, 1) if c1 < c0 and c1 < c2,
 * else (c2, 2), for c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]: one f32 add per cell, so cost, trace and path are
 * those of the float32 restatement bit for bit, ties included.  The path (text_idx / time_idx [B, ld_path] int32, ascending)
 * has path_len[b] <= N + M - 1 entries; n_rows[b] = 0 writes length 0.  n_rows_host / n_cols_host are the HOST copies: they
 * are checked before the launch (0 <= N <= WIPA_ALIGN_MAX_TOKENS, 1 <= M <= WIPA_ALIGN_MAX_FRAMES where N > 0, rows inside
 * rows_avail, N + M <= ld_path); a violation is WIPA_ERR_ARG with nothing launched.  scratch holds the 2-bit trace codes:
 * wipa_dtw_scratch_bytes(B, largest n_rows). */
size_t wipa_dtw_scratch_bytes(int B, int max_rows);
int wipa_dtw_batch(const float* matrix, int64_t batch_stride, int64_t ld, int first_row, int rows_avail, const int32_t* n_rows,
                   const int32_t* n_cols, const int32_t* n_rows_host, const int32_t* n_cols_host, int B, void* scratch,
                   size_t scratch_bytes, int32_t* text_idx, int32_t* time_idx, int64_t ld_path, int32_t* path_len, wipa_stream_t s);

/* ------------------------------------------------------------------ host-side text plumbing (no GPU work)
 * Byte-level BPE of mlx_whisper.tokenizer (tiktoken's CoreBPE) and the token-batch builder of
 * IPADataset._tokenize_ipa_batch (scripts/ipa_data_loader.py:102-131, 146-152).  HOST pointers throughout.
 * The GPT-2 pre-tokeniser regex stays with the caller: encode one pre-split piece at a time.
 * table: n tokens, their bytes concatenated in `blob` (token i has lens[i] bytes) with rank ranks[i]
 *        (multilingual.tiktoken: 50 257 entries; the 256 single bytes must be present). */
typedef struct wipa_bpe wipa_bpe;
wipa_bpe* wipa_bpe_create(const uint8_t* blob, const int32_t* lens, const int32_t* ranks, int n); /* NULL on error */
void wipa_bpe_free(wipa_bpe* b);
/* lowest-rank-first pair merging; returns the number of ids written (<= max_out) or a negative error */
int wipa_bpe_encode_piece(const wipa_bpe* b, const uint8_t* piece, int len, int32_t* out, int max_out);
/* bytes of the ids, concatenated; returns the byte count, a negative WIPA_ERR_*, or -(i+1)-100 if ids[i] is not in the table */
int wipa_bpe_decode(const wipa_bpe* b, const int32_t* ids, int n, uint8_t* out, int max_out);
/* rows = prefix + ids of row r + eot, eot-padded to the longest row; returns the row width (<= ld_out) */
int wipa_build_token_batch(const int32_t* ids, const int32_t* row_lens, int n_rows, const int32_t* prefix, int n_prefix,
                           int32_t eot, int32_t* out, int64_t ld_out);

/* ------------------------------------------------------------------ model runtime
 * Sequencing of the kernels above for a whole encoder / decoder pass, in C++ so the
 * decode loop runs from a hipGraph with no per-kernel host work. */
typedef struct wipa_model_cfg {
    int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
    /* n_audio_ctx = T, 1..1500: the audio positions the model RUNS on (whisper.cpp's --audio-ctx).  The encoder reads a padded mel
     * of 2T frames (WIPA_MEL_ROWS_FRAMES(B, 2T) rows; 3002 per clip at T = 1500), adds the first T rows of its positional table and
     * writes features [B, T, d]; every decoder entry point takes features [clips, T, d] and sizes its cross-attention state, its
     * workspaces and the alignment matrix for T.  Outside 1..1500: WIPA_ERR_ARG (size queries return 0). */
    int32_t dtype; /* WIPA_F32 or WIPA_BF16: matrices, activations, KV caches */
    int32_t f32_split; /* dtype == WIPA_F32 only: 1 lets the encoder / teacher-forced GEMMs and the encoder flash attention
                        * use split-bf16 products (see wipa_gemm_desc.f32_split); 0 = exact f32 products (default) */
    int32_t dec_w_dtype; /* 0: the decoder matrices have `dtype`.  WIPA_FP8_E4M3 (bf16 models): the matrices the decode step streams
                          * (token embedding = logits matrix, self q|k|v, self out, cross query, cross out, mlp1, mlp2) are OCP
                          * e4m3fn codes with per-row f32 scales appended to the weight table (see WIPA_DEC_FP8_*); wipa_decoder_run
                          * / _prefill read them through the fp8 weight-streaming GEMM.  cross.kv stays bf16 (its projection is a
                          * tile GEMM over B*1500 rows); wipa_decoder_logits refuses an fp8 table. */
    int32_t weights_generation; /* bumped by the caller whenever any pointer of a weight table changes: part of the key of
                                 * the cached decode-step graphs (a freed table's host address may be reused) */
    int32_t enc_act_fp8; /* bf16 models with an fp8 encoder tail (WIPA_ENC_FP8_PER_LAYER): 1 = the encoder's q|k, value, mlp1 and
                          * mlp2 projections (11/12 of its GEMM FLOPs) run fp8 x fp8 on the block-scaled fp8 MFMA: LayerNorm outputs
                          * and the GELU output are quantised per row (wipa_layernorm_fp8 / wipa_rowquant_fp8), the weights are the
                          * e4m3 codes.  Attention, the out projection, the residual stream and everything downstream stay as
                          * they are.  0 = bf16 activations on the dequantised weights (the default; what the parity tests call
                          * "the bf16 model on quantised weights"). */
    int32_t dec_cross_absorbed; /* bf16 models, <= 16 heads, d in {384, 512, 768, 1024}, dec_w_dtype = 0: 1 = the decode step's
                                 * cross-attention streams the encoder output with absorbed key / value projections
                                 * (wipa_cross_absorbed_attention): the state's cross_kv region then holds a copy of the features
                                 * [B, n_audio_ctx, d], wipa_decoder_set_audio runs no projection, and the decoder table carries one
                                 * more entry per layer after the regular blocks: Wk^T [d, d] (WIPA_DEC_ABSORBED_PER_LAYER).  0 =
                                 * cached K / V (every other configuration). */
    int32_t dec_cross_splits; /* dec_cross_absorbed = 1: frame splits per clip of the decode step's streaming launch
                               * (wipa_cross_block_desc.cross_splits): 0 = default (4: shortest lone step), 2 = half-chip launches
                               * for callers that keep several passes in flight on one GPU (whisper_ipa_amd.pipeline sets it).
                               * Part of the step graph's and the prefill graph's key: wipa_decoder_prefill and wipa_decoder_run
                               * use the SAME count, so a prompt pass followed by steps rounds as the steps alone do
                               * (tests/test_gpu_model.py::test_prompt_prefill_equals_stepwise_prompt_absorbed). */
    int32_t dec_n_group; /* candidate groups (best-of-N sampling: upstream's n_group = best_of).  0 / 1: one clip per decode row -- every
                          * entry point enqueues exactly what it enqueued before the field existed.  G > 1: B in every wipa_decoder_* call
                          * counts ROWS = clips x G, rows c G .. c G + G - 1 are the candidates of clip c and share its audio:
                          * wipa_decoder_layout sizes cross_kv for B / G clips (everything else for B rows), wipa_decoder_set_audio takes
                          * the features of B / G clips and copies / projects them once per clip, and every launch that reads the
                          * per-clip audio reads clip b / G for row b (grouped instantiations; a grouped row does the arithmetic of an
                          * ungrouped row on the same bytes).  B % G != 0 is WIPA_ERR_ARG with nothing enqueued.  Part of the step graph's
                          * and the prompt-pass graphs' keys.  Served where a sampling decode is served (plain, rules, ragged prompts,
                          * f32 / bf16, cached / absorbed); the fully fused step (WIPA_DECODE_FUSED=1) is refused as sampling refuses it. */
} wipa_model_cfg;

/* Encoder weight table (const void* [WIPA_ENC_GLOBAL + WIPA_ENC_PER_LAYER * n_layer]):
 *   0 conv1.weight [d, K1] T   (mlx layout [d,3,n_mels] flattened, K1 = 3*n_mels padded to the GEMM K multiple)
 *   1 conv1.bias f32   2 conv2.weight [d, 3d] T   3 conv2.bias   4 positional [n_audio_ctx, d] f32
 *   5 ln_post.weight   6 ln_post.bias
 *   per layer: 0 attn_ln.w 1 attn_ln.b 2 qk.w [2d,d] T (query|key) 3 qk.b [2d] (key half zero)
 *              4 value.w [d,d] T 5 value.b 6 out.w 7 out.b 8 mlp_ln.w 9 mlp_ln.b
 *              10 mlp1.w [4d,d] 11 mlp1.b 12 mlp2.w [d,4d] 13 mlp2.b */
#define WIPA_ENC_GLOBAL 7
#define WIPA_ENC_PER_LAYER 14
/* fp8 encoder tables (cfg.enc_act_fp8 = 1) append, after the n_layer regular blocks, per layer:
 *   0 qk codes [2d,d] u8  1 qk scale [2d] f32  2 value codes [d,d]  3 value scale [d]  4 mlp1 codes [4d,d]  5 mlp1 scale [4d]
 *   6 mlp2 codes [d,4d]  7 mlp2 scale [d]      (value = code * scale[row]) */
#define WIPA_ENC_FP8_PER_LAYER 8
/* Decoder weight table (const void* [WIPA_DEC_GLOBAL + WIPA_DEC_PER_LAYER * n_layer]):
 *   0 token_embedding [V, d] T   1 positional_embedding [n_text_ctx, d] f32   2 ln.w   3 ln.b
 *   per layer: 0 attn_ln.w 1 attn_ln.b 2 qkv.w [3d,d] T 3 qkv.b [3d] (key third zero) 4 out.w 5 out.b
 *              6 cross_attn_ln.w 7 cross_attn_ln.b 8 cross.query.w 9 cross.query.b
 *              10 cross.kv.w [2d,d] T (key|value) 11 cross.kv.b [2d] (key half zero) 12 cross.out.w 13 cross.out.b
 *              14 mlp_ln.w 15 mlp_ln.b 16 mlp1.w 17 mlp1.b 18 mlp2.w 19 mlp2.b */
#define WIPA_DEC_GLOBAL 4
#define WIPA_DEC_PER_LAYER 20
/* fp8 decoder tables (cfg.dec_w_dtype = WIPA_FP8_E4M3) append, after the n_layer regular blocks:
 *   token_embedding scale [V] f32, then per layer: qkv scale [3d], out [d], cross.query [d], cross.out [d], mlp1 [4d], mlp2 [d]
 * (value = code * scale[row]); entries 0 and per-layer 2, 4, 8, 12, 16, 18 then point to e4m3 codes. */
#define WIPA_DEC_FP8_PER_LAYER 6
/* absorbed cross-attention tables (cfg.dec_cross_absorbed = 1, never together with fp8 tables) append per layer:
 *   0 cross.key.w transposed, [d_in, d_out] T */
#define WIPA_DEC_ABSORBED_PER_LAYER 1

/* AudioEncoder.__call__ / Whisper.embed_audio (train_whisper_ipa.py:223,
 * transcribe_single.py:54).  mel_padded [B,3002,n_mels] T -> out [B, n_audio_ctx, d] T. */
size_t wipa_encoder_workspace_bytes(const wipa_model_cfg* cfg, int B);
int wipa_encoder_forward(const wipa_model_cfg* cfg, const void* const* weights, const void* mel_padded, void* out,
                         void* workspace, size_t workspace_bytes, int B, wipa_stream_t s);

/* Stage timing (measurement aid, bench.py's MFMA roofline): between wipa_profile_begin(stream) and wipa_profile_end every
 * launch that wipa_encoder_forward and wipa_decoder_set_audio enqueue from THIS host thread on `stream` is bracketed by a
 * pair of HIP events.  wipa_profile_end synchronises the stream and returns the summed kernel time (ms) and launch count per
 * class: [0] GEMM / conv-as-GEMM (MFMA), [1] encoder flash attention, [2] LayerNorm, [3] other. */
#define WIPA_PROFILE_CLASSES 4
int wipa_profile_begin(wipa_stream_t s);
int wipa_profile_end(float* ms_by_class, int* launches_by_class);

/* KV-cached greedy decoding: mlx_whisper.decoding.decode / DecodingTask.run
 * (transcribe_single.py:55, train_whisper_ipa.py:356, evaluate_model.py:200).
 * All decode state lives in ONE caller-owned blob; wipa_decoder_layout gives byte offsets. */
typedef struct wipa_dec_layout {
    int64_t total_bytes;
    int64_t tokens;       /* int32 [B, ld_tok] */
    int64_t ld_tok;       /* elements */
    int64_t pos;          /* int32 scalar: index of the last filled token */
    int64_t not_done;     /* int32 scalar, accumulated by greedy steps */
    int64_t sum_logprobs; /* f32 [B] */
    int64_t logits;       /* f32 [B, ld_logits]: logits of the last step of the last wipa_decoder_run / wipa_decoder_prefill call
                           * (earlier steps of a call may not write them: wipa_logits_greedy) */
    int64_t ld_logits;
    int64_t cross_kv;     /* T [n_layer][B][2H][n_audio_ctx][64] (B / dec_n_group clips with candidate groups) */
    int64_t self_kv;      /* T [n_layer][3][B][n_text_ctx][d]  (slot 0 q staging, 1 K, 2 V) */
    int64_t scratch;
} wipa_dec_layout;
int wipa_decoder_layout(const wipa_model_cfg* cfg, int B, wipa_dec_layout* out);
/* Every entry point that writes into the blob takes `state_bytes`, the size of the caller's allocation, and refuses
 * (WIPA_ERR_ARG) a blob smaller than wipa_decoder_layout(cfg, B).total_bytes: the layout depends on cfg (dtype,
 * dec_cross_absorbed, dec_w_dtype ...), so a blob sized for one configuration must not be reused for another. */
/* cross K/V projection of the encoder output (MultiHeadAttention with xa, computed once). */
int wipa_decoder_set_audio(const wipa_model_cfg* cfg, const void* const* weights, const void* features, void* state,
                           size_t state_bytes, int B, wipa_stream_t s);
/* write the prompt (host int32 [n_init]) to every row, pos = 0, clear counters. */
int wipa_decoder_begin(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, const int32_t* initial_tokens_host,
                       int n_init, wipa_stream_t s);
/* n_steps decoder steps (each: one token position through all layers + greedy update).
 * The prompt is consumed one position per step.  use_graph != 0 captures one step into a
 * hipGraph and replays it.  state.logits holds the logits of the call's LAST step (where the logits projection carries the
 * greedy partials -- wipa_logits_greedy -- the other steps do not write them; a caller that wants every step's logits runs
 * one step per call, as decoding.forced_decode_logits does). */
int wipa_decoder_run(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B, int n_init,
                     int eot, const float* mask_first, const float* mask_always, int n_steps, int use_graph,
                     wipa_stream_t s);
/* The first n_init steps (the prompt positions 0..n_init-1 and the first generated token) as ONE batched pass: same
 * resulting state as wipa_decoder_run(..., n_steps = n_init, ...) right after wipa_decoder_begin, but the cached cross K/V
 * are streamed once for all prompt positions and the small per-step kernels run once (mlx_whisper also feeds the whole
 * prompt through the decoder in one forward).  Continue with wipa_decoder_run for the remaining steps. */
int wipa_decoder_prefill(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, int n_init,
                         int eot, const float* mask_first, const float* mask_always, int use_graph, wipa_stream_t s);
/* ONE DECODE CALL: what a call asks of its steps beyond the plain greedy update.  Every optional field is 0 / NULL for "not used"; a
 * call that holds only n_init, eot and the masks enqueues exactly what wipa_decoder_run / wipa_decoder_prefill enqueue.  The library
 * reads the struct during the call only and keeps no pointer to it: the step and prefill graphs are keyed on the VALUES of its fields
 * (integers, and the addresses the pointers hold), never on the address of the struct.  What the configuration's step cannot serve is
 * refused (WIPA_ERR_ARG, nothing enqueued) in a message that names the entry point and the field -- it is never decoded without it:
 *   rules, sample, sample_rows, starts_dev, beam and cfg.dec_n_group > 1 need the unfused step with the fused tail (not WIPA_DECODE_TAIL=0,
 *   not WIPA_DECODE_FUSED=1);  starts_dev, continuous and beam need bf16 / f32 decoder tables (cfg.dec_w_dtype == 0);  continuous needs
 *   cfg.dec_n_group == 1;  B is a multiple of cfg.dec_n_group.
 * Fields that exclude or need each other: sample and sample_rows exclude each other; sample_rows, no_speech_dev and prompted need
 * continuous; continuous needs starts_dev; no_speech_dev needs rules; beam excludes sample, sample_rows, starts_dev and continuous;
 * wipa_decoder_prefill_ex takes none of starts_dev, continuous, prompted, sample_rows, no_speech_dev (the prompt pass of rows with
 * their own prompts is wipa_decoder_prefill_ragged, that of an admitted clip belongs to wipa_decoder_admit_rows_prompted). */
/* An ADAPTER BANK on a decode call (wipa_decode_call.bank; csrc/lora_bank.hip, "adapter banks" at the end of this header): n unmerged
 * adapters of one rank on one set of sites, a different one per row.  Behind every targeted linear of a step and of the prompt pass
 * stands one wipa_lora_bank_apply (attn.query | key | value share one call over the 3d columns; the term of a residual site -- attn.out,
 * cross_attn.out, mlp2 -- is added into split-K slab 0 and folded in by the next wipa_add_slabs_layernorm; mlp1's GEMM runs without its
 * GELU and the apply call performs it).  With a bank the cross block takes its separate launches (LayerNorm, query GEMM, attention, out
 * GEMM) on both cross-attention forms; the logits projection is untouched.  The terms of cross_attn.key / cross_attn.value are added to
 * the CACHED cross K / V by wipa_decoder_adapt_cross; on the absorbed form (cfg.dec_cross_absorbed) a bank that targets them is refused.
 * Site s of a block, in the order its forward runs them: 0 attn.query, 1 attn.key, 2 attn.value, 3 attn.out, 4 cross_attn.query,
 * 5 cross_attn.key, 6 cross_attn.value, 7 cross_attn.out, 8 mlp1, 9 mlp2.
 * The struct and the two pointer arrays are HOST memory that the caller keeps alive and unchanged while graphs keyed on it may replay;
 * wipa_dec_layout and the state's scratch do not change (the kernels need no workspace). */
#define WIPA_BANK_SITES 10
typedef struct wipa_adapter_bank {
    int32_t n, rank;          /* adapters (1..64), their common rank (a multiple of 4 in 4..64) */
    uint32_t site_mask;       /* bit s: site s carries adapters */
    const float* const* A;    /* host [n_text_layer][WIPA_BANK_SITES] of device pointers: A [n, rank, in] f32; NULL at the other sites */
    const float* const* B;    /* likewise: B [n, out, rank] f32 */
    const float* gain;        /* device f32 [n]: alpha / rank of each adapter */
    const int32_t* ids_dev;   /* device int32 [B]: the adapter of every row, -1 for none; read by the replayed kernels */
} wipa_adapter_bank;
typedef struct wipa_decode_call {
    /* prompt columns (with starts_dev: the common prompt width P, 1..n_text_ctx; continuous: 1..4 initial tokens per clip; the prompt pass:
     * 1..4) and the end-of-text id */
    int32_t n_init, eot;
    /* additive f32 [n_vocab] masks of the first generated token and of every later one */
    const float *mask_first, *mask_always;
    /* The timestamp rules (wipa_decode_rules above) in every greedy update: the step's tail is wipa_timestamp_step_embed, the prompt pass
     * ends with wipa_timestamp_step (rule 4 acts on the first sampled token).  The three values are part of the step graph's and the prefill
     * graph's key.  With rules every step writes its logits and the row-scan tail reads them (the per-wave partials of wipa_logits_greedy
     * cannot carry rules that depend on the row's history), so no step of the call is lean. */
    const wipa_decode_rules* rules;
    /* A temperature above 0: the device sampling record (wipa_sample_record_bytes above); rules may be given or not.  The step's tail is
     * wipa_sample_step_embed, the prompt pass ends with wipa_sample_step; sampling steps write their logits and use the row-scan tail, like
     * steps with rules: the draw needs every alive column of the row.  The graph key holds the record's ADDRESS, not its contents: rewriting
     * seed, attempt, temperature or streams replays the same graph.  wipa_dec_layout does not change. */
    const void* sample;
    /* continuous with a TEMPERATURE PER ROW: the sampling record with a row part (wipa_sample_rows_bytes above, 16-byte aligned).  It takes
     * the place of `sample`, and the steps end in the rows_tail_continuous kernels: the four cases per row, the rules on the row's own
     * sequence, the no-speech store and the counter's own position p - start[b] stay; a row whose 1 / temperature is 0 takes the greedy
     * pick, every other row the draw at its own temperature, attempt and stream -- a retried window beside first attempts and beside
     * retries at other temperatures, in ONE launch.  wipa_decoder_admit_rows is called with sample == NULL, and wipa_sample_rows_set for the
     * same slots.  The step graph's key is that of the call without the record plus a variant bit and the record's address.  On bf16 the
     * logits projection writes the logits.  Without rules a greedy row's pick is row_pick's arg-max (the same token as without the record;
     * its log-probability sums the exponentials in the rules tails' order). */
    const void* sample_rows;
    /* Rows with their own first column, on the device, caller-owned; its ADDRESS is part of the step graph's key, the replayed kernels read
     * it.  With it the step's self-attention, its tail and its head are the RAGGED instantiations, and every step writes its logits and
     * ends in the row-scan tail (as with rules).  What it holds follows the call:
     *   int32 [B]     per-row prompts (after wipa_decoder_begin_ragged): the rows' first own columns; n_init = P.  The prompt is walked one
     *                 column per step ("p + 1 < n_init: the given token is taken"); column P is the first generated one for every row.
     *                 n_steps <= n_text_ctx - 1 (the position lives on the device and a call may include the P - 1 steps of the prompt walk,
     *                 so this is the bound that holds at every position; the caller keeps P + new tokens <= n_text_ctx).
     *   int32 [2][B]  continuous: first own columns, then the tokens each row may generate (see "Continuous batching" below)
     *   int32 [3][B]  continuous and prompted: window starts, token limits, prompt columns (see "a PROMPT PER ROW" below) */
    const int32_t* starts_dev;
    /* Continuous batching: the B rows are slots and the step ends in the CONTINUOUS tails (a prompt end per row); everything before the
     * tail is the ragged step.  The step graph's key is that of the ragged call plus a variant bit; admissions and shifts replay the same
     * graph.  With rules the pick applies them to the row's OWN sequence, the tokens of columns own .. p: its length is p + 1 - own, the pick at
     * p + 1 == own is the first one (mask_first; text dead, timestamps capped by max_initial_timestamp_index), and no token below own is
     * looked at -- those are the slot's previous clip, which usually ended in timestamps, or the prompt.  A shift moves the starts and the
     * tokens together, so a pick cannot see it.  With a sampling record the draw's counter takes the row's own position p - start[b]. */
    int32_t continuous;
    /* continuous with a prompt per row: the step ends in the PROMPTED tails (the sot sequence stands behind the row's prompt): own =
     * start + L + n_init, the no-speech store at column start + L, the rules on tk[own .. p], the draw's counter p - start (the row's position
     * in its own unpadded sequence).  Head and attention are the RAGGED kernels as they are.  The key gains a variant bit of its own. */
    int32_t prompted;
    /* continuous with rules: float [B] on the device, caller-owned.  At the step whose column is a row's first own one (p == start[b],
     * limit > 0: the row's <|startoftranscript|>, upstream's logits[:, sot_index]) the tail writes softmax(logits row)[no_speech_token] of
     * the UNFILTERED row to no_speech_dev[b], with a plain store; the value stays until the slot's next admission reaches that step.  Its
     * address and no_speech_token (a vocabulary column) are part of the step graph's key. */
    float* no_speech_dev;
    int32_t no_speech_token;
    /* Beam search (below): the caller's beam buffer, its size (at least wipa_beam_bytes) and the size of a clip's finished store (1..64).
     * The rows are clips x cfg.dec_n_group beams (1..16); the self-attention reads the cache through the buffer's ancestor table
     * (wipa_decode_attn_beam) and the step ends in the beam tail on the written logits; rules may be given.  The step graph is keyed on
     * the buffer's address and on beam_max_candidates. */
    void* beam;
    size_t beam_bytes;
    int32_t beam_max_candidates;
    /* An adapter bank (above): every row decodes under the adapter bank->ids_dev names for it.  NULL: the call of a model without a bank,
     * launch for launch.  The bank's address, ids_dev's address and (n, rank, site_mask) are part of the step graph's and the prefill
     * graph's key; the ids are not: rewriting them replays the same graph.  Rows with their own prompts take wipa_decoder_prefill_ragged_bank, a
     * prompted admission wipa_decoder_admit_rows_prompted_bank; behind an unprompted admission the caller writes the slot's id and calls
     * wipa_decoder_adapt_cross.  Refused by name, nothing enqueued: with beam, on fp8 decoder tables, with WIPA_DECODE_FUSED=1 or
     * WIPA_DECODE_TAIL=0, and a bank on cross_attn.key / cross_attn.value with cfg.dec_cross_absorbed. */
    const wipa_adapter_bank* bank;
} wipa_decode_call;
/* wipa_decoder_run / wipa_decoder_prefill for a wipa_decode_call; those two are these with a call of n_init, eot and the masks. */
int wipa_decoder_run_ex(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B,
                        const wipa_decode_call* call, int n_steps, int use_graph, wipa_stream_t s);
int wipa_decoder_prefill_ex(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B,
                            const wipa_decode_call* call, int use_graph, wipa_stream_t s);
/* Measurement / test aid: the number of captured decode graphs (steps and prompt passes) this process holds.  Two calls that differ
 * only in what a device array of their key holds (the sampling record, the starts, an adapter bank's ids) leave it unchanged. */
int wipa_decoder_graph_count(void);
/* The cross_attn.key / cross_attn.value terms of an adapter bank, added to the CACHED cross K / V behind wipa_decoder_set_audio (all
 * clips: slots_host NULL, n_rows = B / cfg.dec_n_group, features as wipa_decoder_set_audio took them) or wipa_decoder_admit_rows (the
 * n_rows listed slots; features [n_rows, n_audio_ctx, d] T in that order): K[clip] += 64^-0.25 gain[id] (xa A_k[id]^T) B_k[id]^T and
 * V[clip] += gain[id] (xa A_v[id]^T) B_v[id]^T in the layout [clip][K|V][H][Ta][64], one wipa_lora_bank_apply per layer (per layer and
 * slot with slots_host) with rows_per_id = n_audio_ctx.  A clip's id is bank->ids_dev[clip * cfg.dec_n_group]: that of its first row.
 * A bank without those two sites enqueues nothing.  Refused: cfg.dec_cross_absorbed with such a bank, fp8 decoder tables. */
int wipa_decoder_adapt_cross(const wipa_model_cfg* cfg, const void* const* w, void* state, size_t state_bytes, int B, const void* features,
                             int n_rows, const int32_t* slots_host, const wipa_adapter_bank* bank, wipa_stream_t s);
/* Beam search (upstream's BeamSearchDecoder + MaximumLikelihoodRanker; DecodingOptions.beam_size / patience / length_penalty).  The B rows
 * of a call are B / n_group clips x n_group beams, clip-major, with cfg.dec_n_group = n_group = beam_size (1..16; 1 is one row per clip).
 * Per step and clip, every beam offers the n_group + 1 best columns of its FILTERED row (the row the greedy / rules tails reduce;
 * logprob = l[c] - logsumexp(l), lowest column on ties); the candidates are walked in descending sum_logprobs[row] + logprob (one f32
 * add; ties: lower beam, then lower rank): a candidate ending in eot joins the clip's finished store while that holds fewer than
 * max_candidates = round(beam_size * patience) sequences, any other becomes the next beam until n_group are saved.  On the first
 * generated step only beam 0 offers (the beams of a clip are one sequence there).  Live beams never hold eot: there is no EOT latch.
 * A clip is complete when its store holds max_candidates sequences; it keeps stepping and its store no longer changes.  Where
 * max_candidates < n_group (patience below 1) the completing step itself fills the store up to n_group with that step's new beams + eot,
 * in descending sum_logprobs, as upstream's finalize would right there: the store's row needs columns up to *pos_dev + 2 < ld_tok.
 * The self-attention cache is NOT permuted: new K / V go to row b's own physical row and the ancestor table says where a beam's
 * history lies (wipa_decode_attn_beam).
 * The caller-owned device buffer `beam` of wipa_beam_bytes(B, n_group, max_candidates, ld_tok) bytes, 16-byte aligned, every part
 * rounded up to 256 bytes, cap = max(n_group, max_candidates), clips = B / n_group:
 *   anc        uint8 [B][ld_tok]              group-local physical row that holds column t of row b's history (row stride ld_tok)
 *   candidates {f32 logprob, i32 column} [B][n_group + 1]   the rows' offers of the current step, sorted
 *   src        int32 [B]                      the row (group-local) every beam of the last step descends from
 *   finished   int32 [clips][cap][ld_tok]     the store's sequences from column 0, eot behind the last token
 *   scores     f32   [clips][cap]             their sum_logprobs
 *   lengths    int32 [clips][cap]             their generated tokens before eot
 *   counts     int32 [clips]                  sequences in the store
 *   counters   int32 [64]                     [0] clips of the running step whose store is not full, [1] arrived workgroups
 * wipa_beam_begin clears the counts and the counters and writes the identity table (after wipa_decoder_begin, before the prompt pass).
 * wipa_beam_step is the selection alone on any rows (no embedding, no position advance), like wipa_sample_step: tokens column
 * *pos_dev + 1, the gathered token rows and table, sum_logprobs, the store, and *not_done = the clips whose store is not full after
 * this step.  rules may be NULL.  The prompt pass and the steps of a beam decode are wipa_decoder_prefill_ex / wipa_decoder_run_ex with
 * wipa_decode_call.beam.
 * wipa_beam_finalize (after the last step; n = generated columns): a clip with fewer than n_group finished sequences is filled with its
 * live beams + eot in descending sum_logprobs; then wipa_rank_groups' arithmetic over the store -- (double)sum / penalty[length],
 * penalty f64 [n + 1], first maximum -- and per clip the winner's columns [0, sample_begin + length) followed by eot up to column
 * sample_begin + n, its sum_logprobs and its length. */
size_t wipa_beam_bytes(int B, int n_group, int max_candidates, int64_t ld_tok);
int wipa_beam_begin(void* beam, size_t beam_bytes, int B, int n_group, int max_candidates, int64_t ld_tok, wipa_stream_t s);
int wipa_beam_step(const float* logits, int64_t ldl, int B, int V, const float* mask_first, const float* mask_always, int32_t* tokens,
                   int64_t ld_tok, int32_t* pos_dev, int n_init, int eot, const wipa_decode_rules* rules, void* beam, int n_group,
                   int max_candidates, float* sum_logprobs, int32_t* not_done, wipa_stream_t s);
int wipa_beam_finalize(void* beam, const int32_t* tokens, int64_t ld_tok, int B, int n_group, int max_candidates, int sample_begin, int n,
                       int eot, const float* sum_logprobs, const double* penalty, int32_t* best_tokens, int64_t ld_out, float* best_sum,
                       int32_t* best_len, wipa_stream_t s);
/* Per-row prompts (mlx_whisper.transcribe's condition_on_previous_text / initial_prompt, DecodingOptions.prompt / prefix: each row's
 * initial tokens are [sot_prev] + history + sot_sequence + prefix, 1..n_text_ctx of them), in the layout described at
 * wipa_embed_layernorm_ragged above.
 * wipa_decoder_begin_ragged: wipa_decoder_begin for rows that differ.  tokens_host int32 [B, P] (HOST): row b's own tokens in columns
 *   [starts_host[b], P), 0 below; starts_host int32 [B] (HOST); both are copied in stream order (tokens into the blob, starts into the
 *   caller-owned DEVICE array starts_dev int32 [B], which the later calls take).  pos = 0, counters and log-prob sums cleared.
 *   Refused (WIPA_ERR_ARG, nothing enqueued): P outside 1..n_text_ctx, a start outside 0..P-1 (every row holds at least one token), a
 *   token outside the vocabulary, fp8 decoder tables.
 * The steps of such rows are wipa_decoder_run_ex with wipa_decode_call.starts_dev = starts_dev and n_init = P. */
/* wipa_decoder_prefill_ragged: the first P steps (columns 0 .. P-1 and the first generated token) as ONE batched pass, right after
 *   wipa_decoder_begin_ragged; continue with wipa_decoder_run_ex (starts_dev).  The state it leaves is what stepping the prompt leaves, up to
 *   the rounding of the batched kernels: the pass is the teacher-forced layer body (GEMMs over B * P rows, wipa_attention for both
 *   attentions) writing K / V of every column into the blob's self-attention cache; cross K / V come from the blob's cache, or with
 *   absorbed projections are projected per layer from the blob's copy of the encoder output into the workspace.  Logits exist for two
 *   columns per clip: column P - 1 goes to state.logits and feeds the first greedy / rules / sampling update, and column sot_col (the
 *   rows' <|startoftranscript|>, the same column for every row; -1: none) goes to f32 [B, ld_logits] at OFFSET 0 of the workspace
 *   (upstream's logits[:, sot_index], for no_speech_prob).  workspace: caller-owned, wipa_decoder_prompt_workspace_bytes(cfg, B, P)
 *   bytes, 256-byte aligned; the blob layout does not change.  Captured into a graph like wipa_decoder_prefill: P, sot_col and the
 *   addresses of starts_dev and of the workspace are part of its key.  Refused: what a call with starts_dev is refused for, a workspace
 *   that is too small, P + 1 > n_text_ctx, sot_col outside -1 .. P-1. */
size_t wipa_decoder_prompt_workspace_bytes(const wipa_model_cfg* cfg, int B, int P);
int wipa_decoder_prefill_ragged(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B, int P,
                                int sot_col, int eot, const float* mask_first, const float* mask_always, int use_graph,
                                const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev, void* workspace,
                                size_t workspace_bytes, wipa_stream_t s);
/* wipa_decoder_prefill_ragged with an adapter bank (wipa_decode_call.bank; NULL: that call): row b's prompt columns run under the adapter
 * bank->ids_dev[b], one wipa_lora_bank_apply behind every targeted GEMM of the batched pass (rows_per_id = P; the residual sites add into
 * the f32 stream).  On the absorbed form the per-layer K / V workspace is projected without adapters: a bank on cross_attn.key / .value is
 * refused there as everywhere.  The steps behind it are wipa_decoder_run_ex with the same bank and starts_dev. */
int wipa_decoder_prefill_ragged_bank(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B, int P,
                                int sot_col, int eot, const float* mask_first, const float* mask_always, int use_graph,
                                const wipa_decode_rules* rules, const void* sample, const int32_t* starts_dev, void* workspace,
                                size_t workspace_bytes, const wipa_adapter_bank* bank, wipa_stream_t s);
int wipa_decoder_begin_ragged(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, const int32_t* tokens_host,
                              const int32_t* starts_host, int P, int32_t* starts_dev, wipa_stream_t s);
/* Continuous batching: the B rows of a state are SLOTS.  A clip is admitted into a slot at the column the state
 * stands at, decodes there with its own position embeddings, attention window, sampling counter AND prompt end, and when it has
 * finished the next clip takes the slot while the other rows go on.  starts_dev is int32 [2][B] on the device, caller-owned: starts_dev[b]
 * is the first own column of slot b's clip, starts_dev[B + b] the number of tokens it may generate (all zero: every slot is finished).
 * Per row, with own = start[b] + n_init, the step at column p (which fills column p + 1):
 *   p + 1 < own: the row is idle or in its prompt -- the token of column p + 1 is taken as it stands, nothing is written, nothing is
 *   counted, sum_logprobs[b] is untouched;  p + 1 == own: the pick under mask_first;  own < p + 1 < own + limit: the pick under mask_always;
 *   p + 1 >= own + limit: column p + 1 takes eot, without a log-probability, and the EOT latch holds the row from there on.
 * The latch is the token of column p: a slot leaves it when an admission writes initial tokens over the finished row's last column.
 * Served: both cross-attention forms, bf16 / f32 decoder tables, one row per clip, 1..4 initial tokens.  Refused by name
 * (WIPA_ERR_ARG, nothing enqueued): fp8 tables, candidate groups, a step without the fused tail.  The steps are wipa_decoder_run_ex with
 * wipa_decode_call.continuous (and rules, sample or sample_rows, no_speech_dev as wanted).
 * wipa_decoder_admit_rows: in stream order, for row i of n_rows: features_host[i] (a DEVICE pointer to the clip's encoder output
 *   [n_audio_ctx, d] in cfg.dtype; the array of pointers is on the host) is copied into slot slots_host[i] of the blob's audio copy
 *   (absorbed form), or projected into the slot's K / V of every layer as wipa_decoder_set_audio projects it (cached form: n_text_layer
 *   GEMMs of n_audio_ctx rows per admission; wipa_decoder_begin must have run on this process before, as for every decode); the
 *   n_init tokens initial_tokens_host[i][0 .. n_init) go to columns [c, c + n_init) of the slot, c being the state's position: the column
 *   the next step reads (the finished row's last token, which the caller has copied out, is overwritten; every run call re-embeds column
 *   c before its first step); starts_dev[slot] = c, starts_dev[B + slot] = limits_host[i]; sum_logprobs[slot] = 0; with a sampling record
 *   (sample, the record the run calls take) the slot's Philox stream becomes streams_host[i] = (lo, hi).  An admission whose initial
 *   tokens would not leave one column to generate in the table (c + n_init >= n_text_ctx) is not carried out: shift first.
 * wipa_decoder_shift_columns: for every row, the token columns [shift, pos] move to [0, pos - shift], and so do the self-attention K / V
 *   rows of every layer; pos and every start drop by shift.  A row whose start lies below shift (finished, or never admitted) ends with
 *   start 0 and limit 0.  Source and destination overlap: no scratch buffer, an ORDER -- one workgroup owns a (layer, K | V, row) strip
 *   and walks it in ascending chunks, all loads of a chunk before a barrier and all its stores after it; the destination lies below the
 *   source, so no store reaches bytes a later chunk still has to load.  Plain vector loads and stores.  Position embedding, attention
 *   window and sampling counter are relative to the row's start, and the attention kernel walks a row's keys from its start in the
 *   same partition wherever that start lies, so a shift changes no bit of what a row computes.  Refused: shift outside
 *   1..n_text_ctx-1; a shift above the position is not carried out. */
int wipa_decoder_admit_rows(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B, int n_rows,
                            const int32_t* slots_host,
                            const void* const* features_host, const int32_t* initial_tokens_host, int n_init, const int32_t* limits_host,
                            int32_t* starts_dev, void* sample, const uint32_t* streams_host, wipa_stream_t s);
int wipa_decoder_shift_columns(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, int32_t* starts_dev, int shift,
                               wipa_stream_t s);

/* Continuous batching with a PROMPT PER ROW.  A clip is still admitted at the state's column c; its prompt of L
 * columns ([sot_prev] + history; L = 0: none) stands IN FRONT of that column, at [c - L, c), and its n_init initial tokens at
 * [c, c + n_init), where they stand without a prompt.  The prompted calls take starts_dev as int32 [3][B]: row 0 the window start c - L
 * (what the RAGGED attention, the position rows and the tails' next-input row read), row 1 the token limit, row 2 the prompt columns L.
 * wipa_decoder_shift_columns serves such an array as it is: it moves rows 0 and 1 and does not look past them, and the K / V of
 * prompt columns move with the rest.  The caller keeps the position at or above the widest prompt it will admit:
 * wipa_decoder_seek: puts the position of an IDLE state (after wipa_decoder_begin, no live row) at `column`, and with it the offset
 *   the step's q|k|v GEMM scatters at.  Refused (WIPA_ERR_ARG) unless 0 <= column < n_text_ctx - 1.
 * wipa_decoder_admit_prompted_workspace_bytes: the DEVICE workspace an admission of n_rows rows with prompt width W takes.
 * wipa_decoder_admit_rows_prompted: wipa_decoder_admit_rows (sampling streams included) for rows with prompts.  prompt_lens_host[i] is
 *   L_i, prompt_tokens_host int32 [n_rows][W] holds row i's prompt RIGHT-ALIGNED (columns W - L_i .. W-1; what lies in front is not
 *   looked at), W >= max L_i.  Tokens and the three starts entries are written on the device from the position read there; an admission
 *   with c - W < 0, or without a column left to generate (c + n_init >= n_text_ctx), is not carried out at all.  With W > 0 ONE batched
 *   layer walk over the packed rows [n_rows * W] (local starts W - L_i, cross K / V projected from the admitted clips' features into
 *   the workspace) follows, each layer's q|k|v GEMM followed by a scatter of the prompt columns' K and V rows into
 *   [layer][K | V][slot_i][c - L_i, c) of the self-attention cache; the last layer stops behind its q|k|v GEMM and no logits are
 *   computed (the step at column c produces the sot-column logits itself).  Host arrays may be freed when the call returns.
 *   Refused by name (WIPA_ERR_ARG, nothing enqueued): what wipa_decoder_admit_rows refuses, W or an L_i outside
 *   0 .. n_text_ctx - n_init - 1, L_i > W, a prompt token outside the vocabulary, a workspace that is too small.
 * The steps of a prompted state are wipa_decoder_run_ex with wipa_decode_call.continuous and .prompted, on the [3][B] starts_dev. */
int wipa_decoder_seek(const wipa_model_cfg* cfg, void* state, size_t state_bytes, int B, int column, wipa_stream_t s);
size_t wipa_decoder_admit_prompted_workspace_bytes(const wipa_model_cfg* cfg, int n_rows, int W);
int wipa_decoder_admit_rows_prompted(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B, int n_rows,
                                     const int32_t* slots_host, const void* const* features_host, const int32_t* initial_tokens_host,
                                     int n_init, const int32_t* limits_host, const int32_t* prompt_lens_host,
                                     const int32_t* prompt_tokens_host, int W, int32_t* starts_dev, void* sample,
                                     const uint32_t* streams_host, void* workspace, size_t workspace_bytes, wipa_stream_t s);
/* wipa_decoder_admit_rows_prompted with an adapter bank: ids_host int32 [n_rows] (HOST) names the admitted clips' adapters (-1: none).
 * The call writes bank->ids_dev[slot] with a plain copy before the slot's first step, adds the clip's cross K / V terms to the cached
 * K / V behind its projection (wipa_decoder_adapt_cross) and runs the prompt pass of the admitted rows under their adapters. */
int wipa_decoder_admit_rows_prompted_bank(const wipa_model_cfg* cfg, const void* const* weights, void* state, size_t state_bytes, int B, int n_rows,
                                     const int32_t* slots_host, const void* const* features_host, const int32_t* initial_tokens_host,
                                     int n_init, const int32_t* limits_host, const int32_t* prompt_lens_host,
                                     const int32_t* prompt_tokens_host, int W, int32_t* starts_dev, void* sample,
                                     const uint32_t* streams_host, void* workspace, size_t workspace_bytes, const wipa_adapter_bank* bank,
                                          const int32_t* ids_host, wipa_stream_t s);
/* drop the cached step graphs that reference this state blob (call before freeing it). */
int wipa_decoder_release(void* state);

/* Teacher-forced TextDecoder.__call__ = Whisper.logits (train_whisper_ipa.py:232).
 * tokens [B,T] int32, features [B, n_audio_ctx, d] T -> logits [B*T, ld_logits] f32. */
size_t wipa_decoder_logits_workspace_bytes(const wipa_model_cfg* cfg, int B, int T);
int wipa_decoder_logits(const wipa_model_cfg* cfg, const void* const* weights, const int32_t* tokens, const void* features,
                        float* logits, int64_t ld_logits, void* workspace, size_t workspace_bytes, int B, int T,
                        wipa_stream_t s);

/* find_alignment's device part on the same teacher-forced pass (one layer body shared with wipa_decoder_logits):
 *   tokens [B, T] int32 (rows padded past n_tokens[b] with any valid id), features [B, n_audio_ctx, d];
 *   heads_host: n_heads (layer, head) pairs (HOST int32 [2 n_heads]); after the cross-attention projections of every layer that
 *   has some, wipa_align_weights adds them -- in list order within a layer, layers in stream order -- and the last such call
 *   divides by n_heads;  n_tokens / n_frames int32 [B] on the device, *_host their host copies (checked before any launch);
 *   matrix f32 [B, T, n_audio_ctx] receives the head mean (rows / frames outside a clip's range are 0);
 *   the DTW (wipa_dtw_batch) then runs on rows [first_row, first_row + n_rows[b]) and frames [0, n_frames[b]) into text_idx /
 *   time_idx [B, ld_path], path_len [B]: n_rows[b] = n_tokens[b] - first_row - 1 is upstream's matrix[len(sot_sequence) : -1],
 *   0 leaves the clip without a path (n_rows device, n_rows_host its host copy);
 *   token_probs f32 [B, T]: wipa_token_probs of the final logits, which are projected in blocks of logits_rows rows
 *   (0 = as many as fit 1 GiB of f32 logits) and never exist as a whole.
 * fp8 decoder weight tables are refused, as by wipa_decoder_logits. */
size_t wipa_decoder_align_workspace_bytes(const wipa_model_cfg* cfg, int B, int T, int n_heads, int logits_rows);
int wipa_decoder_align(const wipa_model_cfg* cfg, const void* const* weights, const int32_t* tokens, const void* features,
                       const int32_t* heads_host, int n_heads, const int32_t* n_tokens, const int32_t* n_frames,
                       const int32_t* n_rows, const int32_t* n_tokens_host, const int32_t* n_frames_host, const int32_t* n_rows_host,
                       int first_row, int eot, float* matrix,
                       int32_t* text_idx, int32_t* time_idx, int64_t ld_path, int32_t* path_len, float* token_probs, int logits_rows,
                       void* workspace, size_t workspace_bytes, int B, int T, wipa_stream_t s);

/* ------------------------------------------------------------------ K9 masked CE
 * compute_loss of train_whisper_ipa.py:207-263 on teacher-forced logits.
 * logits [B*T, ldl] f32 (T = tokens_len - 1), tokens [B, ld_tok] int32: input t, target t+1.
 * mask = (tgt != eot) | (cumsum(tgt == eot) == 1).  row_buf f32 [2*B*T] receives the
 * per-row mask*ce and mask; out2[0] = sum(mask*ce), out2[1] = sum(mask) (fixed-order sum). */
int wipa_masked_ce(const float* logits, int64_t ldl, const int32_t* tokens, int64_t ld_tok, int B, int T, int V, int eot,
                   float* row_buf, float* out2, wipa_stream_t s);

/* ------------------------------------------------------------------ fine-tune step (f32)
 * Backward of the teacher-forced decoder + masked CE w.r.t. the decoder parameters, i.e. what
 * nn.value_and_grad(model, loss_fn) computes at scripts/train_whisper_ipa.py:284 with the encoder
 * frozen (:187), then the per-tensor clip (:287-303) and optim.AdamW (:306,513).  The dense
 * contractions are wipa_gemm calls on operands transposed by wipa_transpose; all kernels are
 * deterministic (no float atomics). */
/* out[c][r] = in[r][c]; out columns rows..rows_pad-1 are written as zero (K padding for wipa_gemm). */
int wipa_transpose(const void* in, int64_t ld_in, void* out, int64_t ld_out, int rows, int cols, int rows_pad, int dtype,
                   wipa_stream_t s);
/* out[c] (+)= sum_r x[r][c]  (bias gradients), summed in a fixed order.  workspace (optional, f32): with at least
 * 2*cols floats the rows are cut into up to 64 chunks reduced by separate workgroups (partials in the workspace). */
int wipa_colsum(const float* x, int64_t ld, int rows, int cols, float* out, int accumulate, float* workspace,
                int64_t workspace_floats, wipa_stream_t s);
/* out[i] (+)= sum over k of slabs[k * slab_stride + i], k ascending: the reduction of a split-K wipa_gemm (k_slices > 1). */
int wipa_sum_slabs(const float* slabs, int n_slabs, int64_t slab_stride, float* out, int64_t n, int accumulate, wipa_stream_t s);
/* out[i] = scale * sum over k of slabs[k * slab_stride + i] (k ascending) + (residual ? residual[i] : 0): finishes a split-K GEMM
 * whose slices cannot apply a column scale or a residual themselves (bias rides on slice 0).  residual may alias out. */
int wipa_sum_slabs_ex(const float* slabs, int n_slabs, int64_t slab_stride, float* out, int64_t n, const float* residual,
                      float scale, wipa_stream_t s);
/* LayerNorm backward: dx (+)= ..., dw, db.  stats: f32 scratch of stats_floats elements, at least 2*rows (mean, rstd per row);
 * with room for 2*rows + 64*D the dw / db column sums are cut into up to 32 row chunks reduced by separate workgroups and
 * added in a fixed order.  x, dy, dx contiguous [rows, D]. */
int wipa_layernorm_bwd(const float* x, const float* dy, const float* w, float* dx, int accumulate_dx, float* dw, float* db,
                       float* stats, int64_t stats_floats, int rows, int D, float eps, wipa_stream_t s);
/* exact-erf GELU forward / backward on n (multiple of 4) contiguous f32 values. */
int wipa_gelu(const float* z, float* u, int64_t n, wipa_stream_t s);
int wipa_gelu_bwd(const float* z, const float* du, float* dz, int64_t n, wipa_stream_t s);
/* In place: logits[r][v] <- mask_r * (softmax_r[v] - [v == target_r]) / max(count[0], 1).
 * row_mask = the second half of wipa_masked_ce's row_buf; count = &out2[1] (or its all-reduced value). */
int wipa_masked_ce_bwd(float* logits, int64_t ldl, const int32_t* tokens, int64_t ld_tok, int B, int T, int V,
                       const float* row_mask, const float* count, wipa_stream_t s);
/* d_tok_emb[tokens[r]] += dx[r] (rows visited in order), d_pos_emb[t] = sum_b dx[b*T+t]. tokens_flat int32 [B*T]. */
int wipa_embed_bwd(const int32_t* tokens_flat, const float* dx, int B, int T, int D, float* d_tok_emb, float* d_pos_emb,
                   wipa_stream_t s);
/* Backward of wipa_attention (f32): d is the forward descriptor (q,k,v pre-scaled); out / d_out share the
 * o_* strides; dq,dk,dv share the q/k/v strides; dvec f32 [B,H,Tq] scratch. dq and dk are multiplied by qk_scale.
 * Every batch, row and head stride must be a multiple of 4 floats (16-byte rows), or the call is refused. */
int wipa_attention_bwd(const wipa_attn_desc* d, const float* out, const float* d_out, const float* lse, float* dq, float* dk,
                       float* dv, float* dvec, float qk_scale, wipa_stream_t s);
/* The same call with a choice of arithmetic.  f32_split = 0: wipa_attention_bwd.  1: both kernels take their five matmuls (Q K^T, dO V^T,
 * dS K, P^T dO, dS^T Q) on the bf16 MFMA over f32 operands split in registers, with the helper and the term selection of the encoder's
 * split forward (wipa_flash_attn_enc_f32, f32_split): three terms per operand and six products where a product forms a score or a
 * probability gradient, two terms and three products where it consumes P / dS; exponentials, D and accumulators stay f32.  Same strides,
 * same refusals, deterministic.  For the encoder's Tq = Tk = n_audio_ctx self-attention in the fine-tune step (no reference counterpart). */
int wipa_attention_bwd_ex(const wipa_attn_desc* d, const float* out, const float* d_out, const float* lse, float* dq, float* dk,
                          float* dv, float* dvec, float qk_scale, int f32_split, wipa_stream_t s);
/* Conv stem of the AudioEncoder in the fine-tune step (csrc/conv_bwd.hip; the reference freezes the encoder, train_whisper_ipa.py:187,
 * so these have no counterpart there).  conv1 / conv2 run as wipa_gemm calls over overlapping rows that keep the PRE-activation values.
 * wipa_conv_stem_gelu_pos: x[b][t][:] = gelu(z[b][t][:]) + pos[t][:] for z, x [B*N, d] contiguous, pos [>= N, d]; d a multiple of 4.
 * wipa_conv2_dx: the input gradient of conv2 (k3, s2, p1) folded back onto the 2N conv1 frames and through conv1's GELU:
 *   taps: dz2 W2 of position t of clip b, three blocks of d floats (tap 0, 1, 2) at taps + b*taps_clip_stride + t*3*d;
 *   z1:   conv1's pre-activation of frame s of clip b at z1 + b*z1_clip_stride + s*d;  dz1 likewise with dz1_clip_stride;
 *   dz1[s] = gelu'(z1[s]) * (s even: tap 1 of s/2;  s odd: tap 2 of (s-1)/2, then + tap 0 of (s+1)/2 when (s+1)/2 < N).
 *   Rows 2N .. 2N + zero_rows - 1 of every clip of dz1 are written as zero.  No atomics, a fixed order: the bits of a clip do not
 *   depend on the batch.  Nothing outside the N*3 tap rows and the 2N z1 rows of a clip is read.  Strides in floats, multiples of 4. */
int wipa_conv_stem_gelu_pos(const float* z, const float* pos, float* x, int B, int N, int d, wipa_stream_t s);
int wipa_conv2_dx(const float* taps, int64_t taps_clip_stride, const float* z1, int64_t z1_clip_stride, float* dz1,
                  int64_t dz1_clip_stride, int B, int N, int d, int zero_rows, wipa_stream_t s);
/* Flat multi-tensor optimiser step: per-tensor g *= min(1, max_norm/(|g|+1e-6)), then mlx-style AdamW
 * (no bias correction): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p = p (1 - lr wd) - lr m / (sqrt(v)+eps).
 * Tensors live in flat f32 buffers; a chunk table (<= 4096 elements per chunk, never crossing tensors)
 * drives the kernels: chunk_off/len/seg [n_chunks], seg_first_chunk [n_seg+1]; partial [n_chunks],
 * coef/norms [n_seg] are scratch/outputs.
 * seg_clip int32 [n_seg] or NULL: which tensors the clip reaches.  The reference's clip_grad_dict
 * (scripts/train_whisper_ipa.py:287-303) recurses through dict values only; a list value (decoder.blocks) is neither a
 * dict nor an array and is passed through (:299-300), so a caller reproducing it passes 0 for every decoder.blocks.*
 * tensor (coefficient exactly 1, norm still reported) and 1 for token_embedding.weight, positional_embedding, ln.*.
 * NULL clips every tensor. */
int wipa_clip_adamw(float* params, float* grads, float* m, float* v, const int64_t* chunk_off, const int32_t* chunk_len,
                    const int32_t* chunk_seg, const int32_t* seg_first_chunk, int n_chunks, int n_seg, float* partial,
                    float* coef, float* norms, const int32_t* seg_clip, double max_norm, double lr, double beta1, double beta2,
                    double eps, double weight_decay, wipa_stream_t s);

/* ------------------------------------------------------------------ low-rank adapters (csrc/lora.hip; no reference counterpart)
 * A frozen linear y = (x W^T + b) c gains the term c s (x A^T) Bm^T with A [r, K] and Bm [N, r] contiguous f32, s = alpha / r; only A
 * and Bm are trained.  All operands are f32; every product is an exact f32 product accumulated in f32 (the f32 MFMA, bit-equal to an
 * fmaf chain), never the split-bf16 path.  r is a multiple of 4 in 4..64, K and N are multiples of 4, every pointer and every row is
 * 16-byte aligned (leading dimensions in floats, multiples of 4); anything else is refused with a message that names the argument.
 * No float atomics: the same call gives the same bits twice.
 *
 * wipa_lora_workspace_bytes: the scratch wipa_lora_bwd needs for M rows -- du [M, r] and the fixed-order partial sums of dA and dB, one
 *   [r, K] and one [r, N] block per row chunk (chunks of at least 64 rows, at most 128 of them). */
size_t wipa_lora_workspace_bytes(int M, int K, int N, int r);
/* Forward, two launches.  y [M, ldy] already holds the base output (x W^T + b) c.  Writes u[m][j] = sum_k x[m][k] A[j][k] into u [M, r]
 * (contiguous; kept for the backward), then y[m][n] += gain * sum_j u[m][j] Bm[n][j] with gain = c s (the caller's column scale sits
 * inside it).  ldy may exceed N (the cross key | value halves of one [rows, 2d] buffer): columns >= N of a y row are never touched. */
int wipa_lora_fwd(const float* x, int64_t ldx, const float* A, const float* Bm, float* y, int64_t ldy, float* u, int M, int K, int N,
                  int r, float gain, wipa_stream_t s);
/* Backward, three launches.  du[m][j] = gain sum_n dy[m][n] Bm[n][j] (kept in the workspace);  dB[n][j] = gain sum_m dy[m][n] u[m][j];
 * dA[j][k] = sum_m du[m][j] x[m][k];  with dx != NULL: dx[m][k] (+)= sum_j du[m][j] A[j][k] (accumulate_dx: added to what dx holds);
 * dx == NULL skips that term (an input that carries no gradient: the frozen encoder output).  dA [r, K] and dB [N, r] are overwritten.
 * The sums over m run over row chunks whose partials land in the workspace and are added in ascending chunk order. */
int wipa_lora_bwd(const float* dy, int64_t ldy, const float* x, int64_t ldx, const float* u, const float* A, const float* Bm, float* dA,
                  float* dB, float* dx, int64_t lddx, int accumulate_dx, int M, int K, int N, int r, float gain, void* workspace,
                  size_t workspace_bytes, wipa_stream_t s);
/* W[n][k] = cast(float(base[n][k]) + s sum_j Bm[n][j] A[j][k]) for W, base [N, K] of dtype WIPA_F32 or WIPA_BF16 (leading dimensions in
 * elements): the sum over j ascending as an fmaf chain from zero, one fmaf with the base, one rounding at the end.  W may be base. */
int wipa_lora_merge(void* W, int64_t ldw, int dtype, const void* base, int64_t ld_base, const float* A, const float* Bm, int N, int K,
                    int r, float s, wipa_stream_t stream);

/* ------------------------------------------------------------------ adapter banks (csrc/lora_bank.hip; no reference counterpart)
 * n adapters (1..64) of one rank r and one set of sites, kept UNMERGED and applied per row behind a linear whose base output is in place:
 *   out[m, :] = cast(act(float(y[m, :]) + c gain[id] (x[m, :] A[id]^T) B[id]^T)),   id = ids[(m / rows_per_id) * ids_stride]
 * A [n, r, K] and B [n, N, r] are the site's adapters stacked, contiguous f32; gain [n] f32 holds alpha / r of each adapter; ids is an
 * int32 DEVICE array with one entry per rows_per_id rows, read by the kernel -- a captured graph serves any assignment.  A row whose id is
 * -1 gets act alone, and with act none its bytes are left alone; an id outside -1..n-1 is refused when ids_host (the same array in HOST
 * memory, optional) shows it, and treated as -1 by the kernel.  x [M, K] has x_dtype (f32 or bf16, row stride ldx); y and out have
 * y_dtype (f32 or x_dtype) and share one addressing, that of wipa_gemm_desc: element (m, n) lives at
 *   c_offset + (*c_offset_dev) + (m / rg_in) * rg_stride + (m % rg_in) * ld + (n / cg_in) * cg_stride + (n % cg_in)
 * (rg_in = 0: M, cg_in = 0: N: plain rows of ld elements), so the term lands where the base GEMM wrote -- the self K / V cache at the
 * current position, packed q|k|v rows, the cached cross K / V layout [clip][K|V][H][Ta][64], split-K slab 0 of a residual GEMM.  out may
 * be y.  act: 0 none, 1 the gelu(erf) of wipa_gemm's epilogue (a linear whose GEMM ran without it).  Accumulation is f32, exact f32
 * products; one rounding to y_dtype at the end.
 * Column segments: the N columns are n_seg (1..3) segments of N / n_seg columns that share x (a layer's query | key | value), segment s
 * with its own A[s], B[s] ([n, N / n_seg, r]) and column scale col_scale[s] (the c of the linear: 64^-0.25 on query and key columns);
 * A[s] == B[s] == NULL: the segment carries no adapter.
 * One launch.  rows_per_id < 16 and M <= 1024 (decode rows, the four-row prompt pass): one workgroup per row and 512 columns, u = A[id] x
 * recomputed per column chunk.  Everything else (prompt passes, the cross K / V projection with rows_per_id = Ta): tiles of 16 rows of
 * ONE id on the exact f32 MFMA; a tile never straddles two ids, a segment length that is no multiple of 16 is served.  No float atomics,
 * one writer per output element, the same bits on two calls, and a row's bits do not depend on any other row's id.
 * r a multiple of 4 in 4..64, K and N / n_seg multiples of 4; ld, ldx, rg_stride, cg_stride, cg_in, c_offset and *c_offset_dev multiples
 * of 4; x, y, out, A[s], B[s] 16-byte aligned.  Anything else is refused with a message that names the argument. */
#define WIPA_LORA_BANK_MAX_ADAPTERS 64
#define WIPA_LORA_BANK_MAX_SEG 3
typedef struct wipa_lora_bank_desc {
    const void* x;
    const void* y;
    void* out;
    const float* A[WIPA_LORA_BANK_MAX_SEG];
    const float* B[WIPA_LORA_BANK_MAX_SEG];
    const float* gain;
    const int32_t* ids;      /* device */
    const int32_t* ids_host; /* host, optional: checked before the launch */
    const int64_t* c_offset_dev;
    int64_t ldx, ld, rg_stride, cg_stride, c_offset;
    float col_scale[WIPA_LORA_BANK_MAX_SEG];
    int32_t M, K, N, r, n;
    int32_t rows_per_id, n_seg;
    int32_t ids_stride; /* row group g reads ids[g * ids_stride]; 0: 1 */
    int32_t x_dtype, y_dtype;
    int32_t rg_in, cg_in;
    int32_t act; /* 0 none, 1 gelu(erf) */
} wipa_lora_bank_desc;
int wipa_lora_bank_apply(const wipa_lora_bank_desc* d, wipa_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* WIPA_H */

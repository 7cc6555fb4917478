// A bank of low-rank adapters applied per row, unmerged: behind a linear whose base output y is already in place,
//     out[m, :] = cast(act(float(y[m, :]) + c gain[id] (x[m, :] A[id]^T) B[id]^T)),   id = ids[m / rows_per_id],   id = -1: no adapter
// (wipa_lora_bank_apply, include/wipa.h).  The n adapters of a site are stacked, A [n, r, K] and B [n, N, r] f32; ids lives on the device,
// so a captured decode step serves any assignment of adapters to rows.  ONE launch per call, two kernels by the rows that share an id:
//   row kernel   (rows_per_id < 16 and M <= 1024: decode rows, the few-row prompt pass)   one workgroup per (row, 512 columns).  u = A[id] x is r dot
//                products of length K, wave w taking j = w, w + 4, ... with 16-byte loads and a wave reduction; u is recomputed by every
//                column chunk (r x K multiply-adds against N x r: cheaper than a second launch).  Then one thread per column.
//   tile kernel  (everything else: prompt passes, the cross K / V projection)   one workgroup per (16 rows of ONE id, 512 columns), on
//                the exact f32 MFMA with the operand forms of lora.hip: u in the k-contiguous form, four waves cutting K and summed in
//                wave order through LDS -- which leaves u[row lr][16t + 4g + e] in acc[t][e] of lane (lr, g), exactly the S fragment
//                of the wide form -- then y = u B^T, one wave per 16 x 64 columns.  Tiles start at a segment's first row: none straddles
//                two ids, and a segment length that is no multiple of 16 ends in a partly filled tile.
// A call may cover up to three column segments of equal width that share x (a layer's query | key | value): each has its own A, B and
// column scale, and a segment without A is left alone.  Every output element has one writer, nothing is added atomically, and a row's
// arithmetic depends on its own id alone: the same bits on two calls, and whatever ids the other rows hold.
#include <algorithm>
#include <string.h>

#include "wipa_common.h"

namespace {

constexpr int COLS = 512;  // columns of a workgroup
constexpr int ROW_KERNEL_MAX_ROWS = 1024;  // more rows than a decode step or a four-row prompt pass has go to the tile kernel
constexpr int MAX_SEG = WIPA_LORA_BANK_MAX_SEG;

struct BankArgs {
    const void* x;
    const void* y;
    void* out;
    const float* A[MAX_SEG];
    const float* B[MAX_SEG];
    float c[MAX_SEG];
    const float* gain;
    const int32_t* ids;
    const int64_t* c_offset_dev;
    int64_t ldx, ld, rg_stride, cg_stride, c_offset;
    int M, K, seg_n, r, n, rows_per_id, ids_stride, rg_in, cg_in, act, chunks_per_seg;
};

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// four consecutive elements of a row of T as floats (k a multiple of 4: 16 bytes of f32, 8 of bf16)
template <typename T>
__device__ __forceinline__ f32x4 load4(const T* p, bool ok);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float* p, bool ok) { return ld4(p, ok); }
template <>
__device__ __forceinline__ f32x4 load4<__bf16>(const __bf16* p, bool ok) {
    if (!ok) return f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <typename T>
__device__ __forceinline__ void store4(T* p, f32x4 v);
template <>
__device__ __forceinline__ void store4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <>
__device__ __forceinline__ void store4<__bf16>(__bf16* p, f32x4 v) {
    *reinterpret_cast<bf16x4*>(p) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
}

// the adapter of row group grp, or -1 (an id outside the bank reads nothing: the host check of ids_host is what refuses it)
__device__ __forceinline__ int id_of(const BankArgs& a, int grp) {
    const int id = a.ids[(int64_t)grp * a.ids_stride];
    return id >= 0 && id < a.n ? id : -1;
}
// element offset of (row m, column n of the call) in y and out: wipa_gemm_desc's addressing
__device__ __forceinline__ int64_t out_offset(const BankArgs& a, int64_t base, int m, int n) {
    return base + (int64_t)(m / a.rg_in) * a.rg_stride + (int64_t)(m % a.rg_in) * a.ld + (int64_t)(n / a.cg_in) * a.cg_stride + n % a.cg_in;
}
__device__ __forceinline__ float finish(const BankArgs& a, float y, float scale, float acc) {
    const float v = fmaf(scale, acc, y);
    return a.act == 1 ? gelu_erf2(f32x2{v, v}).x : v;
}

// blockIdx.x: row; blockIdx.y: (segment, 512 columns of it)
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void bank_rows_kernel(const BankArgs a) {
    __shared__ float u[64];
    const int m = blockIdx.x;
    const int seg = blockIdx.y / a.chunks_per_seg, c0 = (blockIdx.y % a.chunks_per_seg) * COLS;
    const int id = a.A[seg] ? id_of(a, m / a.rows_per_id) : -1;
    if (id < 0 && a.act == 0) return;  // its bytes are left alone
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (id >= 0) {
        const TX* xp = (const TX*)a.x + (int64_t)m * a.ldx;
        const float* Ap = a.A[seg] + (int64_t)id * a.r * a.K;
        for (int j = wave; j < a.r; j += 4) {
            const float* aj = Ap + (int64_t)j * a.K;
            float s = 0.f;
            for (int k = 4 * lane; k < a.K; k += 256) {
                const f32x4 xv = load4<TX>(xp + k, true), av = ld4(aj + k, true);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(xv[e], av[e], s);
            }
            s = wave_reduce_sum(s);
            if (lane == 0) u[j] = s;
        }
    }
    __syncthreads();
    const float scale = id >= 0 ? a.c[seg] * a.gain[id] : 0.f;
    const float* Bp = id >= 0 ? a.B[seg] + (int64_t)id * a.seg_n * a.r : nullptr;
    const int64_t base = a.c_offset + (a.c_offset_dev ? *a.c_offset_dev : 0);
    const int cend = min(c0 + COLS, a.seg_n);
    for (int n = c0 + (int)threadIdx.x; n < cend; n += 256) {
        float acc = 0.f;
        if (id >= 0) {
            const float* bn = Bp + (int64_t)n * a.r;
            for (int j = 0; j < a.r; j += 4) {
                const f32x4 bv = ld4(bn + j, true);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fmaf(u[j + e], bv[e], acc);
            }
        }
        const int64_t o = out_offset(a, base, m, seg * a.seg_n + n);
        ((TY*)a.out)[o] = from_f32<TY>(finish(a, to_f32<TY>(((const TY*)a.y)[o]), scale, acc));
    }
}

// blockIdx.x: (row group, 16 rows of it); blockIdx.y: (segment, 512 columns of it)
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void bank_tile_kernel(const BankArgs a, int tiles_per_group) {
    __shared__ float part[4 * 16 * 64];
    const int grp = blockIdx.x / tiles_per_group;
    const int m0 = grp * a.rows_per_id + (blockIdx.x % tiles_per_group) * 16;
    const int mend = min(a.M, (grp + 1) * a.rows_per_id);
    if (m0 >= mend) return;
    const int seg = blockIdx.y / a.chunks_per_seg, c0 = (blockIdx.y % a.chunks_per_seg) * COLS;
    const int id = a.A[seg] ? id_of(a, grp) : -1;
    if (id < 0 && a.act == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int JT = (a.r + 15) >> 4;
    const int row = m0 + lr;
    const bool rok = row < mend;
    f32x4 uf[4];  // uf[t][e] = u[row][16t + 4g + e]
#pragma unroll
    for (int t = 0; t < 4; ++t) uf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (id >= 0) {
        const TX* xp = (const TX*)a.x + (int64_t)(rok ? row : m0) * a.ldx;
        const float* Ap = a.A[seg] + (int64_t)id * a.r * a.K;
        for (int k0 = wave * 16; k0 < a.K; k0 += 64) {
            const int k = k0 + 4 * g;
            const bool kok = k < a.K;
            const f32x4 xf = load4<TX>(xp + k, rok && kok);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < JT) {
                    const int j = 16 * t + lr;
                    const f32x4 wf = ld4(Ap + (int64_t)j * a.K + k, j < a.r && kok);
#pragma unroll
                    for (int e = 0; e < 4; ++e) uf[t] = mma(wf[e], xf[e], uf[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) part[(wave * 16 + t * 4 + e) * 64 + lane] = uf[t][e];
        __syncthreads();
        // every wave adds the four partial tiles in wave order: the same u in all of them
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = part[(t * 4 + e) * 64 + lane];
                for (int w = 1; w < 4; ++w) s += part[(w * 16 + t * 4 + e) * 64 + lane];
                uf[t][e] = s;
            }
    }
    const float scale = id >= 0 ? a.c[seg] * a.gain[id] : 0.f;
    const float* Bp = id >= 0 ? a.B[seg] + (int64_t)id * a.seg_n * a.r : nullptr;
    const int64_t base = a.c_offset + (a.c_offset_dev ? *a.c_offset_dev : 0);
    const int cend = min(c0 + COLS, a.seg_n);
    for (int c = c0 + 64 * wave; c < cend; c += 256) {
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (id >= 0) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                if (kt < JT) {
                    const int k = 16 * kt + 4 * g;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int n = c + 16 * t + lr;
                        const f32x4 wf = ld4(Bp + (int64_t)n * a.r + k, n < a.seg_n && k < a.r);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[t] = mma(wf[e], uf[kt][e], acc[t]);  // acc[t][e] = (u B^T)[row][c + 16t + 4g + e]
                    }
                }
            }
        }
        if (rok)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int n = c + 16 * t + 4 * g;
                if (n < a.seg_n) {  // seg_n and cg_in are multiples of 4: the four columns share a column group
                    const int64_t o = out_offset(a, base, row, seg * a.seg_n + n);
                    const f32x4 y4 = load4<TY>((const TY*)a.y + o, true);
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = finish(a, y4[e], scale, acc[t][e]);
                    store4<TY>((TY*)a.out + o, v);
                }
            }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

template <typename TX, typename TY>
void launch(const BankArgs& a, int n_seg, hipStream_t s) {
    const unsigned gy = (unsigned)(n_seg * a.chunks_per_seg);
    if (a.rows_per_id < 16 && a.M <= ROW_KERNEL_MAX_ROWS) {
        hipLaunchKernelGGL((bank_rows_kernel<TX, TY>), dim3(a.M, gy), dim3(256), 0, s, a);
    } else {
        const int groups = (a.M + a.rows_per_id - 1) / a.rows_per_id, tiles = (a.rows_per_id + 15) / 16;
        hipLaunchKernelGGL((bank_tile_kernel<TX, TY>), dim3(groups * tiles, gy), dim3(256), 0, s, a, tiles);
    }
}

}  // namespace

extern "C" int wipa_lora_bank_apply(const wipa_lora_bank_desc* d, wipa_stream_t stream) {
    const char* who = "wipa_lora_bank_apply";
    WIPA_REQUIRE(d, "%s: d is NULL", who);
    WIPA_REQUIRE(d->r >= 4 && d->r <= 64 && d->r % 4 == 0, "%s: r = %d: the rank is a multiple of 4 in 4..64", who, d->r);
    WIPA_REQUIRE(d->n >= 1 && d->n <= WIPA_LORA_BANK_MAX_ADAPTERS, "%s: n = %d: a bank holds 1..%d adapters", who, d->n, WIPA_LORA_BANK_MAX_ADAPTERS);
    WIPA_REQUIRE(d->M > 0, "%s: M = %d: at least one row", who, d->M);
    WIPA_REQUIRE(d->K > 0 && d->K % 4 == 0, "%s: K = %d: a positive multiple of 4", who, d->K);
    WIPA_REQUIRE(d->n_seg >= 1 && d->n_seg <= MAX_SEG, "%s: n_seg = %d: 1..%d column segments", who, d->n_seg, MAX_SEG);
    WIPA_REQUIRE(d->N > 0 && d->N % (4 * d->n_seg) == 0, "%s: N = %d: n_seg = %d segments of a positive multiple of 4 columns each", who, d->N,
                 d->n_seg);
    WIPA_REQUIRE(d->rows_per_id >= 1, "%s: rows_per_id = %d: at least one row per id", who, d->rows_per_id);
    WIPA_REQUIRE(d->ids_stride >= 0, "%s: ids_stride = %d: 0 (1) or a positive stride", who, d->ids_stride);
    WIPA_REQUIRE(d->x_dtype == WIPA_F32 || d->x_dtype == WIPA_BF16, "%s: x_dtype = %d: WIPA_F32 or WIPA_BF16", who, d->x_dtype);
    WIPA_REQUIRE(d->y_dtype == WIPA_F32 || d->y_dtype == d->x_dtype, "%s: y_dtype = %d: WIPA_F32 or x_dtype", who, d->y_dtype);
    WIPA_REQUIRE(d->act == 0 || d->act == 1, "%s: act = %d: 0 none, 1 gelu(erf)", who, d->act);
    WIPA_REQUIRE(d->x && aligned16(d->x), "%s: x: a 16-byte aligned device pointer", who);
    WIPA_REQUIRE(d->y && aligned16(d->y), "%s: y: a 16-byte aligned device pointer", who);
    WIPA_REQUIRE(d->out && aligned16(d->out), "%s: out: a 16-byte aligned device pointer", who);
    WIPA_REQUIRE(d->gain && d->ids, "%s: gain and ids: device pointers", who);
    WIPA_REQUIRE(d->ldx >= d->K && d->ldx % 4 == 0, "%s: ldx = %lld: a multiple of 4, at least K = %d", who, (long long)d->ldx, d->K);
    const int rg_in = d->rg_in > 0 ? d->rg_in : d->M, cg_in = d->cg_in > 0 ? d->cg_in : d->N;
    const int seg_n = d->N / d->n_seg;
    WIPA_REQUIRE(cg_in % 4 == 0, "%s: cg_in = %d: a multiple of 4", who, cg_in);
    WIPA_REQUIRE(d->ld >= std::min(cg_in, d->N) && d->ld % 4 == 0, "%s: ld = %lld: a multiple of 4, at least min(cg_in, N) = %d", who,
                 (long long)d->ld, std::min(cg_in, d->N));
    WIPA_REQUIRE(d->rg_stride % 4 == 0 && d->cg_stride % 4 == 0 && d->c_offset % 4 == 0,
                 "%s: rg_stride = %lld, cg_stride = %lld, c_offset = %lld: multiples of 4", who, (long long)d->rg_stride, (long long)d->cg_stride,
                 (long long)d->c_offset);
    bool any = false;
    for (int s = 0; s < d->n_seg; ++s) {
        WIPA_REQUIRE((d->A[s] == nullptr) == (d->B[s] == nullptr), "%s: A[%d] and B[%d]: both or neither", who, s, s);
        WIPA_REQUIRE(aligned16(d->A[s]) && aligned16(d->B[s]), "%s: A[%d] and B[%d]: 16-byte aligned device pointers", who, s, s);
        any = any || d->A[s];
    }
    WIPA_REQUIRE(any || d->act == 1, "%s: A: no segment carries an adapter and act is none: nothing to do", who);
    if (d->ids_host) {
        const int groups = (d->M + d->rows_per_id - 1) / d->rows_per_id, stride = d->ids_stride > 0 ? d->ids_stride : 1;
        for (int i = 0; i < groups; ++i)
            WIPA_REQUIRE(d->ids_host[(size_t)i * stride] >= -1 && d->ids_host[(size_t)i * stride] < d->n,
                         "%s: ids_host[%d] = %d: -1 or an adapter of the bank (n = %d)", who, i * stride, d->ids_host[(size_t)i * stride], d->n);
    }
    BankArgs a;
    memset(&a, 0, sizeof(a));
    a.x = d->x; a.y = d->y; a.out = d->out;
    for (int s = 0; s < d->n_seg; ++s) {
        a.A[s] = d->A[s]; a.B[s] = d->B[s]; a.c[s] = d->col_scale[s];
    }
    a.gain = d->gain; a.ids = d->ids; a.c_offset_dev = d->c_offset_dev;
    a.ldx = d->ldx; a.ld = d->ld; a.rg_stride = d->rg_stride; a.cg_stride = d->cg_stride; a.c_offset = d->c_offset;
    a.M = d->M; a.K = d->K; a.seg_n = seg_n; a.r = d->r; a.n = d->n; a.rows_per_id = d->rows_per_id;
    a.ids_stride = d->ids_stride > 0 ? d->ids_stride : 1;
    a.rg_in = rg_in; a.cg_in = cg_in; a.act = d->act; a.chunks_per_seg = (seg_n + COLS - 1) / COLS;
    hipStream_t s = (hipStream_t)stream;
    if (d->x_dtype == WIPA_F32) launch<float, float>(a, d->n_seg, s);
    else if (d->y_dtype == WIPA_F32) launch<__bf16, float>(a, d->n_seg, s);
    else launch<__bf16, __bf16>(a, d->n_seg, s);
    WIPA_LAUNCH_CHECK();
    return WIPA_OK;
}

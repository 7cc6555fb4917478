// Does a default-policy slice of a large LDS-DMA stream stay in the Infinity Cache while the rest of the stream goes by with nt?
//
// The decode step's streaming launch (csrc/cross_absorbed.hip, cross_absorbed_v2_kernel) reads the encoder output xa of a pass
// (64 clips x 1500 frames x 768 channels bf16 = 147.5 MB) once per decoder layer, twelve times a step, and four passes are in
// flight: four 147.5 MB sets cycle through a 256 MiB cache.  This probe reproduces the byte stream alone, no arithmetic:
//
//   W workgroups (128 and 256) of three waves; a wave owns two private 24 KiB LDS slots and fills them by LDS-DMA in 24 KiB groups
//   (24 transfers of 1 KiB, the younger group in flight behind a counted vmcnt wait: stage() of the kernel); a workgroup streams a
//   contiguous range of the buffer, its waves taking groups wave, wave + 3, ...; the FIRST f of the range's groups load with the
//   default policy (aux = 0), the rest with nt (aux = 2).
//   Four such buffers are swept round-robin: 8 "steps" x 12 "layers" x 4 buffers, every sweep timed by events; optionally every
//   sweep is followed by a default-policy sweep of one layer's slice (1/12) of a 306 MB "weights" buffer shared by the four
//   buffers' sweeps (306 MB per pass-step: the decoder weights the four passes share).
//
// Printed per (W, weights, f): median / mean us per xa sweep over steps 2..8 and the rate on the bytes swept, and the same for the
// weights slices.  f = 1 is the kernel's policy before this probe; f = 0 is pure nt.
//
//   hipcc --offload-arch=gfx950 -O3 -o xa_residency_probe tools/micro/xa_residency_probe.hip && ./xa_residency_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

typedef __attribute__((address_space(3))) void* lds_ptr;
constexpr int NWV = 3, GROUP = 24 * 1024, NDMA = GROUP / 1024;
constexpr int SMEM = NWV * 2 * GROUP;  // 144 KiB: one workgroup per CU, as the kernel

template <int AUX>
__device__ __forceinline__ void dma_group(__amdgpu_buffer_rsrc_t r, char* dst, int lane, unsigned byte0) {
#pragma unroll
    for (int i = 0; i < NDMA; ++i)  // lane's 16 bytes of transfer i; the resource's size bounds every read (out of range reads 0)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr)(dst + 1024 * i), 16, 16 * lane, byte0 + 1024 * i, 0, AUX);
}

// groups [wg * gpw, (wg + 1) * gpw) of buf; the first `resident` of them default policy
__global__ __launch_bounds__(64 * NWV, 1) void sweep_kernel(const char* buf, unsigned bytes, int gpw, int resident) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* my = smem + wave * (2 * GROUP);
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)buf, 0, (int)bytes, 0x00020000);
    const int my_n = gpw > wave ? (gpw - wave + NWV - 1) / NWV : 0;
    auto stage = [&](int i, int slot) {
        const int gl = wave + NWV * i;  // wave-uniform
        const unsigned byte0 = (unsigned)(blockIdx.x * gpw + gl) * (unsigned)GROUP;
        if (gl < resident) dma_group<0>(r, my + slot * GROUP, lane, byte0);
        else dma_group<2>(r, my + slot * GROUP, lane, byte0);
    };
    if (my_n > 0) stage(0, 0);
    if (my_n > 1) stage(1, 1);
    for (int i = 0; i < my_n; ++i) {
        if (i + 1 < my_n) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (i + 2 < my_n) stage(i + 2, i & 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

static double median(std::vector<float> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}
static double mean(const std::vector<float>& v) {
    double s = 0;
    for (float x : v) s += x;
    return v.empty() ? 0.0 : s / v.size();
}

int main() {
    constexpr int NBUF = 4, LAYERS = 12, STEPS = 8;
    const size_t xa_groups = 64ull * 1500 * 768 * 2 / GROUP;  // 6000 groups = 147.456 MB
    const size_t xa_bytes = xa_groups * GROUP;
    const size_t w_slice_groups = 306000000ull / LAYERS / GROUP;  // one layer's share of the decoder weights
    const size_t w_bytes = w_slice_groups * GROUP * LAYERS;
    char* xa[NBUF];
    char* wts;
    for (int b = 0; b < NBUF; ++b) {
        CK(hipMalloc(&xa[b], xa_bytes));
        CK(hipMemset(xa[b], b + 1, xa_bytes));
    }
    CK(hipMalloc(&wts, w_bytes));
    CK(hipMemset(wts, 7, w_bytes));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    const int n_ev = STEPS * LAYERS * NBUF * 2 + 1;
    std::vector<hipEvent_t> ev(n_ev);
    for (auto& e : ev) CK(hipEventCreate(&e));
    printf("xa: %d buffers x %.1f MB; weights: %.1f MB in %d slices; %d steps x %d layers; times in us per sweep, steps 2..%d\n", NBUF,
           xa_bytes / 1e6, w_bytes / 1e6, LAYERS, STEPS, LAYERS, STEPS);
    printf("%4s %7s %6s %9s | %9s %9s %7s | %9s %9s %7s\n", "W", "weights", "f", "res MB/buf", "xa med", "xa mean", "TB/s", "w med", "w mean",
           "TB/s");
    const double fs[] = {1.0, 0.0, 0.125, 0.25, 0.375, 0.5};
    for (int W : {128, 256}) {
        const int gpw = (int)(xa_groups / W);     // 46 / 23: the last 112 groups of a buffer are left out
        const int wgpw = (int)(w_slice_groups / W);
        for (int with_w = 0; with_w < 2; ++with_w) {
            for (double f : fs) {
                const int resident = (int)(f * gpw + 0.5);
                int k = 0;
                CK(hipEventRecord(ev[k++], s));
                for (int st = 0; st < STEPS; ++st)
                    for (int l = 0; l < LAYERS; ++l)
                        for (int b = 0; b < NBUF; ++b) {
                            sweep_kernel<<<W, 64 * NWV, SMEM, s>>>(xa[b], (unsigned)xa_bytes, gpw, resident);
                            CK(hipEventRecord(ev[k++], s));
                            if (with_w) {
                                sweep_kernel<<<W, 64 * NWV, SMEM, s>>>(wts + (size_t)l * w_slice_groups * GROUP,
                                                                        (unsigned)(w_slice_groups * GROUP), wgpw, wgpw);
                                CK(hipEventRecord(ev[k++], s));
                            }
                        }
                CK(hipStreamSynchronize(s));
                CK(hipGetLastError());
                std::vector<float> tx, tw;
                const int per = with_w ? 2 : 1;
                for (int i = 0; i + 1 < k; ++i) {
                    const int sweep = i / per;
                    if (sweep < LAYERS * NBUF) continue;  // step 1 fills the cache
                    float ms;
                    CK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
                    ((with_w && (i % 2)) ? tw : tx).push_back(ms * 1e3f);
                }
                const double bx = (double)W * gpw * GROUP, bw = (double)W * wgpw * GROUP;
                printf("%4d %7s %6.3f %9.1f | %9.1f %9.1f %7.2f |", W, with_w ? "yes" : "no", f, (double)W * resident * GROUP / 1e6, median(tx),
                       mean(tx), bx / (median(tx) * 1e-6) / 1e12);
                if (with_w) printf(" %9.1f %9.1f %7.2f\n", median(tw), mean(tw), bw / (median(tw) * 1e-6) / 1e12);
                else printf(" %9s %9s %7s\n", "-", "-", "-");
                fflush(stdout);
            }
        }
    }
    return 0;
}

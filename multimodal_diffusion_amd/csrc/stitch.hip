// Sliding-window stitching for long-form generation:
//   avdiff/models/infer/stream_infer.py:85-116 (crossfade_audio), :119-143 (crossfade_video).
// Weighted overlap-add of N windows of length L placed every `hop` positions, divided by the summed weights
// (clamped at 1e-6).  Gather form, windows accumulated in increasing order with separately rounded multiply and add
// (no FMA contraction), so fp32 results are bit-identical to the reference's numpy loop.  HBM-bound, one pass.
#include "avd_common.h"

namespace avd {

__device__ __forceinline__ void window_range(int64_t p, int L, int hop, int N, int& lo, int& hi) {
    hi = (int)(p / hop);
    if (hi > N - 1) hi = N - 1;
    const int64_t q = p - L + 1;
    lo = q <= 0 ? 0 : (int)((q + hop - 1) / hop);
}

// chunks [N, L, inner] fp32, w [L], out [(N-1)*hop + L, inner]
__global__ __launch_bounds__(256) void crossfade_f32_kernel(const float* __restrict__ chunks, const float* __restrict__ w,
                                                            float* __restrict__ out, int N, int L, int hop, int64_t inner,
                                                            int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t p = i / inner, j = i % inner;
    int lo, hi;
    window_range(p, L, hop, N, lo, hi);
    float acc = 0.f, nrm = 0.f;
    for (int k = lo; k <= hi; ++k) {
        const int q = (int)(p - (int64_t)k * hop);
        const float wq = w[q];
        acc = __fadd_rn(acc, __fmul_rn(chunks[((int64_t)k * L + q) * inner + j], wq));
        nrm = __fadd_rn(nrm, wq);
    }
    out[i] = __fdiv_rn(acc, fmaxf(nrm, 1e-6f));
}

// chunks [N, L, inner] uint8 (inner = H*W*3), w [L], out uint8: (clip(sum(c/255 * w) / sum(w), 0, 1) * 255) truncated
__global__ __launch_bounds__(256) void crossfade_u8_kernel(const uint8_t* __restrict__ chunks, const float* __restrict__ w,
                                                           uint8_t* __restrict__ out, int N, int L, int hop, int64_t inner,
                                                           int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t p = i / inner, j = i % inner;
    int lo, hi;
    window_range(p, L, hop, N, lo, hi);
    float acc = 0.f, nrm = 0.f;
    for (int k = lo; k <= hi; ++k) {
        const int q = (int)(p - (int64_t)k * hop);
        const float wq = w[q];
        const float c = __fdiv_rn((float)chunks[((int64_t)k * L + q) * inner + j], 255.0f);
        acc = __fadd_rn(acc, __fmul_rn(c, wq));
        nrm = __fadd_rn(nrm, wq);
    }
    float v = __fdiv_rn(acc, fmaxf(nrm, 1e-6f));
    v = fminf(fmaxf(v, 0.f), 1.f);
    out[i] = (uint8_t)__fmul_rn(v, 255.0f);
}

// Latent window consensus (MultiDiffusion-style co-denoising of the windows of one canvas; contract in include/avdiff_hip.h).
// z [N, outer, L, inner] in place.  One thread owns VEC consecutive `inner` values of one canvas element (o, p): it alone reads and
// writes every z element of that canvas position, so in place needs no atomics.  Threads run along inner, and along p when
// inner == 1; blockIdx.y strides over `outer`.  A position under one window is left alone.
template <int VEC>
__global__ __launch_bounds__(256) void window_consensus_kernel(float* __restrict__ z, const float* __restrict__ w, int N,
                                                               int64_t outer, int L, int hop, int64_t inner_v, int64_t plane) {
    // Plain operators under the pragma, not __fmul_rn / __fadd_rn: those are inline `x * y` / `x + y` of the HIP headers, compiled under
    // hipcc's default -ffp-contract=fast wherever they are inlined, and here they came out fused (v_pk_fma_f32), one rounding short of
    // the contract.  With contraction off every *, + and / below is rounded on its own.
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    // plane = P * inner_v; below 2^32 (every latent in use) the split is a 32-bit division
    const int64_t p = plane <= 0xffffffffll ? (int64_t)((uint32_t)i / (uint32_t)inner_v) : i / inner_v;
    const int64_t j = i - p * inner_v;
    int lo, hi;
    window_range(p, L, hop, N, lo, hi);
    if (lo >= hi) return;
    float nrm = 0.f;
    for (int k = lo; k <= hi; ++k) nrm = nrm + w[(int)(p - (int64_t)k * hop)];
    for (int64_t o = blockIdx.y; o < outer; o += gridDim.y) {
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int k = lo; k <= hi; ++k) {
            const int q = (int)(p - (int64_t)k * hop);
            const float wq = w[q];
            const float* src = z + ((((int64_t)k * outer + o) * L + q) * inner_v + j) * VEC;
            if constexpr (VEC == 4) {
                const float4 x = *reinterpret_cast<const float4*>(src);
                acc[0] = acc[0] + wq * x.x;
                acc[1] = acc[1] + wq * x.y;
                acc[2] = acc[2] + wq * x.z;
                acc[3] = acc[3] + wq * x.w;
            } else {
                acc[0] = acc[0] + wq * *src;
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / nrm;
        for (int k = lo; k <= hi; ++k) {
            const int q = (int)(p - (int64_t)k * hop);
            float* dst = z + ((((int64_t)k * outer + o) * L + q) * inner_v + j) * VEC;
            if constexpr (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else *dst = acc[0];
        }
    }
}

}  // namespace avd

using namespace avd;

extern "C" int avd_crossfade_f32(const float* chunks, const float* w, float* out, int N, int L, int hop, int64_t inner,
                                 avd_stream_t stream) {
    AVD_REQUIRE(chunks && w && out && N > 0 && L > 0 && hop > 0 && inner > 0, AVD_EINVAL, "crossfade: bad arguments");
    const int64_t total = ((int64_t)(N - 1) * hop + L) * inner;
    static const int tag = prof_tag_id("crossfade_f32_kernel");
    ProfScope prof(tag, 4.0 * ((double)N * L * inner + (double)total), static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(crossfade_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), chunks, w, out, N, L, hop, inner, total);
    AVD_CHECK_LAUNCH("crossfade_f32");
    return AVD_OK;
}

extern "C" int avd_crossfade_u8(const uint8_t* chunks, const float* w, uint8_t* out, int N, int L, int hop, int64_t inner,
                                avd_stream_t stream) {
    AVD_REQUIRE(chunks && w && out && N > 0 && L > 0 && hop > 0 && inner > 0, AVD_EINVAL, "crossfade: bad arguments");
    const int64_t total = ((int64_t)(N - 1) * hop + L) * inner;
    static const int tag = prof_tag_id("crossfade_u8_kernel");
    ProfScope prof(tag, (double)N * L * inner + (double)total, static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(crossfade_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), chunks, w, out, N, L, hop, inner, total);
    AVD_CHECK_LAUNCH("crossfade_u8");
    return AVD_OK;
}

extern "C" int avd_window_consensus_f32(float* z, const float* w, int N, int64_t outer, int L, int hop, int64_t inner,
                                        avd_stream_t stream) {
    AVD_REQUIRE(z && w && N > 0 && outer > 0 && L > 0 && hop > 0 && inner > 0, AVD_EINVAL, "window_consensus: bad arguments");
    if (N == 1 || hop >= L) return AVD_OK;       // no canvas position lies under two windows
    const int64_t P = (int64_t)(N - 1) * hop + L;
    const bool vec4 = inner % 4 == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0;
    const int64_t inner_v = vec4 ? inner / 4 : inner;
    const int64_t plane = P * inner_v, blocks = (plane + 255) / 256;
    AVD_REQUIRE(blocks <= 0x7fffffffll, AVD_EUNSUPPORTED, "window_consensus: %lld canvas elements per outer index exceed one grid",
                (long long)(P * inner));
    // every position of a window lies under a neighbour too, except hop positions at each end of the canvas and, where L < 2 hop,
    // the 2 hop - L middle positions of every inner window
    const int64_t single = 2ll * hop + (int64_t)(N - 2) * (2 * hop > L ? 2 * hop - L : 0);
    static const int tag = prof_tag_id("window_consensus_kernel");
    ProfScope prof(tag, 2.0 * 4.0 * (double)((int64_t)N * L - single) * (double)outer * (double)inner, static_cast<hipStream_t>(stream));
    const dim3 grid((unsigned)blocks, (unsigned)(outer < 65535 ? outer : 65535));
    if (vec4)
        hipLaunchKernelGGL(window_consensus_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), z, w, N, outer, L, hop,
                           inner_v, plane);
    else
        hipLaunchKernelGGL(window_consensus_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), z, w, N, outer, L, hop,
                           inner_v, plane);
    AVD_CHECK_LAUNCH("window_consensus");
    return AVD_OK;
}

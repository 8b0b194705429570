// Token plumbing and the DDIM update — the HBM-bound ends of a denoising step.
//   timestep embedding ........ avdiff/utils/schedule_utils.py:64-86
//   tube patch / unpatch ...... avdiff/utils/ops.py:100-119, 122-144
//   audio chunk / overlap-add . avdiff/models/infer/sample_clip.py:184-188, 191-215 (ops.py:17-45, 48-93)
//   ddim_step ................. avdiff/utils/schedule_utils.py:146-200
//   CFG + unpatch + DDIM ...... avdiff/models/infer/sample_clip.py:381-389 (video), :342-348 (audio)
//   sequence assembly ......... avdiff/models/infer/sample_clip.py:367-371,377 / 328-333,338
// All kernels move 16 bytes per lane, coalesced along the innermost latent axis (W or the feature axis),
// and touch every byte exactly once: fused CFG+unpatch+DDIM reads 2 eps + z and writes z' = 16 B per latent
// element, which is its HBM roofline.
#include "avd_common.h"

#include <stdlib.h>
#include <type_traits>
#include <cmath>
#include <initializer_list>
#include <string>

namespace avd {

// ------------------------------------------------------------------ timestep embedding
__global__ void temb_kernel(const int64_t* __restrict__ t, const float* __restrict__ freqs, float* __restrict__ out,
                            int B, int dim, float neg_log_mp) {
    const int half = dim >> 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int b = i / dim, c = i % dim;
    float v = 0.f;
    if (c < 2 * half) {
        const int k = c < half ? c : c - half;
        // freqs = exp(-ln(max_period) * k / half), all in fp32 like the reference
        // (the caller may pass the host-built table: cos/sin at t ~ 1000 amplify a 1-ulp difference in exp 1000x)
        const float f = freqs ? freqs[k] : expf(neg_log_mp * (float)k / (float)half);
        const float a = (float)t[b] * f;
        v = c < half ? cosf(a) : sinf(a);
    }
    out[i] = v;
}

int temb_f32(const int64_t* t, const float* freqs, float* out, int B, int dim, float max_period, hipStream_t st) {
    AVD_REQUIRE(t && out, AVD_EINVAL, "timestep_embedding: null pointer");
    AVD_REQUIRE(B > 0 && dim > 0 && max_period > 0.f, AVD_EINVAL, "timestep_embedding: bad dims");
    const int n = B * dim;
    hipLaunchKernelGGL(temb_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t, freqs, out, B, dim,
                       -(float)log((double)max_period));
    AVD_CHECK_LAUNCH("timestep_embedding");
    return AVD_OK;
}

// ------------------------------------------------------------------ tube geometry
struct Tube {
    int C, T, H, W, t, h, w;
    int Ht, Wt;        // H/h, W/w
    int D;             // C*t*h*w
    int64_t per;       // C*T*H*W
};

static int make_tube(Tube& g, int C, int T, int H, int W, int t, int h, int w) {
    AVD_REQUIRE(C > 0 && T > 0 && H > 0 && W > 0 && t > 0 && h > 0 && w > 0, AVD_EINVAL, "tube: bad dims");
    AVD_REQUIRE(T % t == 0 && H % h == 0 && W % w == 0, AVD_EINVAL, "tube sizes must divide latent dims");
    AVD_REQUIRE(w % 4 == 0, AVD_EUNSUPPORTED, "tube: w=%d must be a multiple of 4 (16-byte runs)", w);
    g = Tube{C, T, H, W, t, h, w, H / h, W / w, C * t * h * w, (int64_t)C * T * H * W};
    return AVD_OK;
}

// latent float4 index e4 (within one sample, NCDHW order) -> offset of the same 4 floats inside the
// sample's token matrix [Nv, D]
__device__ __forceinline__ int64_t tube_tok_off(const Tube& g, int64_t e4) {
    const int W4 = g.W >> 2;
    const int w0 = (int)(e4 % W4) * 4;
    int64_t r = e4 / W4;
    const int y = (int)(r % g.H);
    r /= g.H;
    const int tt = (int)(r % g.T);
    const int c = (int)(r / g.T);
    const int n = ((tt / g.t) * g.Ht + y / g.h) * g.Wt + w0 / g.w;
    const int k = ((c * g.t + tt % g.t) * g.h + y % g.h) * g.w + w0 % g.w;
    return (int64_t)n * g.D + k;
}

template <bool TO_TOKENS>
__global__ __launch_bounds__(256) void tube_kernel(const float* __restrict__ src, float* __restrict__ dst, Tube g,
                                                   int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t per4 = g.per >> 2;
    const int64_t b = i / per4, e4 = i % per4;
    const int64_t lat = b * g.per + e4 * 4;
    const int64_t tok = b * g.per + tube_tok_off(g, e4);
    if (TO_TOKENS) *reinterpret_cast<f32x4*>(dst + tok) = *reinterpret_cast<const f32x4*>(src + lat);
    else *reinterpret_cast<f32x4*>(dst + lat) = *reinterpret_cast<const f32x4*>(src + tok);
}

int tube_patch_f32(const float* z, float* tok, int B, int C, int T, int H, int W, int t, int h, int w, hipStream_t st) {
    AVD_REQUIRE(z && tok && B > 0, AVD_EINVAL, "tube_patch: bad arguments");
    Tube g;
    if (int rc = make_tube(g, C, T, H, W, t, h, w)) return rc;
    const int64_t total4 = (int64_t)B * (g.per >> 2);
    static const int tag = prof_tag_id("tube_kernel<true>");
    ProfScope prof(tag, 8.0 * (double)B * g.per, st);
    hipLaunchKernelGGL(tube_kernel<true>, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, z, tok, g, total4);
    AVD_CHECK_LAUNCH("tube_patch");
    return AVD_OK;
}

int tube_unpatch_f32(const float* tok, float* z, int B, int C, int T, int H, int W, int t, int h, int w,
                     hipStream_t st) {
    AVD_REQUIRE(z && tok && B > 0, AVD_EINVAL, "tube_unpatch: bad arguments");
    Tube g;
    if (int rc = make_tube(g, C, T, H, W, t, h, w)) return rc;
    const int64_t total4 = (int64_t)B * (g.per >> 2);
    hipLaunchKernelGGL(tube_kernel<false>, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, tok, z, g, total4);
    AVD_CHECK_LAUNCH("tube_unpatch");
    return AVD_OK;
}

// ------------------------------------------------------------------ audio chunk tokens
__global__ void audio_tok_kernel(const float* __restrict__ z, float* __restrict__ tok, int B, int Ca, int F, int len,
                                 int stride, int Na) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int D = Ca * len;
    if (i >= (int64_t)B * Na * D) return;
    const int k = (int)(i % D);
    const int n = (int)((i / D) % Na);
    const int b = (int)(i / ((int64_t)D * Na));
    const int c = k / len, j = k % len;
    tok[i] = z[((int64_t)b * Ca + c) * F + n * stride + j];
}

// overlap-add value for frame f (f < L): windows summed in increasing window order, divided by the summed window weights
// (win == nullptr: rectangular window, i.e. the overlap count; otherwise ops.py:76-93 with apply_hann — multiply and add are
// rounded separately like the reference's `y += windows * win`)
__device__ __forceinline__ float ola_gather(const float* __restrict__ tokb, int D, int c, int len, int stride, int Na,
                                            int f, const float* __restrict__ win = nullptr) {
    int n_hi = f / stride;
    if (n_hi > Na - 1) n_hi = Na - 1;
    int n_lo = (f - len + stride) / stride;   // ceil((f-len+1)/stride)
    if (f - len + 1 <= 0) n_lo = 0;
    float acc = 0.f, cnt = 0.f;
    for (int n = n_lo; n <= n_hi; ++n) {
        const int j = f - n * stride;
        const float v = tokb[(int64_t)n * D + c * len + j];
        if (win) {
            acc = __fadd_rn(acc, __fmul_rn(v, win[j]));
            cnt += win[j];
        } else {
            acc += v;
            cnt += 1.f;
        }
    }
    return acc / fmaxf(cnt, 1e-8f);
}

__global__ void audio_untok_kernel(const float* __restrict__ tok, float* __restrict__ z, int B, int Ca, int F, int len,
                                   int stride, int Na, const float* __restrict__ win) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * Ca * F) return;
    const int f = (int)(i % F);
    const int c = (int)((i / F) % Ca);
    const int b = (int)(i / ((int64_t)F * Ca));
    const int L = (Na - 1) * stride + len;
    const int D = Ca * len;
    z[i] = f < L ? ola_gather(tok + (int64_t)b * Na * D, D, c, len, stride, Na, f, win) : 0.f;
}

static int audio_na(int F, int len, int stride) { return (F - len) / stride + 1; }

int audio_tokens_f32(const float* z, float* tok, int B, int Ca, int F, int len, int stride, hipStream_t st) {
    AVD_REQUIRE(z && tok && B > 0 && Ca > 0, AVD_EINVAL, "audio_tokens: bad arguments");
    AVD_REQUIRE(len > 0 && stride > 0 && F >= len, AVD_EUNSUPPORTED,
                "audio_tokens: need 0 < len <= F and stride > 0 (got F=%d len=%d stride=%d)", F, len, stride);
    const int Na = audio_na(F, len, stride);
    const int64_t n = (int64_t)B * Na * Ca * len;
    hipLaunchKernelGGL(audio_tok_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, z, tok, B, Ca, F, len,
                       stride, Na);
    AVD_CHECK_LAUNCH("audio_tokens");
    return AVD_OK;
}

int audio_untokens_f32(const float* tok, const float* win, float* z, int B, int Ca, int F, int len, int stride, hipStream_t st) {
    AVD_REQUIRE(z && tok && B > 0 && Ca > 0, AVD_EINVAL, "audio_untokens: bad arguments");
    AVD_REQUIRE(len > 0 && stride > 0 && F >= len, AVD_EUNSUPPORTED, "audio_untokens: bad chunking");
    const int Na = audio_na(F, len, stride);
    const int64_t n = (int64_t)B * Ca * F;
    hipLaunchKernelGGL(audio_untok_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tok, z, B, Ca, F, len,
                       stride, Na, win);
    AVD_CHECK_LAUNCH("audio_untokens");
    return AVD_OK;
}

// ------------------------------------------------------------------ DDIM coefficients (per sample)
struct Ddim {
    float sqrt_omb_t, den, sqrt_a_prev, coeff_eps, sigma;
};

__device__ __forceinline__ Ddim ddim_coef(const int64_t* t_now, const int64_t* t_prev, const float* abar, int T_train,
                                          float eta, int b) {
    long long tn = t_now[b], tp = t_prev[b];
    if (tn < 0) tn = 0;
    if (tn > T_train - 1) tn = T_train - 1;           // the reference would raise IndexError; stay in bounds
    const float a_t = abar[tn];
    float a_p = 1.0f;                                   // abar_{-1} := 1
    if (tp >= 0) a_p = abar[tp > T_train - 1 ? T_train - 1 : tp];
    Ddim c;
    c.sqrt_omb_t = sqrtf(fmaxf(1.0f - a_t, 0.f));
    c.den = fmaxf(sqrtf(a_t), 1e-8f);
    c.sqrt_a_prev = sqrtf(a_p);
    c.sigma = 0.f;
    if (eta > 0.f) {
        const float frac = fmaxf((1.0f - a_p) / fmaxf(1.0f - a_t, 1e-8f), 0.f);
        const float omr = fmaxf(1.0f - a_t / fmaxf(a_p, 1e-8f), 0.f);
        c.sigma = eta * sqrtf(frac * omr);
    }
    c.coeff_eps = sqrtf(fmaxf(1.0f - a_p - c.sigma * c.sigma, 0.f));
    return c;
}

// No fp contraction in these two: the reference evaluates them as separate torch ops, one rounding each (schedule_utils.py:186-199,
// sample_clip.py:381), and hipcc's default -ffp-contract=fast picks its fused multiply-adds per CALL SITE — the same expression came out one
// ulp apart in two kernels of this file (round 5: the whole-line CFG kernel against the gather form; round 4 met the same in split8).
// ddim_x0 is also the x0 of the DPM-Solver++(2M) update below: one expression, one rounding, the same bits in both solvers.
// It reads sqrt_omb_t and den alone, which do not depend on eta: the fused SDE kernels take them from ddim_coef(..., eta, b), the
// elementwise DPM kernels from ddim_coef(..., 0.f, b), and both get the same x0.  A Ddim member that ddim_x0 reads must stay free of eta.
__device__ __forceinline__ float ddim_x0(const Ddim& c, float x, float e) {
#pragma clang fp contract(off)
    return (x - c.sqrt_omb_t * e) / c.den;
}
__device__ __forceinline__ float ddim_apply(const Ddim& c, float x, float e, float zn) {
#pragma clang fp contract(off)
    const float x0 = ddim_x0(c, x, e);
    return c.sqrt_a_prev * x0 + c.coeff_eps * e + c.sigma * zn;
}
__device__ __forceinline__ float cfg_combine(float e_cond, float e_null, float guidance) {
#pragma clang fp contract(off)
    return e_null + guidance * (e_cond - e_null);
}

// ------------------------------------------------------------------ DPM-Solver++(2M) (data prediction, multistep; eta > 0: its SDE form)
// The contract is written out in include/avdiff_hip.h (avd_dpmpp_2m_step_f32, avd_dpmpp_2m_sde_step_f32).  One step s = t_now -> t =
// t_prev with the previous step's u = t_last (< 0: no history):  z_out = ((c_x x_s + c_0 x0_s) + c_1 x0_hist) + c_n n,  then
// x0_hist <- x0_s; the noise term exists at eta > 0 only.  The coefficients come from the fp32 table in fp64 and are rounded once to
// fp32, so every form of the update (the elementwise kernels, the three fused CFG kernels) and the numpy mirror of the tests agree
// on them bit for bit.
struct Dpm {
    float c_x, c_0, c_1;     // c_1 == 0: first order (x0_hist is not read)
    float c_n;               // the noise term's weight (eta > 0; 0 at eta == 0, on the final step and at equal lambdas)
};

// a(tau) of the contract: alpha_bar[clamp(tau, 0, T-1)] for tau >= 0, 1 for tau < 0
__device__ __forceinline__ float dpm_abar(const float* abar, int T_train, long long tau) {
    return tau < 0 ? 1.0f : abar[tau > T_train - 1 ? T_train - 1 : tau];
}

// eta == 0 keeps the ODE expressions (and their bits); eta > 0 takes the exponential forms of the SDE contract
__device__ __forceinline__ Dpm dpm_coef(const int64_t* t_last, const int64_t* t_now, const int64_t* t_prev, const float* abar,
                                        int T_train, float eta, int b) {
#pragma clang fp contract(off)
    const long long tu = t_last[b], tp = t_prev[b];
    long long ts = t_now[b];
    if (ts < 0) ts = 0;                                  // as ddim_coef: x0_s is DDIM's x0
    const double as = (double)dpm_abar(abar, T_train, ts), at = (double)dpm_abar(abar, T_train, tp);
    const double al_s = sqrt(as), sg_s = sqrt(fmax(1.0 - as, 0.0));
    const double al_t = sqrt(at), sg_t = sqrt(fmax(1.0 - at, 0.0));
    if (sg_s == 0.0) return Dpm{0.f, 1.f, 0.f, 0.f};    // a_s == 1: x_s is x0_s, return it
    if (eta > 0.f) {
        if (sg_t == 0.0) return Dpm{0.f, (float)al_t, 0.f, 0.f};      // h = +inf (the final step, or a_t == 1): x0_s, no noise
        const double et = (double)eta;
        const double ls = log(al_s) - log(sg_s), lt = log(al_t) - log(sg_t), h = lt - ls;
        const double cx = (sg_t / sg_s) * exp(-et * h);
        const double k = al_t * (-expm1(-(1.0 + et) * h));
        const double cn = sg_t * sqrt(fmax(-expm1(-2.0 * et * h), 0.0));
        double c0 = k, c1 = 0.0;
        if (tu >= 0 && tp >= 0) {                        // second order: the conditions of the ODE form below
            const double au = (double)dpm_abar(abar, T_train, tu);
            const double lu = log(sqrt(au)) - log(sqrt(fmax(1.0 - au, 0.0)));
            if (lu < ls && ls < lt) {
                const double r = (ls - lu) / h;
                c0 = k * (1.0 + 1.0 / (2.0 * r));
                c1 = -k / (2.0 * r);
            }
        }
        return Dpm{(float)cx, (float)c0, (float)c1, (float)cn};
    }
    const double cx = sg_t / sg_s;
    const double k = al_t - cx * al_s;
    double c0 = k, c1 = 0.0;
    // second order needs a history step, a finite target lambda (sigma_t > 0: not the final step) and lambda_u < lambda_s < lambda_t
    if (tu >= 0 && tp >= 0 && sg_t > 0.0) {
        const double au = (double)dpm_abar(abar, T_train, tu);
        const double al_u = sqrt(au), sg_u = sqrt(fmax(1.0 - au, 0.0));
        const double lu = log(al_u) - log(sg_u), ls = log(al_s) - log(sg_s), lt = log(al_t) - log(sg_t);
        if (lu < ls && ls < lt) {
            const double h = lt - ls, r = (ls - lu) / h;
            c0 = k * (1.0 + 1.0 / (2.0 * r));
            c1 = -k / (2.0 * r);
        }
    }
    return Dpm{(float)cx, (float)c0, (float)c1, 0.f};
}

// noisy: eta > 0, the noise term c_n zn ends the update (false: zn is not read, the ODE update as it was)
__device__ __forceinline__ float dpm_apply(const Dpm& c, float x, float x0, float hist, float zn, bool noisy) {
#pragma clang fp contract(off)
    const float y = c.c_x * x + c.c_0 * x0;
    const float y2 = c.c_1 != 0.f ? y + c.c_1 * hist : y;
    return noisy ? y2 + c.c_n * zn : y2;
}

// The fused CFG kernels below take the solver's state as their trailing parameter pack: empty (DDIM, the instantiations that
// existed before the solver, unchanged), NoiseKey (seeded DDIM noise), DpmState (this solver) or DpmState with a key (its SDE form).
struct DpmState {
    const int64_t* t_last;   // int64 [B]
    float* x0_hist;          // [B, per] in the latent's natural layout: read (second-order steps), then overwritten with x0_s
};
// the trailing pack holds the solver state (a DpmState, a key, or a DpmState then a key), then optionally a GuideState (the latent guide below)
// A CondOnly tag ending the pack selects the single-branch form of the fused kernels (a cond-only step of a guidance interval): eps2 is
// then eps1 = [B, Nt, D], the conditional prediction alone; the null rows are not loaded, nothing is combined, `guidance` and `B` are
// not read.  It excludes a CfgState (per-sample guidance and rescale act on the combine: with y = c the rescale is the identity).
struct CondOnly {};
// A SlotTimes item, alone in the pack, selects the slot form of the fused kernels (include/avdiff_hip.h, "slot timesteps"): t_now / t_prev
// are [B, S] tables, one pair per slot of the target's sliding axis (video: the S = T / t token frames; audio: the S = Na chunks, stride
// == len), every element takes ddim_coef of its slot's pair, and a slot whose pair is equal keeps z bit for bit (the hold).  It is the
// DDIM update at eta == 0 without a guide or a control: the pack holds nothing else.
// Behind a DpmState (the pack `DpmState, SlotTimes`, SEEDED false) it is the slot form of the DPM-Solver++(2M) ODE update: DpmState's
// t_last is a [B, S] table as well, every element takes ddim_coef / dpm_coef at its slot's entry, and a held slot keeps z and neither
// reads nor writes its x0_hist elements.
// A SlotKey behind the SlotTimes (SEEDED true: `SlotTimes, SlotKey` and `DpmState, SlotTimes, SlotKey`) is the slot form at eta > 0
// ("clip-keyed slot noise"): a stepping slot's noise term is drawn by the clip position the slot holds (slot_normal4), DDIM's sigma or
// the SDE form's c_n taken at the slot's entry.  A held slot draws nothing.
struct SlotTimes {
    int S;
};
template <class T, class... X> struct PackHas { static constexpr bool value = (std::is_same<T, X>::value || ...); };
struct GuideState;
struct CanvasGuideState;
struct CfgState;
// a well-formed pack: optionally one DpmState; one key exactly when SEEDED (a NoiseKey, or a CanvasKey for the canvas-keyed draw: seeded
// DDIM noise, or with the DpmState the SDE form's noise); then optionally one GuideState or CanvasGuideState (the guide's known noise
// keyed per sample or by canvas position; a canvas-keyed guide never rides with a NoiseKey), then optionally one CfgState or CondOnly.
// The slot form's packs are SlotTimes, behind the DpmState if there is one, and its key is a SlotKey, which rides nowhere else.
struct NoiseKey;
struct CanvasKey;
struct SlotKey;
// A ClipGuideState ends a slot pack ("clip-keyed latent guide"): behind the SlotTimes, and behind the SlotKey when there is one.
struct ClipGuideState;
// A SlotCfgState rides behind the SlotTimes alone ("slot CFG control"): after the SlotKey when there is one, before the ClipGuideState.
struct SlotCfgState;
// A SlotMomentum rides right behind a SlotCfgState in its APG mode ("slot APG momentum"): before the ClipGuideState.
struct SlotMomentum;
// A ClipQueues ends a slot pack that holds a SlotKey or a ClipGuideState ("clip batch keying"): the batch is K queues, each under its own
// seeds and canvases.  A pack without it carries none of its state: no divide, no seed load.
struct ClipQueues;
template <bool SEEDED, class... X> struct PackOk {
    template <class T> static constexpr int n = PackHas<T, X...>::value ? 1 : 0;
    static constexpr bool value = sizeof...(X) == (SEEDED ? 1 : 0) + n<DpmState> + n<GuideState> + n<CanvasGuideState> + n<CfgState> +
                                                      n<CondOnly> + n<SlotTimes> + n<ClipGuideState> + n<SlotCfgState> + n<SlotMomentum> +
                                                      n<ClipQueues> &&
                                  !(n<SlotTimes> && sizeof...(X) != 1 + n<DpmState> + n<SlotKey> + n<ClipGuideState> + n<SlotCfgState> +
                                                                        n<SlotMomentum> + n<ClipQueues>) &&
                                  n<SlotKey> <= n<SlotTimes> && n<ClipGuideState> <= n<SlotTimes> && n<SlotCfgState> <= n<SlotTimes> &&
                                  n<SlotMomentum> <= n<SlotCfgState> && n<ClipQueues> <= (n<SlotKey> || n<ClipGuideState> ? 1 : 0) &&
                                  !(n<CfgState> && n<CondOnly>) && !(n<GuideState> && n<CanvasGuideState>) &&
                                  !(n<CanvasGuideState> && n<NoiseKey>) &&
                                  n<NoiseKey> + n<CanvasKey> + n<SlotKey> == (SEEDED ? 1 : 0);
};
template <class T, class A, class... R> __host__ __device__ __forceinline__ T pack_get(const A& a, const R&... r) {
    if constexpr (std::is_same<T, A>::value) return a;
    else return pack_get<T>(r...);
}

// ------------------------------------------------------------------ seeded normal stream (DDIM eta > 0)
// The public contract is written out in include/avdiff_hip.h (avd_noise_key).  Element e of sample s at timestep t:
//   (x0, x1, x2, x3) = Philox4x32-10(counter (e >> 2, s, t, 0x44444D31), key (seed lo, seed hi))   (Random123 constants)
//   Box-Muller on (x0, x1) -> (n0, n1) and on (x2, x3) -> (n2, n3); e takes n[e & 3]
// The normals are a pure function of (seed, global sample index, t, element): every kernel that draws them must produce the same
// bits, so the Box-Muller arithmetic runs without fp contraction (see ddim_apply below) and on the accurate logf / sqrtf / sincospif.
struct NoiseKey {
    uint32_t k0, k1;   // seed & 0xffffffff, seed >> 32
    uint32_t s0;       // global index of sample 0 of the launch
};

// tag: the counter's domain word (0x44444D31 the DDIM noise, GUIDE_TAG the latent guide's known-region noise)
__device__ __forceinline__ f32x4 philox_normal4(const NoiseKey& nk, uint32_t e4, uint32_t s, uint32_t t, uint32_t tag = 0x44444D31u) {
#pragma clang fp contract(off)
    uint32_t c0 = e4, c1 = s, c2 = t, c3 = tag, k0 = nk.k0, k1 = nk.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    const float u0 = (float)((c0 >> 8) + 1u) * 5.9604644775390625e-8f, v0 = (float)(c1 >> 8) * 5.9604644775390625e-8f;   // 2^-24
    const float u1 = (float)((c2 >> 8) + 1u) * 5.9604644775390625e-8f, v1 = (float)(c3 >> 8) * 5.9604644775390625e-8f;
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u1));
    float s0, co0, s1, co1;
    sincospif(2.0f * v0, &s0, &co0);
    sincospif(2.0f * v1, &s1, &co1);
    return f32x4{r0 * co0, r0 * s0, r1 * co1, r1 * s1};
}

// One position map serves the three keyings of the stream (per sample, by canvas position, by clip position) in the stand-alone passes
// ("the stream's stand-alone passes" below).  Element (o, l, i) of sample b of a batch [B, outer, L, inner] draws at stream position
//   p = base + max(*cursor, 0) * cstep + b * bstep + l
// with element e' = o * inner + i.  The sum wraps in 64 bits and its low word is the contract's p: a negative clip origin arrives as
// its two's complement in base.  The keyings differ in the coefficients alone (stream_map below) and in the time word the caller passes.
struct StreamMap {
    uint32_t k0, k1;            // seed & 0xffffffff, seed >> 32
    uint64_t base, bstep, cstep;
    const int32_t* cursor;      // device int32 or null: only read, it addresses nothing
};
// the Philox call that holds element e' = o * inner + i: e' takes n[e' & 3]; where o * inner and i are multiples of 4 the four values are
// elements i .. i + 3 of the (o, l) slice
__device__ __forceinline__ f32x4 stream_normal4(const StreamMap& m, int b, int64_t o, int l, int64_t i, int64_t inner, uint32_t t,
                                                uint32_t tag) {
    int32_t c = m.cursor ? *m.cursor : 0;
    if (c < 0) c = 0;
    const uint64_t p = m.base + (uint64_t)c * m.cstep + (uint64_t)b * m.bstep + (uint64_t)l;
    return philox_normal4(NoiseKey{m.k0, m.k1, 0u}, (uint32_t)((o * inner + i) >> 2), (uint32_t)p, t, tag);
}
// per sample: the batch is [B, 1, 1, per], sample b at position s0 + b
static StreamMap stream_map(const NoiseKey& k) { return StreamMap{k.k0, k.k1, k.s0, 1, 0, nullptr}; }

static int make_noise_key(const avd_noise_key* key, int B, NoiseKey& nk) {
    AVD_REQUIRE(key, AVD_EINVAL, "noise key: null pointer");
    AVD_REQUIRE(B > 0, AVD_EINVAL, "noise key: B must be > 0 (got %d)", B);
    AVD_REQUIRE(key->sample_offset >= 0 && key->sample_offset + (int64_t)B <= ((int64_t)1 << 32), AVD_EINVAL,
                "noise key: sample_offset %lld + B %d must lie in [0, 2^32]", (long long)key->sample_offset, B);
    nk = NoiseKey{(uint32_t)(key->seed & 0xffffffffu), (uint32_t)(key->seed >> 32), (uint32_t)key->sample_offset};
    return AVD_OK;
}

// The checks the canvas key, the slot key and the clip guide share; `what` is the prefix of their messages.
// the batch's dims, named as the caller's contract names them (bn: "N" or "B"; ln: "L" or "slot_len"), and one position's slice below
// 2^34 elements: e' >> 2 fits the counter's word
static int check_keyed_dims(const char* what, const char* bn, int B, int64_t outer, const char* ln, int L, int64_t inner) {
    AVD_REQUIRE(B > 0 && outer > 0 && L > 0 && inner > 0, AVD_EINVAL, "%s: bad dims (%s %d, outer %lld, %s %d, inner %lld)", what, bn, B,
                (long long)outer, ln, L, (long long)inner);
    AVD_REQUIRE(outer <= (((int64_t)1 << 34) - 1) / inner, AVD_EINVAL, "%s: outer %lld * inner %lld must be < 2^34", what,
                (long long)outer, (long long)inner);
    return AVD_OK;
}
// a clip origin (whose: "slot key" or "clip guide"): stride >= 1 and |first| < 2^32
static int check_clip_origin(const char* what, const char* whose, int stride, int64_t first) {
    const int64_t lim = (int64_t)1 << 32;
    AVD_REQUIRE(stride >= 1, AVD_EINVAL, "%s: the %s's stride must be >= 1 (got %d)", what, whose, stride);
    AVD_REQUIRE(first > -lim && first < lim, AVD_EINVAL, "%s: the %s's first %lld must lie in (-2^32, 2^32)", what, whose, (long long)first);
    return AVD_OK;
}
// a slot table [B, slots] over L positions
static int check_slots(const char* what, int B, int L, int slots, int slot_len) {
    AVD_REQUIRE(slot_len >= 1 && slots >= 1 && (int64_t)slots * slot_len <= L && (int64_t)B * slots <= 0x7fffffff, AVD_EINVAL,
                "%s: slots %d * slot_len %d must lie in [1, L %d] and B %d * slots fit an int", what, slots, slot_len, L, B);
    return AVD_OK;
}

// ------------------------------------------------------------------ canvas keying of the seeded stream (window consensus at eta > 0)
// The contract is written out in include/avdiff_hip.h ("canvas-keyed noise").  A batch is N consecutive windows [N, outer, L, inner] of
// one canvas; element (o, l, i) of window b sits on canvas position p = (w0 + b) * hop + l and takes the per-sample stream's value for
// sample p, timestep t_now[b], element e' = o * inner + i: every window that covers p draws the same bits there.
struct CanvasKey {
    uint32_t k0, k1;   // seed & 0xffffffff, seed >> 32
    uint32_t w0;       // global index of window 0 of the launch
    uint32_t hop;      // canvas positions from one window to the next
};

// the Philox call that holds element e' = o * inner + i of canvas position p (window b, position l): e' takes n[e' & 3]; with
// inner % 4 == 0 and i % 4 == 0 the four values are elements i .. i + 3 of the (o, l) slice
// tag: as philox_normal4 (the canvas-keyed latent guide draws with GUIDE_TAG and t = 0)
__device__ __forceinline__ f32x4 canvas_normal4(const CanvasKey& ck, int b, int64_t o, int l, int64_t i, int64_t inner, uint32_t t,
                                                uint32_t tag = 0x44444D31u) {
    const uint64_t p = ((uint64_t)ck.w0 + (uint32_t)b) * ck.hop + (uint32_t)l;
    return philox_normal4(NoiseKey{ck.k0, ck.k1, 0u}, (uint32_t)((o * inner + i) >> 2), (uint32_t)p, t, tag);
}

// the checks of the canvas keying, all before any HIP call: hop >= 1, every canvas position of the batch below 2^32, and one position's
// slice outer * inner below 2^34 elements
// what: the stream the messages name ("canvas noise", or "canvas guide" for the latent guide's known noise)
int make_canvas_key(const avd_noise_key* key, int N, int64_t outer, int L, int hop, int64_t inner, CanvasKey& ck,
                    const char* what = "canvas noise") {
    AVD_REQUIRE(key, AVD_EINVAL, "%s: null noise key", what);
    if (int rc = check_keyed_dims(what, "N", N, outer, "L", L, inner)) return rc;
    AVD_REQUIRE(hop >= 1, AVD_EINVAL, "%s: hop must be >= 1 (got %d)", what, hop);
    const int64_t lim = (int64_t)1 << 32;
    AVD_REQUIRE(key->sample_offset >= 0 && key->sample_offset < lim && key->sample_offset + N - 1 <= (lim - L) / hop, AVD_EINVAL,
                "%s: (sample_offset %lld + N %d - 1) * hop %d + L %d must lie in [1, 2^32]", what, (long long)key->sample_offset, N,
                hop, L);
    ck = CanvasKey{(uint32_t)(key->seed & 0xffffffffu), (uint32_t)(key->seed >> 32), (uint32_t)key->sample_offset, (uint32_t)hop};
    return AVD_OK;
}

int check_canvas_key(const avd_noise_key* key, int N, int64_t outer, int L, int hop, int64_t inner) {
    CanvasKey ck;
    return make_canvas_key(key, N, outer, L, hop, inner, ck);
}

// window b at position (w0 + b) * hop
static StreamMap stream_map(const CanvasKey& k) { return StreamMap{k.k0, k.k1, (uint64_t)k.w0 * k.hop, k.hop, 0, nullptr}; }

// ------------------------------------------------------------------ clip keying of the seeded stream (slot timesteps at eta > 0)
// The contract is written out in include/avdiff_hip.h ("clip-keyed slot noise").  Sample b of a batch [B, outer, L, inner] holds clip
// slots first + max(*cursor, 0) + b * stride ..; element (o, l, i) sits on clip position p = that slot * slot_len + l (mod 2^32) and
// takes the per-sample stream's value for sample p, its slot's timestep and element e' = o * inner + i under the domain word SLOT_TAG:
// the draw follows the clip slot through the queue, whichever sample holds it.  The cursor is only read, and it addresses nothing.
constexpr uint32_t SLOT_TAG = 0x534C4F54u;      // "SLOT": apart from the stream a slot was initialised from (same positions, t = s_0)
struct SlotKey {
    uint32_t k0, k1;          // seed & 0xffffffff, seed >> 32
    int64_t first;            // clip slot of slot 0 of sample 0, before the cursor
    int32_t stride, slot_len; // clip slots from one sample to the next; positions of one slot
    const int32_t* cursor;    // device int32 or null
};

// as canvas_normal4; t: the timestep of the slot of position l.  The sum wraps in 64 bits, so its low word is the contract's p
__device__ __forceinline__ f32x4 slot_normal4(const SlotKey& sk, int b, int64_t o, int l, int64_t i, int64_t inner, uint32_t t) {
    int32_t m = sk.cursor ? *sk.cursor : 0;
    if (m < 0) m = 0;
    const uint64_t p = ((uint64_t)sk.first + (uint64_t)m + (uint64_t)b * (uint64_t)sk.stride) * (uint64_t)sk.slot_len + (uint64_t)l;
    return philox_normal4(NoiseKey{sk.k0, sk.k1, 0u}, (uint32_t)((o * inner + i) >> 2), (uint32_t)p, t, SLOT_TAG);
}

// the checks of the clip keying, all before any HIP call: stride >= 1, |first| < 2^32 and one position's slice below 2^34 elements
int make_slot_key(const avd_slot_key* key, int B, int64_t outer, int slot_len, int64_t inner, SlotKey& sk, const char* what = "slot noise") {
    AVD_REQUIRE(key, AVD_EINVAL, "%s: null slot key", what);
    if (int rc = check_keyed_dims(what, "B", B, outer, "slot_len", slot_len, inner)) return rc;
    if (int rc = check_clip_origin(what, "slot key", key->stride, key->first)) return rc;
    sk = SlotKey{(uint32_t)(key->seed & 0xffffffffu), (uint32_t)(key->seed >> 32), key->first, key->stride, slot_len, key->cursor};
    return AVD_OK;
}

int check_slot_key(const avd_slot_key* key, int B, int64_t outer, int slot_len, int64_t inner) {
    SlotKey sk;
    return make_slot_key(key, B, outer, slot_len, inner, sk);
}

// sample b at position (first + max(*cursor, 0) + b * stride) * slot_len, multiplied out
static StreamMap stream_map(const SlotKey& k) {
    return StreamMap{k.k0, k.k1, (uint64_t)k.first * (uint64_t)k.slot_len, (uint64_t)k.stride * (uint64_t)k.slot_len, (uint64_t)k.slot_len, k.cursor};
}

// ------------------------------------------------------------------ clip batch keying (K queues in one batch)
// The contract is written out in include/avdiff_hip.h ("clip batch keying").  The batch is K queues of Bq samples: sample b is sample
// b' = b % Bq of queue k = b / Bq, the clip-position walk restarts in every queue (b' takes b's place in slot_normal4 / clip_guide_pos)
// and queue k draws under its own seeds and reads its own canvases.  This is the one per-queue map: every keyed kernel resolves its
// SlotKey, StreamMap or ClipGuideState through it and then calls the one-queue function, so the bits are the one-queue bits.
struct ClipQueues {
    int Bq;                        // samples of one queue
    const uint64_t* step_seeds;    // K device seeds of the step noise; read only where a SlotKey (a draw's StreamMap) rides along
    const uint64_t* guide_seeds;   // K device seeds of the guide's known noise; read only where a ClipGuideState rides along
    int64_t canvas;                // outer * P * inner: floats from one queue's known / mask canvas to the next
};
struct QueueOf {
    int k, b;                      // the queue, and the sample's index inside it
};
__device__ __forceinline__ QueueOf queue_of(const ClipQueues& q, int b) {
    const int k = (int)((uint32_t)b / (uint32_t)q.Bq);
    return QueueOf{k, b - k * q.Bq};
}
__device__ __forceinline__ SlotKey queue_slot_key(const ClipQueues& q, SlotKey sk, int k) {
    const uint64_t seed = q.step_seeds[k];
    sk.k0 = (uint32_t)(seed & 0xffffffffu);
    sk.k1 = (uint32_t)(seed >> 32);
    return sk;
}
__device__ __forceinline__ StreamMap queue_stream_map(const ClipQueues& q, StreamMap m, int k) {
    const uint64_t seed = q.step_seeds[k];
    m.k0 = (uint32_t)(seed & 0xffffffffu);
    m.k1 = (uint32_t)(seed >> 32);
    return m;
}
// the SlotKey a lane of the fused kernels draws with: the pack's own, or under a ClipQueues its queue's (qo: queue_of the lane's sample)
template <class... Key> __device__ __forceinline__ SlotKey lane_slot_key(const QueueOf& qo, const Key&... nk) {
    if constexpr (PackHas<ClipQueues, Key...>::value) return queue_slot_key(pack_get<ClipQueues>(nk...), pack_get<SlotKey>(nk...), qo.k);
    else return pack_get<SlotKey>(nk...);
}
// The host side: the descriptor's checks, all before any HIP call.  step / guide: the launch reads the step seeds / the guide seeds;
// outs: the buffers the launch writes (n floats each, nullptr skipped); known / mask: the K canvases together (nc floats each, null: none)
static int make_clip_queues(const char* what, const avd_clip_queues* cq, int B, bool step, bool guide,
                            std::initializer_list<const float*> outs, int64_t n, const float* known, const float* mask, int64_t nc,
                            int64_t canvas, ClipQueues& q) {
    AVD_REQUIRE(cq, AVD_EINVAL, "%s: null clip queues", what);
    AVD_REQUIRE(cq->K >= 1 && B > 0 && B % cq->K == 0, AVD_EINVAL, "%s: the %d queues must divide the batch %d", what, cq->K, B);
    AVD_REQUIRE(!step || cq->step_seeds, AVD_EINVAL, "%s: eta > 0 in a clip batch needs step_seeds, one per queue", what);
    AVD_REQUIRE(!guide || cq->guide_seeds, AVD_EINVAL, "%s: a clip guide in a clip batch needs guide_seeds, one per queue", what);
    const struct { const uint64_t* p; const char* name; } seeds[2] = {{step ? cq->step_seeds : nullptr, "step_seeds"},
                                                                      {guide ? cq->guide_seeds : nullptr, "guide_seeds"}};
    for (const auto& s : seeds) {
        if (!s.p) continue;
        AVD_REQUIRE((reinterpret_cast<uintptr_t>(s.p) & 7u) == 0, AVD_EINVAL, "%s: %s must be 8-byte aligned", what, s.name);
        const char *sb = reinterpret_cast<const char*>(s.p), *se = sb + 8 * (int64_t)cq->K;
        for (const float* o : outs) {
            const char* ob = reinterpret_cast<const char*>(o);
            AVD_REQUIRE(!o || !(sb < ob + 4 * n && ob < se), AVD_EINVAL, "%s: %s must not overlap out, z_out or x0_hist", what, s.name);
        }
        for (const float* c : {known, mask}) {
            const char* cb = reinterpret_cast<const char*>(c);
            AVD_REQUIRE(!c || !(sb < cb + 4 * nc && cb < se), AVD_EINVAL, "%s: known / mask must not overlap %s", what, s.name);
        }
    }
    q = ClipQueues{B / cq->K, step ? cq->step_seeds : nullptr, guide ? cq->guide_seeds : nullptr, canvas};
    return AVD_OK;
}

// ------------------------------------------------------------------ FIFO queue moves (diagonal denoising)
// The contracts are written out in include/avdiff_hip.h ("FIFO queue shift", "... with history", "... off a device cursor", "Guided FIFO
// queue shift", "FIFO lookahead", "slot APG momentum", "FIFO clip batch").  Every one of them is one move of one slot map.
// The batch [B, outer, L, inner] with L = S * slot_len holds K queues of Bq = B / K windows, queue k in samples k * Bq ..  Window b of
// a queue holds logical slots b * h .. b * h + S - 1 of its Q = ctx + Bq * h slots, h = S - ctx: the first ctx slots of a window are
// held context (duplicates of the window before), the others step.  Logical slot q is read from its owner copy: window 0 slot q for
// q < ctx, window (q - ctx) / h slot ctx + (q - ctx) % h otherwise.  A move writes window b slot s = Old[b * h + s + shift]; Old[Q]
// (shift == 1 only) is the entering tail.  The plain shift and the clip batch are ctx = 0, shift = 1; the one-queue entries are K = 1.
struct QueueGeom {
    int Bq, S, ctx, shift, slot_len;
    int64_t outer, inner;
};
struct QueueSrc {
    int64_t off;      // the source's element offset in a buffer of z's layout; < 0: the entering tail
    bool step;        // s >= ctx: a stepping position, where a rider lives
};
// the source of element (o, j, i) of slot s of window b of queue kq.  q <= Q <= B * S fits an int (the host checks), so the two
// divisions are 32-bit.  This is the one place a queue source is computed: the head, logical slot ctx, is (b, s) = (0, ctx - shift).
__device__ __forceinline__ QueueSrc queue_source(const QueueGeom& g, int kq, int b, int s, int64_t o, int j, int64_t i) {
    const uint32_t h = (uint32_t)(g.S - g.ctx);
    const int q = b * (int)h + s + g.shift;
    const bool step = s >= g.ctx;
    if (q >= g.ctx + g.Bq * (int)h) return QueueSrc{-1, step};
    int bs = 0, ss = q;
    if (q >= g.ctx) {
        bs = (int)((uint32_t)(q - g.ctx) / h);
        ss = g.ctx + (int)((uint32_t)(q - g.ctx) % h);
    }
    const int64_t L = (int64_t)g.S * g.slot_len;
    return QueueSrc{((((int64_t)kq * g.Bq + bs) * g.outer + o) * L + (int64_t)ss * g.slot_len + j) * g.inner + i, step};
}

// The tracks of a move.  The latent track copies every position and draws the tail: the canvas-keyed normals of canvas positions
// c * slot_len + j at timestep t (canvas_normal4 with window index c and hop slot_len, the bits of avd_canvas_noise_f32), under `seed`
// or the queue's own seeds[k], at clip slot c or c + *cursor (the cursor keys the draw, it addresses nothing).  The head of queue k
// (window 0, slot ctx) goes to slot m of canvas k of `heads`, [K, outer, n_clip * slot_len, inner]; m by value or *cursor, compared with
// [0, n_clip) before any address is formed.  The dense one-slot `popped` is n_clip = 1, m = 0, K = 1.  The cursor is only read here.
struct QueueLatent {
    const float* in;
    float *out, *heads;
    int64_t n_clip, m;
    const int32_t* cursor;      // device int32 or null
    const uint64_t* seeds;      // K device seeds or null
    uint64_t seed;
    uint32_t c, t;
};
// A rider (the x0 history, the slot momentum) is a buffer of z's layout that travels with its slot: the latent's source offset on a
// stepping position whose source is not the tail, zeros elsewhere (never read: the tail's t_last is -1).  Nothing of a rider is popped.
struct QueueRiders {
    const float* in[2];
    float* out[2];
};
// A GuideShift ending the arguments ("guided FIFO queue shift") puts the entering tail slot on the clip guide's forward path inside
// this launch: the lane that drew the tail's normals blends them with q_p(t) of clip positions c * slot_len + j.  It is defined with
// the clip guide below, whose gather and blend it calls; a launch without a guide carries none of its state.
struct GuideShift;

template <int V> __device__ __forceinline__ f32x4 load_v(const float* p) {
    if constexpr (V == 4) return *reinterpret_cast<const f32x4*>(p);
    else return f32x4{*p, 0.f, 0.f, 0.f};
}
template <int V> __device__ __forceinline__ void store_v(float* p, f32x4 v) {
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(p) = v;
    else *p = v[0];
}

// lane idx -> (b, o, l, i) of [B, outer, L, inner / V].  At the queues' sizes the move is paced by this arithmetic more than by memory
// (profiles/fifo_move_kernels.txt, table 2: with 64-bit divisions in every lane the one kernel ran 0.3 - 0.7 us behind the parent's
// at B = 32), so a launch of fewer than 2^32 lanes (a uniform test) divides in 32 bits
struct QueueLane {
    int b, l;
    int64_t o, i;
};
template <class T, int V> __device__ __forceinline__ QueueLane queue_lane(T idx, T iv, T L, T outer) {
    const T r = idx / iv, row = r / L;
    return QueueLane{(int)(row / outer), (int)(r % L), (int64_t)(row % outer), (int64_t)(idx % iv) * V};
}

// V == 4: inner % 4 == 0 and every base 16-byte aligned, a lane's float4 lies inside one (o, l) slice; V == 1: one element per lane.
// Lanes in the order idx -> (b, o, l, i).  Lanes [0, n_out) write the tracks, lanes [n_out, n_out + n_heads)
// the K heads of n_pop lanes each (n_heads == 0 at shift == 0 and without the latent track).  R riders; LATENT false is the carry:
// the rider map alone.
template <int V, int R, bool LATENT, class... Guide>
__global__ __launch_bounds__(256) void fifo_move_kernel(QueueGeom g, QueueLatent z, QueueRiders rd, int64_t n_out, int64_t n_pop,
                                                        int64_t n_heads, Guide... guide) {
    static_assert(sizeof...(Guide) == (PackHas<GuideShift, Guide...>::value ? 1 : 0) && (LATENT || sizeof...(Guide) == 0),
                  "the pack: optionally one GuideShift, on a latent track");
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_out + n_heads) return;
    const int64_t iv = g.inner / V;
    if (idx >= n_out) {      // heads[kq, o, m * slot_len + j, i] = the head's owner copy
        if constexpr (LATENT) {
            const int64_t m = z.cursor ? (int64_t)*z.cursor : z.m;
            if (m < 0 || m >= z.n_clip) return;      // a head outside the clip is written nowhere
            int64_t r = idx - n_out;
            const int kq = (int)(r / n_pop);
            r %= n_pop;
            const int64_t i = (r % iv) * V;
            r /= iv;
            const int j = (int)(r % g.slot_len);
            const int64_t o = r / g.slot_len;
            float* dst = z.heads + (((kq * g.outer + o) * z.n_clip + m) * g.slot_len + j) * g.inner + i;
            store_v<V>(dst, load_v<V>(z.in + queue_source(g, kq, 0, g.ctx - g.shift, o, j, i).off));
        }
        return;
    }
    const int L = g.S * g.slot_len;
    const QueueLane ln = n_out + n_heads <= 0xffffffffll ? queue_lane<uint32_t, V>((uint32_t)idx, (uint32_t)iv, (uint32_t)L, (uint32_t)g.outer)
                                                         : queue_lane<int64_t, V>(idx, iv, (int64_t)L, g.outer);
    const int b = ln.b, l = ln.l;
    const int64_t o = ln.o, i = ln.i;
    const int kq = b < g.Bq ? 0 : (int)((uint32_t)b / (uint32_t)g.Bq);      // one queue: no lane divides
    const int s = (int)((uint32_t)l / (uint32_t)g.slot_len), j = l - s * g.slot_len;
    // a rider alone reads nothing on a context position: its source is not looked up
    const QueueSrc src = LATENT || s >= g.ctx ? queue_source(g, kq, b - kq * g.Bq, s, o, j, i) : QueueSrc{-1, false};
    f32x4 v = {0.f, 0.f, 0.f, 0.f}, rv[R > 0 ? R : 1];
#pragma unroll
    for (int a = 0; a < R; ++a) rv[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (src.off >= 0) {      // every load ahead of the stores
        if constexpr (LATENT) v = load_v<V>(z.in + src.off);
        if (src.step) {
#pragma unroll
            for (int a = 0; a < R; ++a) rv[a] = load_v<V>(rd.in[a] + src.off);
        }
    } else if constexpr (LATENT) {      // the tail slot of queue kq: fresh noise of its clip slot
        const uint64_t seed = z.seeds ? z.seeds[kq] : z.seed;
        const CanvasKey ck{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), z.c + (z.cursor ? (uint32_t)*z.cursor : 0u),
                           (uint32_t)g.slot_len};
        v = canvas_normal4(ck, 0, o, j, i, g.inner, z.t);
        if constexpr (V == 1) v[0] = v[(int)((o * g.inner + i) & 3)];
        if constexpr (sizeof...(Guide) > 0) {      // blend(m(p), q_p(t), fresh): the bits of the stand-alone pass on this slot
            v = pack_get<GuideShift>(guide...).template tail<V>(o, j, i, g.inner, z.t, v);
        }
    }
    if constexpr (LATENT) store_v<V>(z.out + idx * V, v);
#pragma unroll
    for (int a = 0; a < R; ++a) store_v<V>(rd.out[a] + idx * V, rv[a]);
}

// What an entry asks of fifo_move.  Every check is made in fifo_move_check, before any HIP call.
struct MoveTrack {
    const float* in;
    float* out;
    const char *in_name, *out_name;
};
struct QueueMove {
    const char* what;                 // the entry's prefix in messages
    const char *family, *opts;        // the profile label: "<family><V<opts>>"
    double bytes;                     // what the entry tells the profile it moves
    int B, K, S, ctx, shift, slot_len;
    int64_t outer, inner;
    bool latent;                      // false: the carry, riders[0] alone
    MoveTrack z, riders[2];           // a rider pair both null or both set
    float* heads;                     // null exactly at shift == 0 (and without the latent track)
    const char* heads_name;
    int64_t n_clip, m;
    const int32_t* cursor;
    const avd_noise_key* key;         // the seed by value, or
    const uint64_t* seeds;            // one device seed per queue
    int64_t t, c;
};

template <int... N, class F> void with_int(int n, F&& f) { (void)((n == N ? (f(std::integral_constant<int, N>{}), true) : false) || ...); }

// what the checks leave for the launch
struct MovePlan {
    QueueGeom g;
    QueueLatent z;
    QueueRiders rd;
    int R, v;
    int64_t n_out, n_pop, n_heads;
};

int fifo_move_check(const QueueMove& d, MovePlan& plan) {
    const char* w = d.what;
    const bool draws = d.latent && d.shift == 1;
    const int64_t lim = (int64_t)1 << 32;
    AVD_REQUIRE(d.shift == 0 || d.shift == 1, AVD_EINVAL, "%s: shift must be 0 or 1 (got %d)", w, d.shift);
    AVD_REQUIRE(d.latent ? d.z.in && d.z.out : d.riders[0].in && d.riders[0].out, AVD_EINVAL, "%s: null pointer", w);
    for (const MoveTrack& r : d.riders)
        AVD_REQUIRE(!r.in == !r.out, AVD_EINVAL, "%s: %s and %s go together", w, r.in_name, r.out_name);
    AVD_REQUIRE(d.B > 0 && d.outer > 0 && d.S > 0 && d.slot_len > 0 && d.inner > 0, AVD_EINVAL,
                "%s: bad dims (B %d, outer %lld, S %d, slot_len %d, inner %lld)", w, d.B, (long long)d.outer, d.S, d.slot_len, (long long)d.inner);
    AVD_REQUIRE(d.ctx >= 0 && d.ctx < d.S, AVD_EINVAL, "%s: ctx %d must lie in [0, slots %d)", w, d.ctx, d.S);
    AVD_REQUIRE((int64_t)d.S * d.slot_len <= 0x7fffffff && (int64_t)d.B * d.S <= 0x7fffffff, AVD_EINVAL,
                "%s: S %d * slot_len %d and B %d * S must fit an int", w, d.S, d.slot_len, d.B);
    AVD_REQUIRE(d.K >= 1 && d.B % d.K == 0, AVD_EINVAL, "%s: the %d queues must divide the batch %d", w, d.K, d.B);
    if (draws) {
        AVD_REQUIRE(d.key || d.seeds, AVD_EINVAL, "%s: null noise key or seeds", w);
        AVD_REQUIRE((reinterpret_cast<uintptr_t>(d.seeds) & 7u) == 0, AVD_EINVAL, "%s: seeds must be 8-byte aligned", w);
        AVD_REQUIRE(d.heads, AVD_EINVAL, "%s: null %s at shift 1", w, d.heads_name);
        AVD_REQUIRE(d.t >= 0 && d.t < lim, AVD_EINVAL, "%s: the noise timestep %lld must lie in [0, 2^32)", w, (long long)d.t);
        // every clip slot the draw can name inside the clip: c alone, or c0 .. c0 + n_clip - 1 off a cursor
        const int64_t nc = d.cursor ? d.n_clip : 1;
        AVD_REQUIRE(d.c >= 0 && d.c < lim && nc >= 1 && nc <= lim && d.c + nc <= lim / d.slot_len, AVD_EINVAL,
                    d.cursor ? "%s: (c0 %lld + n_out %lld) * slot_len %d must lie in [1, 2^32]" : "%s: (c %lld + %lld) * slot_len %d must lie in [1, 2^32]",
                    w, (long long)d.c, (long long)nc, d.slot_len);
        AVD_REQUIRE(d.n_clip >= 1 && d.n_clip <= lim / d.slot_len, AVD_EINVAL, "%s: n_clip %lld * slot_len %d must lie in [1, 2^32]", w,
                    (long long)d.n_clip, d.slot_len);
        AVD_REQUIRE((double)d.K * (double)d.outer * (double)d.n_clip * (double)d.slot_len * (double)d.inner < 9.0e18, AVD_EUNSUPPORTED,
                    "%s: too large a clip canvas", w);
    } else
        AVD_REQUIRE(!d.heads, AVD_EINVAL, "%s: nothing is popped at shift 0, %s must be null", w, d.heads_name);
    AVD_REQUIRE(!d.latent || d.outer <= (((int64_t)1 << 34) - 1) / d.inner, AVD_EINVAL, "%s: outer %lld * inner %lld must be < 2^34", w,
                (long long)d.outer, (long long)d.inner);
    AVD_REQUIRE((double)d.B * (double)d.outer * (double)d.S * (double)d.slot_len * (double)d.inner < 9.0e18, AVD_EUNSUPPORTED,
                "%s: too many values", w);
    const int64_t total = (int64_t)d.B * d.outer * d.S * d.slot_len * d.inner, pop = draws ? d.outer * d.slot_len * d.inner : 0;
    // every buffer apart from every other, by byte spans (null: absent): slot q reads slot q + 1 of every input, across block and sample
    // boundaries.  pair > 0: an in / out pair, adjacent in the list
    struct { const void* p; int64_t bytes; const char* name; int pair; } sp[9];
    int n_sp = 0, R = 0;
    if (d.latent) {
        sp[n_sp++] = {d.z.in, 4 * total, d.z.in_name, 1};
        sp[n_sp++] = {d.z.out, 4 * total, d.z.out_name, 1};
    }
    QueueRiders rd{{nullptr, nullptr}, {nullptr, nullptr}};
    for (const MoveTrack& r : d.riders)
        if (r.in) {
            rd.in[R] = r.in;
            rd.out[R++] = r.out;
            sp[n_sp++] = {r.in, 4 * total, r.in_name, 1 + R};
            sp[n_sp++] = {r.out, 4 * total, r.out_name, 1 + R};
        }
    if (draws) {
        sp[n_sp++] = {d.heads, 4 * pop * d.n_clip * d.K, d.heads_name, 0};
        sp[n_sp++] = {d.seeds, 8 * (int64_t)d.K, "seeds", 0};
        sp[n_sp++] = {d.cursor, 4, "the cursor", 0};
    }
    auto phrase = [&](int k, const char* joint) {      // a buffer alone by its name, a pair's by both: "x_in <joint> x_out"
        if (!sp[k].pair) return std::string(sp[k].name);
        const int first = k > 0 && sp[k - 1].pair == sp[k].pair ? k - 1 : k;
        return std::string(sp[first].name) + joint + sp[first + 1].name;
    };
    for (int b = 1; b < n_sp; ++b)
        for (int a = 0; a < b; ++a) {
            const char *pa = static_cast<const char*>(sp[a].p), *pb = static_cast<const char*>(sp[b].p);
            if (!pa || !pb || !(pa < pb + sp[b].bytes && pb < pa + sp[a].bytes)) continue;
            if (sp[a].pair && sp[a].pair == sp[b].pair)
                return avd::set_error(AVD_EINVAL, "%s: %s must not overlap %s (one out-of-place launch)", w, sp[b].name, sp[a].name);
            return avd::set_error(AVD_EINVAL, "%s: %s must not overlap %s", w, phrase(b, " and ").c_str(), phrase(a, " or ").c_str());
        }
    bool vec = d.inner % 4 == 0 && aligned16(d.heads);
    for (int k = 0; k < n_sp; ++k)
        if (sp[k].pair) vec = vec && aligned16(sp[k].p);
    const int v = vec ? 4 : 1;
    const int64_t n_out = total / v, n_pop = pop / v, n_heads = n_pop * d.K;
    AVD_REQUIRE((n_out + n_heads + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "%s: %lld lanes are too many for one launch", w,
                (long long)(n_out + n_heads));
    plan = MovePlan{QueueGeom{d.B / d.K, d.S, d.ctx, d.shift, d.slot_len, d.outer, d.inner},
                    QueueLatent{d.z.in, d.z.out, d.heads, d.n_clip, d.m, d.cursor, d.seeds, d.key ? d.key->seed : 0, (uint32_t)d.c, (uint32_t)d.t},
                    rd, R, v, n_out, n_pop, n_heads};
    return AVD_OK;
}

template <class... Guide> int fifo_move_launch(const QueueMove& d, const MovePlan& p, hipStream_t st, Guide... guide) {
    // a label names a launch family (the entry and its options), not a symbol: the profiles and the bench tools key on it
    ProfScope prof(g_prof_on ? prof_tag_id("%s<%d%s>", d.family, p.v, d.opts) : 0, d.bytes, st);
    const dim3 grid((unsigned)((p.n_out + p.n_heads + 255) / 256));
    auto launch = [&](auto V, auto Rc, auto Lat) {
        hipLaunchKernelGGL((fifo_move_kernel<decltype(V)::value, decltype(Rc)::value, decltype(Lat)::value, Guide...>), grid, dim3(256), 0, st,
                           p.g, p.z, p.rd, p.n_out, p.n_pop, p.n_heads, guide...);
    };
    with_int<1, 4>(p.v, [&](auto V) {
        if constexpr (sizeof...(Guide) > 0) with_int<0, 1>(p.R, [&](auto Rc) { launch(V, Rc, std::true_type{}); });      // the history at most
        else if (d.latent) with_int<0, 1, 2>(p.R, [&](auto Rc) { launch(V, Rc, std::true_type{}); });
        else launch(V, std::integral_constant<int, 1>{}, std::false_type{});
    });
    AVD_CHECK_LAUNCH(d.what);
    return AVD_OK;
}

int fifo_move(const QueueMove& d, hipStream_t st) {
    MovePlan plan;
    if (int rc = fifo_move_check(d, plan)) return rc;
    return fifo_move_launch(d, plan, st);
}

// the profile's byte counts below: one slot's and the batch's floats, in double (they are formed before the checks)
static double slot_floats(int64_t outer, int slot_len, int64_t inner) { return (double)outer * slot_len * (double)inner; }

// hist_in / hist_out: both null (the plain shift) or both set (the shift with history).  cursor: null = the by-value shift (clip slot c,
// `popped` one slot).  Set = the shift off a device cursor: c is c0, the kernel takes clip slot c0 + *cursor, and `popped` is the clip
// canvas [outer, n_clip * slot_len, inner].  what / guided: fifo_shift_guided_f32's (below the clip guide), which adds the tail's reads
QueueMove fifo_shift_move(const avd_noise_key* key, int64_t t, int64_t c, const float* z_in, float* z_out, float* popped, int B,
                          int64_t outer, int S, int slot_len, int64_t inner, const float* hist_in, float* hist_out,
                          const int32_t* cursor = nullptr, int64_t n_clip = 1, bool guided = false) {
    const double slot = slot_floats(outer, slot_len, inner), total = (double)B * S * slot;
    const char* opts = guided ? (hist_in ? ", HistShift, GuideShift" : ", GuideShift")
                     : cursor ? (hist_in ? ", HistShift, CursorShift" : ", CursorShift") : (hist_in ? ", HistShift" : "");
    // read + write of the queue (and of the history), the popped slot's write (and the guide's known / mask reads of the tail slot)
    return QueueMove{guided ? "fifo_shift_guided" : "fifo_shift", "fifo_shift_kernel", opts,
                     4.0 * ((hist_in ? 4.0 : 2.0) * total + (guided ? 3.0 : 1.0) * slot), B, 1, S, 0, 1, slot_len, outer, inner, true,
                     {z_in, z_out, "z_in", "z_out"}, {{hist_in, hist_out, "hist_in", "hist_out"}, {nullptr, nullptr, "", ""}}, popped,
                     cursor ? "the clip canvas" : "popped", n_clip, 0, cursor, key, nullptr, t, c};
}
int fifo_shift_f32(const avd_noise_key* key, int64_t t, int64_t c, const float* z_in, float* z_out, float* popped, int B, int64_t outer,
                   int S, int slot_len, int64_t inner, hipStream_t st, const float* hist_in = nullptr, float* hist_out = nullptr,
                   const int32_t* cursor = nullptr, int64_t n_clip = 1) {
    return fifo_move(fifo_shift_move(key, t, c, z_in, z_out, popped, B, outer, S, slot_len, inner, hist_in, hist_out, cursor, n_clip), st);
}

// hist_in / hist_out: both null or both set.  shift == 0 refreshes the duplicates only: key, t and c are not read, popped must be null
int fifo_lookahead_f32(const avd_noise_key* key, int64_t t, int64_t c, int shift, const float* z_in, float* z_out, float* popped, int B,
                       int64_t outer, int S, int ctx, int slot_len, int64_t inner, hipStream_t st, const float* hist_in = nullptr,
                       float* hist_out = nullptr) {
    // every owner read once (the duplicates' reads hit the cache), B * S slots written; twice that with the history; the popped slot
    const double slot = slot_floats(outer, slot_len, inner), Q = (double)ctx + (double)B * (S - ctx);
    return fifo_move(QueueMove{"fifo_lookahead", "fifo_lookahead_kernel", hist_in ? ", hist" : "",
                               4.0 * ((hist_in ? 2.0 : 1.0) * (Q + (double)B * S) * slot + (shift ? slot : 0.0)), B, 1, S, ctx, shift, slot_len,
                               outer, inner, true, {z_in, z_out, "z_in", "z_out"},
                               {{hist_in, hist_out, "hist_in", "hist_out"}, {nullptr, nullptr, "", ""}}, popped, "popped", 1, 0, nullptr, key,
                               nullptr, t, c}, st);
}

// the rider map alone ("slot APG momentum").  Neither a clip slot nor a cursor enters: one launch serves the eager loops and a graph
int fifo_carry_f32(const float* in, float* out, int B, int64_t outer, int S, int ctx, int shift, int slot_len, int64_t inner,
                   hipStream_t st) {
    // every stepping owner but the head read once, B * S slots written
    return fifo_move(QueueMove{"fifo_carry", "fifo_carry_kernel", "",
                               4.0 * ((double)B * (S - ctx) - shift + (double)B * S) * slot_floats(outer, slot_len, inner), B, 1, S, ctx, shift,
                               slot_len, outer, inner, false, {nullptr, nullptr, "", ""},
                               {{in, out, "in", "out"}, {nullptr, nullptr, "", ""}}, nullptr, "popped", 1, 0, nullptr, nullptr, nullptr, 0, 0}, st);
}

// K queues in lockstep: the seed of a lane's queue is read from `seeds`, the head goes into slot m of the queue's own clip canvas.
// r1_in / r1_out and r2_in / r2_out: the rider pairs, each both null or both set (the history, the slot momentum: either alone or both)
int fifo_shift_clips_f32(const uint64_t* seeds, int64_t t, int64_t c, const float* z_in, float* z_out, float* clips, int64_t n_clip,
                         int64_t m, const float* r1_in, float* r1_out, const float* r2_in, float* r2_out, int B, int K, int64_t outer, int S,
                         int slot_len, int64_t inner, hipStream_t st) {
    const int R = (r1_in ? 1 : 0) + (r2_in ? 1 : 0);
    static const char* const opts[3] = {", 0", ", 1", ", 2"};
    // read + write of the queues and of every rider, the K heads' writes
    const double slot = slot_floats(outer, slot_len, inner);
    return fifo_move(QueueMove{"fifo_shift_clips", "fifo_shift_clips_kernel", opts[R], 4.0 * (2.0 * (1 + R) * (double)B * S + (double)K) * slot,
                               B, K, S, 0, 1, slot_len, outer, inner, true, {z_in, z_out, "z_in", "z_out"},
                               {{r1_in, r1_out, "hist_in", "hist_out"}, {r2_in, r2_out, "carry_in", "carry_out"}}, clips,
                               "the clip canvases", n_clip, m, nullptr, nullptr, seeds, t, c}, st);
}

// ------------------------------------------------------------------ device cursors of the FIFO queue
// The contracts are written out in include/avdiff_hip.h ("FIFO device cursors").  A cursor is one int32 on the device; no kernel below
// addresses by it without a clamp or a guard, and it moves only in cursor_add_kernel, a launch of its own behind its last reader.
__global__ void cursor_add_kernel(int32_t* cursor, int delta) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *cursor += delta;
}

// out_k[j] = tab_k[row, j] for the NT tables, row = clamp(*cursor, 0, n_rows - 1), j < n: the slot analogue of sched_advance_kernel
struct SlotTabs {
    const int64_t* tab[3];
    int64_t* out[3];
};
template <int NT>
__global__ __launch_bounds__(256) void slot_tables_select_kernel(SlotTabs tb, const int32_t* __restrict__ cursor, int n_rows, int n) {
    int r = *cursor;
    r = r < 0 ? 0 : (r > n_rows - 1 ? n_rows - 1 : r);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
#pragma unroll
    for (int k = 0; k < NT; ++k) tb.out[k][j] = tb.tab[k][(int64_t)r * n + j];
}

// out[b, o, l, i] = canvas[o, (m + b * S) * hop + l, i] where that position is below P, else 0; m = max(*cursor, 0).  V lanes as
// fifo_move_kernel; every index is 64-bit.  n: B * outer * len * inner / V lanes.
template <int V>
__global__ __launch_bounds__(256) void fifo_prompt_gather_kernel(const float* __restrict__ canvas, float* __restrict__ out,
                                                                 const int32_t* __restrict__ cursor, int S, int64_t hop, int64_t outer,
                                                                 int64_t P, int64_t len, int64_t inner, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    int64_t m = *cursor;
    if (m < 0) m = 0;
    const int64_t iv = inner / V;
    const int64_t i = (idx % iv) * V;
    int64_t r = idx / iv;
    const int64_t l = r % len;
    r /= len;
    const int64_t o = r % outer, b = r / outer;
    const int64_t p = (m + b * S) * hop + l;      // m, B * S, hop and len each fit an int (the host checks): below 2^63
    if constexpr (V == 4) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < P) v = *reinterpret_cast<const f32x4*>(canvas + (o * P + p) * inner + i);
        *reinterpret_cast<f32x4*>(out + idx * 4) = v;
    } else
        out[idx] = p < P ? canvas[(o * P + p) * inner + i] : 0.f;
}

// The gather above on a rational hop num / den (include/avdiff_hip.h, "fractional prompt hop"): sample b holds clip slot q = first +
// clamp(*cursor, 0, m_cap) + b * stride (no cursor: q = first + b * stride), i0 = floor(q * num / den), rem = q * num - i0 * den.
// m_cap is the host's: from it on every window of the call lies past the canvas end, so the clamp changes no value and keeps q * num
// below 2^63 whatever the cursor holds.  q, i0 and rem are per sample: once per lane, from b.  A position is compared with [0, P)
// before it is loaded, in either operand.
constexpr int kPromptNearest = 0, kPromptLinear = 1;

__device__ __forceinline__ float prompt_lerp(float a, float b, float f) {
#pragma clang fp contract(off)
    return a + f * (b - a);
}

template <int V, int INTERP>
__global__ __launch_bounds__(256) void fifo_prompt_gather_frac_kernel(const float* __restrict__ canvas, float* __restrict__ out,
                                                                      const int32_t* __restrict__ cursor, int64_t m_cap, int64_t first,
                                                                      int64_t stride, int64_t num, int64_t den, int64_t outer, int64_t P,
                                                                      int64_t len, int64_t inner, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    int64_t m = 0;
    if (cursor) {
        m = *cursor;
        m = m < 0 ? 0 : (m > m_cap ? m_cap : m);
    }
    const int64_t iv = inner / V;
    const int64_t i = (idx % iv) * V;
    int64_t r = idx / iv;
    const int64_t l = r % len;
    r /= len;
    const int64_t o = r % outer, b = r / outer;
    const int64_t t = (first + m + b * stride) * num;      // |q| * num < 2^62 (the host checks)
    int64_t i0 = t / den, rem = t - i0 * den;
    if (rem < 0) {      // C++ division truncates: make it a floor
        rem += den;
        --i0;
    }
    int64_t pa = i0 + l;
    if constexpr (INTERP == kPromptNearest) pa += 2 * rem >= den ? 1 : 0;
    const bool in_a = pa >= 0 && pa < P;
    const bool blend = INTERP == kPromptLinear && rem != 0;      // rem == 0: a itself, b is not read
    const bool in_b = blend && pa + 1 >= 0 && pa + 1 < P;
    const float f = blend ? (float)rem / (float)den : 0.f;
    const float* row = canvas + o * P * inner + i;      // position p of this lane is row + p * inner, formed under in_a / in_b only
    if constexpr (V == 4) {
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (in_a) a = *reinterpret_cast<const f32x4*>(row + pa * inner);
        if (blend) {
            f32x4 nb = f32x4{0.f, 0.f, 0.f, 0.f};
            if (in_b) nb = *reinterpret_cast<const f32x4*>(row + (pa + 1) * inner);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = prompt_lerp(a[j], nb[j], f);
        }
        *reinterpret_cast<f32x4*>(out + idx * 4) = a;
    } else {
        float a = in_a ? row[pa * inner] : 0.f;
        if (blend) a = prompt_lerp(a, in_b ? row[(pa + 1) * inner] : 0.f, f);
        out[idx] = a;
    }
}

__global__ __launch_bounds__(256) void ddim_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                   const int64_t* __restrict__ t_now, const int64_t* __restrict__ t_prev,
                                                   const float* __restrict__ abar, int T_train, float eta,
                                                   const float* __restrict__ noise, float* __restrict__ out,
                                                   int64_t per, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / per);
    const Ddim c = ddim_coef(t_now, t_prev, abar, T_train, eta, b);
    out[i] = ddim_apply(c, x[i], eps[i], eta > 0.f ? noise[i] : 0.f);
}

int ddim_step_f32(const float* x_t, const float* eps, const int64_t* t_now, const int64_t* t_prev, const float* abar,
                  int T_train, float eta, const float* noise, float* x_prev, int B, int64_t per, hipStream_t st) {
    AVD_REQUIRE(x_t && eps && t_now && t_prev && abar && x_prev, AVD_EINVAL, "ddim_step: null pointer");
    AVD_REQUIRE(B > 0 && per > 0 && T_train > 0, AVD_EINVAL, "ddim_step: bad dims");
    AVD_REQUIRE(eta >= 0.f, AVD_EINVAL, "ddim_step: eta must be >= 0");
    AVD_REQUIRE(eta == 0.f || noise != nullptr, AVD_EINVAL, "ddim_step: eta > 0 needs a noise tensor");
    const int64_t total = (int64_t)B * per;
    hipLaunchKernelGGL(ddim_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x_t, eps, t_now, t_prev,
                       abar, T_train, eta, noise, x_prev, per, total);
    AVD_CHECK_LAUNCH("ddim_step");
    return AVD_OK;
}

// true when [a, a + n) and [b, b + n) overlap (n floats each)
bool overlaps(const float* a, const float* b, int64_t n) { return a < b + n && b < a + n; }

__global__ __launch_bounds__(256) void dpmpp_2m_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                       float* __restrict__ x0_hist, const int64_t* __restrict__ t_last,
                                                       const int64_t* __restrict__ t_now, const int64_t* __restrict__ t_prev,
                                                       const float* __restrict__ abar, int T_train, float* __restrict__ out,
                                                       int64_t per, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / per);
    const Ddim c = ddim_coef(t_now, t_prev, abar, T_train, 0.f, b);
    const Dpm d = dpm_coef(t_last, t_now, t_prev, abar, T_train, 0.f, b);
    const float x0 = ddim_x0(c, x[i], eps[i]);
    out[i] = dpm_apply(d, x[i], x0, d.c_1 != 0.f ? x0_hist[i] : 0.f, 0.f, false);
    x0_hist[i] = x0;
}

// the SDE form on explicit noise (read at eta > 0 only); at eta == 0 the arithmetic of dpmpp_2m_kernel
__global__ __launch_bounds__(256) void dpmpp_2m_sde_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                           float* __restrict__ x0_hist, const int64_t* __restrict__ t_last,
                                                           const int64_t* __restrict__ t_now, const int64_t* __restrict__ t_prev,
                                                           const float* __restrict__ abar, int T_train, float eta,
                                                           const float* __restrict__ noise, float* __restrict__ out, int64_t per,
                                                           int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / per);
    const Ddim c = ddim_coef(t_now, t_prev, abar, T_train, 0.f, b);
    const Dpm d = dpm_coef(t_last, t_now, t_prev, abar, T_train, eta, b);
    const float x0 = ddim_x0(c, x[i], eps[i]);
    const bool noisy = eta > 0.f;
    out[i] = dpm_apply(d, x[i], x0, d.c_1 != 0.f ? x0_hist[i] : 0.f, noisy ? noise[i] : 0.f, noisy);
    x0_hist[i] = x0;
}

int dpmpp_2m_step_f32(const float* x_t, const float* eps, float* x0_hist, const int64_t* t_last, const int64_t* t_now,
                      const int64_t* t_prev, const float* abar, int T_train, float* x_out, int B, int64_t per, hipStream_t st) {
    AVD_REQUIRE(x_t && eps && x0_hist && t_last && t_now && t_prev && abar && x_out, AVD_EINVAL, "dpmpp_2m_step: null pointer");
    AVD_REQUIRE(B > 0 && per > 0 && T_train > 0, AVD_EINVAL, "dpmpp_2m_step: bad dims");
    const int64_t total = (int64_t)B * per;
    AVD_REQUIRE(!overlaps(x0_hist, x_t, total) && !overlaps(x0_hist, eps, total) && !overlaps(x0_hist, x_out, total), AVD_EINVAL,
                "dpmpp_2m_step: x0_hist must not overlap x_t, eps_hat or x_out");
    AVD_REQUIRE((total + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "dpmpp_2m_step: %lld values is too many for one launch",
                (long long)total);
    hipLaunchKernelGGL(dpmpp_2m_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x_t, eps, x0_hist, t_last, t_now,
                       t_prev, abar, T_train, x_out, per, total);
    AVD_CHECK_LAUNCH("dpmpp_2m_step");
    return AVD_OK;
}

int dpmpp_2m_sde_step_f32(const float* x_t, const float* eps, float* x0_hist, const int64_t* t_last, const int64_t* t_now,
                          const int64_t* t_prev, const float* abar, int T_train, float eta, const float* noise, float* x_out, int B,
                          int64_t per, hipStream_t st) {
    AVD_REQUIRE(x_t && eps && x0_hist && t_last && t_now && t_prev && abar && x_out, AVD_EINVAL, "dpmpp_2m_sde_step: null pointer");
    AVD_REQUIRE(B > 0 && per > 0 && T_train > 0, AVD_EINVAL, "dpmpp_2m_sde_step: bad dims");
    AVD_REQUIRE(eta >= 0.f, AVD_EINVAL, "dpmpp_2m_sde_step: eta must be >= 0");
    AVD_REQUIRE(eta == 0.f || noise != nullptr, AVD_EINVAL, "dpmpp_2m_sde_step: eta > 0 needs a noise tensor");
    const int64_t total = (int64_t)B * per;
    AVD_REQUIRE(!overlaps(x0_hist, x_t, total) && !overlaps(x0_hist, eps, total) && !overlaps(x0_hist, x_out, total), AVD_EINVAL,
                "dpmpp_2m_sde_step: x0_hist must not overlap x_t, eps_hat or x_out");
    AVD_REQUIRE(eta == 0.f || (!overlaps(noise, x0_hist, total) && !overlaps(noise, x_out, total)), AVD_EINVAL,
                "dpmpp_2m_sde_step: noise must not overlap x0_hist or x_out");
    AVD_REQUIRE((total + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "dpmpp_2m_sde_step: %lld values is too many for one launch",
                (long long)total);
    hipLaunchKernelGGL(dpmpp_2m_sde_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x_t, eps, x0_hist, t_last, t_now,
                       t_prev, abar, T_train, eta, noise, x_out, per, total);
    AVD_CHECK_LAUNCH("dpmpp_2m_sde_step");
    return AVD_OK;
}

// ------------------------------------------------------------------ latent guide (inpainting / SDEdit)
// The contract is written out in include/avdiff_hip.h (avd_latent_guide).  Per sample b and element e of the latent's natural layout:
//   q(tau) = A x_k + S n_k  (A = sqrt(a(tau)), S = sqrt(max(1 - a, 0)); q = x_k when a == 1),  n_k = philox_normal4 at counter
//   (e >> 2, s, 0, GUIDE_TAG): one fixed normal per element for the whole trajectory;
//   blend(m, q, z) = z (m == 0), q (m == 1), (1 - m) z + m q otherwise.
// guide_q / guide_blend are the only places these are written: the elementwise kernel and the three fused CFG kernels call them,
// without contraction, so every form agrees bit for bit (the lesson of ddim_apply above).
constexpr uint32_t GUIDE_TAG = 0x4B4E5731u;     // "KNW1"

struct GuideState {
    const float* known;     // [B, per]
    const float* mask;      // [per] (mask_bstride 0) or [B, per]; nullptr = 1 everywhere
    int64_t mask_bstride;
    NoiseKey nk;            // the known-noise stream's seed and sample offset
};

struct GuideCoef {
    float A, S;
    bool one;               // a == 1.0f: q = x_k, no arithmetic (and no generator call)
};

__device__ __forceinline__ GuideCoef guide_coef(const float* abar, int T_train, long long tau) {
    const float a = dpm_abar(abar, T_train, tau);
    return GuideCoef{sqrtf(a), sqrtf(fmaxf(1.0f - a, 0.f)), a == 1.0f};
}
__device__ __forceinline__ float guide_q(const GuideCoef& g, float xk, float n) {
#pragma clang fp contract(off)
    return g.one ? xk : g.A * xk + g.S * n;
}
__device__ __forceinline__ float guide_blend(float m, float q, float z) {
#pragma clang fp contract(off)
    return m == 0.f ? z : (m == 1.f ? q : (1.0f - m) * z + m * q);
}
// A lane of V values (4 or 1) rides in an f32x4 (load_v / store_v); a one-value lane keeps of a generator call the normal its element
// e takes
template <int V> __device__ __forceinline__ f32x4 lane_pick(f32x4 n, int64_t e) {
    if constexpr (V == 1) n[0] = n[(int)(e & 3)];
    return n;
}
// the V consecutive elements el .. el + V - 1 (V == 4: el % 4 == 0) of sample b at lat = b * per + el
template <int V>
__device__ __forceinline__ f32x4 guide_apply(const GuideState& gs, const GuideCoef& gc, int b, int64_t lat, int64_t el, f32x4 z) {
    const f32x4 m = gs.mask ? load_v<V>(gs.mask + b * gs.mask_bstride + el) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 xk = load_v<V>(gs.known + lat);
    f32x4 n = {0.f, 0.f, 0.f, 0.f};
    if (!gc.one) n = lane_pick<V>(philox_normal4(gs.nk, (uint32_t)(el >> 2), gs.nk.s0 + (uint32_t)b, 0u, GUIDE_TAG), el);
#pragma unroll
    for (int k = 0; k < V; ++k) z[k] = guide_blend(m[k], guide_q(gc, xk[k], n[k]), z[k]);
    return z;
}

// The canvas keying of the guide (include/avdiff_hip.h, "canvas-keyed known noise"): the batch is N consecutive windows of one canvas
// and n_k of element (o, l, i) of window b is the per-sample guide stream's value for sample p = (w0 + b) * hop + l, element
// e' = o * inner + i — canvas_normal4 with GUIDE_TAG and no timestep.  q and the blend are guide_q / guide_blend, as above.
struct CanvasGuideState {
    const float* known;     // [N, outer, L, inner]
    const float* mask;      // one window's (mask_bstride 0) or the batch's; nullptr = 1 everywhere
    int64_t mask_bstride;
    CanvasKey ck;           // the known-noise stream's seed, the global index of window 0 (guide.key.sample_offset) and the hop
};
// the V consecutive elements at lat = b * per + el, elements i .. i + V - 1 of the (o, l) slice (V == 4: inner % 4 == 0, i % 4 == 0)
template <int V>
__device__ __forceinline__ f32x4 canvas_guide_apply(const CanvasGuideState& gs, const GuideCoef& gc, int b, int64_t lat, int64_t el,
                                                    int64_t o, int l, int64_t i, int64_t inner, f32x4 z) {
    const f32x4 m = gs.mask ? load_v<V>(gs.mask + b * gs.mask_bstride + el) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 xk = load_v<V>(gs.known + lat);
    f32x4 n = {0.f, 0.f, 0.f, 0.f};
    if (!gc.one) n = lane_pick<V>(canvas_normal4(gs.ck, b, o, l, i, inner, 0u, GUIDE_TAG), o * inner + i);
#pragma unroll
    for (int k = 0; k < V; ++k) z[k] = guide_blend(m[k], guide_q(gc, xk[k], n[k]), z[k]);
    return z;
}

// The clip keying of the guide (include/avdiff_hip.h, "clip-keyed latent guide"): known / mask are canvases [outer, P, inner] of the
// whole clip, and element (o, l, i) of sample b sits on clip position p = (first + max(*cursor, 0) + b * stride) * slot_len + l, signed
// and unwrapped.  Outside [0, P) the element is unguided and nothing is read; inside, x_k and m are gathered at (o, p, i) and n_k is
// canvas_normal4's value for canvas position p (GUIDE_TAG, no timestep).  q and the blend are guide_q / guide_blend, as above.
struct ClipGuideState {
    const float* known;       // [outer, P, inner]
    const float* mask;        // [outer, P, inner]; nullptr = 1 everywhere
    int64_t P;
    uint32_t k0, k1;          // seed & 0xffffffff, seed >> 32
    int64_t first;            // as SlotKey
    int32_t stride, slot_len;
    const int32_t* cursor;    // device int32 or null: it selects the position, which is compared with [0, P) before it addresses
    int vec;                  // inner % 4 == 0 and known / mask 16-byte aligned: the canvases are read as f32x4
};
__device__ __forceinline__ int64_t clip_guide_pos(const ClipGuideState& cg, int b, int l) {
    int64_t m = cg.cursor ? *cg.cursor : 0;
    if (m < 0) m = 0;
    return (cg.first + m + (int64_t)b * cg.stride) * cg.slot_len + l;      // the host bounds every term: no overflow
}
template <int V> __device__ __forceinline__ f32x4 clip_canvas(const float* c, int64_t at, bool vec) {
    if (V == 1 || vec) return load_v<V>(c + at);
    return f32x4{c[at], c[at + 1], c[at + 2], c[at + 3]};
}
// elements i .. i + V - 1 of the (o, l) slice (V == 4: inner % 4 == 0, i % 4 == 0); a lane whose mask values are all 0 skips the
// generator: the blend would not read q
template <int V>
__device__ __forceinline__ f32x4 clip_guide_apply(const ClipGuideState& cg, const GuideCoef& gc, int b, int64_t o, int l, int64_t i,
                                                  int64_t inner, f32x4 z) {
    const int64_t p = clip_guide_pos(cg, b, l);
    if (p < 0 || p >= cg.P) return z;
    const int64_t at = (o * cg.P + p) * inner + i;
    f32x4 m = {1.f, 1.f, 1.f, 1.f};
    if constexpr (V == 4) {
        if (cg.mask) {
            m = clip_canvas<V>(cg.mask, at, cg.vec);
            if (m[0] == 0.f && m[1] == 0.f && m[2] == 0.f && m[3] == 0.f) return z;
        }
    } else {
        if (cg.mask) m = clip_canvas<V>(cg.mask, at, cg.vec);
        if (m[0] == 0.f) return z;
    }
    f32x4 xk = {0.f, 0.f, 0.f, 0.f};
    if constexpr (V == 4) xk = clip_canvas<V>(cg.known, at, cg.vec);
    f32x4 n = {0.f, 0.f, 0.f, 0.f};
    if (!gc.one)
        n = lane_pick<V>(philox_normal4(NoiseKey{cg.k0, cg.k1, 0u}, (uint32_t)((o * inner + i) >> 2), (uint32_t)p, 0u, GUIDE_TAG), o * inner + i);
    if constexpr (V == 1) xk = clip_canvas<V>(cg.known, at, cg.vec);
#pragma unroll
    for (int k = 0; k < V; ++k) z[k] = guide_blend(m[k], guide_q(gc, xk[k], n[k]), z[k]);
    return z;
}
// queue k's guide ("clip batch keying"): canvas k of known / mask and the known-noise stream under guide_seeds[k].  The canvas stride is
// a multiple of 4 floats wherever vec is set, so canvas k is as aligned as canvas 0
__device__ __forceinline__ ClipGuideState queue_clip_guide(const ClipQueues& q, ClipGuideState cg, int k) {
    const uint64_t seed = q.guide_seeds[k];
    cg.k0 = (uint32_t)(seed & 0xffffffffu);
    cg.k1 = (uint32_t)(seed >> 32);
    cg.known += (int64_t)k * q.canvas;
    if (cg.mask) cg.mask += (int64_t)k * q.canvas;
    return cg;
}
// as lane_slot_key: the ClipGuideState a lane of the fused kernels blends with
template <class... Key> __device__ __forceinline__ ClipGuideState lane_clip_guide(const QueueOf& qo, const Key&... nk) {
    if constexpr (PackHas<ClipQueues, Key...>::value) return queue_clip_guide(pack_get<ClipQueues>(nk...), pack_get<ClipGuideState>(nk...), qo.k);
    else return pack_get<ClipGuideState>(nk...);
}

// the clip guide's checks, all before any HIP call (the list is in the header); outs: buffers known / mask must not overlap, each of
// B * outer * L * inner floats, nullptr skipped.  K > 1 ("clip batch keying"): known / mask hold K canvases, walked by B / K samples each
int make_clip_guide(const avd_clip_guide* g, int B, int64_t outer, int L, int slots, int slot_len, int64_t inner,
                    std::initializer_list<const float*> outs, ClipGuideState& cg, const char* what = "clip_guide", int K = 1) {
    AVD_REQUIRE(g, AVD_EINVAL, "%s: null clip guide", what);
    AVD_REQUIRE(g->known, AVD_EINVAL, "%s: null known canvas", what);
    if (int rc = check_keyed_dims(what, "B", B, outer, "L", L, inner)) return rc;
    AVD_REQUIRE(g->P >= 1 && g->P <= (int64_t)1 << 32, AVD_EINVAL, "%s: the clip guide's P %lld must lie in [1, 2^32]", what, (long long)g->P);
    if (int rc = check_clip_origin(what, "clip guide", g->stride, g->first)) return rc;
    if (int rc = check_slots(what, B, L, slots, slot_len)) return rc;
    // every term of the position: |first| < 2^32, the cursor < 2^31, B * stride < 2^62, so the slot index stays below 2^62.1 only
    // when B * stride does; times slot_len plus l it must stay inside int64
    AVD_REQUIRE(K >= 1 && B % K == 0, AVD_EINVAL, "%s: the %d queues must divide the batch %d", what, K, B);
    AVD_REQUIRE(((double)(B / K) * g->stride + 8.6e9) * (double)slot_len + (double)L < 9.0e18, AVD_EINVAL,
                "%s: B %d * stride %d * slot_len %d leaves the signed 64-bit positions", what, B / K, g->stride, slot_len);
    AVD_REQUIRE((double)K * (double)outer * (double)g->P * (double)inner < 9.0e18 &&
                    (double)B * (double)outer * (double)L * (double)inner < 9.0e18,
                AVD_EUNSUPPORTED, "%s: too many values", what);
    const int64_t nc = K * outer * g->P * inner, n = (int64_t)B * outer * L * inner;
    for (const float* p : outs) {
        if (!p) continue;
        AVD_REQUIRE(!(p < g->known + nc && g->known < p + n) && !(g->mask && p < g->mask + nc && g->mask < p + n), AVD_EINVAL,
                    "%s: known / mask must not overlap out, z_out or x0_hist", what);
    }
    cg = ClipGuideState{g->known, g->mask, g->P, (uint32_t)(g->seed & 0xffffffffu), (uint32_t)(g->seed >> 32), g->first, g->stride,
                        slot_len, g->cursor, inner % 4 == 0 && aligned16(g->known) && aligned16(g->mask) ? 1 : 0};
    return AVD_OK;
}

int check_clip_guide(const avd_clip_guide* g, int B, int64_t outer, int L, int slots, int slot_len, int64_t inner, const float* out,
                     const float* x0_hist, int K = 1) {
    ClipGuideState cg;
    return make_clip_guide(g, B, outer, L, slots, slot_len, inner, {out, x0_hist}, cg, "clip_guide", K);
}
// the descriptor's checks for the whole step, before the model runs: g (null: no guide) has passed check_clip_guide with cq->K;
// step: the update reads the step seeds (eta > 0)
int check_clip_queues(const avd_clip_queues* cq, const avd_clip_guide* g, bool step, int B, int64_t outer, int L, int64_t inner,
                      const float* out, const float* x0_hist) {
    ClipQueues q;
    const int64_t canvas = g ? outer * g->P * inner : 0;
    return make_clip_queues("clip_queues", cq, B, step, g != nullptr, {out, x0_hist}, (int64_t)B * outer * L * inner, g ? g->known : nullptr,
                            g ? g->mask : nullptr, (cq ? cq->K : 0) * canvas, canvas, q);
}

// The stand-alone pass (avd_clip_guide_slots_f32): out = blend(m(p), q_p(tau[b, s]), z) per slot.  A block lies inside one slot of one
// (b, o) row — bpr blocks cover the longest row, the last slot's with the uncovered tail — so the slot's tau is block-uniform, and a
// block whose slot is left (AVD_SLOT_LEAVE) returns before it loads anything when the call is in place, and copies z otherwise.
// V lanes as fifo_move_kernel.  Q: empty, or one ClipQueues ("clip batch keying"): b is block-uniform, so the queue's guide is resolved
// once per block, behind the left block's return, and the positions walk by the sample's index inside its queue.
template <int V, class... Q>
__global__ __launch_bounds__(256) void clip_guide_slots_kernel(ClipGuideState cg, const int64_t* __restrict__ tau,
                                                               const float* __restrict__ abar, int T_train, const float* z, float* out,
                                                               int64_t outer, int L, int S, int64_t inner, int bpr, Q... q) {      // z may be out
    static_assert(sizeof...(Q) == (PackHas<ClipQueues, Q...>::value ? 1 : 0), "the pack: optionally one ClipQueues");
    int64_t r = blockIdx.x;
    const int chunk = (int)(r % bpr);
    r /= bpr;
    const int s = (int)(r % S);
    r /= S;
    const int64_t o = r % outer;
    const int b = (int)(r / outer);
    const int64_t t = tau[(int64_t)b * S + s];
    const bool leave = t == INT64_MIN;
    if (leave && out == z) return;
    [[maybe_unused]] int bq = b;      // the sample index the positions walk by
    if constexpr (sizeof...(Q) > 0) {
        const QueueOf qo = queue_of(q..., b);
        cg = queue_clip_guide(q..., cg, qo.k);
        bq = qo.b;
    }
    const int l0 = s * cg.slot_len;
    const int nl = s == S - 1 ? L - l0 : cg.slot_len;      // the uncovered tail follows the last slot
    const int64_t j = ((int64_t)chunk * 256 + threadIdx.x) * V;      // the lane's first element of the slot's [nl, inner] piece
    if (j >= (int64_t)nl * inner) return;
    const int l = l0 + (int)(j / inner);
    const int64_t i = j % inner;
    const int64_t at = (((int64_t)b * outer + o) * L + l) * inner + i;
    f32x4 v = load_v<V>(z + at);
    if (!leave) v = clip_guide_apply<V>(cg, guide_coef(abar, T_train, t), bq, o, l, i, inner, v);
    store_v<V>(out + at, v);
}

// The guided FIFO queue shift (avd_fifo_shift_guided_f32; contract in include/avdiff_hip.h, "clip-keyed latent guide"):
// fifo_move_kernel's GuideShift.  cg has first = c, stride unused and no cursor, so with sample 0 and position j clip_guide_pos gives
// p = c * slot_len + j, what the stand-alone pass computes for the tail slot; the coefficients, the gather and the blend are its own.
struct GuideShift {
    ClipGuideState cg;
    const float* abar;
    int T_train;
    template <int V> __device__ __forceinline__ f32x4 tail(int64_t o, int j, int64_t i, int64_t inner, uint32_t t, f32x4 v) const {
        return clip_guide_apply<V>(cg, guide_coef(abar, T_train, (long long)t), 0, o, j, i, inner, v);
    }
};

int fifo_shift_guided_f32(const avd_noise_key* key, int64_t t, int64_t c, const avd_clip_guide* guide, const float* abar, int T_train,
                          int everywhere, const float* z_in, float* z_out, float* popped, const float* hist_in, float* hist_out, int B,
                          int64_t outer, int S, int slot_len, int64_t inner, hipStream_t st) {
    const QueueMove d = fifo_shift_move(key, t, c, z_in, z_out, popped, B, outer, S, slot_len, inner, hist_in, hist_out, nullptr, 1, true);
    MovePlan plan;
    if (int rc = fifo_move_check(d, plan)) return rc;      // the shift's own checks first, then the guide's
    AVD_REQUIRE(guide, AVD_EINVAL, "fifo_shift_guided: null clip guide");
    AVD_REQUIRE(abar && T_train > 0, AVD_EINVAL, "fifo_shift_guided: null alpha_bar or bad T_train");
    avd_clip_guide g = *guide;      // c names the clip slot: first / stride / cursor are not read
    g.first = c;
    g.stride = 1;
    g.cursor = nullptr;
    GuideShift gs{ClipGuideState{}, abar, T_train};
    if (int rc = make_clip_guide(&g, B, outer, S * slot_len, S, slot_len, inner, {z_out, hist_out}, gs.cg, "fifo_shift_guided")) return rc;
    const int64_t nc = outer * g.P * inner, pop = outer * slot_len * inner;
    AVD_REQUIRE(!(popped < g.known + nc && g.known < popped + pop) && !(g.mask && popped < g.mask + nc && g.mask < popped + pop), AVD_EINVAL,
                "fifo_shift_guided: known / mask must not overlap popped");
    if (everywhere) gs.cg.mask = nullptr;      // the mask reads as 1 on every in-canvas position
    gs.cg.vec = inner % 4 == 0 && aligned16(gs.cg.known) && aligned16(gs.cg.mask);
    return fifo_move_launch(d, plan, st, gs);
}

// the checks every guided entry makes before any HIP call; out and x0_hist (either may be nullptr) must not overlap known / mask
int check_latent_guide(const avd_latent_guide* g, int B, int64_t per, const float* out, const float* x0_hist) {
    AVD_REQUIRE(g, AVD_EINVAL, "latent_guide: null guide");
    AVD_REQUIRE(g->known, AVD_EINVAL, "latent_guide: null known latent");
    AVD_REQUIRE(B > 0 && per > 0 && per < ((int64_t)1 << 34), AVD_EINVAL, "latent_guide: bad dims (B %d, per_sample %lld)", B,
                (long long)per);
    AVD_REQUIRE(g->mask_batch_stride == 0 || g->mask_batch_stride == per, AVD_EINVAL,
                "latent_guide: mask_batch_stride %lld must be 0 or per_sample %lld", (long long)g->mask_batch_stride, (long long)per);
    AVD_REQUIRE(g->key.sample_offset >= 0 && g->key.sample_offset + (int64_t)B <= ((int64_t)1 << 32), AVD_EINVAL,
                "latent_guide: key sample_offset %lld + B %d must lie in [0, 2^32]", (long long)g->key.sample_offset, B);
    AVD_REQUIRE(aligned16(g->known) && (!g->mask || aligned16(g->mask)), AVD_EUNSUPPORTED,
                "latent_guide: known and mask must be 16-byte aligned");
    const int64_t n = (int64_t)B * per, nm = g->mask_batch_stride ? n : per;
    for (const float* p : {out, x0_hist}) {
        if (!p) continue;
        AVD_REQUIRE(!overlaps(p, g->known, n) && !(g->mask && (p < g->mask + nm && g->mask < p + n)), AVD_EINVAL,
                    "latent_guide: known / mask must not overlap z_out or x0_hist");
    }
    return AVD_OK;
}

static int make_guide(const avd_latent_guide* g, int B, int64_t per, const float* out, const float* x0_hist, GuideState& gs) {
    if (int rc = check_latent_guide(g, B, per, out, x0_hist)) return rc;
    NoiseKey nk;
    if (int rc = make_noise_key(&g->key, B, nk)) return rc;
    gs = GuideState{g->known, g->mask, g->mask_batch_stride, nk};
    return AVD_OK;
}

// the canvas-keyed guide's checks, all before any HIP call: the canvas limits on the guide's key (hop >= 1, every canvas position of
// the batch below 2^32, one position's slice below 2^34 elements), then check_latent_guide's
static int make_canvas_guide(const avd_latent_guide* g, int N, int64_t outer, int L, int hop, int64_t inner, const float* out,
                             const float* x0_hist, CanvasGuideState& gs) {
    AVD_REQUIRE(g, AVD_EINVAL, "latent_guide: null guide");
    CanvasKey ck;
    if (int rc = make_canvas_key(&g->key, N, outer, L, hop, inner, ck, "canvas guide")) return rc;
    AVD_REQUIRE((double)outer * (double)L * (double)inner < 17179869184.0, AVD_EINVAL,
                "canvas guide: a window of outer %lld * L %d * inner %lld values must hold < 2^34", (long long)outer, L, (long long)inner);
    if (int rc = check_latent_guide(g, N, outer * L * inner, out, x0_hist)) return rc;
    gs = CanvasGuideState{g->known, g->mask, g->mask_batch_stride, ck};
    return AVD_OK;
}

int check_canvas_guide(const avd_latent_guide* g, int N, int64_t outer, int L, int hop, int64_t inner, const float* out,
                       const float* x0_hist) {
    CanvasGuideState gs;
    return make_canvas_guide(g, N, outer, L, hop, inner, out, x0_hist, gs);
}

// ------------------------------------------------------------------ renoise (RePaint resampling: the forward jump t_from -> t_to)
// The contract is written out in include/avdiff_hip.h ("renoise").  Per sample b, with a_f = a(t_from[b]) and a_t = a(t_to[b]):
//   !(a_t < a_f): out = z, no arithmetic and no generator call;  else rho = a_t / a_f, out = sqrt(rho) z + sqrt(max(1 - rho, 0)) n_r,
//   n_r = philox_normal4 at counter (e >> 2, s, visit, RENOISE_TAG) — or its canvas keying (the StreamMap's) — fresh per visit;
//   with a guide the launch ends in blend(mask, q(t_to[b]), out): guide_coef / guide_q / guide_blend, as every guided kernel.
constexpr uint32_t RENOISE_TAG = 0x52504E31u;   // "RPN1"

struct RenoiseCoef {
    float A, S;
    bool same;              // !(a_t < a_f): out = z
};

__device__ __forceinline__ RenoiseCoef renoise_coef(const float* abar, int T_train, long long t_from, long long t_to) {
#pragma clang fp contract(off)
    const float af = dpm_abar(abar, T_train, t_from), at = dpm_abar(abar, T_train, t_to);
    if (!(at < af)) return RenoiseCoef{1.f, 0.f, true};
    const float rho = at / af;
    return RenoiseCoef{sqrtf(rho), sqrtf(fmaxf(1.0f - rho, 0.f)), false};
}
__device__ __forceinline__ float renoise_apply(const RenoiseCoef& c, float z, float n) {
#pragma clang fp contract(off)
    return c.same ? z : c.A * z + c.S * n;
}

// ------------------------------------------------------------------ the stream's stand-alone passes
// The eight elementwise entries of the stream (avd_gaussian_noise_f32, avd_canvas_noise_f32, avd_slot_noise_f32, avd_latent_guide_f32 /
// _canvas_f32, avd_renoise_f32 / _canvas_f32, avd_clip_guide_slots_f32; contracts in include/avdiff_hip.h) are one descriptor, one check
// function and one launch function.  All but the last run on one lane loop over [B, outer, L, inner] with a StreamMap per stream; the
// per-sample entries are the batch [B, 1, 1, per] under stream_map(NoiseKey).  A lane takes one of three forms:
//   Float4    inner % 4 == 0 and every base 16-byte aligned: the lane's float4 lies inside one (o, l) slice, one Philox call per four;
//   Guarded4  four elements of one slice by scalar access, the slice's last lane fewer: where inner % 4 == 0 but a base is unaligned,
//             and where outer == 1 (so e' = i and a lane's four elements share a call whatever inner is);
//   One       one Philox call per element: everything else, which is every audio latent (inner == 1).
enum class Lanes { One, Guarded4, Float4 };
template <Lanes F> constexpr int lane_width = F == Lanes::One ? 1 : 4;

// n: the lane's elements (lane_width, or fewer on a Guarded4 tail)
template <Lanes F> __device__ __forceinline__ f32x4 lane_load(const float* p, int n) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (F == Lanes::Float4) v = *reinterpret_cast<const f32x4*>(p);
    else
#pragma unroll
        for (int k = 0; k < lane_width<F>; ++k)
            if (k < n) v[k] = p[k];
    return v;
}
template <Lanes F> __device__ __forceinline__ void lane_store(float* p, f32x4 v, int n) {
    if constexpr (F == Lanes::Float4) *reinterpret_cast<f32x4*>(p) = v;
    else
#pragma unroll
        for (int k = 0; k < lane_width<F>; ++k)
            if (k < n) p[k] = v[k];
}

struct PassDims {
    int64_t outer, inner, per;      // per = outer * L * inner
    int L, S, slot_len;             // the time tables are [B, S], position l in slot min(l / slot_len, S - 1)
};
struct PassLane {
    int b, l, n;                    // n: as lane_load
    int64_t o, i, at;               // at: the element offset of (b, o, l, i)
};
// the lane's four normals in element order; a One lane keeps the one its element takes
template <Lanes F>
__device__ __forceinline__ f32x4 lane_normal4(const StreamMap& m, const PassDims& d, const PassLane& ln, uint32_t t, uint32_t tag) {
    f32x4 v = stream_normal4(m, ln.b, ln.o, ln.l, ln.i, d.inner, t, tag);
    if constexpr (F == Lanes::One) v[0] = v[(int)((ln.o * d.inner + ln.i) & 3)];
    return v;
}

// the draw: out = n at the time word of the position's slot
struct DrawBody {
    const int64_t* t_now;           // [B, S]
    float* out;
    StreamMap map;
    uint32_t tag;
    template <Lanes F, bool> __device__ __forceinline__ void lane(const PassDims& d, const PassLane& ln) const { draw<F>(d, ln, map, ln.b); }
    // m, bm: the stream and the sample index the position walks by (the lane's own, or its queue's); the time word is the sample's
    template <Lanes F> __device__ __forceinline__ void draw(const PassDims& d, const PassLane& ln, const StreamMap& m, int bm) const {
        int s = 0;
        if (d.S > 1) {
            s = ln.l / d.slot_len;
            if (s > d.S - 1) s = d.S - 1;
        }
        PassLane lm = ln;
        lm.b = bm;
        lane_store<F>(out + ln.at, lane_normal4<F>(m, d, lm, (uint32_t)t_now[(int64_t)ln.b * d.S + s], tag), ln.n);
    }
};
// the draw of a clip batch ("clip batch keying"): queue k's seed in the map, the sample's index inside its queue in b's place
struct QueueDrawBody {
    DrawBody d;
    ClipQueues q;
    template <Lanes F, bool> __device__ __forceinline__ void lane(const PassDims& pd, const PassLane& ln) const {
        const QueueOf qo = queue_of(q, ln.b);
        d.template draw<F>(pd, ln, queue_stream_map(q, d.map, qo.k), qo.b);
    }
};

// the blend: v = renoise_apply(renoise_coef(t_from, t_to), z, n_r), then under a guide (known != nullptr) blend(m, q(t_to), v).  The
// latent guide is the jump t_from == t_to, where renoise_coef gives `same`, v = z and nothing is drawn: RENOISE false says so at
// compile time, which keeps the guide's launches at their cost (profiles/stream_pass_kernels.txt).  z == nullptr (the guide's pure
// forward noising) arrives with mask == nullptr: v = 0 and blend(1, q, .) selects q.  z may be out (in place).
struct BlendBody {
    const int64_t *t_from, *t_to;   // [B]; RENOISE false: t_to alone, the guide's tau
    const float* abar;
    int T_train;
    const float* z;
    float* out;
    StreamMap rmap;                 // the renoise stream
    uint32_t visit;
    const float *known, *mask;      // mask: [per] (mask_bstride 0) or the batch's; nullptr = 1 everywhere
    int64_t mask_bstride;
    StreamMap gmap;                 // the guide's known noise
    template <Lanes F, bool RENOISE> __device__ __forceinline__ void lane(const PassDims& d, const PassLane& ln) const {
        f32x4 v = z ? lane_load<F>(z + ln.at, ln.n) : f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (RENOISE) {
            const RenoiseCoef rc = renoise_coef(abar, T_train, t_from[ln.b], t_to[ln.b]);
            f32x4 nr = {0.f, 0.f, 0.f, 0.f};
            if (!rc.same) nr = lane_normal4<F>(rmap, d, ln, visit, RENOISE_TAG);
#pragma unroll
            for (int k = 0; k < lane_width<F>; ++k) v[k] = renoise_apply(rc, v[k], nr[k]);
        }
        if (known) {
            const GuideCoef gc = guide_coef(abar, T_train, t_to[ln.b]);
            f32x4 nk = {0.f, 0.f, 0.f, 0.f}, m = {1.f, 1.f, 1.f, 1.f};
            if (!gc.one) nk = lane_normal4<F>(gmap, d, ln, 0u, GUIDE_TAG);
            if (mask) m = lane_load<F>(mask + ln.b * mask_bstride + (ln.at - ln.b * d.per), ln.n);
            const f32x4 xk = lane_load<F>(known + ln.at, ln.n);
#pragma unroll
            for (int k = 0; k < lane_width<F>; ++k) v[k] = guide_blend(m[k], guide_q(gc, xk[k], nk[k]), v[k]);
        }
        lane_store<F>(out + ln.at, v, ln.n);
    }
};

// The lane loop: lane idx -> (b, o, l, i) of [B, outer, L, ceil(inner / width)], queue_lane's arithmetic (32-bit below 2^32 lanes).
// n: the launch's lanes.  RENOISE: the blend's renoise half (false: the guide alone).
template <Lanes F, class Body, bool RENOISE = true>
__global__ __launch_bounds__(256) void stream_pass_kernel(Body body, PassDims d, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    constexpr int V = lane_width<F>;
    const int64_t iv = (d.inner + V - 1) / V;
    const bool narrow = n <= 0xffffffffll;
    const QueueLane q = narrow ? queue_lane<uint32_t, V>((uint32_t)idx, (uint32_t)iv, (uint32_t)d.L, (uint32_t)d.outer)
                               : queue_lane<int64_t, V>(idx, iv, (int64_t)d.L, d.outer);
    PassLane ln{q.b, q.l, V, q.o, q.i, idx * V};
    if constexpr (F == Lanes::Guarded4) {
        const int64_t slice = narrow ? (int64_t)((uint32_t)idx / (uint32_t)iv) : idx / iv;
        ln.at = slice * d.inner + q.i;
        if (d.inner - q.i < 4) ln.n = (int)(d.inner - q.i);
    }
    body.template lane<F, RENOISE>(d, ln);
}

// What an entry asks of stream_pass.  Every check is made in stream_pass_check, before any HIP call.
enum class Keying { Sample, Canvas, Clip };
enum class Pass { Draw, Guide, Renoise, ClipSlots };      // Guide and Renoise are the blend, without and with a stream of its own
struct StreamPass {
    const char *what, *key_what;      // the entry's prefix in messages; its keying's (make_canvas_key, make_slot_key)
    const char* label;                // the profile label, which names the entry's form; label_lanes: "<4>" (Float4) or "<1>" follows
    bool label_lanes;
    Keying keying;
    Pass kind;
    int B, L;                         // the batch [B, outer, L, inner]; the per-sample entries are [B, 1, 1, per]
    int64_t outer, inner;
    int hop, slots, slot_len;         // Canvas: hop.  Clip: the [B, slots] tables
    const void* key;                  // Draw, Renoise: the pass's own stream, an avd_noise_key or (Clip) an avd_slot_key
    uint32_t word;                    // Draw: the domain word.  Renoise: the visit
    const void* guide;                // an avd_latent_guide (Guide; Renoise: or null) or (ClipSlots) an avd_clip_guide
    int everywhere, T_train;
    const int64_t *t_from, *t_to;     // the draw's t_now is t_to; a guide's tau is both
    const float *abar, *z;            // z: may be null under Guide
    float* out;
    const avd_clip_queues* queues;    // Clip keying alone, or null: the batch is K queues ("clip batch keying")
};
// what the checks leave for the launch
struct PassPlan {
    PassDims d;
    DrawBody draw;
    BlendBody blend;
    ClipGuideState cg;
    bool queues;                      // cq rides along: the draw's QueueDrawBody, the clip guide's pack
    ClipQueues cq;
    Lanes lanes;
    int64_t n;                        // lanes; ClipSlots: blocks
    int bpr;
    double bytes;                     // what the entry tells the profile it moves
};

int stream_pass_check(const StreamPass& d, PassPlan& p) {
    const char* w = d.what;
    const bool draw = d.kind == Pass::Draw, clip = d.kind == Pass::ClipSlots;
    const bool keyed = draw || d.kind == Pass::Renoise;      // the pass draws a stream of its own
    const avd_latent_guide* g = clip ? nullptr : static_cast<const avd_latent_guide*>(d.guide);
    p = PassPlan{};
    StreamMap map{}, gmap{};
    const float *known = nullptr, *mask = nullptr;
    if (keyed && d.keying == Keying::Sample) {
        NoiseKey nk;
        if (int rc = make_noise_key(static_cast<const avd_noise_key*>(d.key), d.B, nk)) return rc;
        map = stream_map(nk);
    } else if (keyed && d.keying == Keying::Canvas) {
        CanvasKey ck;
        if (int rc = make_canvas_key(static_cast<const avd_noise_key*>(d.key), d.B, d.outer, d.L, d.hop, d.inner, ck, d.key_what)) return rc;
        AVD_REQUIRE(draw || (double)d.outer * (double)d.L * (double)d.inner < 17179869184.0, AVD_EINVAL,
                    "%s: a window of outer %lld * L %d * inner %lld values must hold < 2^34", d.key_what, (long long)d.outer, d.L,
                    (long long)d.inner);
        map = stream_map(ck);
    } else if (keyed) {
        SlotKey sk;
        if (int rc = make_slot_key(static_cast<const avd_slot_key*>(d.key), d.B, d.outer, d.slot_len, d.inner, sk, d.key_what)) return rc;
        map = stream_map(sk);
    }
    // the guide's checks come first in a pass of the guide alone, and behind the pass's own otherwise
    auto guide = [&]() -> int {
        if (clip)
            return make_clip_guide(static_cast<const avd_clip_guide*>(d.guide), d.B, d.outer, d.L, d.slots, d.slot_len, d.inner, {d.out}, p.cg, w,
                                   d.queues ? d.queues->K : 1);
        if (keyed && !g) return AVD_OK;
        if (d.keying == Keying::Sample) {
            if (int rc = check_latent_guide(g, d.B, d.inner, d.out, nullptr)) return rc;
            NoiseKey nk;
            if (int rc = make_noise_key(&g->key, d.B, nk)) return rc;
            gmap = stream_map(nk);
        } else {
            CanvasGuideState gs;
            if (int rc = make_canvas_guide(g, d.B, d.outer, d.L, d.hop, d.inner, d.out, nullptr, gs)) return rc;
            gmap = stream_map(gs.ck);
        }
        known = g->known;
        mask = d.z ? g->mask : nullptr;      // pure forward noising: the mask reads as 1 everywhere
        return AVD_OK;
    };
    if (!keyed)
        if (int rc = guide()) return rc;
    if (draw)
        AVD_REQUIRE(d.t_to && d.out, AVD_EINVAL, "%s: null pointer", w);
    else
        AVD_REQUIRE(d.t_from && d.t_to && d.abar && d.out && (d.z || d.kind == Pass::Guide) && d.T_train > 0, AVD_EINVAL,
                    "%s: null pointer or bad T_train", w);
    if (keyed && d.keying == Keying::Sample)
        AVD_REQUIRE(d.inner > 0 && d.inner < ((int64_t)1 << 34), AVD_EINVAL, "%s: per_sample %lld must be in [1, 2^34)", w, (long long)d.inner);
    if (draw && d.keying == Keying::Clip)
        if (int rc = check_slots(w, d.B, d.L, d.slots, d.slot_len)) return rc;
    AVD_REQUIRE((double)d.B * (double)d.outer * (double)d.L * (double)d.inner < 9.0e18, AVD_EUNSUPPORTED, "%s: too many values", w);
    const int64_t total = (int64_t)d.B * d.outer * d.L * d.inner;
    AVD_REQUIRE(draw || d.kind == Pass::Guide || d.out == d.z || !overlaps(d.out, d.z, total), AVD_EINVAL,
                "%s: out must be z or not overlap it", w);      // the guide entries' contract asks it of known / mask alone
    if (keyed)
        if (int rc = guide()) return rc;
    if (d.queues) {      // the entries that take a descriptor require it; the canvases as the guide holds them, before `everywhere`
        const int64_t canvas = clip ? d.outer * p.cg.P * d.inner : 0;
        if (int rc = make_clip_queues(w, d.queues, d.B, draw, clip, {d.out}, total, clip ? p.cg.known : nullptr, clip ? p.cg.mask : nullptr,
                                      d.queues->K * canvas, canvas, p.cq)) return rc;
        p.queues = true;
    }
    const bool tables = d.keying == Keying::Clip;
    p.d = PassDims{d.outer, d.inner, d.outer * d.L * d.inner, d.L, tables ? d.slots : 1, tables ? d.slot_len : 1};
    if (clip) {
        if (d.everywhere) p.cg.mask = nullptr;      // the mask reads as 1 on every in-canvas position
        p.cg.vec = d.inner % 4 == 0 && aligned16(p.cg.known) && aligned16(p.cg.mask);
        const bool vec = p.cg.vec && aligned16(d.z) && aligned16(d.out);
        p.lanes = vec ? Lanes::Float4 : Lanes::One;
        const int64_t row = (int64_t)(d.L - (d.slots - 1) * d.slot_len) * d.inner / (vec ? 4 : 1);      // lanes of the longest slot piece
        const int64_t bpr = (row + 255) / 256;
        p.n = (int64_t)d.B * d.outer * d.slots * bpr;
        AVD_REQUIRE(bpr <= 0x7fffffff && p.n <= 0x7fffffff, AVD_EUNSUPPORTED, "%s: %lld blocks are too many for one launch", w, (long long)p.n);
        p.bpr = (int)bpr;
        p.bytes = 4.0 * (double)total * 4;      // an upper bound: left slots move nothing
        return AVD_OK;
    }
    const bool aligned = aligned16(d.out) && aligned16(d.z) && aligned16(known) && aligned16(mask);
    p.lanes = d.inner % 4 == 0 ? (aligned ? Lanes::Float4 : Lanes::Guarded4) : (d.outer == 1 && d.inner > 1 ? Lanes::Guarded4 : Lanes::One);
    const int v = p.lanes == Lanes::One ? 1 : 4;
    p.n = total / d.inner * ((d.inner + v - 1) / v);
    AVD_REQUIRE((p.n + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "%s: %lld lanes are too many for one launch", w, (long long)p.n);
    p.draw = DrawBody{d.t_to, d.out, map, d.word};
    p.blend = BlendBody{d.t_from, d.t_to, d.abar, d.T_train, d.z, d.out, map, d.word, known, mask, known ? g->mask_batch_stride : 0, gmap};
    p.bytes = 4.0 * (double)total * (draw ? 1 : (keyed ? g != nullptr : d.z != nullptr) ? 4 : 2);
    return AVD_OK;
}

int stream_pass_launch(const StreamPass& d, const PassPlan& p, hipStream_t st) {
    const int v = p.lanes == Lanes::Float4 ? 4 : 1;
    ProfScope prof(g_prof_on ? (d.label_lanes ? prof_tag_id("%s<%d>", d.label, v) : prof_tag_id("%s", d.label)) : 0, p.bytes, st);
    const dim3 grid((unsigned)((p.n + 255) / 256));
    if (d.kind == Pass::ClipSlots)
        with_int<1, 4>(v, [&](auto V) {
            if (p.queues)
                hipLaunchKernelGGL((clip_guide_slots_kernel<decltype(V)::value, ClipQueues>), dim3((unsigned)p.n), dim3(256), 0, st, p.cg,
                                   d.t_to, d.abar, d.T_train, d.z, d.out, d.outer, d.L, d.slots, d.inner, p.bpr, p.cq);
            else
                hipLaunchKernelGGL(clip_guide_slots_kernel<decltype(V)::value>, dim3((unsigned)p.n), dim3(256), 0, st, p.cg, d.t_to, d.abar,
                                   d.T_train, d.z, d.out, d.outer, d.L, d.slots, d.inner, p.bpr);
        });
    else
        with_int<(int)Lanes::One, (int)Lanes::Guarded4, (int)Lanes::Float4>((int)p.lanes, [&](auto F) {
            constexpr Lanes f = (Lanes) decltype(F)::value;
            if (d.kind == Pass::Draw && p.queues)
                hipLaunchKernelGGL((stream_pass_kernel<f, QueueDrawBody>), grid, dim3(256), 0, st, QueueDrawBody{p.draw, p.cq}, p.d, p.n);
            else if (d.kind == Pass::Draw)
                hipLaunchKernelGGL((stream_pass_kernel<f, DrawBody>), grid, dim3(256), 0, st, p.draw, p.d, p.n);
            else if (d.kind == Pass::Renoise)
                hipLaunchKernelGGL((stream_pass_kernel<f, BlendBody>), grid, dim3(256), 0, st, p.blend, p.d, p.n);
            else
                hipLaunchKernelGGL((stream_pass_kernel<f, BlendBody, false>), grid, dim3(256), 0, st, p.blend, p.d, p.n);
        });
    AVD_CHECK_LAUNCH(d.what);
    return AVD_OK;
}

int stream_pass(const StreamPass& d, hipStream_t st) {
    PassPlan plan;
    if (int rc = stream_pass_check(d, plan)) return rc;
    return stream_pass_launch(d, plan, st);
}

int gaussian_noise_f32(const avd_noise_key* key, const int64_t* t_now, float* out, int B, int64_t per, hipStream_t st) {
    return stream_pass(StreamPass{"gaussian_noise", "", "gaussian_noise_kernel", false, Keying::Sample, Pass::Draw, B, 1, 1, per, 0, 0, 0, key,
                                  0x44444D31u, nullptr, 0, 0, nullptr, t_now, nullptr, nullptr, out}, st);
}
int canvas_noise_f32(const avd_noise_key* key, const int64_t* t_now, float* out, int N, int64_t outer, int L, int hop, int64_t inner,
                     hipStream_t st) {
    return stream_pass(StreamPass{"canvas_noise", "canvas noise", "canvas_noise_kernel", true, Keying::Canvas, Pass::Draw, N, L, outer, inner,
                                  hop, 0, 0, key, 0x44444D31u, nullptr, 0, 0, nullptr, t_now, nullptr, nullptr, out}, st);
}
// cq != nullptr: the batch is K queues ("clip batch keying"), the entry avd_slot_noise_clips_f32
int slot_noise_f32(const avd_slot_key* key, const int64_t* t_now, float* out, int B, int64_t outer, int L, int slots, int slot_len,
                   int64_t inner, hipStream_t st, const avd_clip_queues* cq = nullptr) {
    return stream_pass(StreamPass{cq ? "slot_noise_clips" : "slot_noise", "slot noise", cq ? "slot_noise_clips_kernel" : "slot_noise_kernel",
                                  true, Keying::Clip, Pass::Draw, B, L, outer, inner, 0, slots, slot_len, key, SLOT_TAG, nullptr, 0, 0,
                                  nullptr, t_now, nullptr, nullptr, out, cq}, st);
}
int latent_guide_f32(const avd_latent_guide* g, const int64_t* tau, const float* abar, int T_train, const float* z, float* out, int B,
                     int64_t per, hipStream_t st) {
    return stream_pass(StreamPass{"latent_guide", "", "latent_guide_kernel", false, Keying::Sample, Pass::Guide, B, 1, 1, per, 0, 0, 0, nullptr,
                                  0, g, 0, T_train, tau, tau, abar, z, out}, st);
}
int latent_guide_canvas_f32(const avd_latent_guide* g, const int64_t* tau, const float* abar, int T_train, const float* z, float* out,
                            int N, int64_t outer, int L, int hop, int64_t inner, hipStream_t st) {
    return stream_pass(StreamPass{"latent_guide_canvas", "canvas guide", "canvas_latent_guide_kernel", true, Keying::Canvas, Pass::Guide, N,
                                  L, outer, inner, hop, 0, 0, nullptr, 0, g, 0, T_train, tau, tau, abar, z, out}, st);
}
int renoise_f32(const avd_noise_key* key, uint32_t visit, const avd_latent_guide* g, const int64_t* t_from, const int64_t* t_to,
                const float* abar, int T_train, const float* z, float* out, int B, int64_t per, hipStream_t st) {
    return stream_pass(StreamPass{"renoise", "", "renoise_kernel", false, Keying::Sample, Pass::Renoise, B, 1, 1, per, 0, 0, 0, key, visit, g, 0,
                                  T_train, t_from, t_to, abar, z, out}, st);
}
int renoise_canvas_f32(const avd_noise_key* key, uint32_t visit, const avd_latent_guide* g, const int64_t* t_from, const int64_t* t_to,
                       const float* abar, int T_train, const float* z, float* out, int N, int64_t outer, int L, int hop, int64_t inner,
                       hipStream_t st) {
    // the two maps of this entry share their base: its own check (a null key is stream_pass_check's to report)
    AVD_REQUIRE(!g || !key || g->key.sample_offset == key->sample_offset, AVD_EINVAL,
                "renoise_canvas: the guide's key and the renoise key must carry the same sample_offset (got %lld and %lld)",
                g ? (long long)g->key.sample_offset : 0ll, key ? (long long)key->sample_offset : 0ll);
    return stream_pass(StreamPass{"renoise_canvas", "canvas renoise", "canvas_renoise_kernel", true, Keying::Canvas, Pass::Renoise, N, L, outer,
                                  inner, hop, 0, 0, key, visit, g, 0, T_train, t_from, t_to, abar, z, out}, st);
}
int clip_guide_slots_f32(const avd_clip_guide* g, const int64_t* tau, const float* abar, int T_train, int everywhere, const float* z,
                         float* out, int B, int64_t outer, int L, int slots, int slot_len, int64_t inner, hipStream_t st,
                         const avd_clip_queues* cq = nullptr) {      // cq: as slot_noise_f32, the entry avd_clip_guide_slots_clips_f32
    return stream_pass(StreamPass{cq ? "clip_guide_slots_clips" : "clip_guide_slots", "", cq ? "clip_guide_slots_clips_kernel" : "clip_guide_slots_kernel",
                                  true, Keying::Clip, Pass::ClipSlots, B, L, outer, inner, 0, slots, slot_len, nullptr, 0, g, everywhere,
                                  T_train, tau, tau, abar, z, out, cq}, st);
}

// ------------------------------------------------------------------ CFG control: per-sample guidance, guidance rescale
// The contract is written out in include/avdiff_hip.h (avd_cfg_control).  The statistics pass below writes one fp64 partial of
// (sum c, sum c^2, sum y, sum y^2) per CFG_CHUNK elements of a sample, the finalize pass sums them in index order and stores s_b; the
// fused kernels then read (g_b, phi_b, s_b) per sample through a CfgState in their trailing pack and step on r(y).
constexpr int CFG_CHUNK = 1024;          // elements per partial: 256 lanes x 4 consecutive elements; fixed, so s_b depends on n alone

struct CfgState {
    const float* guidance;   // [B] or nullptr (the scalar)
    const float* rescale;    // [B] or nullptr (phi = 0)
    const float* scale;      // [B] s_b, written by cfg_stats_finalize_kernel (read only when rescale is set)
    // adaptive projected guidance (below): nullptr = none, and the kernels take the path they took before it existed
    const float* apg;        // [B][4] (s_b, k_b, w_b, g_b), written by apg_finalize_kernel
    float* apg_mom;          // [B, per] the momentum buffer in latent layout, or nullptr (beta == 0)
    float apg_beta;
};
struct CfgCoef {
    float g, phi, s;
};
__device__ __forceinline__ CfgCoef cfg_coef(const CfgState& cs, float guidance, int b) {
    CfgCoef c{cs.guidance ? cs.guidance[b] : guidance, 0.f, 1.f};
    if (cs.rescale) {
        c.phi = cs.rescale[b];
        c.s = cs.scale[b];
    }
    return c;
}
// r(e) of the contract: selects at phi 0 and 1, else diffusers' blend without contraction
__device__ __forceinline__ float cfg_rescale(float e, float phi, float s) {
#pragma clang fp contract(off)
    return phi == 0.f ? e : (phi == 1.f ? e * s : phi * (e * s) + (1.0f - phi) * e);
}
// the eps a fused kernel steps on: today's combine (the instantiations without a CfgState), or r(combine with g_b)
template <bool CTL, bool COND = false>
__device__ __forceinline__ float cfg_eps(float ec, float en, float guidance, const CfgCoef& cc) {
    if constexpr (COND) return ec;      // the single-branch form: eps = eps_cond exactly
    else if constexpr (CTL) return cfg_rescale(cfg_combine(ec, en, cc.g), cc.phi, cc.s);
    else return cfg_combine(ec, en, guidance);
}

static int64_t cfg_chunks(int64_t per) { return (per + CFG_CHUNK - 1) / CFG_CHUNK; }
static int64_t cfg_scale_off(int B, int64_t per) { return ((int64_t)B * cfg_chunks(per) * 32 + 15) & ~(int64_t)15; }
int64_t cfg_stats_bytes(int B, int64_t per) {
    if (B <= 0 || per < 2 || per >= ((int64_t)1 << 34)) return -1;
    return cfg_scale_off(B, per) + (((int64_t)B * 4 + 15) & ~(int64_t)15);
}

// Where c and y come from.  PAIR: latent-layout tensors c = a[b], y = y[b] (avd_cfg_rescale_f32).  VIDEO: the cond / null token
// rows of the fused step, c = cond, y = cfg_combine(cond, null, g_b) (U is a permutation: the moments are those of the tokens).
// AUDIO: U is the overlap-add mean, computed per element as cfg_untoken_ddim_audio_kernel does.
enum { CFG_SRC_PAIR = 0, CFG_SRC_VIDEO = 1, CFG_SRC_AUDIO = 2 };

struct AudioGeom {
    int Ca, F, len, stride, Na;
};

// grid (chunks, B): block (j, b) writes part[(b * chunks + j) * 4 + {0..3}] = sums over elements [j * 1024, (j + 1) * 1024) of sample b.
// a / y: sample b's source at a + b * sstride (PAIR, VIDEO: cond tokens; AUDIO: cond tokens) and y + b * sstride (PAIR: y; VIDEO,
// AUDIO: null tokens).
template <int SRC>
__global__ __launch_bounds__(256) void cfg_stats_kernel(const float* __restrict__ a, const float* __restrict__ y, int64_t sstride,
                                                        const float* __restrict__ gvec, float guidance, double* __restrict__ part,
                                                        int64_t per, AudioGeom ag) {
#pragma clang fp contract(off)
    __shared__ double red[4][4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float gb = gvec ? gvec[b] : guidance;
    const float* sa = a + (int64_t)b * sstride;
    const float* sy = y + (int64_t)b * sstride;
    const int64_t el0 = (int64_t)blockIdx.x * CFG_CHUNK + threadIdx.x * 4;
    f32x4 cv = {0.f, 0.f, 0.f, 0.f}, yv = {0.f, 0.f, 0.f, 0.f};
    int nv = 0;                                        // valid elements of this lane (elements >= per add nothing)
    if (el0 < per) {
        nv = per - el0 < 4 ? (int)(per - el0) : 4;
        if constexpr (SRC == CFG_SRC_VIDEO) {          // per % 4 == 0 (w % 4 == 0): a whole float4
            const f32x4 ec = *reinterpret_cast<const f32x4*>(sa + el0), en = *reinterpret_cast<const f32x4*>(sy + el0);
            cv = ec;
#pragma unroll
            for (int k = 0; k < 4; ++k) yv[k] = cfg_combine(ec[k], en[k], gb);
        } else {
            for (int k = 0; k < nv; ++k) {
                const int64_t el = el0 + k;
                if constexpr (SRC == CFG_SRC_PAIR) {
                    cv[k] = sa[el];
                    yv[k] = sy[el];
                } else {                                // as cfg_untoken_ddim_audio_kernel: same windows, same order
                    const int f = (int)(el % ag.F), ch = (int)(el / ag.F);
                    const int L = (ag.Na - 1) * ag.stride + ag.len, D = ag.Ca * ag.len;
                    float c = 0.f, e = 0.f;
                    if (f < L) {
                        int n_hi = f / ag.stride;
                        if (n_hi > ag.Na - 1) n_hi = ag.Na - 1;
                        const int n_lo = (f - ag.len + 1 <= 0) ? 0 : (f - ag.len + ag.stride) / ag.stride;
                        float acc = 0.f, accc = 0.f, cnt = 0.f;
                        for (int n = n_lo; n <= n_hi; ++n) {
                            const int64_t o = (int64_t)n * D + ch * ag.len + (f - n * ag.stride);
                            acc += cfg_combine(sa[o], sy[o], gb);
                            accc += sa[o];
                            cnt += 1.f;
                        }
                        e = acc / fmaxf(cnt, 1e-8f);
                        c = accc / fmaxf(cnt, 1e-8f);
                    }
                    cv[k] = c;
                    yv[k] = e;
                }
            }
        }
    }
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < nv; ++k) {
        const double c = (double)cv[k], e = (double)yv[k];
        m[0] += c;
        m[1] += c * c;
        m[2] += e;
        m[3] += e * e;
    }
    // fixed-order block sum: a butterfly within each wave (lane 0's result is a fixed function of the inputs), then waves 0..3
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int o = 32; o > 0; o >>= 1) m[q] += __shfl_xor(m[q], o, 64);
    if (lane == 0)
        for (int q = 0; q < 4; ++q) red[wv][q] = m[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        part[((int64_t)b * gridDim.x + blockIdx.x) * 4 + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// one lane per sample: the partials summed in index order, then s_b of the contract
__global__ void cfg_stats_finalize_kernel(const double* __restrict__ part, float* __restrict__ scale, int B, int chunks, int64_t per) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const double* p = part + (int64_t)b * chunks * 4;
    for (int j = 0; j < chunks; ++j)
        for (int q = 0; q < 4; ++q) s[q] += p[(int64_t)j * 4 + q];
    const double n = (double)per;
    const double sig_c = sqrt((s[1] - s[0] * s[0] / n) / (n - 1.0));
    const double sig_y = sqrt((s[3] - s[2] * s[2] / n) / (n - 1.0));
    float r = (float)(sig_c / sig_y);
    if (sig_y == 0.0 || !isfinite(r)) r = 1.f;
    scale[b] = r;
}

__global__ __launch_bounds__(256) void cfg_rescale_kernel(const float* e, const float* __restrict__ phi, const float* __restrict__ scale,
                                                          float* out, int64_t per, int64_t total) {       // e may be out
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / per);
    out[i] = cfg_rescale(e[i], phi[b], scale[b]);
}

// true when the byte ranges [a, a + na) and [b, b + nb) overlap
static bool overlaps_bytes(const void* a, int64_t na, const void* b, int64_t nb) {
    const char *p = static_cast<const char*>(a), *q = static_cast<const char*>(b);
    return p < q + nb && q < p + na;
}

// The checks of a CFG control before any launch; with rescale set, the scratch's size / alignment, and no overlap with out / x0_hist
static int make_cfg(const avd_cfg_control* ctl, int B, int64_t per, const float* out, const float* x0_hist, CfgState& cs) {
    AVD_REQUIRE(ctl, AVD_EINVAL, "cfg_control: null control");
    AVD_REQUIRE(B > 0 && B <= 65535 && per >= 2 && per < ((int64_t)1 << 34), AVD_EINVAL,
                "cfg_control: bad dims (B %d in [1, 65535], per_sample %lld must be >= 2)", B, (long long)per);
    cs = CfgState{ctl->guidance, ctl->rescale, nullptr, nullptr, nullptr, 0.f};
    if (!ctl->rescale) return AVD_OK;
    const int64_t need = cfg_stats_bytes(B, per);
    AVD_REQUIRE(ctl->stats, AVD_EINVAL, "cfg_control: rescale needs the statistics scratch (stats)");
    AVD_REQUIRE(aligned16(ctl->stats), AVD_EUNSUPPORTED, "cfg_control: stats must be 16-byte aligned");
    AVD_REQUIRE(ctl->stats_bytes >= need, AVD_EINVAL, "cfg_control: stats holds %lld bytes, %lld needed", (long long)ctl->stats_bytes,
                (long long)need);
    for (const float* p : {out, x0_hist})
        AVD_REQUIRE(!p || !overlaps_bytes(ctl->stats, need, p, (int64_t)B * per * 4), AVD_EINVAL,
                    "cfg_control: stats must not overlap z_out or x0_hist");
    cs.scale = reinterpret_cast<const float*>(static_cast<const char*>(ctl->stats) + cfg_scale_off(B, per));
    return AVD_OK;
}

// make_cfg's checks alone: the composite step runs them before the model (as check_latent_guide)
int check_cfg_control(const avd_cfg_control* ctl, int B, int64_t per, const float* out, const float* x0_hist) {
    CfgState cs;
    return make_cfg(ctl, B, per, out, x0_hist, cs);
}

// the statistics pass: partials, then s_b into the scratch's scale slot
template <int SRC>
static int run_cfg_stats(const avd_cfg_control* ctl, const float* a, const float* y, int64_t sstride, float guidance, int B, int64_t per,
                         AudioGeom ag, hipStream_t st) {
    const int64_t chunks = cfg_chunks(per);
    double* part = static_cast<double*>(ctl->stats);
    static const int tag = prof_tag_id("cfg_stats_kernel");
    ProfScope prof(tag, 8.0 * (double)B * per, st);
    hipLaunchKernelGGL(cfg_stats_kernel<SRC>, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, st, a, y, sstride, ctl->guidance,
                       guidance, part, per, ag);
    hipLaunchKernelGGL(cfg_stats_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, part,
                       reinterpret_cast<float*>(static_cast<char*>(ctl->stats) + cfg_scale_off(B, per)), B, (int)chunks, per);
    AVD_CHECK_LAUNCH("cfg_stats");
    return AVD_OK;
}

int cfg_rescale_f32(const float* e_cond, const float* e_cfg, const float* phi, void* stats, int64_t stats_bytes, float* out, int B,
                    int64_t per, hipStream_t st) {
    AVD_REQUIRE(e_cond && e_cfg && phi && out, AVD_EINVAL, "cfg_rescale: null pointer");
    const avd_cfg_control ctl{nullptr, phi, stats, stats_bytes};
    CfgState cs;
    if (int rc = make_cfg(&ctl, B, per, out, nullptr, cs)) return rc;
    const int64_t total = (int64_t)B * per;
    AVD_REQUIRE(!overlaps_bytes(stats, stats_bytes, e_cond, total * 4) && !overlaps_bytes(stats, stats_bytes, e_cfg, total * 4),
                AVD_EINVAL, "cfg_rescale: stats must not overlap e_cond or e_cfg");
    AVD_REQUIRE(out == e_cfg || !overlaps(out, e_cfg, total), AVD_EINVAL, "cfg_rescale: out must be e_cfg or not overlap it");
    AVD_REQUIRE(!overlaps(out, e_cond, total), AVD_EINVAL, "cfg_rescale: out must not overlap e_cond");
    AVD_REQUIRE((total + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "cfg_rescale: %lld values is too many for one launch", (long long)total);
    if (int rc = run_cfg_stats<CFG_SRC_PAIR>(&ctl, e_cond, e_cfg, per, 0.f, B, per, AudioGeom{}, st)) return rc;
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, e_cfg, phi, cs.scale, out, per, total);
    AVD_CHECK_LAUNCH("cfg_rescale");
    return AVD_OK;
}

// ------------------------------------------------------------------ adaptive projected guidance (APG)
// The contract is written out in include/avdiff_hip.h ("adaptive projected guidance").  As the CFG control above: a statistics pass
// writes one fp64 partial of (sum d^2, sum d c, sum c^2) per CFG_CHUNK latent-order elements of a sample, a finalize pass sums them in
// index order and stores (s_b, k_b, w_b, g_b); the fused kernels read the pair (w_b, k_b) through the CfgState's APG part and step on
// e = c + w_b (d - k_b c).  d = (c - u) + beta m_prev, and the fused kernel stores d back into the momentum buffer: the statistics pass
// has read m_prev before that launch starts (same stream), and both evaluate d with the same two functions below.
__device__ __forceinline__ float apg_d0(float c, float u) {
#pragma clang fp contract(off)
    return c - u;
}
// d of the contract from d0 and the buffer's value; beta == 0 (no buffer) is d0 itself
__device__ __forceinline__ float apg_dir(float d0, float beta, float m) {
#pragma clang fp contract(off)
    return beta != 0.f ? d0 + beta * m : d0;
}
__device__ __forceinline__ float apg_eps(float c, float d, float w, float k) {
#pragma clang fp contract(off)
    return c + w * (d - k * c);
}
// item 5 of the contract for the four elements at latent address lat of sample b, from c and d0: reads m_prev and stores d when the
// buffer is set
__device__ __forceinline__ f32x4 apg_eps4(const CfgState& cs, int b, int64_t lat, const f32x4& c, const f32x4& d0) {
    const float k = cs.apg[(int64_t)b * 4 + 1], w = cs.apg[(int64_t)b * 4 + 2];
    f32x4 m = {0.f, 0.f, 0.f, 0.f}, d, e;
    if (cs.apg_mom) m = *reinterpret_cast<const f32x4*>(cs.apg_mom + lat);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d[j] = apg_dir(d0[j], cs.apg_beta, m[j]);
        e[j] = apg_eps(c[j], d[j], w, k);
    }
    if (cs.apg_mom) *reinterpret_cast<f32x4*>(cs.apg_mom + lat) = d;
    return e;
}
// the eps an update steps on: the APG value where the launch carries one, else cfg_eps (all a non-CTL instantiation compiles)
template <bool CTL, bool COND>
__device__ __forceinline__ float step_eps(bool apg, float ea, float ec, float en, float guidance, const CfgCoef& cc) {
    if constexpr (CTL) {
        if (apg) return ea;
    }
    return cfg_eps<CTL, COND>(ec, en, guidance, cc);
}

constexpr int APG_MOMENTS = 3;
static int64_t apg_coef_off(int B, int64_t per) { return ((int64_t)B * cfg_chunks(per) * APG_MOMENTS * 8 + 15) & ~(int64_t)15; }
int64_t apg_stats_bytes(int B, int64_t per) {
    if (B <= 0 || B > 65535 || per < 2 || per >= ((int64_t)1 << 34)) return -1;
    return apg_coef_off(B, per) + (int64_t)B * 16;
}

// grid (chunks, B): block (j, b) writes part[(b * chunks + j) * 3 + {0, 1, 2}] = the sums of (d^2, d c, c^2) over latent elements
// [j * 1024, (j + 1) * 1024) of sample b.  a / u: sample b's source at a + b * sstride and u + b * sstride.  PAIR: latent-layout c and
// u.  VIDEO: the cond / null token rows, read through the latent -> token offset map, one float4 of latent per lane (the gather form of
// the fused kernel), so that the partition and the momentum read follow the latent.  AUDIO: the two overlap-add means per element.
template <int SRC>
__global__ __launch_bounds__(256) void apg_stats_kernel(const float* __restrict__ a, const float* __restrict__ u, int64_t sstride,
                                                        const float* __restrict__ mom, float beta, double* __restrict__ part,
                                                        int64_t per, Tube g, AudioGeom ag) {
#pragma clang fp contract(off)
    __shared__ double red[4][APG_MOMENTS];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* sa = a + (int64_t)b * sstride;
    const float* su = u + (int64_t)b * sstride;
    const int64_t el0 = (int64_t)blockIdx.x * CFG_CHUNK + threadIdx.x * 4;
    f32x4 cv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
    int nv = 0;                                        // valid elements of this lane (elements >= per add nothing)
    if (el0 < per) {
        nv = per - el0 < 4 ? (int)(per - el0) : 4;
        const float* sm = mom ? mom + (int64_t)b * per + el0 : nullptr;
        if constexpr (SRC == CFG_SRC_VIDEO) {          // per % 4 == 0 (w % 4 == 0): a whole float4, 16-byte aligned in all three
            const int64_t toff = tube_tok_off(g, el0 >> 2);
            const f32x4 ec = *reinterpret_cast<const f32x4*>(sa + toff), en = *reinterpret_cast<const f32x4*>(su + toff);
            f32x4 m = {0.f, 0.f, 0.f, 0.f};
            if (sm) m = *reinterpret_cast<const f32x4*>(sm);
            cv = ec;
#pragma unroll
            for (int k = 0; k < 4; ++k) dv[k] = apg_dir(apg_d0(ec[k], en[k]), beta, m[k]);
        } else {
            for (int k = 0; k < nv; ++k) {
                const int64_t el = el0 + k;
                float c, n;
                if constexpr (SRC == CFG_SRC_PAIR) {
                    c = sa[el];
                    n = su[el];
                } else {                                // as cfg_untoken_ddim_audio_kernel's APG branch: the same two means
                    const int f = (int)(el % ag.F), ch = (int)(el / ag.F);
                    const int L = (ag.Na - 1) * ag.stride + ag.len, D = ag.Ca * ag.len;
                    c = f < L ? ola_gather(sa, D, ch, ag.len, ag.stride, ag.Na, f) : 0.f;
                    n = f < L ? ola_gather(su, D, ch, ag.len, ag.stride, ag.Na, f) : 0.f;
                }
                cv[k] = c;
                dv[k] = apg_dir(apg_d0(c, n), beta, sm ? sm[k] : 0.f);
            }
        }
    }
    double m[APG_MOMENTS] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nv; ++k) {
        const double c = (double)cv[k], d = (double)dv[k];
        m[0] += d * d;
        m[1] += d * c;
        m[2] += c * c;
    }
    // fixed-order block sum, as cfg_stats_kernel: a butterfly within each wave, then waves 0..3
#pragma unroll
    for (int q = 0; q < APG_MOMENTS; ++q)
        for (int o = 32; o > 0; o >>= 1) m[q] += __shfl_xor(m[q], o, 64);
    if (lane == 0)
        for (int q = 0; q < APG_MOMENTS; ++q) red[wv][q] = m[q];
    __syncthreads();
    if (threadIdx.x < APG_MOMENTS) {
        const int q = threadIdx.x;
        part[((int64_t)b * gridDim.x + blockIdx.x) * APG_MOMENTS + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// one lane per sample: the partials summed in index order, then item 4 of the contract; coef[b] = (s_b, k_b, w_b, g_b), one store
__global__ void apg_finalize_kernel(const double* __restrict__ part, float* __restrict__ coef, const float* __restrict__ gvec,
                                    float guidance, float r, float eta_p, int B, int chunks) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s[APG_MOMENTS] = {0.0, 0.0, 0.0};
    const double* p = part + (int64_t)b * chunks * APG_MOMENTS;
    for (int j = 0; j < chunks; ++j)
        for (int q = 0; q < APG_MOMENTS; ++q) s[q] += p[(int64_t)j * APG_MOMENTS + q];
    float sb = 1.f, kb = 0.f;
    if (r != 0.f && s[0] != 0.0) {
        const float v = (float)fmin(1.0, (double)r / sqrt(s[0]));
        if (isfinite(v)) sb = v;
    }
    if (s[2] != 0.0) {
        const float v = (float)((1.0 - (double)eta_p) * s[1] / s[2]);
        if (isfinite(v)) kb = v;
    }
    const float gb = gvec ? gvec[b] : guidance;
    *reinterpret_cast<f32x4*>(coef + (int64_t)b * 4) = f32x4{sb, kb, (gb - 1.0f) * sb, gb};
}

// the combine alone on latent-layout c, u (avd_apg_guidance_f32)
__global__ __launch_bounds__(256) void apg_combine_kernel(const float* __restrict__ c, const float* __restrict__ u,
                                                          const float* __restrict__ coef, float* mom, float beta,
                                                          float* __restrict__ out, int64_t per, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / per;
    const float cv = c[i], d = apg_dir(apg_d0(cv, u[i]), beta, mom ? mom[i] : 0.f);
    if (mom) mom[i] = d;
    out[i] = apg_eps(cv, d, coef[b * 4 + 2], coef[b * 4 + 1]);
}

// The checks of an APG control, all before any HIP call: the parameters' ranges, no rescale beside it, the scratch's size and
// alignment, the momentum buffer set exactly when beta != 0 and 16-byte aligned, and no overlap of either with the call's latent-sized
// tensors `lat` (the step: z, z_out, x0_hist; the elementwise entry: e_cond, e_null, out; nullptr entries are skipped), the eps source
// or each other.  eps: the bytes the statistics pass and the fused kernel read the predictions from (nullptr: they are in `lat`).
// Fills the CfgState's APG part on top of what make_cfg left.
static int make_apg(const avd_apg_control* apg, const avd_cfg_control* ctl, int B, int64_t per, std::initializer_list<const float*> lat,
                    const void* eps, int64_t eps_bytes, CfgState& cs) {
    AVD_REQUIRE(apg, AVD_EINVAL, "apg_control: null control");
    AVD_REQUIRE(B > 0 && B <= 65535 && per >= 2 && per < ((int64_t)1 << 34), AVD_EINVAL,
                "apg_control: bad dims (B %d in [1, 65535], per_sample %lld must be >= 2)", B, (long long)per);
    AVD_REQUIRE(apg->norm_threshold >= 0.f && std::isfinite(apg->norm_threshold), AVD_EINVAL,
                "apg_control: norm_threshold must be finite and >= 0 (0: no cap), got %g", (double)apg->norm_threshold);
    AVD_REQUIRE(apg->eta_parallel >= 0.f && apg->eta_parallel <= 1.f, AVD_EINVAL, "apg_control: eta_parallel must lie in [0, 1], got %g",
                (double)apg->eta_parallel);
    AVD_REQUIRE(std::isfinite(apg->momentum), AVD_EINVAL, "apg_control: momentum must be finite, got %g", (double)apg->momentum);
    AVD_REQUIRE(!(ctl && ctl->rescale), AVD_EINVAL,
                "apg_control: guidance rescale together with APG is refused (its statistics would need the APG output)");
    AVD_REQUIRE((apg->momentum != 0.f) == (apg->momentum_buf != nullptr), AVD_EINVAL,
                "apg_control: momentum_buf must be set exactly when momentum != 0 (momentum %g, buffer %s)", (double)apg->momentum,
                apg->momentum_buf ? "set" : "NULL");
    const int64_t need = apg_stats_bytes(B, per), lat_bytes = (int64_t)B * per * 4;
    AVD_REQUIRE(apg->stats, AVD_EINVAL, "apg_control: APG needs the statistics scratch (stats)");
    AVD_REQUIRE(aligned16(apg->stats), AVD_EUNSUPPORTED, "apg_control: stats must be 16-byte aligned");
    AVD_REQUIRE(apg->stats_bytes >= need, AVD_EINVAL, "apg_control: stats holds %lld bytes, %lld needed (avd_apg_stats_bytes)",
                (long long)apg->stats_bytes, (long long)need);
    AVD_REQUIRE(aligned16(apg->momentum_buf), AVD_EUNSUPPORTED, "apg_control: momentum_buf must be 16-byte aligned");
    for (const float* p : lat) {
        AVD_REQUIRE(!p || !overlaps_bytes(apg->stats, need, p, lat_bytes), AVD_EINVAL,
                    "apg_control: stats must not overlap the call's latents (z, z_out, x0_hist; e_cond, e_null, out)");
        AVD_REQUIRE(!p || !apg->momentum_buf || !overlaps_bytes(apg->momentum_buf, lat_bytes, p, lat_bytes), AVD_EINVAL,
                    "apg_control: momentum_buf must not overlap the call's latents (z, z_out, x0_hist; e_cond, e_null, out)");
    }
    AVD_REQUIRE(!apg->momentum_buf || !overlaps_bytes(apg->momentum_buf, lat_bytes, apg->stats, need), AVD_EINVAL,
                "apg_control: momentum_buf must not overlap the statistics scratch");
    if (eps) {
        AVD_REQUIRE(!overlaps_bytes(apg->stats, need, eps, eps_bytes), AVD_EINVAL, "apg_control: stats must not overlap the eps tokens");
        AVD_REQUIRE(!apg->momentum_buf || !overlaps_bytes(apg->momentum_buf, lat_bytes, eps, eps_bytes), AVD_EINVAL,
                    "apg_control: momentum_buf must not overlap the eps tokens");
    }
    if (!ctl) cs = CfgState{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f};
    cs.apg = reinterpret_cast<const float*>(static_cast<const char*>(apg->stats) + apg_coef_off(B, per));
    cs.apg_mom = apg->momentum_buf;
    cs.apg_beta = apg->momentum;
    return AVD_OK;
}

// make_apg's checks alone: the composite step runs them before the model, with the whole workspace as the eps source
int check_apg_control(const avd_apg_control* apg, const avd_cfg_control* ctl, int B, int64_t per, const float* z, const float* out,
                      const float* x0_hist, const void* eps, int64_t eps_bytes) {
    CfgState cs{};
    return make_apg(apg, ctl, B, per, {z, out, x0_hist}, eps, eps_bytes, cs);
}

// the statistics pass: partials, then (s_b, k_b, w_b, g_b) into the scratch's coefficient slot
template <int SRC>
static int run_apg_stats(const avd_apg_control* apg, const float* gvec, float guidance, const float* a, const float* u, int64_t sstride,
                         int B, int64_t per, Tube g, AudioGeom ag, hipStream_t st) {
    const int64_t chunks = cfg_chunks(per);
    double* part = static_cast<double*>(apg->stats);
    static const int tag = prof_tag_id("apg_stats_kernel");
    ProfScope prof(tag, (apg->momentum_buf ? 12.0 : 8.0) * (double)B * per, st);
    hipLaunchKernelGGL(apg_stats_kernel<SRC>, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, st, a, u, sstride, apg->momentum_buf,
                       apg->momentum, part, per, g, ag);
    hipLaunchKernelGGL(apg_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, part,
                       reinterpret_cast<float*>(static_cast<char*>(apg->stats) + apg_coef_off(B, per)), gvec, guidance,
                       apg->norm_threshold, apg->eta_parallel, B, (int)chunks);
    AVD_CHECK_LAUNCH("apg_stats");
    return AVD_OK;
}

int apg_guidance_f32(const float* e_cond, const float* e_null, const float* gvec, float guidance, const avd_apg_control* apg, float* out,
                     int B, int64_t per, hipStream_t st) {
    AVD_REQUIRE(e_cond && e_null && out, AVD_EINVAL, "apg_guidance: null pointer");
    AVD_REQUIRE(std::isfinite(guidance), AVD_EINVAL, "apg_guidance: the scalar guidance must be finite");
    CfgState cs{};
    if (int rc = make_apg(apg, nullptr, B, per, {e_cond, e_null, out}, nullptr, 0, cs)) return rc;
    const int64_t total = (int64_t)B * per;
    AVD_REQUIRE(!overlaps(out, e_cond, total) && !overlaps(out, e_null, total), AVD_EINVAL,
                "apg_guidance: out must not overlap e_cond or e_null");
    AVD_REQUIRE(!gvec || (!overlaps_bytes(gvec, (int64_t)B * 4, out, total * 4) &&
                          !overlaps_bytes(gvec, (int64_t)B * 4, apg->stats, apg->stats_bytes) &&
                          !(apg->momentum_buf && overlaps_bytes(gvec, (int64_t)B * 4, apg->momentum_buf, total * 4))),
                AVD_EINVAL, "apg_guidance: guidance must not overlap out, the scratch or momentum_buf");
    AVD_REQUIRE((total + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "apg_guidance: %lld values is too many for one launch", (long long)total);
    if (int rc = run_apg_stats<CFG_SRC_PAIR>(apg, gvec, guidance, e_cond, e_null, per, B, per, Tube{}, AudioGeom{}, st)) return rc;
    static const int tag = prof_tag_id("apg_combine_kernel");
    ProfScope prof(tag, (apg->momentum_buf ? 20.0 : 12.0) * (double)total, st);
    hipLaunchKernelGGL(apg_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, e_cond, e_null, cs.apg, cs.apg_mom,
                       cs.apg_beta, out, per, total);
    AVD_CHECK_LAUNCH("apg_guidance");
    return AVD_OK;
}

// ------------------------------------------------------------------ slot CFG control: guidance by noise level, per-slot rescale and APG
// The contract is written out in include/avdiff_hip.h ("slot CFG control").  The slot forms of the two controls above: g and phi are
// looked up by the slot's noise level t_now[b, s] in device tables, and the rescale / APG moments run over ONE slot's elements, not the
// sample's (a sample of a queue holds S slots at S noise levels).  The statistics pass writes fp64 partials per CFG_CHUNK elements of a
// slot, the finalize pass sums them in index order and stores four floats per slot; the fused kernels read them by tb = b * S + s
// through a SlotCfgState in their trailing pack.  The arithmetic is cfg_combine / cfg_rescale / apg_d0 / apg_eps, as per sample.
enum { SLOT_CFG_TABLE = 0, SLOT_CFG_RESCALE = 1, SLOT_CFG_APG = 2 };
struct SlotCfgState {
    const float* guidance_t;   // [T_train] or nullptr (the scalar); read by the TABLE mode and the statistics passes
    const float* rescale_t;    // [T_train], set in the RESCALE mode
    const float* coef;         // [B * S][4]: RESCALE (s, g, phi, 0), APG (s, k, w, g); nullptr in the TABLE mode
    int mode;
};
struct SlotCfgCoef {
    float g, phi, s, k, w;
    bool apg;
};
// "slot APG momentum": behind a SlotCfgState in its APG mode, a pack element of its own, so that the packs without it keep their code.
// buf is the [B, per] latent-layout buffer whose elements travel with their slot (avd_fifo_carry_f32); a stepping slot's lanes read
// m_prev at their latent address and store d there, a held slot's lanes touch nothing.
struct SlotMomentum {
    float* buf;
    float beta;      // != 0
};
// the statistics pass's view of it: the buffer read-only, and what turns a slot's element index into its latent address
struct SlotMomentumAt {
    const float* buf;
    float beta;
    int64_t per;     // one sample's latent elements
    int len, F;      // audio: the chunk length and the latent's frames (video: unused, the Tube has the geometry)
};
// the level of the contract: the clamp of ddim_coef
__device__ __forceinline__ int slot_level(const int64_t* t_now, int T_train, int tb) {
    long long tn = t_now[tb];
    if (tn < 0) tn = 0;
    if (tn > T_train - 1) tn = T_train - 1;
    return (int)tn;
}
// a stepping slot's coefficients (a held slot never gets here)
__device__ __forceinline__ SlotCfgCoef slot_cfg_coef(const SlotCfgState& sc, const int64_t* t_now, int T_train, float guidance, int tb) {
    SlotCfgCoef c{guidance, 0.f, 1.f, 0.f, 0.f, false};
    if (sc.mode == SLOT_CFG_TABLE) {
        if (sc.guidance_t) c.g = sc.guidance_t[slot_level(t_now, T_train, tb)];
        return c;
    }
    const f32x4 v = *reinterpret_cast<const f32x4*>(sc.coef + (int64_t)tb * 4);
    if (sc.mode == SLOT_CFG_APG) c = SlotCfgCoef{v[3], 0.f, v[0], v[1], v[2], true};
    else c = SlotCfgCoef{v[1], v[2], v[0], 0.f, 0.f, false};
    return c;
}
// the eps a slot steps on, per element: r(combine with g) or the APG value at beta == 0 (d = d0: no momentum, so it needs no exchange)
__device__ __forceinline__ float slot_cfg_eps(const SlotCfgCoef& c, float ec, float en) {
    if (c.apg) return apg_eps(ec, apg_d0(ec, en), c.w, c.k);
    return cfg_rescale(cfg_combine(ec, en, c.g), c.phi, c.s);
}
// the momentum form for the four elements at latent address lat (the lane owns it), from c and d0 = c - u: reads m_prev, stores d and
// returns e = c + w (d - k c); apg_eps4 with the slot's coefficients
__device__ __forceinline__ f32x4 slot_mom_eps4(const SlotMomentum& sm, const SlotCfgCoef& sf, int64_t lat, const f32x4& c, const f32x4& d0) {
    const f32x4 m = *reinterpret_cast<const f32x4*>(sm.buf + lat);
    f32x4 d, e;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d[j] = apg_dir(d0[j], sm.beta, m[j]);
        e[j] = apg_eps(c[j], d[j], sf.w, sf.k);
    }
    *reinterpret_cast<f32x4*>(sm.buf + lat) = d;
    return e;
}

static int64_t slot_cfg_coef_off(int64_t BS, int64_t per_slot) { return (BS * cfg_chunks(per_slot) * 32 + 15) & ~(int64_t)15; }
int64_t slot_cfg_stats_bytes(int B, int slots, int64_t per_slot) {
    if (B <= 0 || slots <= 0 || (int64_t)B * slots > 65535 || per_slot < 2 || per_slot >= ((int64_t)1 << 34)) return -1;
    return slot_cfg_coef_off((int64_t)B * slots, per_slot) + (int64_t)B * slots * 16;
}

// the geometry of one slot inside its sample's token rows and latent
struct SlotGeom {
    int S;
    int64_t per_slot;      // video C p0 H W, audio Ca len
    int64_t tok_slot;      // floats of a slot's token rows: video Ht Wt D (contiguous), audio D (token s)
    int64_t lat_slice;     // video: p0 H W, the slot's latent elements per channel (audio: unused)
};

// grid (chunks per slot, B * S): block (j, tb) writes part[(tb * chunks + j) * 4 + q], the sums over elements [j * 1024, (j + 1) * 1024)
// of slot tb.  RESCALE: (sum c, sum c^2, sum y, sum y^2) in token order from the slot's first token element, y = cfg_combine(c, u, g).
// APG: (sum d^2, sum d c, sum c^2, 0) in the slot's own latent order ((c, t in slot, h, w); audio (ch, j), which is its token order).
// A held slot's blocks return before they load anything: its partials are never read.
// A SlotMomentumAt ending the arguments (APG only; an empty pack otherwise, which keeps the argument layout and the code) makes d =
// d0 + beta m_prev, m_prev read at the element's latent address as apg_stats_kernel reads it: the fused update that stores d starts
// after this launch (same stream) and evaluates d with the same two functions.
template <int SRC, bool APG, class... Mom>
__global__ __launch_bounds__(256) void slot_cfg_stats_kernel(const float* __restrict__ a, const float* __restrict__ u, int64_t sstride,
                                                             const int64_t* __restrict__ t_now, const int64_t* __restrict__ t_prev,
                                                             const float* __restrict__ gtab, float guidance, int T_train,
                                                             double* __restrict__ part, SlotGeom sg, Tube g, Mom... mm) {
#pragma clang fp contract(off)
    constexpr bool MOM = sizeof...(Mom) == 1;
    static_assert(sizeof...(Mom) <= 1 && (!MOM || APG), "the pack: empty, or one SlotMomentumAt behind an APG pass");
    __shared__ double red[4][4];
    const int tb = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (t_now[tb] == t_prev[tb]) return;
    const int b = tb / sg.S, s = tb % sg.S;
    [[maybe_unused]] float gb = guidance;
    if constexpr (!APG)
        if (gtab) gb = gtab[slot_level(t_now, T_train, tb)];
    const float* sa = a + (int64_t)b * sstride;
    const float* su = u + (int64_t)b * sstride;
    const int64_t el0 = (int64_t)blockIdx.x * CFG_CHUNK + threadIdx.x * 4;
    f32x4 cv = {0.f, 0.f, 0.f, 0.f}, uv = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] f32x4 mv = {0.f, 0.f, 0.f, 0.f};  // m_prev of the lane's elements (MOM)
    int nv = 0;                                        // valid elements of this lane (elements >= per_slot add nothing)
    if (el0 < sg.per_slot) {
        nv = sg.per_slot - el0 < 4 ? (int)(sg.per_slot - el0) : 4;
        if constexpr (SRC == CFG_SRC_VIDEO) {          // per_slot % 4 == 0 (w % 4 == 0): a whole float4, 16-byte aligned
            int64_t off = (int64_t)s * sg.tok_slot + el0;      // RESCALE: token order
            if constexpr (APG) {                       // the slot's latent order -> the sample's latent float4 -> its token offset
                const int64_t c = el0 / sg.lat_slice, r = el0 % sg.lat_slice;
                off = tube_tok_off(g, ((c * g.T + (int64_t)s * g.t) * ((int64_t)g.H * g.W) + r) >> 2);
                if constexpr (MOM) {                   // the same latent float4 of the buffer
                    const SlotMomentumAt ma = pack_get<SlotMomentumAt>(mm...);
                    mv = *reinterpret_cast<const f32x4*>(ma.buf + (int64_t)b * ma.per + (c * g.T + (int64_t)s * g.t) * ((int64_t)g.H * g.W) + r);
                }
            }
            cv = *reinterpret_cast<const f32x4*>(sa + off);
            uv = *reinterpret_cast<const f32x4*>(su + off);
        } else {                                       // audio token s: (ch, j) in either order
            for (int k = 0; k < nv; ++k) {
                cv[k] = sa[(int64_t)s * sg.tok_slot + el0 + k];
                uv[k] = su[(int64_t)s * sg.tok_slot + el0 + k];
                if constexpr (MOM) {                   // element (ch, j) of chunk s is latent (ch, s len + j)
                    const SlotMomentumAt ma = pack_get<SlotMomentumAt>(mm...);
                    const int64_t el = el0 + k;
                    mv[k] = ma.buf[(int64_t)b * ma.per + (el / ma.len) * ma.F + (int64_t)s * ma.len + el % ma.len];
                }
            }
        }
    }
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < nv; ++k) {
        const double c = (double)cv[k];
        if constexpr (MOM) {
            const double d = (double)apg_dir(apg_d0(cv[k], uv[k]), pack_get<SlotMomentumAt>(mm...).beta, mv[k]);
            m[0] += d * d;
            m[1] += d * c;
            m[2] += c * c;
        } else if constexpr (APG) {
            const double d = (double)apg_d0(cv[k], uv[k]);
            m[0] += d * d;
            m[1] += d * c;
            m[2] += c * c;
        } else {
            const double e = (double)cfg_combine(cv[k], uv[k], gb);
            m[0] += c;
            m[1] += c * c;
            m[2] += e;
            m[3] += e * e;
        }
    }
    // fixed-order block sum, as cfg_stats_kernel: a butterfly within each wave, then waves 0..3
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int o = 32; o > 0; o >>= 1) m[q] += __shfl_xor(m[q], o, 64);
    if (lane == 0)
        for (int q = 0; q < 4; ++q) red[wv][q] = m[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        part[((int64_t)tb * gridDim.x + blockIdx.x) * 4 + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
}

// one lane per slot: the partials summed in index order, then the coefficients of the contract in one store.  A held slot gets the
// neutral (1, 0, 0, 0) and reads neither its partials nor the tables.
template <bool APG>
__global__ void slot_cfg_finalize_kernel(const double* __restrict__ part, float* __restrict__ coef, const int64_t* __restrict__ t_now,
                                         const int64_t* __restrict__ t_prev, const float* __restrict__ gtab,
                                         const float* __restrict__ ptab, float guidance, int T_train, float r, float eta_p, int BS,
                                         int chunks, int64_t per_slot) {
#pragma clang fp contract(off)
    const int tb = blockIdx.x * blockDim.x + threadIdx.x;
    if (tb >= BS) return;
    if (t_now[tb] == t_prev[tb]) {
        *reinterpret_cast<f32x4*>(coef + (int64_t)tb * 4) = f32x4{1.f, 0.f, 0.f, 0.f};
        return;
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const double* p = part + (int64_t)tb * chunks * 4;
    for (int j = 0; j < chunks; ++j)
        for (int q = 0; q < 4; ++q) s[q] += p[(int64_t)j * 4 + q];
    const int lv = slot_level(t_now, T_train, tb);
    const float gb = gtab ? gtab[lv] : guidance;
    if constexpr (APG) {      // item 4 of "adaptive projected guidance", the expressions of apg_finalize_kernel
        float sb = 1.f, kb = 0.f;
        if (r != 0.f && s[0] != 0.0) {
            const float v = (float)fmin(1.0, (double)r / sqrt(s[0]));
            if (isfinite(v)) sb = v;
        }
        if (s[2] != 0.0) {
            const float v = (float)((1.0 - (double)eta_p) * s[1] / s[2]);
            if (isfinite(v)) kb = v;
        }
        *reinterpret_cast<f32x4*>(coef + (int64_t)tb * 4) = f32x4{sb, kb, (gb - 1.0f) * sb, gb};
    } else {                  // step 3 of avd_cfg_control, the expressions of cfg_stats_finalize_kernel
        const double n = (double)per_slot;
        const double sig_c = sqrt((s[1] - s[0] * s[0] / n) / (n - 1.0));
        const double sig_y = sqrt((s[3] - s[2] * s[2] / n) / (n - 1.0));
        float sc = (float)(sig_c / sig_y);
        if (sig_y == 0.0 || !isfinite(sc)) sc = 1.f;
        *reinterpret_cast<f32x4*>(coef + (int64_t)tb * 4) = f32x4{sc, gb, ptab ? ptab[lv] : 0.f, 0.f};
    }
}

// The checks of a slot control, all before any HIP call, in the contract's order; fills the pack's state.  lat: the call's latent-sized
// tensors (z, z_out, x0_hist; nullptr entries are skipped); eps: the bytes the predictions are read from.
// sm: the momentum element of the pack ("slot APG momentum"), buf == nullptr when the control carries none; its checks mirror
// make_apg's for avd_apg_control's buffer.
static int make_slot_cfg(const avd_slot_cfg* cfg, int B, int S, int64_t per_slot, int64_t per, std::initializer_list<const float*> lat,
                         const void* eps, int64_t eps_bytes, SlotCfgState& sc, SlotMomentum& sm) {
    AVD_REQUIRE(cfg, AVD_EINVAL, "slot_cfg: null control");
    AVD_REQUIRE(!(cfg->apg && cfg->rescale_t), AVD_EINVAL,
                "slot_cfg: guidance rescale together with APG is refused (its statistics would need the APG output)");
    if (cfg->apg) {
        AVD_REQUIRE(cfg->norm_threshold >= 0.f && std::isfinite(cfg->norm_threshold), AVD_EINVAL,
                    "slot_cfg: norm_threshold must be finite and >= 0 (0: no cap), got %g", (double)cfg->norm_threshold);
        AVD_REQUIRE(cfg->eta_parallel >= 0.f && cfg->eta_parallel <= 1.f, AVD_EINVAL, "slot_cfg: eta_parallel must lie in [0, 1], got %g",
                    (double)cfg->eta_parallel);
    }
    sm = SlotMomentum{nullptr, 0.f};
    if (cfg->apg == AVD_SLOT_APG_MOMENTUM) {      // the control is the first member of an avd_slot_cfg_momentum: its two fields follow
        const avd_slot_cfg_momentum* m = reinterpret_cast<const avd_slot_cfg_momentum*>(cfg);
        AVD_REQUIRE(std::isfinite(m->momentum), AVD_EINVAL, "slot_cfg: momentum must be finite, got %g", (double)m->momentum);
        AVD_REQUIRE((m->momentum != 0.f) == (m->momentum_buf != nullptr), AVD_EINVAL,
                    "slot_cfg: momentum_buf must be set exactly when momentum != 0 (momentum %g, buffer %s)", (double)m->momentum,
                    m->momentum_buf ? "set" : "NULL");
        sm = SlotMomentum{m->momentum_buf, m->momentum};
    }
    sc = SlotCfgState{cfg->guidance_t, cfg->rescale_t, nullptr, cfg->apg ? SLOT_CFG_APG : cfg->rescale_t ? SLOT_CFG_RESCALE : SLOT_CFG_TABLE};
    if (sc.mode == SLOT_CFG_TABLE) return AVD_OK;
    const int64_t need = slot_cfg_stats_bytes(B, S, per_slot);
    AVD_REQUIRE(need > 0, AVD_EINVAL, "slot_cfg: bad dims (B %d * slots %d in [1, 65535], per_slot %lld must be >= 2)", B, S,
                (long long)per_slot);
    AVD_REQUIRE(cfg->stats, AVD_EINVAL, "slot_cfg: rescale and APG need the statistics scratch (stats)");
    AVD_REQUIRE(cfg->stats_bytes >= need, AVD_EINVAL, "slot_cfg: stats holds %lld bytes, %lld needed (avd_slot_cfg_stats_bytes)",
                (long long)cfg->stats_bytes, (long long)need);
    AVD_REQUIRE(aligned16(cfg->stats), AVD_EUNSUPPORTED, "slot_cfg: stats must be 16-byte aligned");
    for (const float* p : lat)
        AVD_REQUIRE(!p || !overlaps_bytes(cfg->stats, need, p, (int64_t)B * per * 4), AVD_EINVAL,
                    "slot_cfg: stats must not overlap z, z_out or x0_hist");
    AVD_REQUIRE(!eps || !overlaps_bytes(cfg->stats, need, eps, eps_bytes), AVD_EINVAL, "slot_cfg: stats must not overlap the eps tokens");
    if (sm.buf) {
        const int64_t lat_bytes = (int64_t)B * per * 4;
        AVD_REQUIRE(aligned16(sm.buf), AVD_EUNSUPPORTED, "slot_cfg: momentum_buf must be 16-byte aligned");
        for (const float* p : lat)
            AVD_REQUIRE(!p || !overlaps_bytes(sm.buf, lat_bytes, p, lat_bytes), AVD_EINVAL,
                        "slot_cfg: momentum_buf must not overlap z, z_out or x0_hist");
        AVD_REQUIRE(!overlaps_bytes(sm.buf, lat_bytes, cfg->stats, need), AVD_EINVAL,
                    "slot_cfg: momentum_buf must not overlap the statistics scratch");
        AVD_REQUIRE(!eps || !overlaps_bytes(sm.buf, lat_bytes, eps, eps_bytes), AVD_EINVAL,
                    "slot_cfg: momentum_buf must not overlap the eps tokens");
    }
    sc.coef = reinterpret_cast<const float*>(static_cast<const char*>(cfg->stats) + slot_cfg_coef_off((int64_t)B * S, per_slot));
    return AVD_OK;
}

// make_slot_cfg's checks alone: the composite step runs them before the model, with the whole workspace as the eps source
int check_slot_cfg(const avd_slot_cfg* cfg, int B, int S, int64_t per_slot, int64_t per, const float* z, const float* out,
                   const float* x0_hist, const void* eps, int64_t eps_bytes) {
    SlotCfgState sc;
    SlotMomentum sm;
    return make_slot_cfg(cfg, B, S, per_slot, per, {z, out, x0_hist}, eps, eps_bytes, sc, sm);
}

// the statistics pass of a RESCALE or APG control: partials, then four floats per slot into the scratch's tail
template <int SRC>
static int run_slot_cfg_stats(const avd_slot_cfg* cfg, const SlotCfgState& sc, const float* a, const float* u, int64_t sstride,
                              const int64_t* t_now, const int64_t* t_prev, float guidance, int T_train, int B, const SlotGeom& sg, Tube g,
                              hipStream_t st, const SlotMomentumAt& ma = SlotMomentumAt{}) {
    const int64_t chunks = cfg_chunks(sg.per_slot);
    const int BS = B * sg.S;
    double* part = static_cast<double*>(cfg->stats);
    float* coef = const_cast<float*>(sc.coef);
    static const int tag = prof_tag_id("slot_cfg_stats_kernel");
    static const int tag_mom = prof_tag_id("slot_cfg_stats_kernel<momentum>");
    static const int tag_fin = prof_tag_id("slot_cfg_finalize_kernel");
    const dim3 grid((unsigned)chunks, (unsigned)BS), fgrid((unsigned)((BS + 63) / 64));
    {
        ProfScope prof(ma.buf ? tag_mom : tag, (ma.buf ? 12.0 : 8.0) * (double)BS * sg.per_slot, st);
        if (ma.buf)      // make_slot_cfg: a momentum rides with the APG mode alone
            hipLaunchKernelGGL((slot_cfg_stats_kernel<SRC, true, SlotMomentumAt>), grid, dim3(256), 0, st, a, u, sstride, t_now, t_prev,
                               sc.guidance_t, guidance, T_train, part, sg, g, ma);
        else if (sc.mode == SLOT_CFG_APG)
            hipLaunchKernelGGL((slot_cfg_stats_kernel<SRC, true>), grid, dim3(256), 0, st, a, u, sstride, t_now, t_prev, sc.guidance_t,
                               guidance, T_train, part, sg, g);
        else
            hipLaunchKernelGGL((slot_cfg_stats_kernel<SRC, false>), grid, dim3(256), 0, st, a, u, sstride, t_now, t_prev, sc.guidance_t,
                               guidance, T_train, part, sg, g);
    }
    {
        ProfScope prof(tag_fin, 32.0 * (double)BS * chunks, st);
        if (sc.mode == SLOT_CFG_APG)
            hipLaunchKernelGGL(slot_cfg_finalize_kernel<true>, fgrid, dim3(64), 0, st, part, coef, t_now, t_prev, sc.guidance_t,
                               sc.rescale_t, guidance, T_train, cfg->norm_threshold, cfg->eta_parallel, BS, (int)chunks, sg.per_slot);
        else
            hipLaunchKernelGGL(slot_cfg_finalize_kernel<false>, fgrid, dim3(64), 0, st, part, coef, t_now, t_prev, sc.guidance_t,
                               sc.rescale_t, guidance, T_train, 0.f, 0.f, BS, (int)chunks, sg.per_slot);
    }
    AVD_CHECK_LAUNCH("slot_cfg_stats");
    return AVD_OK;
}

// ------------------------------------------------------------------ fused CFG + unpatch + DDIM (video target)
int g_cfg_rows = 1;     // avd_tune_set "cfg_rows": 0 = the 16-bytes-per-lane gather form
// SEEDED: zn comes from the seeded normal stream (philox_normal4: one call is exactly this lane's float4) instead of `noise`.  The key
// rides as a trailing parameter pack that is empty when !SEEDED, so the unseeded instantiations keep the kernel-argument layout (the
// hidden arguments such as blockDim sit right behind the explicit ones) and compile to the same code as before the stream existed.
// A CanvasKey in the key's place (SEEDED true) draws zn by canvas position instead (canvas_normal4): one more compile-time case, the
// instantiations with a NoiseKey are untouched.
// A DpmState in the pack replaces the DDIM update by the DPM-Solver++(2M) one (dpm_coef / dpm_apply) on the same x0: alone (SEEDED false)
// the ODE update; followed by a key (SEEDED true, eta > 0) the SDE form, whose noise term is the same zn the DDIM step would draw.
// The three kernels below differ in their fronts alone: how a lane gets its combined eps and where its elements sit in the latent.
// Each builds an UpdateLane once per lane from its own indices and hands it, x and eps to update_tail, the one copy of the draw, the
// solver, the guide blends and the store.
struct UpdateLane {
    int b, tb;            // the sample; the entry of t_now / t_prev the lane steps with (the slot's in the slot form, else b)
    int64_t lat, el;      // the lane's first element: its latent offset, and its offset inside the sample
    int64_t o;            // the slice coordinates of the keyed draws and guides (canvas_normal4): elements i .. of the (o, l) slice
    int l;
    int64_t i, inner;
};
// "clip batch keying": the lane's queue, taken where a keyed call needs it; {0, b} in a pack without a ClipQueues, which is not touched
template <class... Key> __device__ __forceinline__ QueueOf lane_queue(int b, const Key&... nk) {
    if constexpr (PackHas<ClipQueues, Key...>::value) return queue_of(pack_get<ClipQueues>(nk...), b);
    else return QueueOf{0, b};
}
// the coefficients of DDIM (entry tb), of a DpmState's update (entry tb) and of a per-sample or canvas-keyed guide (at t_prev[b])
struct UpdateCoef {
    Ddim c;
    Dpm d;
    GuideCoef gc;
};
// V: the lane's values (4 or 1), in an f32x4.  x: z at the lane; e: the combined eps.  blk: the coefficients a block computed once
// (the rows form), or nullptr: each is then computed per lane where it is first read, which keeps it out of the registers until then
// (the call is inlined, so the choice costs nothing at run time).  The clip guide's, at the slot's own t_prev, are per lane everywhere.
template <int V, bool SEEDED, class... Key>
__device__ __forceinline__ void update_tail(const UpdateLane& ln, f32x4 x, f32x4 e, const UpdateCoef* blk, const int64_t* t_now,
                                            const int64_t* t_prev, const float* abar, int T_train, float eta, const float* noise,
                                            float* z_out, const Key&... nk) {
    constexpr bool DPM = PackHas<DpmState, Key...>::value, GUIDED = PackHas<GuideState, Key...>::value;
    constexpr bool CTL = PackHas<CfgState, Key...>::value, COND = PackHas<CondOnly, Key...>::value;
    [[maybe_unused]] f32x4 zn = {0.f, 0.f, 0.f, 0.f};      // the unkeyed DPM update (eta == 0) draws nothing
    if constexpr (PackHas<SlotKey, Key...>::value) {      // the clip-keyed draw of a stepping slot: by clip position, at the slot's timestep
        const QueueOf qo = lane_queue(ln.b, nk...);
        zn = lane_pick<V>(slot_normal4(lane_slot_key(qo, nk...), qo.b, ln.o, ln.l, ln.i, ln.inner, (uint32_t)t_now[ln.tb]),
                          ln.o * ln.inner + ln.i);
    } else if constexpr (PackHas<CanvasKey, Key...>::value) {      // the canvas-keyed draw: canvas position from l, element (o, i) of its slice
        zn = lane_pick<V>(canvas_normal4(pack_get<CanvasKey>(nk...), ln.b, ln.o, ln.l, ln.i, ln.inner, (uint32_t)t_now[ln.b]),
                          ln.o * ln.inner + ln.i);
    } else if constexpr (SEEDED) {
        NoiseKey k;      // a one-item pack is copied as before the guide existed: through pack_get its argument loads reorder
        if constexpr (GUIDED || CTL || COND || DPM) k = pack_get<NoiseKey>(nk...);
        else k = NoiseKey(nk...);
        zn = lane_pick<V>(philox_normal4(k, (uint32_t)(ln.el >> 2), k.s0 + (uint32_t)ln.b, (uint32_t)t_now[ln.b]), ln.el);
    } else if constexpr (!DPM) {
        if (eta > 0.f) zn = load_v<V>(noise + ln.lat);
    }
    const Ddim c = blk ? blk->c : ddim_coef(t_now, t_prev, abar, T_train, eta, ln.tb);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if constexpr (DPM) {
        const DpmState ds = pack_get<DpmState>(nk...);
        const Dpm d = blk ? blk->d : dpm_coef(ds.t_last, t_now, t_prev, abar, T_train, SEEDED ? eta : 0.f, ln.tb);
        f32x4 hist = {0.f, 0.f, 0.f, 0.f}, x0 = {0.f, 0.f, 0.f, 0.f};
        if (d.c_1 != 0.f) hist = load_v<V>(ds.x0_hist + ln.lat);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            x0[k] = ddim_x0(c, x[k], e[k]);
            o[k] = dpm_apply(d, x[k], x0[k], hist[k], zn[k], SEEDED);
        }
        store_v<V>(ds.x0_hist + ln.lat, x0);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = ddim_apply(c, x[k], e[k], zn[k]);
    }
    [[maybe_unused]] GuideCoef gc{0.f, 0.f, false};
    if constexpr (GUIDED || PackHas<CanvasGuideState, Key...>::value) gc = blk ? blk->gc : guide_coef(abar, T_train, t_prev[ln.b]);
    if constexpr (GUIDED) o = guide_apply<V>(pack_get<GuideState>(nk...), gc, ln.b, ln.lat, ln.el, o);
    if constexpr (PackHas<CanvasGuideState, Key...>::value)      // n_k by canvas position: the slice of the canvas-keyed draw above
        o = canvas_guide_apply<V>(pack_get<CanvasGuideState>(nk...), gc, ln.b, ln.lat, ln.el, ln.o, ln.l, ln.i, ln.inner, o);
    if constexpr (PackHas<ClipGuideState, Key...>::value) {      // the clip-keyed guide of a stepping slot: q at the slot's own t_prev
        const QueueOf qo = lane_queue(ln.b, nk...);
        o = clip_guide_apply<V>(lane_clip_guide(qo, nk...), guide_coef(abar, T_train, t_prev[ln.tb]), qo.b, ln.o, ln.l, ln.i, ln.inner, o);
    }
    store_v<V>(z_out + ln.lat, o);
}

template <bool SEEDED, class... Key>
__global__ __launch_bounds__(256) void cfg_unpatch_ddim_kernel(
    const float* __restrict__ eps2, const float* __restrict__ z, const int64_t* __restrict__ t_now,
    const int64_t* __restrict__ t_prev, const float* __restrict__ abar, int T_train, float guidance, float eta,
    const float* __restrict__ noise, float* __restrict__ z_out, Tube g, int B, int64_t total4, Key... nk) {
    constexpr bool CTL = PackHas<CfgState, Key...>::value, COND = PackHas<CondOnly, Key...>::value;
    static_assert(PackOk<SEEDED, Key...>::value, "not a pack of the fused update kernels (see PackOk)");
    constexpr bool SLOT = PackHas<SlotTimes, Key...>::value;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t per4 = g.per >> 2;
    const int b = (int)(i / per4);
    const int64_t e4 = i % per4;
    const int64_t lat = (int64_t)b * g.per + e4 * 4;
    [[maybe_unused]] int tb = b;      // the entry of t_now / t_prev this lane steps with
    if constexpr (SLOT) {             // per lane: the slot of latent frame tt is tt / t; a held slot keeps z
        // tt is divided out here on its own, not shared with the lane's position below: the shared quotient would stay in registers
        // across the front, which costs the DPM slot packs a wave per SIMD (profiles/update_tail_kernels.txt, item 3)
        const int tt = (int)((e4 / ((int64_t)(g.W >> 2) * g.H)) % g.T);
        tb = b * pack_get<SlotTimes>(nk...).S + tt / g.t;
        if (t_now[tb] == t_prev[tb]) {
            *reinterpret_cast<f32x4*>(z_out + lat) = *reinterpret_cast<const f32x4*>(z + lat);
            return;
        }
    }
    const int64_t toff = tube_tok_off(g, e4);
    const f32x4 ec = *reinterpret_cast<const f32x4*>(eps2 + (int64_t)b * g.per + toff);
    [[maybe_unused]] f32x4 en = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!COND) en = *reinterpret_cast<const f32x4*>(eps2 + ((int64_t)B + b) * g.per + toff);
    const f32x4 x = *reinterpret_cast<const f32x4*>(z + lat);
    f32x4 e = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PackHas<SlotMomentum, Key...>::value) {      // "slot APG momentum": this lane owns the latent address (APG mode)
        const SlotCfgCoef sf = slot_cfg_coef(pack_get<SlotCfgState>(nk...), t_now, T_train, guidance, tb);
        f32x4 d0;
#pragma unroll
        for (int k = 0; k < 4; ++k) d0[k] = apg_d0(ec[k], en[k]);
        e = slot_mom_eps4(pack_get<SlotMomentum>(nk...), sf, lat, ec, d0);
    } else if constexpr (PackHas<SlotCfgState, Key...>::value) {      // the slot control's eps: coefficients by tb, not by b
        const SlotCfgCoef sf = slot_cfg_coef(pack_get<SlotCfgState>(nk...), t_now, T_train, guidance, tb);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = slot_cfg_eps(sf, ec[k], en[k]);
    } else {
        [[maybe_unused]] CfgCoef cc{guidance, 0.f, 1.f};
        [[maybe_unused]] bool apg = false;      // a run-time branch of the CTL instantiations: the launch carries an APG part
        [[maybe_unused]] f32x4 ea = {0.f, 0.f, 0.f, 0.f};
        if constexpr (CTL) {
            const CfgState cs = pack_get<CfgState>(nk...);
            cc = cfg_coef(cs, guidance, b);
            apg = cs.apg != nullptr;
            if (apg) {
                f32x4 d0;
#pragma unroll
                for (int k = 0; k < 4; ++k) d0[k] = apg_d0(ec[k], en[k]);
                ea = apg_eps4(cs, b, lat, ec, d0);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = step_eps<CTL, COND>(apg, ea[k], ec[k], en[k], guidance, cc);
    }
    const int64_t hw4 = ((int64_t)g.H * g.W) >> 2, r = e4 / hw4;      // the lane's float4 lies inside one (c, t) slice (W % 4 == 0)
    const UpdateLane ln{b, tb, lat, e4 * 4, r / g.T, (int)(r % g.T), (e4 % hw4) * 4, hw4 * 4};
    update_tail<4, SEEDED>(ln, x, e, nullptr, t_now, t_prev, abar, T_train, eta, noise, z_out, nk...);
}

// Coalesced form (round 5).  In the kernel above a lane's 16 bytes of latent (4 consecutive w) are one 16-byte piece of a token row, and
// the NEXT 16 bytes of latent belong to the next token, 1 KiB further on: every wave-wide token read touches 64 cache lines for 16 bytes
// each (FETCH_SIZE 63 MB per launch at C3 against 37.7 MB algorithmic).  Here a block owns GT tokens that are neighbours along w' — GT x w
// = one 128-byte line of latent per (c, t, h) — reads their cond / null rows as whole contiguous rows (GT x D floats each, 16 B per lane),
// combines (CFG) in registers, parks the combined eps in LDS as [token][feature] and reads it back as [(c, t, h)][GT x w]: eight lanes then
// cover one full 128-byte line of z / z_out.  Same arithmetic per element, in the same order: bit-identical to the kernel above.
template <int GT, bool SEEDED, class... Key>      // tokens per block; SEEDED / Key as cfg_unpatch_ddim_kernel
__global__ __launch_bounds__(256) void cfg_unpatch_ddim_rows_kernel(
    const float* __restrict__ eps2, const float* __restrict__ z, const int64_t* __restrict__ t_now,
    const int64_t* __restrict__ t_prev, const float* __restrict__ abar, int T_train, float guidance, float eta,
    const float* __restrict__ noise, float* __restrict__ z_out, Tube g, int B, int groups_per_sample, Key... nk) {
    constexpr bool DPM = PackHas<DpmState, Key...>::value;
    constexpr bool CTL = PackHas<CfgState, Key...>::value, COND = PackHas<CondOnly, Key...>::value;
    static_assert(PackOk<SEEDED, Key...>::value, "not a pack of the fused update kernels (see PackOk)");
    constexpr bool SLOT = PackHas<SlotTimes, Key...>::value;
    extern __shared__ __attribute__((aligned(16))) float ebuf[];       // [GT][D + 4]: the pad keeps the transposed 16-byte reads off one bank group
    // an APG launch parks two values per element, c in ebuf and d0 = c - u in a second [GT][D + 4] behind it: the momentum buffer is in
    // latent layout, so m_prev is read, d stored and e built after the exchange, by the lane that owns the element's latent address
    const int LD = g.D + 4;
    const int b = blockIdx.x / groups_per_sample, grp = blockIdx.x % groups_per_sample;
    const int n0 = grp * GT;                                            // first token of the group (GT divides W / w: one (t', h') row)
    [[maybe_unused]] int tb = b;      // the entry of t_now / t_prev this block steps with
    [[maybe_unused]] bool hold = false;
    if constexpr (SLOT) {             // the block's tokens share t': one slot, one pair, and the hold is block-uniform
        tb = b * pack_get<SlotTimes>(nk...).S + n0 / (g.Wt * g.Ht);
        hold = t_now[tb] == t_prev[tb];
    }
    const float* tc = eps2 + ((int64_t)b * (g.per / g.D) + n0) * g.D;
    [[maybe_unused]] const float* tn = eps2 + (((int64_t)B + b) * (g.per / g.D) + n0) * g.D;
    const int nf4 = SLOT && hold ? 0 : GT * g.D / 4;      // a held slot reads no eps
    [[maybe_unused]] CfgCoef cc{guidance, 0.f, 1.f};
    if constexpr (CTL) cc = cfg_coef(pack_get<CfgState>(nk...), guidance, b);
    [[maybe_unused]] bool apg = false;      // block-uniform: the launch carries an APG part
    if constexpr (CTL) apg = pack_get<CfgState>(nk...).apg != nullptr;
    constexpr bool SCFG = PackHas<SlotCfgState, Key...>::value;
    constexpr bool SMOM = PackHas<SlotMomentum, Key...>::value;      // "slot APG momentum": two planes, as the APG part
    [[maybe_unused]] SlotCfgCoef sf{guidance, 0.f, 1.f, 0.f, 0.f, false};      // the slot control: block-uniform, by tb (a held slot reads nothing)
    if constexpr (SCFG)
        if (!hold) sf = slot_cfg_coef(pack_get<SlotCfgState>(nk...), t_now, T_train, guidance, tb);
    for (int i = threadIdx.x; i < nf4; i += 256) {
        const f32x4 ec = *reinterpret_cast<const f32x4*>(tc + (int64_t)i * 4);
        [[maybe_unused]] f32x4 en = {0.f, 0.f, 0.f, 0.f};
        if constexpr (!COND) en = *reinterpret_cast<const f32x4*>(tn + (int64_t)i * 4);
        const int tok = (i * 4) / g.D, k0 = (i * 4) % g.D;
        if (SMOM || (CTL && apg)) {      // c and d0 parked: d and e are built by the owner of the latent address below
            f32x4 d0;
#pragma unroll
            for (int k = 0; k < 4; ++k) d0[k] = apg_d0(ec[k], en[k]);
            *reinterpret_cast<f32x4*>(ebuf + tok * LD + k0) = ec;
            *reinterpret_cast<f32x4*>(ebuf + (GT + tok) * LD + k0) = d0;
            continue;
        }
        f32x4 e;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (SCFG) e[k] = slot_cfg_eps(sf, ec[k], en[k]);      // beta == 0: the APG value needs no second plane
            else e[k] = cfg_eps<CTL, COND>(ec[k], en[k], guidance, cc);
        }
        *reinterpret_cast<f32x4*>(ebuf + tok * LD + k0) = e;
    }
    __syncthreads();
    UpdateCoef uc{ddim_coef(t_now, t_prev, abar, T_train, eta, tb), Dpm{0.f, 0.f, 0.f, 0.f}, GuideCoef{0.f, 0.f, false}};      // once per block
    if constexpr (DPM) uc.d = dpm_coef(pack_get<DpmState>(nk...).t_last, t_now, t_prev, abar, T_train, SEEDED ? eta : 0.f, tb);
    if constexpr (PackHas<GuideState, Key...>::value || PackHas<CanvasGuideState, Key...>::value) uc.gc = guide_coef(abar, T_train, t_prev[b]);
    // token coordinates of the group: n = (t' Ht + h') Wt + w'
    const int wq = n0 % g.Wt, hq = (n0 / g.Wt) % g.Ht, tq = n0 / (g.Wt * g.Ht);
    const int segs = g.D / g.w;                                          // (c, t, h) combinations of a token
    const int per_seg4 = GT * g.w / 4;                                   // float4s of one latent line piece
    for (int i = threadIdx.x; i < segs * per_seg4; i += 256) {
        const int sg = i / per_seg4, j = i % per_seg4;                   // piece j of line sg: token j * 4 / w, offset (j * 4) % w
        const int tok = (j * 4) / g.w, wo = (j * 4) % g.w;
        const int hh = sg % g.h, tt = (sg / g.h) % g.t, co = sg / (g.h * g.t);
        f32x4 e = *reinterpret_cast<const f32x4*>(ebuf + tok * LD + sg * g.w + wo);
        const int64_t lat = (int64_t)b * g.per + (((int64_t)co * g.T + (tq * g.t + tt)) * g.H + (hq * g.h + hh)) * g.W + (wq + tok) * g.w + wo;
        if constexpr (CTL) {
            if (apg)      // e holds c: this lane owns the latent address of the four elements, on this side of the exchange
                e = apg_eps4(pack_get<CfgState>(nk...), b, lat, e, *reinterpret_cast<const f32x4*>(ebuf + (GT + tok) * LD + sg * g.w + wo));
        }
        const f32x4 x = *reinterpret_cast<const f32x4*>(z + lat);
        if constexpr (SLOT) {
            if (hold) {      // z, bit for bit; a DpmState's x0_hist is left alone
                *reinterpret_cast<f32x4*>(z_out + lat) = x;
                continue;
            }
        }
        if constexpr (SMOM)      // e holds c: a stepping slot's lane on this side of the exchange reads m_prev, stores d and builds e
            e = slot_mom_eps4(pack_get<SlotMomentum>(nk...), sf, lat, e, *reinterpret_cast<const f32x4*>(ebuf + (GT + tok) * LD + sg * g.w + wo));
        // element (c, t, h, w) of sample b: position t of the sliding axis, element h W + w of the (c, t) slice
        const UpdateLane ln{b, tb, lat, lat - (int64_t)b * g.per, co, tq * g.t + tt,
                            (int64_t)(hq * g.h + hh) * g.W + (wq + tok) * g.w + wo, (int64_t)g.H * g.W};
        update_tail<4, SEEDED>(ln, x, e, &uc, t_now, t_prev, abar, T_train, eta, noise, z_out, nk...);
    }
}

// ---- the host side of the fused updates, both targets
// the arguments every fused update kernel starts with
struct UpdateArgs {
    const float *eps, *z;      // eps: cond / null [2B, Nt, D], or the cond rows alone [B, Nt, D] (the single-branch form)
    const int64_t *t_now, *t_prev;
    const float* abar;
    int T_train;
    float guidance, eta;       // guidance: not read by the single-branch form
    const float* noise;
    float* z_out;
    int B;
};
// what the kernels' trailing pack is made of: filled by check_fused_update, read by with_update_pack
struct UpdateKeys {
    bool dpm, seeded, canvas, guide, cguide, ctl;
    bool slots;        // the slot form: the pack is sl, or ds then sl for DPM-Solver++(2M) (set by check_slot_update after check_fused_update)
    SlotTimes sl;
    bool skey;         // the slot form at eta > 0: sk ends the slot pack (clip-keyed slot noise)
    SlotKey sk;
    bool clip;         // the slot form under a clip-keyed latent guide: cg ends the slot pack
    ClipGuideState cg;
    bool scfg;         // the slot form under a slot CFG control: sc rides behind the slot key, before the clip guide
    SlotCfgState sc;
    bool smom;         // the slot CFG control carries a momentum buffer: sm rides right behind sc
    SlotMomentum sm;
    bool queues;       // the slot form of a clip batch whose pack holds sk or cg: cq ends the slot pack (clip batch keying)
    ClipQueues cq;
    DpmState ds;
    NoiseKey nk;
    CanvasKey ck;      // canvas: the seeded draw is keyed by canvas position (ck replaces nk in the pack)
    GuideState gs;
    CanvasGuideState cgs;      // cguide: the guide's known noise is keyed by canvas position (cgs replaces gs in the pack)
    CfgState cs;
};

// The checks the four launchers share, all before any HIP call.  per: the values of one sample's latent.
// key != nullptr with eta > 0: the noise term is drawn from the seeded stream inside the kernel (`noise` is not read); eta == 0 ignores both
// x0_hist != nullptr: the DPM-Solver++(2M) update (needs t_last; at eta > 0 its SDE form, which needs key) instead of DDIM; x0_hist must
// not overlap z or z_out
// guide != nullptr: the latent guide's blend ends the update (after either solver), right before z_out is stored
// ctl != nullptr: per-sample guidance and / or rescale (avd_cfg_control); with rescale set the launcher runs the statistics pass first
// cv != nullptr: the batch is windows of one canvas and the seeded draw is keyed by canvas position (needs key and eta > 0)
// gcv != nullptr: the guide's known noise is keyed by canvas position (needs guide; a seeded draw must then be canvas-keyed with the
// same hop: per-sample step noise under a canvas-keyed guide is refused)
// apg != nullptr: adaptive projected guidance rides in the CfgState (with or without ctl, whose rescale it excludes); the launcher runs
// its statistics pass first; eps_bytes: the bytes of a.eps, which the scratch and the momentum buffer must not overlap
struct CanvasDims {
    int64_t outer;
    int L, hop;
    int64_t inner;
};
static int check_fused_update(const char* what, const UpdateArgs& a, int64_t per, const avd_noise_key* key, const int64_t* t_last,
                              float* x0_hist, const avd_latent_guide* guide, const avd_cfg_control* ctl, UpdateKeys& k,
                              const CanvasDims* cv = nullptr, const CanvasDims* gcv = nullptr, const avd_apg_control* apg = nullptr,
                              int64_t eps_bytes = 0, const avd_slot_key* skey = nullptr) {
    AVD_REQUIRE(a.eps && a.z && a.t_now && a.t_prev && a.abar && a.z_out, AVD_EINVAL, "%s: null pointer", what);
    AVD_REQUIRE(a.eta >= 0.f && (a.eta == 0.f || a.noise || key || skey), AVD_EINVAL, "%s: eta > 0 needs a noise tensor or a noise key", what);
    AVD_REQUIRE(a.z != a.z_out, AVD_EINVAL, "%s: z_out must not alias z", what);
    AVD_REQUIRE(!t_last == !x0_hist, AVD_EINVAL, "%s: t_last and x0_hist go together (the DPM-Solver++(2M) update)", what);
    k = UpdateKeys{};
    k.dpm = x0_hist != nullptr;
    k.ds = DpmState{t_last, x0_hist};
    if (k.dpm) {
        AVD_REQUIRE(a.eta == 0.f || ((key || skey) && !a.noise), AVD_EINVAL,
                    "%s: the DPM-Solver++(2M) update with eta > 0 draws its noise from a noise key (no unseeded or explicit noise)", what);
        AVD_REQUIRE(!overlaps(x0_hist, a.z, a.B * per) && !overlaps(x0_hist, a.z_out, a.B * per), AVD_EINVAL,
                    "%s: x0_hist must not overlap z or z_out", what);
    }
    k.seeded = key && a.eta > 0.f;
    k.canvas = cv != nullptr;
    if (cv) {
        AVD_REQUIRE(k.seeded, AVD_EINVAL, "%s: the canvas-keyed draw is a seeded eta > 0 step (needs a noise key and eta > 0)", what);
        if (int rc = make_canvas_key(key, a.B, cv->outer, cv->L, cv->hop, cv->inner, k.ck)) return rc;
    } else if (k.seeded) {
        if (int rc = make_noise_key(key, a.B, k.nk)) return rc;
        AVD_REQUIRE(per < ((int64_t)1 << 34), AVD_EINVAL, "%s: a seeded sample must hold < 2^34 values", what);
    }
    AVD_REQUIRE(guide || !gcv, AVD_EINVAL, "%s: the canvas keying of a latent guide needs the guide", what);
    k.guide = guide != nullptr && !gcv;
    k.cguide = guide != nullptr && gcv;
    k.ctl = ctl != nullptr || apg != nullptr;
    if (guide || ctl || apg)
        AVD_REQUIRE(a.eta == 0.f || k.seeded, AVD_EINVAL, "%s: a guided or controlled step with eta > 0 needs a noise key", what);
    if (k.cguide) {
        AVD_REQUIRE(!k.seeded || (cv && cv->hop == gcv->hop), AVD_EINVAL,
                    "%s: under a canvas-keyed latent guide the eta > 0 noise must be canvas-keyed with the guide's hop %d (per-sample "
                    "step noise is refused)", what, gcv->hop);
        if (int rc = make_canvas_guide(guide, a.B, gcv->outer, gcv->L, gcv->hop, gcv->inner, a.z_out, x0_hist, k.cgs)) return rc;
    } else if (guide)
        if (int rc = make_guide(guide, a.B, per, a.z_out, x0_hist, k.gs)) return rc;
    if (ctl)
        if (int rc = make_cfg(ctl, a.B, per, a.z_out, x0_hist, k.cs)) return rc;
    if (apg)
        if (int rc = make_apg(apg, ctl, a.B, per, {a.z, a.z_out, x0_hist}, a.eps, eps_bytes, k.cs)) return rc;
    return AVD_OK;
}

// The slot form's checks, before any HIP call: slots == 0 is the per-sample update; otherwise `slots` must be the geometry's S and the
// update is DDIM or, with t_last / x0_hist (checked as a pair by check_fused_update; t_last is then a [B, S] table too), DPM-Solver++(2M),
// at eta == 0 with nothing else in the pack (the scope of "slot timesteps" in include/avdiff_hip.h), or at eta > 0 with a slot key
// ("clip-keyed slot noise"; skd: the key's (outer, slot_len, inner)), which at eta == 0 is not read.  cguide != nullptr ends the slot
// update in the clip-keyed latent guide's blend, at any eta (L: the sliding length its positions run over); a slot key riding along
// must carry the guide's geometry
struct SlotKeyDims {
    int64_t outer;
    int slot_len;
    int64_t inner;
};
static int check_slot_update(const char* what, const UpdateArgs& a, int slots, int S, const avd_noise_key* key,
                             const avd_latent_guide* guide, const avd_cfg_control* ctl, int canvas_hop, int guide_hop, UpdateKeys& k,
                             const avd_slot_key* skey, const SlotKeyDims& skd, const avd_clip_guide* cguide = nullptr, int L = 0,
                             const avd_clip_queues* cq = nullptr) {
    AVD_REQUIRE(slots || !skey, AVD_EINVAL, "%s: a slot key rides with slot timesteps (slots > 0)", what);
    AVD_REQUIRE(slots || !cguide, AVD_EINVAL, "%s: a clip guide rides with slot timesteps (slots > 0)", what);
    AVD_REQUIRE(slots || !cq, AVD_EINVAL, "%s: clip queues ride with slot timesteps (slots > 0)", what);
    if (!slots) return AVD_OK;
    AVD_REQUIRE(slots == S, AVD_EINVAL, "%s: slots %d must equal the geometry's %d slots along the sliding axis", what, slots, S);
    AVD_REQUIRE((a.eta == 0.f || skey) && !a.noise && !key, AVD_EINVAL,
                "%s: slot timesteps take the update at eta == 0 (no noise, no key), or at eta > 0 with a slot key", what);
    AVD_REQUIRE(!guide && !ctl && !canvas_hop && !guide_hop, AVD_EINVAL,
                "%s: slot timesteps take no latent guide, CFG control or canvas keying", what);
    AVD_REQUIRE((int64_t)a.B * S <= 0x7fffffff, AVD_EINVAL, "%s: B %d * slots %d does not fit an int", what, a.B, S);
    k.slots = true;
    k.sl = SlotTimes{S};
    k.skey = skey && a.eta > 0.f;
    if (k.skey)
        if (int rc = make_slot_key(skey, a.B, skd.outer, skd.slot_len, skd.inner, k.sk, what)) return rc;
    k.clip = cguide != nullptr;
    if (cguide) {      // L: the sliding length the positions run over (the guide's checks: include/avdiff_hip.h, "clip-keyed latent guide")
        if (int rc = make_clip_guide(cguide, a.B, skd.outer, L, S, skd.slot_len, skd.inner, {a.z_out, k.ds.x0_hist}, k.cg, what,
                                     cq ? cq->K : 1)) return rc;
        AVD_REQUIRE(!k.skey || (skey->first == cguide->first && skey->stride == cguide->stride && skey->cursor == cguide->cursor), AVD_EINVAL,
                    "%s: the slot key's first / stride / cursor must equal the clip guide's (one clip position per element)", what);
    }
    if (cq) {      // L: as the guide's; a descriptor beside neither a key that is read nor a guide is checked and changes nothing
        const int64_t canvas = k.clip ? skd.outer * k.cg.P * skd.inner : 0;
        if (int rc = make_clip_queues(what, cq, a.B, k.skey, k.clip, {a.z_out, k.ds.x0_hist}, (int64_t)a.B * skd.outer * L * skd.inner,
                                      k.clip ? k.cg.known : nullptr, k.clip ? k.cg.mask : nullptr, cq->K * canvas, canvas, k.cq)) return rc;
        k.queues = k.skey || k.clip;
    }
    return AVD_OK;
}

// Calls launch(pack...) with the kernels' whole trailing pack; the slot form's is SlotTimes, behind the DpmState if there is one and
// before the SlotKey of an eta > 0 step.
// Otherwise: the solver's state (DpmState, the NoiseKey of a seeded eta > 0 step or
// the CanvasKey of a canvas-keyed one, DpmState then that key for the SDE form, or nothing), then the guide if there is one, then the
// CFG control if there is one or, for the single-branch form, the CondOnly tag.  A canvas-keyed guide rides in the guide's place, after
// the solver states that can reach it: none, DpmState, CanvasKey, DpmState then CanvasKey (never a NoiseKey: check_fused_update).
template <class F>
static void with_update_pack(const UpdateKeys& k, bool cond_only, F launch) {
    if (k.slots) {      // a clip-keyed guide ends the slot pack
        auto qtail = [&](auto... state) {      // the clip queues end a pack that holds a slot key or a clip guide
            if constexpr (PackHas<SlotKey, decltype(state)...>::value || PackHas<ClipGuideState, decltype(state)...>::value) {
                if (k.queues) return launch(state..., k.cq);
            }
            launch(state...);
        };
        auto gtail = [&](auto... state) {
            if (k.clip) qtail(state..., k.cg);
            else qtail(state...);
        };
        auto stail = [&](auto... state) {      // a slot CFG control rides behind the key, before the guide; its momentum behind it
            if (k.scfg && k.smom) gtail(state..., k.sc, k.sm);
            else if (k.scfg) gtail(state..., k.sc);
            else gtail(state...);
        };
        if (k.dpm && k.skey) stail(k.ds, k.sl, k.sk);
        else if (k.dpm) stail(k.ds, k.sl);
        else if (k.skey) stail(k.sl, k.sk);
        else stail(k.sl);
        return;
    }
    if (k.cguide) {
        auto ctail = [&](auto... state) {
            if (cond_only) launch(state..., k.cgs, CondOnly{});
            else if (k.ctl) launch(state..., k.cgs, k.cs);
            else launch(state..., k.cgs);
        };
        if (k.dpm && k.seeded) ctail(k.ds, k.ck);
        else if (k.dpm) ctail(k.ds);
        else if (k.seeded) ctail(k.ck);
        else ctail();
        return;
    }
    auto tail = [&](auto... state) {
        if (cond_only && k.guide) launch(state..., k.gs, CondOnly{});
        else if (cond_only) launch(state..., CondOnly{});
        else if (k.guide && k.ctl) launch(state..., k.gs, k.cs);
        else if (k.guide) launch(state..., k.gs);
        else if (k.ctl) launch(state..., k.cs);
        else launch(state...);
    };
    if (k.dpm && k.seeded && k.canvas) tail(k.ds, k.ck);
    else if (k.dpm && k.seeded) tail(k.ds, k.nk);
    else if (k.dpm) tail(k.ds);
    else if (k.seeded && k.canvas) tail(k.ck);
    else if (k.seeded) tail(k.nk);
    else tail();
}

// the video launch for one pack: the whole-line kernel where the geometry allows it, the gather form otherwise
template <class... P>
static void launch_unpatch(const UpdateArgs& a, const Tube& g, hipStream_t st, P... p) {
    constexpr bool SEEDED = PackHas<NoiseKey, P...>::value || PackHas<CanvasKey, P...>::value || PackHas<SlotKey, P...>::value;
    // whole-line form: groups of tokens along w' that make up 128 bytes (or the whole row when W is shorter) of latent per (c, t, h)
    const int gt = (g.W < 32 ? g.W : 32) / g.w;
    int planes = 1;      // an APG launch parks c and d0: twice the LDS (the gather form where that does not fit)
    if constexpr (PackHas<CfgState, P...>::value) planes = pack_get<CfgState>(p...).apg ? 2 : 1;
    if constexpr (PackHas<SlotMomentum, P...>::value) planes = 2;      // a slot momentum launch likewise
    const int64_t lds = (int64_t)planes * gt * (g.D + 4) * 4;
    if (g_cfg_rows && (gt == 8 || gt == 4) && g.Wt % gt == 0 && g.D % 4 == 0 && lds <= 64 * 1024) {
        const int groups = (int)(g.per / g.D) / gt;
        hipLaunchKernelGGL((gt == 8 ? cfg_unpatch_ddim_rows_kernel<8, SEEDED, P...> : cfg_unpatch_ddim_rows_kernel<4, SEEDED, P...>),
                           dim3((unsigned)(a.B * groups)), dim3(256), (size_t)lds, st, a.eps, a.z, a.t_now, a.t_prev, a.abar,
                           a.T_train, a.guidance, a.eta, a.noise, a.z_out, g, a.B, groups, p...);
    } else {
        const int64_t total4 = (int64_t)a.B * (g.per >> 2);
        hipLaunchKernelGGL((cfg_unpatch_ddim_kernel<SEEDED, P...>), dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, a.eps, a.z,
                           a.t_now, a.t_prev, a.abar, a.T_train, a.guidance, a.eta, a.noise, a.z_out, g, a.B, total4, p...);
    }
}

// what may ride with an update: key, t_last / x0_hist, guide, ctl, apg: see check_fused_update; slots, skey, cguide, cq: see
// check_slot_update; scfg != nullptr: the call came through a *_slots_cfg entry
struct UpdateRiders {
    const avd_noise_key* key;
    const int64_t* t_last;
    float* x0_hist;
    const avd_latent_guide* guide;
    const avd_cfg_control* ctl;
    int slots;
    const avd_apg_control* apg;
    const avd_slot_key* skey;
    const avd_clip_guide* cguide;
    const avd_slot_cfg* scfg;
    const avd_clip_queues* cq;
};
// what the host body needs of a target (the statistics source rides as fused_update's SRC)
struct UpdateTarget {
    const char* what;          // the message prefix: the entry's name
    const int* tags;           // the profile labels (update_tags)
    int64_t per, half;         // one sample's latent values, and the floats of its eps rows
    int64_t eps_bytes;         // the bytes of the CFG form's eps, which scratch and momentum buffers must not overlap
    CanvasDims cv, gcv;        // the canvas keying of the draw and of the guide; hop 0: per-sample keying (the B samples are not windows)
    SlotKeyDims skd;
    int S, L;                  // the slots of the sliding axis, and its length
    SlotGeom sg;
    Tube g;                    // the video target's geometry (audio: empty)
    AudioGeom ag;              // the audio target's (video: empty)
};
// the labels of a target's launches: the CFG form's six, then the single-branch form's
enum { TAG_PLAIN, TAG_APG, TAG_CLIP, TAG_SCFG, TAG_SMOM, TAG_QUEUES, TAG_EPS, UPDATE_TAGS };
struct UpdateTags {
    int id[UPDATE_TAGS];
    UpdateTags(const char* cfg, const char* eps) {
        const char* const form[] = {"", "<apg>", "<clip guide>", "<slot cfg>", "<slot momentum>", "<clip queues>"};
        for (int i = 0; i < TAG_EPS; ++i) id[i] = prof_tag_id("%s_kernel%s", cfg, form[i]);
        id[TAG_EPS] = prof_tag_id("%s_kernel", eps);
    }
};

// The one host body of the fused updates: the checks, all before any HIP call (a slot CFG control first, then check_fused_update, then
// check_slot_update), the statistics passes a control asks for, on st, and the launch of the pack.  cond_only: the single-branch form
// (a.eps holds the cond rows alone, and no control rides).  launch(pack...) is the target's launch_unpatch / launch_untoken.
template <int SRC, class Launch>
static int fused_update(const UpdateTarget& tg, const UpdateArgs& a, const UpdateRiders& r, bool cond_only, hipStream_t st, Launch launch) {
    constexpr bool VIDEO = SRC == CFG_SRC_VIDEO;      // its kernels read float4: the alignment checks are the video target's
    SlotCfgState sc{};
    SlotMomentum sm{};
    if (r.scfg) {
        AVD_REQUIRE(r.slots > 0, AVD_EINVAL, "%s: a slot CFG control rides with slot timesteps (slots > 0)", tg.what);
        if (int rc = make_slot_cfg(r.scfg, a.B, tg.sg.S, tg.sg.per_slot, tg.per, {a.z, a.z_out, r.x0_hist}, a.eps, tg.eps_bytes, sc, sm))
            return rc;
    }
    AVD_REQUIRE(!VIDEO || aligned16(r.x0_hist), AVD_EUNSUPPORTED, "%s: x0_hist must be 16-byte aligned", tg.what);
    UpdateKeys k;
    if (int rc = check_fused_update(tg.what, a, tg.per, r.key, r.t_last, r.x0_hist, r.guide, r.ctl, k, tg.cv.hop ? &tg.cv : nullptr,
                                    tg.gcv.hop ? &tg.gcv : nullptr, r.apg, tg.eps_bytes, r.skey)) return rc;
    if (int rc = check_slot_update(tg.what, a, r.slots, tg.S, r.key, r.guide, r.ctl, tg.cv.hop, tg.gcv.hop, k, r.skey, tg.skd, r.cguide,
                                   tg.L, r.cq)) return rc;
    k.scfg = r.scfg != nullptr;
    k.sc = sc;
    k.smom = sm.buf != nullptr;
    k.sm = sm;
    const float* null_rows = a.eps + (int64_t)a.B * tg.half;
    if (r.scfg && sc.mode != SLOT_CFG_TABLE)      // video: 16-byte aligned token rows (the entry has checked eps, and per % 4 == 0)
        if (int rc = run_slot_cfg_stats<SRC>(r.scfg, sc, a.eps, null_rows, tg.half, a.t_now, a.t_prev, a.guidance, a.T_train, a.B, tg.sg,
                                             tg.g, st, SlotMomentumAt{sm.buf, sm.beta, tg.per, tg.ag.len, tg.ag.F})) return rc;
    if (r.apg) {
        AVD_REQUIRE(!VIDEO || (aligned16(a.eps) && aligned16(null_rows) && aligned16(a.z) && aligned16(a.z_out)), AVD_EUNSUPPORTED,
                    "%s: the APG statistics pass reads 16-byte aligned token rows", tg.what);
        if (int rc = run_apg_stats<SRC>(r.apg, r.ctl ? r.ctl->guidance : nullptr, a.guidance, a.eps, null_rows, tg.half, a.B, tg.per, tg.g,
                                        tg.ag, st)) return rc;
    }
    if (r.ctl && r.ctl->rescale) {
        AVD_REQUIRE(!VIDEO || (aligned16(a.eps) && aligned16(null_rows)), AVD_EUNSUPPORTED,
                    "%s: the statistics pass reads 16-byte aligned token rows", tg.what);
        if (int rc = run_cfg_stats<SRC>(r.ctl, a.eps, null_rows, tg.half, a.guidance, a.B, tg.per, tg.ag, st)) return rc;
    }
    // the fused launch of an APG step is timed apart, as are the clip-guided slot update, the slot update under a slot CFG control and
    // under its momentum, and the keyed or guided update of a clip batch; the work: bytes per latent element
    const int tag = cond_only ? TAG_EPS : k.queues ? TAG_QUEUES : k.smom ? TAG_SMOM : r.scfg ? TAG_SCFG : r.apg ? TAG_APG
                                                                                             : r.cguide ? TAG_CLIP : TAG_PLAIN;
    const double bytes = cond_only ? 12.0 : (r.apg && r.apg->momentum_buf) || k.smom ? 24.0 : r.cguide ? (r.cguide->mask ? 24.0 : 20.0) : 16.0;
    ProfScope prof(tg.tags[tag], bytes * (double)a.B * tg.per, st);
    with_update_pack(k, cond_only, launch);
    AVD_CHECK_LAUNCH(tg.what);
    return AVD_OK;
}

// The video target's geometry.  canvas_hop != 0: the B samples are consecutive windows of one canvas, canvas_hop positions apart along
// T (F for audio), and the seeded draw is keyed by canvas position (CanvasDims); guide_hop likewise for the guide's known noise
static int unpatch_update(const char* what, bool cond_only, const UpdateArgs& a, int C, int T, int H, int W, int t, int h, int w,
                          hipStream_t st, const UpdateRiders& r, int canvas_hop, int guide_hop) {
    AVD_REQUIRE(a.B > 0 && a.T_train > 0, AVD_EINVAL, "%s: bad dims", what);
    Tube g;
    if (int rc = make_tube(g, C, T, H, W, t, h, w)) return rc;
    static const UpdateTags tags("cfg_unpatch_ddim", "eps_unpatch_ddim");
    const UpdateTarget tg{what, tags.id, g.per, g.per, (int64_t)2 * a.B * g.per * 4, CanvasDims{C, T, canvas_hop, (int64_t)H * W},
                          CanvasDims{C, T, guide_hop, (int64_t)H * W}, SlotKeyDims{C, t, (int64_t)H * W}, T / t, T,
                          SlotGeom{T / t, (int64_t)C * t * H * W, (int64_t)g.Ht * g.Wt * g.D, (int64_t)t * H * W}, g, AudioGeom{}};
    return fused_update<CFG_SRC_VIDEO>(tg, a, r, cond_only, st, [&](auto... p) { launch_unpatch(a, g, st, p...); });
}
int cfg_unpatch_ddim_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                         const float* abar, int T_train, float guidance, float eta, const float* noise, float* z_out,
                         int B, int C, int T, int H, int W, int t, int h, int w, hipStream_t st, const avd_noise_key* key,
                         const int64_t* t_last, float* x0_hist, const avd_latent_guide* guide, const avd_cfg_control* ctl,
                         int canvas_hop, int guide_hop, int slots, const avd_apg_control* apg, const avd_slot_key* skey = nullptr,
                         const avd_clip_guide* cguide = nullptr, const avd_slot_cfg* scfg = nullptr, const avd_clip_queues* cq = nullptr) {
    return unpatch_update("cfg_unpatch_ddim", false, UpdateArgs{eps2, z, t_now, t_prev, abar, T_train, guidance, eta, noise, z_out, B}, C, T,
                          H, W, t, h, w, st, UpdateRiders{key, t_last, x0_hist, guide, ctl, slots, apg, skey, cguide, scfg, cq}, canvas_hop,
                          guide_hop);
}
// The single-branch fused update of a cond-only step: eps1 = [B, Nv, D], the conditional prediction alone (12 B per latent element:
// one eps stream less than the CFG form).  key, t_last / x0_hist and guide as in cfg_unpatch_ddim_f32; the same rows / gather choice.
int eps_unpatch_ddim_f32(const float* eps1, const float* z, const int64_t* t_now, const int64_t* t_prev, const float* abar, int T_train,
                         float eta, const float* noise, float* z_out, int B, int C, int T, int H, int W, int t, int h, int w,
                         hipStream_t st, const avd_noise_key* key, const int64_t* t_last, float* x0_hist, const avd_latent_guide* guide,
                         int canvas_hop, int guide_hop) {
    return unpatch_update("eps_unpatch_ddim", true, UpdateArgs{eps1, z, t_now, t_prev, abar, T_train, 0.f, eta, noise, z_out, B}, C, T, H, W,
                          t, h, w, st, UpdateRiders{key, t_last, x0_hist, guide}, canvas_hop, guide_hop);
}

// ------------------------------------------------------------------ fused CFG + overlap-add + DDIM (audio target)
template <bool SEEDED, class... Key>      // as cfg_unpatch_ddim_kernel; one generator call per element (e = c F + f of the sample)
__global__ void cfg_untoken_ddim_audio_kernel(const float* __restrict__ eps2, const float* __restrict__ z,
                                              const int64_t* __restrict__ t_now, const int64_t* __restrict__ t_prev,
                                              const float* __restrict__ abar, int T_train, float guidance, float eta,
                                              const float* __restrict__ noise, float* __restrict__ z_out, int B, int Ca,
                                              int F, int len, int stride, int Na, Key... nk) {
    constexpr bool CTL = PackHas<CfgState, Key...>::value, COND = PackHas<CondOnly, Key...>::value;
    static_assert(PackOk<SEEDED, Key...>::value, "not a pack of the fused update kernels (see PackOk)");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * Ca * F) return;
    const int f = (int)(i % F);
    const int c = (int)((i / F) % Ca);
    const int b = (int)(i / ((int64_t)F * Ca));
    const int L = (Na - 1) * stride + len;
    const int D = Ca * len;
    constexpr bool SLOT = PackHas<SlotTimes, Key...>::value;
    [[maybe_unused]] int tb = b;      // the entry of t_now / t_prev this lane steps with
    if constexpr (SLOT) {             // per lane (stride == len): chunk f / len, the uncovered tail follows the last chunk; a held slot keeps z
        const int sl = f / len;
        tb = b * Na + (sl > Na - 1 ? Na - 1 : sl);
        if (t_now[tb] == t_prev[tb]) {
            z_out[i] = z[i];
            return;
        }
    }
    [[maybe_unused]] CfgCoef cc{guidance, 0.f, 1.f};
    if constexpr (CTL) cc = cfg_coef(pack_get<CfgState>(nk...), guidance, b);
    constexpr bool SCFG = PackHas<SlotCfgState, Key...>::value;
    [[maybe_unused]] SlotCfgCoef sf{guidance, 0.f, 1.f, 0.f, 0.f, false};      // the slot control's coefficients, by tb
    if constexpr (SCFG) sf = slot_cfg_coef(pack_get<SlotCfgState>(nk...), t_now, T_train, guidance, tb);
    float e = 0.f;
    [[maybe_unused]] bool apg = false;      // a run-time branch of the CTL instantiations: the launch carries an APG part
    if constexpr (CTL) {
        const CfgState cs = pack_get<CfgState>(nk...);
        apg = cs.apg != nullptr;
        if (apg) {      // two separate overlap-add means (zero on the uncovered tail), then items 2 and 5 of the contract
            const float cv = f < L ? ola_gather(eps2 + (int64_t)b * Na * D, D, c, len, stride, Na, f) : 0.f;
            const float uv = f < L ? ola_gather(eps2 + ((int64_t)B + b) * Na * D, D, c, len, stride, Na, f) : 0.f;
            const float dv = apg_dir(apg_d0(cv, uv), cs.apg_beta, cs.apg_mom ? cs.apg_mom[i] : 0.f);
            if (cs.apg_mom) cs.apg_mom[i] = dv;
            e = apg_eps(cv, dv, cs.apg[(int64_t)b * 4 + 2], cs.apg[(int64_t)b * 4 + 1]);
        }
    }
    if constexpr (COND) {
        // the single-branch form: the overlap-add mean of the cond tokens, the arithmetic of audio_untok_kernel
        if (f < L) e = ola_gather(eps2 + (int64_t)b * Na * D, D, c, len, stride, Na, f);
    } else if (!(CTL && apg) && f < L) {
        // CFG combine is linear, but the reference combines per token first and overlap-adds after:
        // gather both halves with the same window order, combine per window
        int n_hi = f / stride;
        if (n_hi > Na - 1) n_hi = Na - 1;
        int n_lo = (f - len + 1 <= 0) ? 0 : (f - len + stride) / stride;
        float acc = 0.f, cnt = 0.f;
        const float* tc = eps2 + (int64_t)b * Na * D;
        const float* tn = eps2 + ((int64_t)B + b) * Na * D;
        for (int n = n_lo; n <= n_hi; ++n) {
            const int64_t o = (int64_t)n * D + c * len + (f - n * stride);
            const float vn = tn[o];
            acc += cfg_combine(tc[o], vn, SCFG ? sf.g : CTL ? cc.g : guidance);
            cnt += 1.f;
        }
        e = acc / fmaxf(cnt, 1e-8f);
        if constexpr (SCFG) {      // the slot's token alone (stride == len: one window); the uncovered tail keeps eps = 0
            if (sf.apg) {          // the two means of the per-sample APG branch
                const float cv = ola_gather(tc, D, c, len, stride, Na, f), uv = ola_gather(tn, D, c, len, stride, Na, f);
                if constexpr (PackHas<SlotMomentum, Key...>::value) {      // "slot APG momentum": element i is this lane's latent address
                    const SlotMomentum sm = pack_get<SlotMomentum>(nk...);
                    const float dv = apg_dir(apg_d0(cv, uv), sm.beta, sm.buf[i]);
                    sm.buf[i] = dv;
                    e = apg_eps(cv, dv, sf.w, sf.k);
                } else e = apg_eps(cv, apg_d0(cv, uv), sf.w, sf.k);
            } else e = cfg_rescale(e, sf.phi, sf.s);
        }
    }
    if constexpr (CTL) e = cfg_rescale(e, cc.phi, cc.s);      // r(y) on the whole latent, the zero pad included
    // element (c, f) of sample b: position f of the sliding axis, element c of its slice (inner == 1)
    const UpdateLane ln{b, tb, i, i - (int64_t)b * Ca * F, c, f, 0, 1};
    update_tail<1, SEEDED>(ln, f32x4{z[i], 0.f, 0.f, 0.f}, f32x4{e, 0.f, 0.f, 0.f}, nullptr, t_now, t_prev, abar, T_train, eta, noise, z_out,
                           nk...);
}

template <class... P>
static void launch_untoken(const UpdateArgs& a, const AudioGeom& ag, hipStream_t st, P... p) {
    constexpr bool SEEDED = PackHas<NoiseKey, P...>::value || PackHas<CanvasKey, P...>::value || PackHas<SlotKey, P...>::value;
    const int64_t n = (int64_t)a.B * ag.Ca * ag.F;
    hipLaunchKernelGGL((cfg_untoken_ddim_audio_kernel<SEEDED, P...>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.eps, a.z,
                       a.t_now, a.t_prev, a.abar, a.T_train, a.guidance, a.eta, a.noise, a.z_out, a.B, ag.Ca, ag.F, ag.len, ag.stride,
                       ag.Na, p...);
}

// the audio target's geometry; canvas_hop, guide_hop: as unpatch_update
static int untoken_update(const char* what, bool cond_only, const UpdateArgs& a, int Ca, int F, int len, int stride, hipStream_t st,
                          const UpdateRiders& r, int canvas_hop, int guide_hop) {
    AVD_REQUIRE(a.B > 0 && Ca > 0 && a.T_train > 0, AVD_EINVAL, "%s: bad dims", what);
    AVD_REQUIRE(len > 0 && stride > 0 && F >= len, AVD_EUNSUPPORTED, "%s: bad chunking", what);
    AVD_REQUIRE(!r.slots || stride == len, AVD_EUNSUPPORTED, "%s: slot timesteps need non-overlapping chunks (stride %d == len %d)", what,
                stride, len);
    const AudioGeom ag{Ca, F, len, stride, audio_na(F, len, stride)};
    const int64_t half = (int64_t)ag.Na * Ca * len;      // one sample's token rows
    static const UpdateTags tags("cfg_untoken_ddim_audio", "eps_untoken_ddim_audio");
    const UpdateTarget tg{what, tags.id, (int64_t)Ca * F, half, 2 * a.B * half * 4, CanvasDims{Ca, F, canvas_hop, 1},
                          CanvasDims{Ca, F, guide_hop, 1}, SlotKeyDims{Ca, len, 1}, ag.Na, F,
                          SlotGeom{ag.Na, (int64_t)Ca * len, (int64_t)Ca * len, 0}, Tube{}, ag};
    return fused_update<CFG_SRC_AUDIO>(tg, a, r, cond_only, st, [&](auto... p) { launch_untoken(a, ag, st, p...); });
}
// key, t_last, x0_hist, guide, ctl: as cfg_unpatch_ddim_f32
int cfg_untoken_ddim_audio_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                               const float* abar, int T_train, float guidance, float eta, const float* noise,
                               float* z_out, int B, int Ca, int F, int len, int stride, hipStream_t st, const avd_noise_key* key,
                               const int64_t* t_last, float* x0_hist, const avd_latent_guide* guide, const avd_cfg_control* ctl,
                               int canvas_hop, int guide_hop, int slots, const avd_apg_control* apg, const avd_slot_key* skey = nullptr,
                               const avd_clip_guide* cguide = nullptr, const avd_slot_cfg* scfg = nullptr,
                               const avd_clip_queues* cq = nullptr) {
    return untoken_update("cfg_untoken_ddim_audio", false, UpdateArgs{eps2, z, t_now, t_prev, abar, T_train, guidance, eta, noise, z_out, B},
                          Ca, F, len, stride, st, UpdateRiders{key, t_last, x0_hist, guide, ctl, slots, apg, skey, cguide, scfg, cq},
                          canvas_hop, guide_hop);
}
// the single-branch form (eps1 = [B, Na, Ca * len]): as eps_unpatch_ddim_f32
int eps_untoken_ddim_audio_f32(const float* eps1, const float* z, const int64_t* t_now, const int64_t* t_prev, const float* abar,
                               int T_train, float eta, const float* noise, float* z_out, int B, int Ca, int F, int len, int stride,
                               hipStream_t st, const avd_noise_key* key, const int64_t* t_last, float* x0_hist,
                               const avd_latent_guide* guide, int canvas_hop, int guide_hop) {
    return untoken_update("eps_untoken_ddim_audio", true, UpdateArgs{eps1, z, t_now, t_prev, abar, T_train, 0.f, eta, noise, z_out, B}, Ca, F,
                          len, stride, st, UpdateRiders{key, t_last, x0_hist, guide}, canvas_hop, guide_hop);
}

// ------------------------------------------------------------------ CFG-stacked sequence assembly
// X2[2B, N, d]: the GEMM has already written adapter(target tokens) into the cond half's target rows,
// columns [0, d-tdim).  This pass fills everything else in one sweep.
__global__ __launch_bounds__(256) void assemble_kernel(float* __restrict__ X2, const float* __restrict__ temb,
                                                       const float* __restrict__ Xp, int B, int N, int d, int tdim,
                                                       int Nt, int Np, int target_first, int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int d4 = d >> 2;
    const int col = (int)(i % d4) * 4;
    const int64_t row = i / d4;
    const int n = (int)(row % N);
    const int bb = (int)(row / N);          // 0..2B-1
    const int half = bb >= B, b = half ? bb - B : bb;
    const int t0 = target_first ? 0 : Np;   // first target row
    const bool is_t = n >= t0 && n < t0 + Nt;
    f32x4 v;
    if (is_t) {
        if (col >= d - tdim) {
            v = *reinterpret_cast<const f32x4*>(temb + (int64_t)b * tdim + (col - (d - tdim)));
        } else {
            if (!half) return;               // already in place
            v = *reinterpret_cast<const f32x4*>(X2 + ((int64_t)b * N + n) * d + col);
        }
    } else {
        const int np = target_first ? n - Nt : n;
        v = half ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(Xp + ((int64_t)b * Np + np) * d + col);
    }
    *reinterpret_cast<f32x4*>(X2 + row * d + col) = v;
}

int assemble_f32(float* X2, const float* temb, const float* Xp, int B, int N, int d, int tdim, int Nt, int Np,
                 int target_first, hipStream_t st) {
    const int64_t total4 = (int64_t)2 * B * N * (d >> 2);
    static const int tag = prof_tag_id("assemble_kernel");
    ProfScope prof(tag, 4.0 * (2.0 * B * N * d + (double)B * Nt * (d - tdim) + (double)B * Np * d), st);
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, X2, temb, Xp, B, N, d,
                       tdim, Nt, Np, target_first, total4);
    AVD_CHECK_LAUNCH("assemble");
    return AVD_OK;
}

// Fused form for the sampler's concat embedding (sample_clip.py:59-70, 371, 377): one wave per row of X2 fills everything the
// adapter GEMM did not write — the sinusoidal timestep columns are computed in place (no [B, tdim] buffer, no separate
// kernel), the null half's target rows are copied from the cond half, prompt rows come from Xp / zeros — and, while the row
// is in registers, its sum of squares goes to ss[row] (the table the first folded RMSNorm reads: no rowss pass).
// A SlotMap ending the arguments (an empty pack otherwise: the per-sample instantiation keeps its argument layout and code) selects the
// slot form ("slot timesteps"): t_now is [B, S] and target row n embeds t_now[b, (n - first target row) / tok], in both halves.
struct SlotMap {
    int S, tok;      // slots per sample, target tokens per slot (video: Ht * Wt, audio: 1)
};
template <class... Slot>
__global__ __launch_bounds__(256) void assemble_rows_kernel(float* __restrict__ X2, const int64_t* __restrict__ t_now,
                                                            const float* __restrict__ freqs, const float* __restrict__ Xp,
                                                            float* __restrict__ ss, int B, int N, int d, int tdim, int Nt, int Np,
                                                            int target_first, float neg_log_mp, RowSegs seg, Slot... sl) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= seg.rows()) return;
    int n, bb;
    seg.locate(row, bb, n);
    const int half = bb >= B, b = half ? bb - B : bb;
    const int t0 = target_first ? 0 : Np;
    const bool is_t = n >= t0 && n < t0 + Nt;
    const int da = d - tdim, th = tdim >> 1;
    float tf = 0.f;
    if constexpr (sizeof...(Slot) != 0) {
        const SlotMap sm = SlotMap(sl...);
        if (is_t) tf = (float)t_now[b * sm.S + (n - t0) / sm.tok];
    } else {
        tf = is_t ? (float)t_now[b] : 0.f;
    }
    float acc = 0.f;
    for (int col = lane * 4; col < d; col += 256) {
        f32x4 v;
        bool store = true;
        if (is_t) {
            if (col >= da) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = col - da + e;
                    float x = 0.f;
                    if (c < 2 * th) {
                        const int k = c < th ? c : c - th;
                        const float f = freqs ? freqs[k] : expf(neg_log_mp * (float)k / (float)th);
                        const float a = tf * f;
                        x = c < th ? cosf(a) : sinf(a);
                    }
                    v[e] = x;
                }
            } else {
                v = *reinterpret_cast<const f32x4*>(X2 + ((int64_t)b * N + n) * d + col);      // the adapter GEMM's output (cond half)
                store = half != 0;
            }
        } else {
            const int np = target_first ? n - Nt : n;
            v = half ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(Xp + ((int64_t)b * Np + np) * d + col);
        }
        if (store) *reinterpret_cast<f32x4*>(X2 + row * d + col) = v;
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    acc = wave_sum(acc);
    if (ss && lane == 0) ss[row] = acc;
}

// short_null (null = the plain [2B, N, d] layout): the caller's two-segment layout — target rows first, B cond samples of N rows, then B
// null samples that keep ONE of their Np prompt rows (they are all the zero row): Nt + 1 rows each (composite.hip)
int assemble_rows_f32(float* X2, const int64_t* t_now, const float* freqs, const float* Xp, float* ss, int B, int N, int d, int tdim,
                      int Nt, int Np, int target_first, float max_period, hipStream_t st, const RowSegs* short_null, int slots,
                      int slot_tok) {
    AVD_REQUIRE(!slots || (slot_tok > 0 && (int64_t)slots * slot_tok == Nt), AVD_EINVAL,
                "assemble_rows: %d slots of %d tokens are not the %d target rows", slots, slot_tok, Nt);
    AVD_REQUIRE(!short_null || (target_first && Np >= 1 && short_null->samples[0] == B && short_null->samples[1] == B && short_null->tok[0] == N &&
                                short_null->tok[1] == Nt + 1 && short_null->m0 == (int64_t)B * N), AVD_EINVAL,
                "assemble_rows: a short null half is B samples of N rows, then B of the target rows and one prompt row behind them");
    const RowSegs seg = short_null ? *short_null : RowSegs::uniform(2 * B, N);
    const int64_t rows = seg.rows();
    static const int tag = prof_tag_id("assemble_rows_kernel");
    ProfScope prof(tag, 4.0 * ((double)rows * d + (double)B * Nt * (d - tdim) + (double)B * Np * d), st);
    if (slots)
        hipLaunchKernelGGL(assemble_rows_kernel<SlotMap>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X2, t_now, freqs, Xp, ss, B, N,
                           d, tdim, Nt, Np, target_first, -(float)log((double)max_period), seg, SlotMap{slots, slot_tok});
    else
        hipLaunchKernelGGL(assemble_rows_kernel<>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X2, t_now, freqs, Xp, ss, B, N, d, tdim,
                           Nt, Np, target_first, -(float)log((double)max_period), seg);
    AVD_CHECK_LAUNCH("assemble_rows");
    return AVD_OK;
}

// The k and v rows of a null CFG sample's one prompt row (token `src` of samples first_sample .. of the qkv3 image), copied into key
// slots src + 1 .. n_keys - 1 of the same (sample, head): the attention then reads the n_keys keys of the full layout, with the values
// the in_proj GEMM would have written there (the duplicate rows' inputs are equal, so are their k and v).  A row is three planes of
// eight 16-byte chunks, chunk c at slot c ^ qkv3_swizzle(part, token): the copy re-applies the swizzle of the slot it fills.
// One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void qkv3_replicate_kernel(unsigned char* __restrict__ img, int Bt, int H, int Npad, int first_sample,
                                                             int n_samples, int src, int n_keys) {
    const int dup = n_keys - 1 - src;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)2 * n_samples * H * dup * 24;
    if (i >= total) return;
    const int c = (int)(i % 8), plane = (int)(i / 8 % 3);
    int64_t r = i / 24;
    const int j = (int)(r % dup);
    r /= dup;
    const int h = (int)(r % H);
    r /= H;
    const int b = (int)(r % n_samples), part = 1 + (int)(r / n_samples);
    unsigned char* base = img + (((int64_t)part * Bt + first_sample + b) * H + h) * (int64_t)Npad * QKV3_ROWB;
    const int dst = src + 1 + j;
    const u32x4 v = *reinterpret_cast<const u32x4*>(base + (int64_t)src * QKV3_ROWB + plane * 128 + ((c ^ qkv3_swizzle(part, src)) << 4));
    *reinterpret_cast<u32x4*>(base + (int64_t)dst * QKV3_ROWB + plane * 128 + ((c ^ qkv3_swizzle(part, dst)) << 4)) = v;
}

int qkv3_replicate(void* img, int img_samples, int H, int n_keys, int first_sample, int n_samples, int src, hipStream_t st) {
    AVD_REQUIRE(img && aligned16(img), AVD_EINVAL, "qkv3_replicate: null or misaligned image");
    AVD_REQUIRE(H > 0 && n_keys > 0 && src >= 0 && src < n_keys && first_sample >= 0 && n_samples > 0 && first_sample + n_samples <= img_samples,
                AVD_EINVAL, "qkv3_replicate: bad geometry (samples %d + %d of %d, token %d of %d keys)", first_sample, n_samples, img_samples,
                src, n_keys);
    const int dup = n_keys - 1 - src;
    if (dup == 0) return AVD_OK;
    const int64_t total = (int64_t)2 * n_samples * H * dup * 24;
    AVD_REQUIRE((total + 255) / 256 < (1ll << 31), AVD_EUNSUPPORTED, "qkv3_replicate: grid too large");
    static const int tag = prof_tag_id("qkv3_replicate_kernel");
    ProfScope prof(tag, 32.0 * (double)total, st);
    hipLaunchKernelGGL(qkv3_replicate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, static_cast<unsigned char*>(img),
                       img_samples, H, qkv3_npad(n_keys), first_sample, n_samples, src, n_keys);
    AVD_CHECK_LAUNCH("qkv3_replicate");
    return AVD_OK;
}

// ------------------------------------------------------------------ single-branch sequence assembly (cond-only steps)
// X1[B, N, d]: the cond half of the CFG-stacked sequence alone.  Both kernels write, per cond row, what their two-branch forms above
// write there — the same value expressions, so X1 and ss are bit-identical to the cond half of X2 and of its ss — and handle B * N
// rows: no null rows, no copies of the target rows.
__global__ __launch_bounds__(256) void assemble_cond_kernel(float* __restrict__ X1, const float* __restrict__ temb,
                                                            const float* __restrict__ Xp, int B, int N, int d, int tdim, int Nt,
                                                            int Np, int target_first, int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int d4 = d >> 2;
    const int col = (int)(i % d4) * 4;
    const int64_t row = i / d4;
    const int n = (int)(row % N);
    const int b = (int)(row / N);           // 0..B-1
    const int t0 = target_first ? 0 : Np;   // first target row
    const bool is_t = n >= t0 && n < t0 + Nt;
    f32x4 v;
    if (is_t) {
        if (col < d - tdim) return;          // the adapter GEMM's output: already in place
        v = *reinterpret_cast<const f32x4*>(temb + (int64_t)b * tdim + (col - (d - tdim)));
    } else {
        const int np = target_first ? n - Nt : n;
        v = *reinterpret_cast<const f32x4*>(Xp + ((int64_t)b * Np + np) * d + col);
    }
    *reinterpret_cast<f32x4*>(X1 + row * d + col) = v;
}

int assemble_cond_f32(float* X1, const float* temb, const float* Xp, int B, int N, int d, int tdim, int Nt, int Np, int target_first,
                      hipStream_t st) {
    const int64_t total4 = (int64_t)B * N * (d >> 2);
    static const int tag = prof_tag_id("assemble_cond_kernel");
    ProfScope prof(tag, 4.0 * 2.0 * ((double)B * Nt * tdim + (double)B * Np * d), st);
    hipLaunchKernelGGL(assemble_cond_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, X1, temb, Xp, B, N, d, tdim, Nt, Np,
                       target_first, total4);
    AVD_CHECK_LAUNCH("assemble_cond");
    return AVD_OK;
}

__global__ __launch_bounds__(256) void assemble_rows_cond_kernel(float* __restrict__ X1, const int64_t* __restrict__ t_now,
                                                                 const float* __restrict__ freqs, const float* __restrict__ Xp,
                                                                 float* __restrict__ ss, int B, int N, int d, int tdim, int Nt, int Np,
                                                                 int target_first, float neg_log_mp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B * N) return;
    const int n = (int)(row % N);
    const int b = (int)(row / N);
    const int t0 = target_first ? 0 : Np;
    const bool is_t = n >= t0 && n < t0 + Nt;
    const int da = d - tdim, th = tdim >> 1;
    const float tf = is_t ? (float)t_now[b] : 0.f;
    float acc = 0.f;
    for (int col = lane * 4; col < d; col += 256) {
        f32x4 v;
        bool store = true;
        if (is_t) {
            if (col >= da) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = col - da + e;
                    float x = 0.f;
                    if (c < 2 * th) {
                        const int k = c < th ? c : c - th;
                        const float f = freqs ? freqs[k] : expf(neg_log_mp * (float)k / (float)th);
                        const float a = tf * f;
                        x = c < th ? cosf(a) : sinf(a);
                    }
                    v[e] = x;
                }
            } else {
                v = *reinterpret_cast<const f32x4*>(X1 + row * d + col);      // the adapter GEMM's output, in place
                store = false;
            }
        } else {
            const int np = target_first ? n - Nt : n;
            v = *reinterpret_cast<const f32x4*>(Xp + ((int64_t)b * Np + np) * d + col);
        }
        if (store) *reinterpret_cast<f32x4*>(X1 + row * d + col) = v;
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    acc = wave_sum(acc);
    if (ss && lane == 0) ss[row] = acc;
}

int assemble_rows_cond_f32(float* X1, const int64_t* t_now, const float* freqs, const float* Xp, float* ss, int B, int N, int d,
                           int tdim, int Nt, int Np, int target_first, float max_period, hipStream_t st) {
    const int64_t rows = (int64_t)B * N;
    static const int tag = prof_tag_id("assemble_rows_cond_kernel");
    ProfScope prof(tag, 4.0 * ((double)B * N * d + (double)B * Np * d), st);
    hipLaunchKernelGGL(assemble_rows_cond_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X1, t_now, freqs, Xp, ss, B, N, d,
                       tdim, Nt, Np, target_first, -(float)log((double)max_period));
    AVD_CHECK_LAUNCH("assemble_rows_cond");
    return AVD_OK;
}

// ------------------------------------------------------------------ device-side schedule cursor
__global__ void sched_advance_kernel(const int64_t* __restrict__ sched, int n_sched, int32_t* cursor,
                                     int64_t* __restrict__ t_now, int64_t* __restrict__ t_prev, int B) {
    __shared__ int cur;
    if (threadIdx.x == 0) cur = *cursor;
    __syncthreads();
    int i = cur;
    if (i < 0) i = 0;
    if (i > n_sched - 2) i = n_sched - 2;
    const int64_t a = sched[i], p = sched[i + 1];
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        t_now[b] = a;
        t_prev[b] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) *cursor = cur + 1;
}

// as sched_advance_kernel, and t_last[b] = the entry before t_now (-1 at the start of the schedule, and after an up-jump of a
// resampling schedule, where that entry does not lie above t_now): the multistep solvers' history
__global__ void sched_advance_ms_kernel(const int64_t* __restrict__ sched, int n_sched, int32_t* cursor, int64_t* __restrict__ t_last,
                                        int64_t* __restrict__ t_now, int64_t* __restrict__ t_prev, int B) {
    __shared__ int cur;
    if (threadIdx.x == 0) cur = *cursor;
    __syncthreads();
    int i = cur;
    if (i < 0) i = 0;
    if (i > n_sched - 2) i = n_sched - 2;
    const int64_t a = sched[i], p = sched[i + 1];
    const int64_t l = i > 0 && sched[i - 1] > a ? sched[i - 1] : -1;      // an entry at or below t_now: we have just jumped up, no history
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        t_last[b] = l;
        t_now[b] = a;
        t_prev[b] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) *cursor = cur + 1;
}

}  // namespace avd

using namespace avd;

extern "C" int avd_timestep_embedding_f32(const int64_t* t, const float* freqs, float* out, int B, int dim,
                                          float max_period, avd_stream_t stream) {
    return temb_f32(t, freqs, out, B, dim, max_period, static_cast<hipStream_t>(stream));
}
extern "C" int avd_tube_patch_f32(const float* z, float* tok, int B, int C, int T, int H, int W, int t, int h, int w,
                                  avd_stream_t stream) {
    AVD_REQUIRE(aligned16(z) && aligned16(tok), AVD_EUNSUPPORTED, "tube_patch: pointers must be 16-byte aligned");
    return tube_patch_f32(z, tok, B, C, T, H, W, t, h, w, static_cast<hipStream_t>(stream));
}
extern "C" int avd_tube_unpatch_f32(const float* tok, float* z, int B, int C, int T, int H, int W, int t, int h, int w,
                                    avd_stream_t stream) {
    AVD_REQUIRE(aligned16(z) && aligned16(tok), AVD_EUNSUPPORTED, "tube_unpatch: pointers must be 16-byte aligned");
    return tube_unpatch_f32(tok, z, B, C, T, H, W, t, h, w, static_cast<hipStream_t>(stream));
}
extern "C" int avd_audio_tokens_f32(const float* z, float* tok, int B, int Ca, int F, int len, int stride,
                                    avd_stream_t stream) {
    return audio_tokens_f32(z, tok, B, Ca, F, len, stride, static_cast<hipStream_t>(stream));
}
extern "C" int avd_audio_untokens_f32(const float* tok, const float* window, float* z, int B, int Ca, int F, int len, int stride,
                                      avd_stream_t stream) {
    return audio_untokens_f32(tok, window, z, B, Ca, F, len, stride, static_cast<hipStream_t>(stream));
}
extern "C" int avd_ddim_step_f32(const float* x_t, const float* eps_hat, const int64_t* t_now, const int64_t* t_prev,
                                 const float* alpha_bar, int T_train, float eta, const float* noise, float* x_prev,
                                 int B, int64_t per_sample, avd_stream_t stream) {
    return ddim_step_f32(x_t, eps_hat, t_now, t_prev, alpha_bar, T_train, eta, noise, x_prev, B, per_sample,
                         static_cast<hipStream_t>(stream));
}
extern "C" int avd_cfg_unpatch_ddim_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                        const float* alpha_bar, int T_train, float guidance, float eta,
                                        const float* noise, float* z_out, int B, int C, int T, int H, int W, int t,
                                        int h, int w, avd_stream_t stream) {
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out) && (!noise || aligned16(noise)), AVD_EUNSUPPORTED,
                "cfg_unpatch_ddim: pointers must be 16-byte aligned");
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, noise, z_out, B, C, T, H, W, t,
                                h, w, static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr);
}
extern "C" int avd_cfg_unpatch_ddim_slots_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                              const float* alpha_bar, int T_train, float guidance, int slots, float* z_out, int B, int C,
                                              int T, int H, int W, int t, int h, int w, avd_stream_t stream) {
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out), AVD_EUNSUPPORTED,
                "cfg_unpatch_ddim_slots: pointers must be 16-byte aligned");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_unpatch_ddim_slots: slots must be > 0 (got %d)", slots);
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, 0.f, nullptr, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, slots, nullptr);
}
extern "C" int avd_cfg_untoken_ddim_audio_slots_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                                    const float* alpha_bar, int T_train, float guidance, int slots, float* z_out, int B,
                                                    int Ca, int F, int len, int stride, avd_stream_t stream) {
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_untoken_ddim_audio_slots: slots must be > 0 (got %d)", slots);
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, 0.f, nullptr, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, slots, nullptr);
}
extern "C" int avd_fifo_shift_f32(const avd_noise_key* key, int64_t t, int64_t c, const float* z_in, float* z_out, float* popped, int B,
                                  int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream) {
    return fifo_shift_f32(key, t, c, z_in, z_out, popped, B, outer, slots, slot_len, inner, static_cast<hipStream_t>(stream));
}
// the slot forms of the DPM-Solver++(2M) update ("slot timesteps" in the header): t_last, t_now, t_prev are [B, slots] tables
extern "C" int avd_cfg_unpatch_dpmpp_2m_slots_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                  const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, int slots,
                                                  float* x0_hist, float* z_out, int B, int C, int T, int H, int W, int t, int h, int w,
                                                  avd_stream_t stream) {
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out), AVD_EUNSUPPORTED,
                "cfg_unpatch_dpmpp_2m_slots: pointers must be 16-byte aligned");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_unpatch_dpmpp_2m_slots: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(t_last && x0_hist, AVD_EINVAL, "cfg_unpatch_dpmpp_2m_slots: null t_last or x0_hist");
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, 0.f, nullptr, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr);
}
extern "C" int avd_cfg_untoken_dpmpp_2m_audio_slots_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                        const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance,
                                                        int slots, float* x0_hist, float* z_out, int B, int Ca, int F, int len, int stride,
                                                        avd_stream_t stream) {
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_untoken_dpmpp_2m_audio_slots: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(t_last && x0_hist, AVD_EINVAL, "cfg_untoken_dpmpp_2m_audio_slots: null t_last or x0_hist");
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, 0.f, nullptr, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr);
}
// the slot forms at eta > 0 ("clip-keyed slot noise" in the header): the key is required, and read only when eta > 0; t_last / x0_hist
// both null = DDIM, both set = the SDE form of the DPM-Solver++(2M) slot update
extern "C" int avd_cfg_unpatch_ddim_slots_seeded_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                     const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                                     const avd_slot_key* key, int slots, float* x0_hist, float* z_out, int B, int C, int T,
                                                     int H, int W, int t, int h, int w, avd_stream_t stream) {
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out), AVD_EUNSUPPORTED,
                "cfg_unpatch_ddim_slots_seeded: pointers must be 16-byte aligned");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_unpatch_ddim_slots_seeded: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(key, AVD_EINVAL, "cfg_unpatch_ddim_slots_seeded: null slot key");
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr, key);
}
extern "C" int avd_cfg_untoken_ddim_audio_slots_seeded_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                           const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance,
                                                           float eta, const avd_slot_key* key, int slots, float* x0_hist, float* z_out,
                                                           int B, int Ca, int F, int len, int stride, avd_stream_t stream) {
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_seeded: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(key, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_seeded: null slot key");
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr, key);
}
// the slot forms under a clip-keyed latent guide ("clip-keyed latent guide" in the header): the seeded entries' arguments and the guide;
// the key is read at eta > 0 only and may be null at eta == 0
extern "C" int avd_cfg_unpatch_ddim_slots_guided_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                     const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                                     const avd_slot_key* key, const avd_clip_guide* guide, int slots, float* x0_hist,
                                                     float* z_out, int B, int C, int T, int H, int W, int t, int h, int w,
                                                     avd_stream_t stream) {
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out), AVD_EUNSUPPORTED,
                "cfg_unpatch_ddim_slots_guided: pointers must be 16-byte aligned");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_unpatch_ddim_slots_guided: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(guide, AVD_EINVAL, "cfg_unpatch_ddim_slots_guided: null clip guide");
    AVD_REQUIRE(key || !(eta > 0.f), AVD_EINVAL, "cfg_unpatch_ddim_slots_guided: eta > 0 needs a slot key");
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr, key, guide);
}
extern "C" int avd_cfg_untoken_ddim_audio_slots_guided_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                           const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance,
                                                           float eta, const avd_slot_key* key, const avd_clip_guide* guide, int slots,
                                                           float* x0_hist, float* z_out, int B, int Ca, int F, int len, int stride,
                                                           avd_stream_t stream) {
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_guided: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(guide, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_guided: null clip guide");
    AVD_REQUIRE(key || !(eta > 0.f), AVD_EINVAL, "cfg_untoken_ddim_audio_slots_guided: eta > 0 needs a slot key");
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr, key,
                                      guide);
}
// the slot forms under a slot CFG control ("slot CFG control" in the header): the guided entries' arguments and the control; key and
// guide may be null
extern "C" int avd_cfg_unpatch_ddim_slots_cfg_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                  const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                                  const avd_slot_key* key, const avd_clip_guide* guide, int slots, float* x0_hist,
                                                  float* z_out, int B, int C, int T, int H, int W, int t, int h, int w,
                                                  const avd_slot_cfg* cfg, avd_stream_t stream) {
    AVD_REQUIRE(cfg, AVD_EINVAL, "cfg_unpatch_ddim_slots_cfg: null slot CFG control");
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out), AVD_EUNSUPPORTED,
                "cfg_unpatch_ddim_slots_cfg: pointers must be 16-byte aligned");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_unpatch_ddim_slots_cfg: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(key || !(eta > 0.f), AVD_EINVAL, "cfg_unpatch_ddim_slots_cfg: eta > 0 needs a slot key");
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr,
                                eta > 0.f ? key : nullptr, guide, cfg);
}
extern "C" int avd_cfg_untoken_ddim_audio_slots_cfg_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                        const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance,
                                                        float eta, const avd_slot_key* key, const avd_clip_guide* guide, int slots,
                                                        float* x0_hist, float* z_out, int B, int Ca, int F, int len, int stride,
                                                        const avd_slot_cfg* cfg, avd_stream_t stream) {
    AVD_REQUIRE(cfg, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_cfg: null slot CFG control");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_cfg: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(key || !(eta > 0.f), AVD_EINVAL, "cfg_untoken_ddim_audio_slots_cfg: eta > 0 needs a slot key");
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr,
                                      eta > 0.f ? key : nullptr, guide, cfg);
}
// the slot forms of a clip batch ("clip batch keying" in the header): the controlled entries' arguments and the descriptor; cfg, key and
// guide may be null
extern "C" int avd_cfg_unpatch_ddim_slots_clips_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                    const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                                    const avd_slot_key* key, const avd_clip_guide* guide, const avd_clip_queues* queues,
                                                    int slots, float* x0_hist, float* z_out, int B, int C, int T, int H, int W, int t, int h,
                                                    int w, const avd_slot_cfg* cfg, avd_stream_t stream) {
    AVD_REQUIRE(queues, AVD_EINVAL, "cfg_unpatch_ddim_slots_clips: null clip queues");
    AVD_REQUIRE(aligned16(eps2) && aligned16(z) && aligned16(z_out), AVD_EUNSUPPORTED,
                "cfg_unpatch_ddim_slots_clips: pointers must be 16-byte aligned");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_unpatch_ddim_slots_clips: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(key || !(eta > 0.f), AVD_EINVAL, "cfg_unpatch_ddim_slots_clips: eta > 0 needs a slot key");
    return cfg_unpatch_ddim_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr,
                                eta > 0.f ? key : nullptr, guide, cfg, queues);
}
extern "C" int avd_cfg_untoken_ddim_audio_slots_clips_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                          const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance,
                                                          float eta, const avd_slot_key* key, const avd_clip_guide* guide,
                                                          const avd_clip_queues* queues, int slots, float* x0_hist, float* z_out, int B,
                                                          int Ca, int F, int len, int stride, const avd_slot_cfg* cfg,
                                                          avd_stream_t stream) {
    AVD_REQUIRE(queues, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_clips: null clip queues");
    AVD_REQUIRE(slots > 0, AVD_EINVAL, "cfg_untoken_ddim_audio_slots_clips: slots must be > 0 (got %d)", slots);
    AVD_REQUIRE(key || !(eta > 0.f), AVD_EINVAL, "cfg_untoken_ddim_audio_slots_clips: eta > 0 needs a slot key");
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, nullptr, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), nullptr, t_last, x0_hist, nullptr, nullptr, 0, 0, slots, nullptr,
                                      eta > 0.f ? key : nullptr, guide, cfg, queues);
}
extern "C" int avd_clip_guide_slots_clips_f32(const avd_clip_guide* g, const avd_clip_queues* queues, const int64_t* tau,
                                              const float* alpha_bar, int T_train, int everywhere, const float* z, float* out, int B,
                                              int64_t outer, int L, int slots, int slot_len, int64_t inner, avd_stream_t stream) {
    AVD_REQUIRE(queues, AVD_EINVAL, "clip_guide_slots_clips: null clip queues");
    return clip_guide_slots_f32(g, tau, alpha_bar, T_train, everywhere, z, out, B, outer, L, slots, slot_len, inner,
                                static_cast<hipStream_t>(stream), queues);
}
extern "C" int avd_slot_noise_clips_f32(const avd_slot_key* key, const avd_clip_queues* queues, const int64_t* t_now, float* out, int B,
                                        int64_t outer, int L, int slots, int slot_len, int64_t inner, avd_stream_t stream) {
    AVD_REQUIRE(queues, AVD_EINVAL, "slot_noise_clips: null clip queues");
    return slot_noise_f32(key, t_now, out, B, outer, L, slots, slot_len, inner, static_cast<hipStream_t>(stream), queues);
}
extern "C" int64_t avd_slot_cfg_stats_bytes(int B, int slots, int64_t per_slot) { return slot_cfg_stats_bytes(B, slots, per_slot); }
extern "C" int avd_clip_guide_slots_f32(const avd_clip_guide* g, const int64_t* tau, const float* alpha_bar, int T_train, int everywhere,
                                        const float* z, float* out, int B, int64_t outer, int L, int slots, int slot_len, int64_t inner,
                                        avd_stream_t stream) {
    return clip_guide_slots_f32(g, tau, alpha_bar, T_train, everywhere, z, out, B, outer, L, slots, slot_len, inner,
                                static_cast<hipStream_t>(stream));
}
extern "C" int avd_slot_noise_f32(const avd_slot_key* key, const int64_t* t_now, float* out, int B, int64_t outer, int L, int slots,
                                  int slot_len, int64_t inner, avd_stream_t stream) {
    return slot_noise_f32(key, t_now, out, B, outer, L, slots, slot_len, inner, static_cast<hipStream_t>(stream));
}
extern "C" int avd_fifo_shift_hist_f32(const avd_noise_key* key, int64_t t, int64_t c, const float* z_in, float* z_out, float* popped,
                                       const float* hist_in, float* hist_out, int B, int64_t outer, int slots, int slot_len, int64_t inner,
                                       avd_stream_t stream) {
    AVD_REQUIRE(hist_in && hist_out, AVD_EINVAL, "fifo_shift_hist: null hist_in or hist_out");
    return fifo_shift_f32(key, t, c, z_in, z_out, popped, B, outer, slots, slot_len, inner, static_cast<hipStream_t>(stream), hist_in, hist_out);
}
extern "C" int avd_fifo_shift_guided_f32(const avd_noise_key* key, int64_t t, int64_t c, const avd_clip_guide* guide,
                                         const float* alpha_bar, int T_train, int everywhere, const float* z_in, float* z_out,
                                         float* popped, const float* hist_in, float* hist_out, int B, int64_t outer, int slots,
                                         int slot_len, int64_t inner, avd_stream_t stream) {
    return fifo_shift_guided_f32(key, t, c, guide, alpha_bar, T_train, everywhere, z_in, z_out, popped, hist_in, hist_out, B, outer, slots,
                                 slot_len, inner, static_cast<hipStream_t>(stream));
}
extern "C" int avd_fifo_shift_cursor_f32(const avd_noise_key* key, int64_t t, int64_t c0, const int32_t* cursor, int64_t n_out,
                                         const float* z_in, float* z_out, float* clip, int B, int64_t outer, int slots, int slot_len,
                                         int64_t inner, avd_stream_t stream) {
    AVD_REQUIRE(cursor, AVD_EINVAL, "fifo_shift_cursor: null cursor");
    return fifo_shift_f32(key, t, c0, z_in, z_out, clip, B, outer, slots, slot_len, inner, static_cast<hipStream_t>(stream), nullptr, nullptr,
                          cursor, n_out);
}
extern "C" int avd_fifo_shift_cursor_hist_f32(const avd_noise_key* key, int64_t t, int64_t c0, const int32_t* cursor, int64_t n_out,
                                              const float* z_in, float* z_out, float* clip, const float* hist_in, float* hist_out, int B,
                                              int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream) {
    AVD_REQUIRE(cursor, AVD_EINVAL, "fifo_shift_cursor_hist: null cursor");
    AVD_REQUIRE(hist_in && hist_out, AVD_EINVAL, "fifo_shift_cursor_hist: null hist_in or hist_out");
    return fifo_shift_f32(key, t, c0, z_in, z_out, clip, B, outer, slots, slot_len, inner, static_cast<hipStream_t>(stream), hist_in, hist_out,
                          cursor, n_out);
}
extern "C" int avd_fifo_lookahead_f32(const avd_noise_key* key, int64_t t, int64_t c, int shift, const float* z_in, float* z_out,
                                      float* popped, int B, int64_t outer, int slots, int ctx, int slot_len, int64_t inner,
                                      avd_stream_t stream) {
    return fifo_lookahead_f32(key, t, c, shift, z_in, z_out, popped, B, outer, slots, ctx, slot_len, inner, static_cast<hipStream_t>(stream));
}
extern "C" int avd_fifo_lookahead_hist_f32(const avd_noise_key* key, int64_t t, int64_t c, int shift, const float* z_in, float* z_out,
                                           float* popped, const float* hist_in, float* hist_out, int B, int64_t outer, int slots, int ctx,
                                           int slot_len, int64_t inner, avd_stream_t stream) {
    AVD_REQUIRE(hist_in && hist_out, AVD_EINVAL, "fifo_lookahead_hist: null hist_in or hist_out");
    return fifo_lookahead_f32(key, t, c, shift, z_in, z_out, popped, B, outer, slots, ctx, slot_len, inner, static_cast<hipStream_t>(stream),
                              hist_in, hist_out);
}
extern "C" int avd_fifo_carry_f32(const float* in, float* out, int B, int64_t outer, int slots, int ctx, int shift, int slot_len,
                                  int64_t inner, avd_stream_t stream) {
    return fifo_carry_f32(in, out, B, outer, slots, ctx, shift, slot_len, inner, static_cast<hipStream_t>(stream));
}
extern "C" int avd_fifo_shift_clips_f32(const uint64_t* seeds, int64_t t, int64_t c, const float* z_in, float* z_out, float* clips,
                                        int64_t n_clip, int64_t m, const float* hist_in, float* hist_out, const float* carry_in,
                                        float* carry_out, int B, int K, int64_t outer, int slots, int slot_len, int64_t inner,
                                        avd_stream_t stream) {
    return fifo_shift_clips_f32(seeds, t, c, z_in, z_out, clips, n_clip, m, hist_in, hist_out, carry_in, carry_out, B, K, outer, slots,
                                slot_len, inner, static_cast<hipStream_t>(stream));
}
extern "C" int avd_cursor_add(int32_t* cursor, int delta, avd_stream_t stream) {
    AVD_REQUIRE(cursor, AVD_EINVAL, "cursor_add: null cursor");
    hipLaunchKernelGGL(cursor_add_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), cursor, delta);
    AVD_CHECK_LAUNCH("cursor_add");
    return AVD_OK;
}
extern "C" int avd_slot_tables_select(const int64_t* tab0, const int64_t* tab1, const int64_t* tab2, int n_rows, int n,
                                      const int32_t* cursor, int64_t* out0, int64_t* out1, int64_t* out2, avd_stream_t stream) {
    AVD_REQUIRE(tab0 && tab1 && out0 && out1 && cursor, AVD_EINVAL, "slot_tables_select: null pointer");
    AVD_REQUIRE(!tab2 == !out2, AVD_EINVAL, "slot_tables_select: the third table and its buffer go together");
    AVD_REQUIRE(n_rows >= 1 && n >= 1, AVD_EINVAL, "slot_tables_select: bad dims (n_rows %d, n %d)", n_rows, n);
    const SlotTabs tb{{tab0, tab1, tab2}, {out0, out1, out2}};
    const dim3 grid((unsigned)((n + 255) / 256));
    if (tab2)
        hipLaunchKernelGGL(slot_tables_select_kernel<3>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), tb, cursor, n_rows, n);
    else
        hipLaunchKernelGGL(slot_tables_select_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), tb, cursor, n_rows, n);
    AVD_CHECK_LAUNCH("slot_tables_select");
    return AVD_OK;
}
extern "C" int avd_fifo_prompt_gather_f32(const float* canvas, const int32_t* cursor, float* out, int B, int slots, int prompt_hop,
                                          int64_t outer, int64_t P, int64_t prompt_len, int64_t inner, avd_stream_t stream) {
    AVD_REQUIRE(canvas && cursor && out, AVD_EINVAL, "fifo_prompt_gather: null pointer");
    AVD_REQUIRE(B > 0 && slots > 0 && prompt_hop > 0 && outer > 0 && P > 0 && prompt_len > 0 && inner > 0, AVD_EINVAL,
                "fifo_prompt_gather: bad dims (B %d, slots %d, prompt_hop %d, outer %lld, P %lld, prompt_len %lld, inner %lld)", B, slots,
                prompt_hop, (long long)outer, (long long)P, (long long)prompt_len, (long long)inner);
    AVD_REQUIRE((int64_t)B * slots <= 0x7fffffff && prompt_len <= 0x7fffffff, AVD_EINVAL,
                "fifo_prompt_gather: B %d * slots %d and prompt_len %lld must fit an int", B, slots, (long long)prompt_len);
    AVD_REQUIRE((double)outer * (double)P * (double)inner < 9.0e18 && (double)B * (double)outer * (double)prompt_len * (double)inner < 9.0e18,
                AVD_EUNSUPPORTED, "fifo_prompt_gather: too many values");
    const int64_t n_c = outer * P * inner, n_o = (int64_t)B * outer * prompt_len * inner;
    AVD_REQUIRE(!(out < canvas + n_c && canvas < out + n_o), AVD_EINVAL, "fifo_prompt_gather: out must not overlap the prompt canvas");
    const bool vec = inner % 4 == 0 && aligned16(canvas) && aligned16(out);
    const int64_t n = n_o / (vec ? 4 : 1);
    AVD_REQUIRE((n + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "fifo_prompt_gather: %lld lanes are too many for one launch", (long long)n);
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(fifo_prompt_gather_kernel<4>, grid, dim3(256), 0, st, canvas, out, cursor, slots, (int64_t)prompt_hop, outer, P,
                           prompt_len, inner, n);
    else
        hipLaunchKernelGGL(fifo_prompt_gather_kernel<1>, grid, dim3(256), 0, st, canvas, out, cursor, slots, (int64_t)prompt_hop, outer, P,
                           prompt_len, inner, n);
    AVD_CHECK_LAUNCH("fifo_prompt_gather");
    return AVD_OK;
}
extern "C" int avd_fifo_prompt_gather_frac_f32(const float* canvas, const int32_t* cursor, float* out, int B, int64_t first, int stride,
                                               int num, int den, int interp, int64_t outer, int64_t P, int64_t prompt_len, int64_t inner,
                                               avd_stream_t stream) {
    AVD_REQUIRE(canvas && out, AVD_EINVAL, "fifo_prompt_gather_frac: null pointer");
    AVD_REQUIRE(B > 0 && stride > 0 && outer > 0 && P > 0 && prompt_len > 0 && inner > 0, AVD_EINVAL,
                "fifo_prompt_gather_frac: bad dims (B %d, stride %d, outer %lld, P %lld, prompt_len %lld, inner %lld)", B, stride,
                (long long)outer, (long long)P, (long long)prompt_len, (long long)inner);
    AVD_REQUIRE(num >= 1 && den >= 1, AVD_EINVAL, "fifo_prompt_gather_frac: the hop num / den needs num >= 1 and den >= 1 (got %d / %d)", num,
                den);
    AVD_REQUIRE(interp == kPromptNearest || interp == kPromptLinear, AVD_EINVAL,
                "fifo_prompt_gather_frac: interp must be 0 (nearest) or 1 (linear), got %d", interp);
    AVD_REQUIRE(first > -(1ll << 31) && first < (1ll << 31) && (int64_t)B * stride <= 0x7fffffff && prompt_len <= 0x7fffffff, AVD_EINVAL,
                "fifo_prompt_gather_frac: |first| %lld, B %d * stride %d and prompt_len %lld must be below 2^31", (long long)first, B, stride,
                (long long)prompt_len);
    AVD_REQUIRE((double)outer * (double)P * (double)inner < 9.0e18 && (double)B * (double)outer * (double)prompt_len * (double)inner < 9.0e18,
                AVD_EUNSUPPORTED, "fifo_prompt_gather_frac: too many values");
    // the cursor's clamp: from m_cap on sample 0, the first of the call, starts at or past P, so every larger cursor gives the same zeros
    __int128 cap = ((__int128)P * den + num - 1) / num - first;
    cap = cap < 0 ? 0 : (cap > 0x7fffffff ? 0x7fffffff : cap);
    const int64_t m_cap = cursor ? (int64_t)cap : 0;
    const __int128 q_hi = (__int128)first + m_cap + (__int128)(B - 1) * stride, q_lo = first;
    const __int128 q_abs = (q_hi < 0 ? -q_hi : q_hi) > (q_lo < 0 ? -q_lo : q_lo) ? (q_hi < 0 ? -q_hi : q_hi) : (q_lo < 0 ? -q_lo : q_lo);
    AVD_REQUIRE(q_abs * num < ((__int128)1 << 62), AVD_EINVAL,
                "fifo_prompt_gather_frac: the largest clip slot %lld times num %d leaves the 64-bit range of the walk", (long long)q_abs, num);
    const int64_t n_c = outer * P * inner, n_o = (int64_t)B * outer * prompt_len * inner;
    AVD_REQUIRE(!(out < canvas + n_c && canvas < out + n_o), AVD_EINVAL, "fifo_prompt_gather_frac: out must not overlap the prompt canvas");
    const bool vec = inner % 4 == 0 && aligned16(canvas) && aligned16(out);
    const int64_t n = n_o / (vec ? 4 : 1);
    AVD_REQUIRE((n + 255) / 256 <= 0x7fffffff, AVD_EUNSUPPORTED, "fifo_prompt_gather_frac: %lld lanes are too many for one launch",
                (long long)n);
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    static const int tags[4] = {prof_tag_id("fifo_prompt_gather_frac_kernel<1, nearest>"), prof_tag_id("fifo_prompt_gather_frac_kernel<4, nearest>"),
                                prof_tag_id("fifo_prompt_gather_frac_kernel<1, linear>"), prof_tag_id("fifo_prompt_gather_frac_kernel<4, linear>")};
    ProfScope prof(tags[(interp == kPromptLinear ? 2 : 0) + (vec ? 1 : 0)], 4.0 * (interp == kPromptLinear ? 3.0 : 2.0) * (double)n_o, st);
#define AVD_PROMPT_FRAC(V, I)                                                                                                         \
    hipLaunchKernelGGL((fifo_prompt_gather_frac_kernel<V, I>), grid, dim3(256), 0, st, canvas, out, cursor, m_cap, first, (int64_t)stride, \
                       (int64_t)num, (int64_t)den, outer, P, prompt_len, inner, n)
    if (interp == kPromptLinear) {
        if (vec) AVD_PROMPT_FRAC(4, kPromptLinear);
        else AVD_PROMPT_FRAC(1, kPromptLinear);
    } else {
        if (vec) AVD_PROMPT_FRAC(4, kPromptNearest);
        else AVD_PROMPT_FRAC(1, kPromptNearest);
    }
#undef AVD_PROMPT_FRAC
    AVD_CHECK_LAUNCH("fifo_prompt_gather_frac");
    return AVD_OK;
}
extern "C" int avd_cfg_untoken_ddim_audio_f32(const float* eps2, const float* z, const int64_t* t_now,
                                              const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance,
                                              float eta, const float* noise, float* z_out, int B, int Ca, int F, int len,
                                              int stride, avd_stream_t stream) {
    return cfg_untoken_ddim_audio_f32(eps2, z, t_now, t_prev, alpha_bar, T_train, guidance, eta, noise, z_out, B, Ca, F,
                                      len, stride, static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr);
}
extern "C" int avd_eps_unpatch_ddim_f32(const float* eps, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                        const float* alpha_bar, int T_train, float eta, const float* noise, float* z_out, int B, int C,
                                        int T, int H, int W, int t, int h, int w, const avd_noise_key* key, const int64_t* t_last,
                                        float* x0_hist, const avd_latent_guide* guide, avd_stream_t stream) {
    AVD_REQUIRE(aligned16(eps) && aligned16(z) && aligned16(z_out) && (!noise || aligned16(noise)), AVD_EUNSUPPORTED,
                "eps_unpatch_ddim: pointers must be 16-byte aligned");
    return eps_unpatch_ddim_f32(eps, z, t_now, t_prev, alpha_bar, T_train, eta, noise, z_out, B, C, T, H, W, t, h, w,
                                static_cast<hipStream_t>(stream), key, t_last, x0_hist, guide, 0, 0);
}
extern "C" int avd_eps_untoken_ddim_audio_f32(const float* eps, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                              const float* alpha_bar, int T_train, float eta, const float* noise, float* z_out, int B,
                                              int Ca, int F, int len, int stride, const avd_noise_key* key, const int64_t* t_last,
                                              float* x0_hist, const avd_latent_guide* guide, avd_stream_t stream) {
    return eps_untoken_ddim_audio_f32(eps, z, t_now, t_prev, alpha_bar, T_train, eta, noise, z_out, B, Ca, F, len, stride,
                                      static_cast<hipStream_t>(stream), key, t_last, x0_hist, guide, 0, 0);
}
extern "C" int avd_gaussian_noise_f32(const avd_noise_key* key, const int64_t* t_now, float* out, int B, int64_t per_sample,
                                      avd_stream_t stream) {
    return gaussian_noise_f32(key, t_now, out, B, per_sample, static_cast<hipStream_t>(stream));
}
extern "C" int avd_canvas_noise_f32(const avd_noise_key* key, const int64_t* t_now, float* out, int N, int64_t outer, int L, int hop,
                                    int64_t inner, avd_stream_t stream) {
    return canvas_noise_f32(key, t_now, out, N, outer, L, hop, inner, static_cast<hipStream_t>(stream));
}
extern "C" int avd_sched_advance(const int64_t* sched, int n_sched, int32_t* cursor, int64_t* t_now, int64_t* t_prev,
                                 int B, avd_stream_t stream) {
    AVD_REQUIRE(sched && cursor && t_now && t_prev && n_sched >= 2 && B > 0, AVD_EINVAL, "sched_advance: bad arguments");
    hipLaunchKernelGGL(sched_advance_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sched, n_sched,
                       cursor, t_now, t_prev, B);
    AVD_CHECK_LAUNCH("sched_advance");
    return AVD_OK;
}
extern "C" int avd_sched_advance_ms(const int64_t* sched, int n_sched, int32_t* cursor, int64_t* t_last, int64_t* t_now,
                                    int64_t* t_prev, int B, avd_stream_t stream) {
    AVD_REQUIRE(sched && cursor && t_last && t_now && t_prev && n_sched >= 2 && B > 0, AVD_EINVAL, "sched_advance_ms: bad arguments");
    hipLaunchKernelGGL(sched_advance_ms_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sched, n_sched,
                       cursor, t_last, t_now, t_prev, B);
    AVD_CHECK_LAUNCH("sched_advance_ms");
    return AVD_OK;
}
extern "C" int avd_dpmpp_2m_step_f32(const float* x_t, const float* eps_hat, float* x0_hist, const int64_t* t_last,
                                     const int64_t* t_now, const int64_t* t_prev, const float* alpha_bar, int T_train, float* x_out,
                                     int B, int64_t per_sample, avd_stream_t stream) {
    return dpmpp_2m_step_f32(x_t, eps_hat, x0_hist, t_last, t_now, t_prev, alpha_bar, T_train, x_out, B, per_sample,
                             static_cast<hipStream_t>(stream));
}
extern "C" int avd_dpmpp_2m_sde_step_f32(const float* x_t, const float* eps_hat, float* x0_hist, const int64_t* t_last,
                                         const int64_t* t_now, const int64_t* t_prev, const float* alpha_bar, int T_train, float eta,
                                         const float* noise, float* x_out, int B, int64_t per_sample, avd_stream_t stream) {
    return dpmpp_2m_sde_step_f32(x_t, eps_hat, x0_hist, t_last, t_now, t_prev, alpha_bar, T_train, eta, noise, x_out, B, per_sample,
                                 static_cast<hipStream_t>(stream));
}
extern "C" int64_t avd_cfg_stats_bytes(int B, int64_t per_sample) { return cfg_stats_bytes(B, per_sample); }
extern "C" int64_t avd_apg_stats_bytes(int B, int64_t per_sample) { return apg_stats_bytes(B, per_sample); }
extern "C" int avd_apg_guidance_f32(const float* e_cond, const float* e_null, const float* guidance, float guidance_scalar,
                                    const avd_apg_control* apg, float* out, int B, int64_t per_sample, avd_stream_t stream) {
    return apg_guidance_f32(e_cond, e_null, guidance, guidance_scalar, apg, out, B, per_sample, static_cast<hipStream_t>(stream));
}
extern "C" int avd_cfg_rescale_f32(const float* e_cond, const float* e_cfg, const float* phi, void* stats, int64_t stats_bytes, float* out,
                                   int B, int64_t per_sample, avd_stream_t stream) {
    return cfg_rescale_f32(e_cond, e_cfg, phi, stats, stats_bytes, out, B, per_sample, static_cast<hipStream_t>(stream));
}
extern "C" int avd_latent_guide_f32(const avd_latent_guide* g, const int64_t* tau, const float* alpha_bar, int T_train, const float* z,
                                    float* out, int B, int64_t per_sample, avd_stream_t stream) {
    return latent_guide_f32(g, tau, alpha_bar, T_train, z, out, B, per_sample, static_cast<hipStream_t>(stream));
}
extern "C" int avd_renoise_f32(const avd_noise_key* key, uint32_t visit, const avd_latent_guide* g, const int64_t* t_from,
                               const int64_t* t_to, const float* alpha_bar, int T_train, const float* z, float* out, int B,
                               int64_t per_sample, avd_stream_t stream) {
    return renoise_f32(key, visit, g, t_from, t_to, alpha_bar, T_train, z, out, B, per_sample, static_cast<hipStream_t>(stream));
}
extern "C" int avd_renoise_canvas_f32(const avd_noise_key* key, uint32_t visit, const avd_latent_guide* g, const int64_t* t_from,
                                      const int64_t* t_to, const float* alpha_bar, int T_train, const float* z, float* out, int N,
                                      int64_t outer, int L, int hop, int64_t inner, avd_stream_t stream) {
    return renoise_canvas_f32(key, visit, g, t_from, t_to, alpha_bar, T_train, z, out, N, outer, L, hop, inner,
                              static_cast<hipStream_t>(stream));
}
extern "C" int avd_latent_guide_canvas_f32(const avd_latent_guide* g, const int64_t* tau, const float* alpha_bar, int T_train,
                                           const float* z, float* out, int N, int64_t outer, int L, int hop, int64_t inner,
                                           avd_stream_t stream) {
    return latent_guide_canvas_f32(g, tau, alpha_bar, T_train, z, out, N, outer, L, hop, inner, static_cast<hipStream_t>(stream));
}

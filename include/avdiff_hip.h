/* avdiff_hip.h — C ABI of libavdiff_hip.so: the MI355X (gfx950) denoising hot path of
 * mauruszach/multimodal_diffusion behind the reference's Python nn.Module / sampler API.
 *
 * The reference has no FFI/plugin layer: its boundary for this path is a set of
 * Python call signatures.  Each entry point below names the reference call it stands under
 * (paths relative to the reference repo).  The host side (the multimodal_diffusion_amd package) binds these
 * with ctypes and keeps the reference's class names, constructor kwargs, forward signatures and
 * state_dict keys.
 *
 * Conventions
 *   - every function returns 0 on success, a negative AVD_E* code on failure;
 *     avd_last_error() returns a thread-local human-readable message for the last failure.
 *   - all tensor pointers are DEVICE pointers owned by the caller, fp32, contiguous unless a leading
 *     dimension is given, 16-byte aligned; int64 for timesteps (as in the reference).
 *   - nothing allocates, synchronises or copies to the host: every call only enqueues kernels on
 *     `stream` (a hipStream_t passed as void*), so calls are stream-ordered and hipGraph-capturable.
 *   - inputs are never written; outputs never alias inputs unless stated.
 */
#ifndef AVDIFF_HIP_H
#define AVDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVD_ABI_VERSION 7

#define AVD_OK            0
#define AVD_EINVAL       -1   /* bad shape / argument (reference: AssertionError / ValueError) */
#define AVD_EUNSUPPORTED -2   /* shape outside what the gfx950 kernels are built for */
#define AVD_ELAUNCH      -3   /* HIP launch error */
#define AVD_EWORKSPACE   -4   /* workspace too small */

#define AVD_ACT_NONE 0
#define AVD_ACT_GELU 1        /* exact erf GELU (torch.nn.functional.gelu default) */
#define AVD_ACT_SILU 2
#define AVD_ACT_TANH 3        /* conv1d only (AudioCodec.decode output) */
#define AVD_ACT_RELU 4        /* avd_layernorm_act_f32 / noise head only (heads/noise_heads.py:28-36) */
#define AVD_ACT_LEAKY_RELU 5  /* slope 0.1, same scope */

typedef void* avd_stream_t;   /* hipStream_t */

int         avd_abi_version(void);
const char* avd_last_error(void);
/* gfx arch name of device 0 as seen by the library ("gfx950"); diagnostic only. */
int         avd_device_arch(char* buf, int buflen);
/* Measurement / test hooks, process-wide, never needed for correct results: "gemm_tile" (-1 auto, 0 = 128x128, 1 = 128x64,
 * 2 = 64x64 LDS-DMA tile of avd_gemm_bias_act_f32), "gemm_stages" (0 by size, 2 / 3 LDS stages), "gemm_splitk" (largest number of K slices of the fp32 fc2 launch of
 * avd_core_forward_f32 when its 64x64 blocks cover less than half of the CUs — batches of a few hundred rows; 0 = never, default and maximum 4;
 * partial sums added in slice order, no atomics), "s3_tile" (-1 per epilogue, 0 = 8-wave
 * 256x256, 1 = 4-wave 256x128 blocks of the split-operand GEMMs), "s3_stagger" (first-generation stagger of co-resident 4-wave blocks,
 * x 1024 cycles; -1 automatic), "cfg_rows" (1 default: the fused CFG + un-patch + DDIM kernel reads token rows whole and writes whole 128-byte lines of latent through an LDS
 * transpose; 0: one 16-byte gather per lane; bit-identical), "vae_lat" (1 default: avd_vae_decode_f32 takes the latent-composed first convolution when the descriptor
 * carries conv0_lat_w3; 0: from_lat -> upsample -> 64-channel convolution), "vae_fold" (1 default: the three-plane two-block decoder hands conv 0's output to conv 1 as its operand image, folds the GroupNorm
 * between them into conv 1's per-sample weights and finishes to_img from per-group partial sums; 0: fp32 activations between the kernels), "codec_mfma" (1 default: avd_conv1d_act_f32 runs 64 -> 64 layers with k = 7 / 9 on the fp32 matrix pipe; 0: the vector kernel), "s3_sn" / "s3_super4" / "s3_super8" (super-tile of the split GEMMs' block order — the blocks an XCD runs together: width in column blocks /
 * blocks per super-tile of the two-per-CU / one-per-CU kernels; 0 = default; bit-identical, measurement aid of profiles/r05_fetch_ab.txt), "s3_min_rows" (smallest 2B*N that takes the split-operand kernels: -1 default = 2,048 rows for the core in the six-term bf16x3 mode, 6,144 otherwise; >= 0 = that many in every mode), "no_fold" (1 = keep RMSNorm as
 * separate kernels in avd_core_forward_f32, in every mode), "s3_m16" (1 default: bf16x3 GEMMs on v_mfma_f32_16x16x32_bf16 with two product
 * terms per instruction; 0: the 32x32x16 kernel), "s3_rt" (rows per block of the bf16x3 residual + image epilogue: 0 automatic,
 * 7 = 224 rows, 8 = 256 rows, 6 = 192 rows (four-wave kernel only); results are bit-identical), "s3_rt4" (rows per 256x128-class four-wave
 * block of the bf16x3 in_proj / fc1 / out_proj / fc2 launches, in units of 32: 0 = the host picks per launch what leaves the fewest CUs idle —
 * mid-size and small batches — 2 .. 8 forced (in_proj / fc1: at least 5); bit-identical), "s3_deep4" (1 default: an out_proj / fc2 launch whose four-wave blocks fit the CUs once runs
 * one block per CU on a four-stage LDS ring instead of a two-stage one; 0: never; bit-identical), "s3_w128" (1 default: the bf16x3 residual + image GEMMs run as four waves
 * with a 128 x 128 wave tile and accumulators in AGPRs; 0: eight waves with 128 x 64 tiles; bit-identical), "s3_splitk" (largest number of K slices of the fc2 launch when its blocks
 * fill at most half of the chip's block slots — small and mid-size batches; 0 = never, default and maximum 4; partial sums are added in
 * slice order by a reduction kernel, no atomics), "attn_pipe" (1 default: the three-plane split-operand attention runs as one software
 * pipeline per wave — the next tile's score MFMAs beside this tile's softmax; 0: the plain kernel everywhere, 2: the pipeline in every
 * split mode), "attn_m16" (1 default: that pipeline on v_mfma_f32_16x16x32 in the three-plane modes — same cycles per FLOP, less power, so a higher clock under the cap; 0: the 32x32x16 kernels; 2: the 16x16x32 kernel in every split mode), "core_trim" (1 default: the last block of avd_core_forward_f32 runs out_proj / fc1 / fc2 / the final norm on the caller's
 * row window only; 0: on every row; the window's results are bit-identical), "mlp_fused" (0 default; 1: fc1 -> GELU -> fc2 of the six-term
 * bf16x3 path as ONE launch whose hidden activations stay on the CU — d = 512 only; bit-identical to the two launches, and measures
 * 1.5x slower: DESIGN.md 4.9). */
int         avd_tune_set(const char* key, int64_t value);
/* The null half of the one-stream CFG step without its duplicate prompt rows (default 1 = on; also the AVD_CFG_DEDUP environment
 * variable, read when the library loads).  With the target rows first, every prompt row of a null sample is the zero row at the
 * input and stays one and the same row through every block, so avd_denoise_step_*_f32 carries one of them per null sample and
 * copies its k / v into the key slots of the others before each attention: the attention sees the keys and values of the full
 * layout and the step's results are bit-identical to it.  Taken by the stacked one-stream step (split_streams 0) and by the
 * two-chain step that asks for it (split_streams 2, at avd_step_desc below; split_streams 1 keeps the full layout) in concat timestep
 * mode with target_first, Np >= 2, on the folded bf16x3 path (six or nine terms) with the trimmed last block and its residual row map —
 * today the six-term 16x16x32 kernels have that map, so "bf16x3_strict" still runs the full layout; every other step runs the full
 * layout whatever the switch says.  Workspace sizes do not depend on it and it may change between calls (not inside a captured
 * graph's replay: a capture keeps the route it recorded).  Returns the previous value.  Process-wide, single host thread. */
int         avd_cfg_dedup_set(int on);

/* ---- a6: RMSNorm — avdiff/models/mmdt.py:33-42 (RMSNorm.forward)
 * y = scale * x / (||x||_2 / sqrt(d) + eps), eps OUTSIDE the sqrt. x,y: [rows,d]. */
int avd_rmsnorm_f32(const float* x, const float* scale, float* y, int64_t rows, int d, float eps,
                    avd_stream_t stream);

/* ---- a3/a6/a7: Linear (+bias)(+act)(+residual) — torch.nn.Linear as used at
 * avdiff/models/mmdt.py:60 (packed in_proj / out_proj inside nn.MultiheadAttention), :77-83 (MLP fc1/fc2),
 * avdiff/models/heads/noise_heads.py:206-223, avdiff/models/infer/sample_clip.py:54-56 (LinearAdapter).
 * C[M,N] = act(A[M,K] · W[N,K]^T + bias[N]) + residual[M,N].   bias/residual may be NULL.
 * lda/ldr/ldc are row strides in floats (multiples of 4).  K % 4 == 0, N % 4 == 0.
 * f32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products, fp32 accumulate. */
int avd_gemm_bias_act_f32(const float* A, int64_t lda, const float* W, const float* bias,
                          const float* residual, int64_t ldr, float* C, int64_t ldc,
                          int64_t M, int N, int K, int act, avd_stream_t stream);

/* The same Linear with the neighbouring RMSNorms (mmdt.py:39-42) folded in, as avd_core_forward_f32 uses it (A [M,K], C [M,N]
 * contiguous; K % 32 == 0, N % 128 == 0):
 *   ss_in  != NULL: A is the UN-normalised stream and W carries the norm's scale (W * scale[None,:]); every output row is
 *                   multiplied by 1 / (sqrt(sum_j ss_in[row][j]) / sqrt(K) + eps) before the bias.  ss_in: [M, ss_in_cols].
 *   ss_out != NULL: the epilogue also writes the sum of squares of each final output row per 32-column chunk, [M, N/32]
 *                   (fixed summation order: deterministic) — the table the next folded Linear reads as ss_in. */
int avd_gemm_rmsfold_f32(const float* A, const float* W, const float* bias, const float* residual, float* C, int64_t M,
                         int N, int K, int act, const float* ss_in, int ss_in_cols, float eps, float* ss_out,
                         avd_stream_t stream);

/* ---- a6: multi-head self-attention core — nn.MultiheadAttention(batch_first=True) at
 * avdiff/models/mmdt.py:51-61 between in_proj and out_proj: out = softmax(q k^T * scale) v per head,
 * no mask, eval.  qkv: [B,N,3*H*Dh] (q | k | v along the last dim, heads contiguous inside each),
 * out: [B,N,H*Dh].  Dh must be 64.  n_query <= N limits the query rows computed (rows >= n_query of
 * `out` are left untouched); pass N for the reference behaviour.
 * key_padding_mask: NULL, or bytes [B,N] with non-zero = this key is padding and gets no attention weight
 * (MMDiT.forward's key_padding_mask, mmdt.py:57-60,134-149).  A sample whose keys are ALL padded is undefined in the reference
 * (NaN); here it attends uniformly: every query row of it is the mean of its N value rows, for any N. */
int avd_attn_fwd_f32(const float* qkv, float* out, int B, int N, int H, int Dh, float scale,
                     int n_query, const uint8_t* key_padding_mask, avd_stream_t stream);

/* ---- a7: LayerNorm(d, eps, affine) followed by an activation — the Linear→LayerNorm→GELU block of
 * avdiff/models/heads/noise_heads.py:141-147.  x,y: [rows,d]. */
int avd_layernorm_act_f32(const float* x, const float* gamma, const float* beta, float* y,
                          int64_t rows, int d, float eps, int act, avd_stream_t stream);

/* ---- a4: sinusoidal timestep embedding — avdiff/utils/schedule_utils.py:64-86.
 * out[B,dim] = [cos(t*f) | sin(t*f)], f_i = exp(-ln(max_period)*i/half); odd dim zero-padded.
 * freqs: optional device table [dim/2] of f_i built by the host exactly as the reference builds it
 * (cos/sin at t ~ 1000 turn a 1-ulp difference in exp into 6e-5); NULL computes f_i in the kernel. */
int avd_timestep_embedding_f32(const int64_t* t, const float* freqs, float* out, int B, int dim, float max_period,
                               avd_stream_t stream);

/* ---- a1 / a8: tube patch / unpatch — avdiff/utils/ops.py:100-119, 122-144.
 * z: [B,C,T,H,W]  <->  tok: [B, (T/t)(H/h)(W/w), C*t*h*w].  w % 4 == 0 and W % 4 == 0. */
int avd_tube_patch_f32(const float* z, float* tok, int B, int C, int T, int H, int W, int t, int h, int w,
                       avd_stream_t stream);
int avd_tube_unpatch_f32(const float* tok, float* z, int B, int C, int T, int H, int W, int t, int h, int w,
                         avd_stream_t stream);

/* ---- a2 / a8': audio chunk tokens and their overlap-add inverse —
 * avdiff/models/infer/sample_clip.py:184-188 and :191-215 (-> avdiff/utils/ops.py:17-45, 48-93).
 * z: [B,Ca,F] -> tok: [B,Na,Ca*len], Na = (F-len)/stride + 1.  Inverse: overlap-add weighted by `window` [len] and divided
 * by the summed weights (window == NULL: rectangular, i.e. the overlap count; a Hann table gives ops.py's apply_hann=True),
 * cropped / zero-padded to F frames. */
int avd_audio_tokens_f32(const float* z, float* tok, int B, int Ca, int F, int len, int stride,
                         avd_stream_t stream);
int avd_audio_untokens_f32(const float* tok, const float* window, float* z, int B, int Ca, int F, int len, int stride,
                           avd_stream_t stream);

/* ---- a8: DDIM update — avdiff/utils/schedule_utils.py:146-200 (ddim_step).
 * x_t, eps_hat, x_prev: [B, per_sample]; t_now,t_prev: int64[B] (t_prev may be -1 => abar_prev = 1);
 * alpha_bar: fp32[T_train].  eta > 0 requires `noise` (same shape as x_t); eta == 0 ignores it. */
int avd_ddim_step_f32(const float* x_t, const float* eps_hat, const int64_t* t_now, const int64_t* t_prev,
                      const float* alpha_bar, int T_train, float eta, const float* noise,
                      float* x_prev, int B, int64_t per_sample, avd_stream_t stream);

/* ---- DPM-Solver++(2M) update (multistep, data prediction; this entry: eta == 0, the ODE solver; eta > 0: the SDE form below) — an
 * opt-in alternative to DDIM (a public contract).
 * For a timestep tau: a(tau) = alpha_bar[clamp(tau, 0, T_train-1)] for tau >= 0 and a(-1) = 1;
 *   alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log alpha - log sigma.
 * One step goes from s = t_now to t = t_prev; the step before it came from u = t_last (t_last < 0: no history).  Per element:
 *   1. eps  = the CFG-combined noise prediction (fused step: exactly as DDIM's);
 *   2. x0_s = (x_s - sqrt(1 - a_s) eps) / max(sqrt(a_s), 1e-8) in fp32, the same expression and rounding as DDIM's x0
 *      (t_now < 0 is read as 0, as in DDIM);
 *   3. per-sample coefficients, computed in fp64 from the fp32 table and rounded once to fp32:
 *        c_x = sigma_t / sigma_s,  k = alpha_t - c_x alpha_s;
 *        second order when t_last >= 0, t_prev >= 0, sigma_t > 0 and lambda_u < lambda_s < lambda_t:
 *          h = lambda_t - lambda_s,  r = (lambda_s - lambda_u) / h,  c_0 = k (1 + 1/(2r)),  c_1 = -k/(2r);
 *        otherwise first order: c_0 = k, c_1 = 0 (the first step, the final step to t_prev = -1, a non-increasing lambda);
 *        sigma_s = 0 (a_s == 1.0f): c_x = 0, c_0 = 1, c_1 = 0 (the step returns x0_s);
 *   4. z_out = (c_x x_s + c_0 x0_s) + c_1 x0_hist in fp32, in that order, without contraction; when c_1 == 0 the last term is
 *      not added and x0_hist is not read (it may hold anything).  Then x0_hist <- x0_s, each element read before it is written.
 * A first-order step is DDIM at eta = 0 in exact arithmetic; at t_prev = -1 both return x0_s bit for bit.
 * x_t, eps_hat, x0_hist, x_out: fp32 [B, per_sample]; t_last, t_now, t_prev: int64 [B].  x0_hist must not overlap x_t, eps_hat or
 * x_out. */
int avd_dpmpp_2m_step_f32(const float* x_t, const float* eps_hat, float* x0_hist, const int64_t* t_last, const int64_t* t_now,
                          const int64_t* t_prev, const float* alpha_bar, int T_train, float* x_out, int B, int64_t per_sample,
                          avd_stream_t stream);

/* ---- SDE-DPM-Solver++(2M): the update above at eta > 0 (a public contract).  k-diffusion's "DPM++ 2M SDE" (midpoint) in VP form; at
 * eta = 1 Lu et al.'s SDE-DPM-Solver++(2M).  Notation (a, alpha, sigma, lambda; s = t_now, t = t_prev, u = t_last) and x0_s (DDIM's
 * fp32 x0) as above.  For eta > 0 the per-sample coefficients, in fp64 from the fp32 table and rounded once to fp32:
 *        h   = lambda_t - lambda_s                         (+inf when sigma_t = 0)
 *        c_x = (sigma_t / sigma_s) exp(-eta h)
 *        k   = alpha_t (-expm1(-(1 + eta) h))
 *        c_n = sigma_t sqrt(max(-expm1(-2 eta h), 0))
 *        second order under exactly the ODE conditions (t_last >= 0, t_prev >= 0, sigma_t > 0, lambda_u < lambda_s < lambda_t):
 *          r = (lambda_s - lambda_u) / h,  c_0 = k (1 + 1/(2r)),  c_1 = -k/(2r);   otherwise first order: c_0 = k, c_1 = 0;
 *        sigma_s = 0: (c_x, c_0, c_1, c_n) = (0, 1, 0, 0);
 *        sigma_t = 0 (the final step, or a_t == 1.0f): c_x = 0, c_0 = alpha_t, c_1 = 0, c_n = 0 — no exp(-inf), no 0 * inf: the step
 *        returns x0_s bit for bit, as the ODE step does.
 *   z_out = ((c_x x_s + c_0 x0_s) [+ c_1 x0_hist]) + c_n n in fp32, in that order, without contraction; the c_1 term is added, and
 *   x0_hist read, only when c_1 != 0; the noise term is added only when eta > 0.  Then x0_hist <- x0_s.
 * Its first-order step is DDIM at eta = 1 in exact arithmetic; at eta -> 0 the formulas reduce to the ODE ones, and eta == 0 itself
 * evaluates the ODE expressions above (the same bits as avd_dpmpp_2m_step_f32; `noise` is not read).
 * The noise n of the fused step is the DDIM stream below, with no tag of its own: key (seed, sample_offset + b, t_now[b], element)
 * with tag 0x44444D31, or its canvas keying — a DDIM eta > 0 step and an SDE step with the same seed draw the same normals at the same
 * (sample, t, element).  This entry takes n as an explicit tensor (what avd_gaussian_noise_f32 or avd_canvas_noise_f32 wrote, for
 * instance): `noise` fp32 [B, per_sample], required when eta > 0.  Overlap rules as avd_dpmpp_2m_step_f32, and `noise` must not
 * overlap x0_hist or x_out.
 * Limits: the fused steps draw seeded noise only (no unseeded or explicit noise there).  A latent guide's known noise is keyed per
 * sample by this entry's fused twin (avd_denoise_step_dpmpp_2m_sde_f32) and by canvas position by avd_denoise_step_canvas_guided_f32. */
int avd_dpmpp_2m_sde_step_f32(const float* x_t, const float* eps_hat, float* x0_hist, const int64_t* t_last, const int64_t* t_now,
                              const int64_t* t_prev, const float* alpha_bar, int T_train, float eta, const float* noise, float* x_out,
                              int B, int64_t per_sample, avd_stream_t stream);

/* ---- seeded normal stream of the DDIM eta > 0 noise term (a public contract: the values are fixed by what follows).
 * For sample s = sample_offset + b of a launch, timestep t = t_now[b] and element e of that sample's latent in its natural layout
 * ([C,T,H,W] for video, [Ca,F] for audio, row-major):
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (e >> 2, (uint32) s, (uint32) t, 0x44444D31)          (the last word tags this use of the generator)
 *   (x0, x1, x2, x3) = Philox4x32-10(counter, key)                   (Random123: multipliers 0xD2511F53 / 0xCD9E8D57,
 *                                                                      key increments 0x9E3779B9 / 0xBB67AE85)
 *   Box-Muller on each pair (xa, xb) = (x0, x1) -> (n0, n1) and (x2, x3) -> (n2, n3), in fp32:
 *     u = ((xa >> 8) + 1) * 2^-24  in (0, 1],   v = (xb >> 8) * 2^-24,   r = sqrt(-2 ln u)
 *     n_even = r cos(2 pi v),  n_odd = r sin(2 pi v)
 *   element e takes n[e & 3].
 * The normals are a pure function of (seed, global sample index, t, e): the same bits from avd_gaussian_noise_f32 and from the
 * fused step, at any batch size, rank count, sample_offset split, eager or graph launch, split_streams, matmul mode or DDIM kernel
 * variant.  A captured graph draws fresh noise every step because t comes from the device-side schedule cursor. */
typedef struct {
    uint64_t seed;
    int64_t sample_offset;   /* global index of sample 0 of the call; sample_offset + B <= 2^32 */
} avd_noise_key;
/* out[b, e] = the stream above for sample sample_offset + b at t_now[b], e < per_sample (< 2^34); out: fp32 [B, per_sample].
 * Its output can be passed as the explicit `noise` of the DDIM entries. */
int avd_gaussian_noise_f32(const avd_noise_key* key, const int64_t* t_now, float* out, int B, int64_t per_sample,
                           avd_stream_t stream);

/* ---- canvas-keyed noise: a second keying of the seeded stream above, for windows of one canvas (a public contract).
 * A batch is N consecutive windows of one canvas, `hop` positions apart along the sliding axis, with (outer, L, inner) as in
 * avd_window_consensus_f32: video latent [N,C,T,H,W]: outer = C, L = T, inner = H*W; audio latent [N,Ca,F]: outer = Ca, L = F,
 * inner = 1.  Window b of a call has the global window index w = key.sample_offset + b; its element (o, l, i) sits on canvas position
 *     p = w*hop + l                                                  (computed in 64 bits)
 * and its normal is the value the per-sample stream (avd_noise_key) gives for sample s = p, timestep t = t_now[b] and element
 * e' = o*inner + i: counter (e' >> 2, (uint32) p, (uint32) t, 0x44444D31), the element takes n[e' & 3].  In other words the canvas
 * noise at [b, o, l, i] has the bits of avd_gaussian_noise_f32(key {seed, 0}, t, B = P, per_sample = outer*inner) at [p, e'].
 * Every window that covers a canvas position draws the same bits there, so with z_out_k = det_k + sigma n(p) any weighted mean over
 * the windows under p is mean_w(det_k) + sigma n(p): the noise term passes through avd_window_consensus_f32 for any weights, and
 * consensus sampling at eta > 0 is as well defined as at eta = 0.  The definition does not contain the canvas length: extending a
 * canvas leaves the noise of the positions already there unchanged.  Windows that share a canvas share their timesteps.
 * Arguments, checked before any launch (AVD_EINVAL): hop >= 1; (sample_offset + N - 1)*hop + L <= 2^32; outer*inner < 2^34.
 * Philox, Box-Muller and rounding are those of the per-sample stream (one implementation).  When inner % 4 == 0 and the base is
 * 16-byte aligned a lane's four values lie inside one (o, l) slice and come from one Philox call; otherwise (every audio latent:
 * inner = 1) one call per element.  Same bits either way, and the same bits from avd_canvas_noise_f32 and from the fused step.
 * A latent guide's known-noise stream (avd_latent_guide) has the same two keyings: per sample (sample = key.sample_offset + b; what
 * avd_denoise_step_canvas_f32 and avd_denoise_step_dpmpp_2m_sde_f32 keep when handed a guide) and by canvas position ("canvas-keyed
 * known noise" below; avd_denoise_step_canvas_guided_f32).  DPM-Solver++(2M) at eta > 0 (avd_denoise_step_dpmpp_2m_sde_f32) draws the
 * same canvas-keyed normals as the DDIM step; at eta == 0 it draws nothing. */
/* out[b, o, l, i] = the canvas-keyed normal above; out: fp32 [N, outer, L, inner]; t_now: int64 [N].  Argument order as
 * avd_window_consensus_f32.  Its output can be passed as the explicit `noise` of the DDIM entries. */
int avd_canvas_noise_f32(const avd_noise_key* key, const int64_t* t_now, float* out, int N, int64_t outer, int L, int hop,
                         int64_t inner, avd_stream_t stream);

/* ---- slot timesteps: one (t_now, t_prev) pair per position of the target's sliding axis instead of one per sample (a public contract).
 * Every other entry reads t_now[b], t_prev[b].  The *_slots entries read int64 tables t_now[B*S], t_prev[B*S], row-major [B, S], where a
 * slot is one token position along the sliding axis:
 *   video target: slot s is latent frames s*p0 .. s*p0 + p0 - 1 of a tube (p0, p1, p2); S = T / p0; token n = (t'*Ht + h')*Wt + w' is
 *     in slot t';
 *   audio target: non-overlapping chunks only (stride == len, anything else is AVD_EUNSUPPORTED); slot s is chunk s; S = Na; latent
 *     position f is in slot min(f / len, Na - 1), so the uncovered tail f >= Na*len follows the last slot with eps = 0, as in the
 *     per-sample update.
 * Per slot the semantics are the per-sample ones, with t_now[b, s], t_prev[b, s] in the place of t_now[b], t_prev[b]:
 *   - a target token's timestep columns embed t_now[b, s] (same clamp, frequency table and cos-first order; both CFG halves);
 *   - every latent element of the slot takes the DDIM update with its slot's coefficients; t_prev < 0 means alpha_bar = 1;
 *   - the hold: where t_prev[b, s] == t_now[b, s], z_out is z bit for bit on the slot's elements.  A held token is still embedded
 *     at t_now and still takes part in attention; only its update is skipped (its eps is not read).
 * A table filled with one pair per sample gives the bits of the per-sample entry; a slot gives the bits the per-sample entry gives
 * there when its whole sample runs at the slot's pair.  Attention and the GEMMs are the per-sample step's, launch for launch.
 * Scope, everything else is refused before any launch (AVD_EINVAL): DDIM or DPM-Solver++(2M) (below) at eta == 0 (no noise, no key) or,
 * through the *_slots_seeded entries, at eta > 0 with a slot key ("clip-keyed slot noise" below; no unseeded or explicit noise), the
 * CFG step with the scalar guidance (or, through the *_slots_cfg entries, a "slot CFG control" below), the concat embedding (temb_add ==
 * 0), no latent guide, per-sample CFG control or canvas keying.  Both targets,
 * every matmul / attention mode, both stream layouts (split_streams) and the null half's short layout are taken as by the plain step.
 * `slots` must equal the geometry's S.  Samplers whose positions sit at different noise levels (FIFO-Diffusion, rolling diffusion,
 * continuation from held clean context) are loops over avd_denoise_step_slots_f32. */
/* The fused updates alone, as avd_cfg_unpatch_ddim_f32 / avd_cfg_untoken_ddim_audio_f32 at eta == 0 with t_now, t_prev: int64 [B*slots]. */
int avd_cfg_unpatch_ddim_slots_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                   const float* alpha_bar, int T_train, float guidance, int slots, float* z_out,
                                   int B, int C, int T, int H, int W, int t, int h, int w, avd_stream_t stream);
int avd_cfg_untoken_ddim_audio_slots_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                         const float* alpha_bar, int T_train, float guidance, int slots, float* z_out,
                                         int B, int Ca, int F, int len, int stride, avd_stream_t stream);
/* The slot form of the DPM-Solver++(2M) update (ODE, eta == 0): t_last is a third int64 [B*slots] table and x0_hist [B, per_sample]
 * the history in the latent's natural layout, one value per latent element, so a slot's history is the x0_hist elements of its latent
 * positions.  Per slot the semantics are avd_dpmpp_2m_step_f32's with the triple (t_last, t_now, t_prev)[b, s] in the place of [b]:
 *   - t_last[b, s] < 0 (or a t_last that is not above t_now in noise level: the lambda condition) is a first-order step;
 *   - the slot's x0_hist elements are read only where c_1 != 0, then overwritten with the slot's x0 (DDIM's x0 expression);
 *   - the hold: where t_prev[b, s] == t_now[b, s], z_out is z bit for bit and the slot's x0_hist elements are neither read nor
 *     written (t_last[b, s] is not read either): a slot waiting in a queue's ramp picks up no history;
 *   - audio target: the uncovered tail follows the last slot with eps = 0, its x0_hist elements included.
 * A table that repeats one triple per sample gives the bits of the per-sample DPM step in z_out and in x0_hist
 * (avd_dpmpp_2m_step_f32 on the combined eps; the whole step: avd_denoise_step_dpmpp_2m_f32).  x0_hist must not overlap z or z_out (AVD_EINVAL) and, for the video
 * target and the whole step, must be 16-byte aligned (AVD_EUNSUPPORTED). */
int avd_cfg_unpatch_dpmpp_2m_slots_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                       const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, int slots,
                                       float* x0_hist, float* z_out, int B, int C, int T, int H, int W, int t, int h, int w,
                                       avd_stream_t stream);
int avd_cfg_untoken_dpmpp_2m_audio_slots_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                             const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, int slots,
                                             float* x0_hist, float* z_out, int B, int Ca, int F, int len, int stride,
                                             avd_stream_t stream);

/* ---- clip-keyed slot noise: the slot entries at eta > 0 (a public contract).  Slots of one call sit at different timesteps and move
 * through a queue, so a slot's step noise follows the CLIP POSITION the slot holds, not its place in the batch: the same clip slot
 * draws the same normals in a plain queue or a lookahead queue, eagerly or replayed, whichever sample holds it and whenever.
 * For a batch [B, outer, L, inner] ((outer, L, inner) as in "canvas-keyed noise"), slot_len the tube's p0 (video) or the chunk length
 * (audio) and s = min(l / slot_len, S - 1) the slot of sliding position l (the audio tail follows the last slot, as in "slot
 * timesteps"), element (b, o, l, i) sits on clip position
 *     p = ((first + max(*cursor, 0) + b*stride)*slot_len + l)  mod 2^32       (the sum in 64 bits, then truncated: negative slots wrap,
 *                                                                              as the lookahead's context positions do)
 * and its normal is the per-sample stream's construction (avd_noise_key: the same Philox4x32-10, Box-Muller, rounding, "element takes
 * n[e' & 3]") with counter (e' >> 2, (uint32) p, (uint32) t_now[b, s], 0x534C4F54), e' = o*inner + i.  The last word ("SLOT") is a
 * domain word of its own, and it has to be: a FIFO queue starts, and its tail is filled, with canvas-keyed normals of tag 0x44444D31
 * at positions c*slot_len + j and timestep s_0, and a slot's first step has t_now = s_0 — under the old tag the first step's noise
 * term would be the very normals the slot was initialised with.
 *   - a held slot (t_prev == t_now) draws nothing and stays bit for bit (its x0_hist elements too);
 *   - at eta == 0 nothing is drawn and the key's fields are not read: the bits of the eta == 0 slot entries;
 *   - the final step to t_prev = -1 has DDIM's sigma = 0 and the SDE form's c_n = 0, as in the per-sample contracts;
 *   - the key addresses nothing: whatever the cursor holds no kernel leaves its buffers, and the kernels only read the cursor.
 * Checked before any launch (AVD_EINVAL): a non-null key; at eta > 0 stride >= 1, |first| < 2^32, outer*inner < 2^34.
 * A uniform table (one pair per sample) with explicit noise = avd_slot_noise_f32's output gives the bits of the per-sample entries. */
typedef struct {
    uint64_t seed;
    int64_t  first;          /* clip slot held by slot 0 of sample 0 of the call; may be negative */
    int32_t  stride;         /* clip slots from one sample to the next: S for a queue of samples, S - ctx for lookahead windows; >= 1 */
    const int32_t* cursor;   /* optional device int32 (a "FIFO device cursor"): max(*cursor, 0) is added to first; NULL: 0 */
} avd_slot_key;
/* out[b, o, l, i] = the clip-keyed normal above; out: fp32 [B, outer, L, inner]; t_now: int64 [B*slots]; slots*slot_len <= L (positions
 * past the last slot follow it).  16-byte lanes (one Philox call per four values) when inner % 4 == 0 and out is 16-byte aligned, one
 * element per lane otherwise; same bits either way, and the same bits as the fused draw.  The key is read whatever eta a step has. */
int avd_slot_noise_f32(const avd_slot_key* key, const int64_t* t_now, float* out, int B, int64_t outer, int L, int slots, int slot_len,
                       int64_t inner, avd_stream_t stream);
/* The fused updates alone at eta >= 0: the seeded twins of avd_cfg_unpatch_ddim_slots_f32 / avd_cfg_untoken_ddim_audio_slots_f32.
 * t_last and x0_hist both NULL: the DDIM slot update with sigma(eta) at each slot's pair.  Both set: the slot form of the
 * DPM-Solver++(2M) update in its SDE form (avd_dpmpp_2m_sde_step_f32's coefficients at each slot's triple; x0_hist as in the ODE slot
 * form).  Everything else as those entries. */
int avd_cfg_unpatch_ddim_slots_seeded_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                          const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                          const avd_slot_key* key, int slots, float* x0_hist, float* z_out, int B, int C, int T, int H,
                                          int W, int t, int h, int w, avd_stream_t stream);
int avd_cfg_untoken_ddim_audio_slots_seeded_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                                const avd_slot_key* key, int slots, float* x0_hist, float* z_out, int B, int Ca, int F,
                                                int len, int stride, avd_stream_t stream);

/* ---- clip-keyed latent guide: inpainting / SDEdit for the slot entries (a public contract).  A latent guide needs q(t_prev) at the
 * slot's own noise level, and its known noise has to follow the CLIP POSITION a slot holds while the slot moves through the queue:
 * the shape "clip-keyed slot noise" gives the step noise, applied to the guide.
 * A clip guide is the clean clip canvas known [outer, P, inner] (video [C, P, H, W], inner = H*W; audio [Ca, P], inner = 1), an
 * optional mask canvas of the same layout with values in [0, 1] (NULL: 1 everywhere), a seed, and the slot geometry of avd_slot_key.
 * For a batch [B, outer, L, inner], slot_len and s = min(l / slot_len, S - 1) as above, element (b, o, l, i) sits on clip position
 *     p = (first + max(*cursor, 0) + b*stride)*slot_len + l           in SIGNED 64 bits, NOT wrapped
 *   - p < 0 or p >= P: the element is unguided.  The mask reads as 0 there and known / mask are not read: the comparison comes before
 *     the read, so no cursor value makes a kernel leave the canvases;
 *   - 0 <= p < P: x_k = known[o, p, i], m = mask[o, p, i], and n_k is the per-sample guide stream's value for sample p, element
 *     e' = o*inner + i: counter (e' >> 2, (uint32) p, 0, 0x4B4E5731), the element takes n[e' & 3].  Bit for bit the normal that
 *     "canvas-keyed known noise" puts on canvas position p: a clip guided through the queue and one guided through the consensus loop
 *     share their forward paths.
 * q(tau) = A x_k + S n_k and blend(m, q, z) are avd_latent_guide's, including the a == 1 shortcut and "no contraction".
 * The guided slot step: a stepping slot takes the (seeded) slot update of "slot timesteps" / "clip-keyed slot noise" giving z_out,
 * then, in the same kernel, z_out <- blend(m, q(t_prev[b, s]), z_out).
 *   - a held slot (t_prev == t_now) is z bit for bit: it reads neither the canvases nor the generator, its x0_hist elements are untouched;
 *   - DPM-Solver++(2M)'s x0_hist receives the model's x0_s, not a blended value;
 *   - the final step (t_prev = -1) returns x_k bit for bit where m == 1;
 *   - an all-zero mask, or a canvas every position of the batch misses, gives the bits of the unguided entry;
 *   - when a slot key rides along (eta > 0) its first / stride / cursor must equal the guide's (AVD_EINVAL before any launch).
 * Checked before any launch (AVD_EINVAL): non-null guide and known; 1 <= P <= 2^32; outer*inner < 2^34; stride >= 1; |first| < 2^32;
 * slot_len >= 1 with slots*slot_len <= L; known / mask must not overlap out / z_out / x0_hist.
 * 16-byte lanes (one Philox call per four values) when inner % 4 == 0 and every base is 16-byte aligned, known and mask included; one
 * element per lane otherwise (every audio latent); the same bits either way.
 * Quality is not measured here (no trained weights): the contract is the arithmetic. */
typedef struct {
    const float* known;      /* fp32 [outer, P, inner]: the clean clip canvas */
    const float* mask;       /* fp32 [outer, P, inner] in [0, 1], or NULL = 1 everywhere */
    int64_t  P;              /* clip positions of the canvases */
    uint64_t seed;           /* of the guide's known-noise stream */
    int64_t  first;          /* as avd_slot_key */
    int32_t  stride;
    const int32_t* cursor;
} avd_clip_guide;
#define AVD_SLOT_LEAVE INT64_MIN
/* The stand-alone pass: out = blend(m(p), q_p(tau[b, s]), z) per slot; tau: int64 [B*slots].  tau[b, s] == AVD_SLOT_LEAVE leaves that
 * slot's elements as z, bit for bit.  everywhere != 0 reads the mask as 1 on every in-canvas position (SDEdit's start: q everywhere).
 * out may be z; an in-place call with one slot set touches that slot's bytes alone (a block whose slot is left returns before it
 * loads anything): it is what puts a queue's start, and each entering tail slot, on the forward path at s_0. */
int avd_clip_guide_slots_f32(const avd_clip_guide* g, const int64_t* tau, const float* alpha_bar, int T_train, int everywhere,
                             const float* z, float* out, int B, int64_t outer, int L, int slots, int slot_len, int64_t inner,
                             avd_stream_t stream);
/* The fused updates alone: avd_cfg_unpatch_ddim_slots_seeded_f32 / avd_cfg_untoken_ddim_audio_slots_seeded_f32 ending in the clip
 * guide's blend.  key may be NULL at eta == 0; t_last / x0_hist both NULL or both set, as there. */
int avd_cfg_unpatch_ddim_slots_guided_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                          const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                          const avd_slot_key* key, const avd_clip_guide* guide, int slots, float* x0_hist, float* z_out,
                                          int B, int C, int T, int H, int W, int t, int h, int w, avd_stream_t stream);
int avd_cfg_untoken_ddim_audio_slots_guided_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                                const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                                const avd_slot_key* key, const avd_clip_guide* guide, int slots, float* x0_hist,
                                                float* z_out, int B, int Ca, int F, int len, int stride, avd_stream_t stream);
/* Guided FIFO queue shift (a public contract): the queue step of a guided queue in one launch, the entering slot put on the guide's
 * forward path where it is drawn.  (z_in -> z_out, popped) is avd_fifo_shift_f32's, and with hist_in / hist_out (both NULL or both
 * set) avd_fifo_shift_hist_f32's, except z_out's tail slot, which is
 *     blend(m(p), q_p(t), fresh),   p = c*slot_len + j   in SIGNED 64 bits, compared with [0, P) before anything is read,
 * where fresh is the shift's own canvas-keyed normal for clip slot c at timestep t, and q_p, m and the known-noise stream are
 * avd_clip_guide_slots_f32's (tau = t; alpha_bar [T_train]); everywhere != 0 reads the mask as 1 on every in-canvas position, a NULL
 * mask is 1 everywhere.  Bit for bit the shift followed by the in-place avd_clip_guide_slots_f32 call that leaves every slot but the
 * tail, with `first` chosen so that the tail holds clip slot c: the same "no contraction" rule and a == 1 shortcut, and a lane whose
 * mask values are all 0 skips the generator call.  An all-zero mask, or a tail past the canvas end (c*slot_len >= P), gives the plain
 * shift's bits; a tail that straddles the end is guided on its positions below P only.  popped, every other slot and the history
 * are the plain shift's (the tail's history is zero).
 * guide->first, stride and cursor are NOT read: c names the clip slot.  Checked before the launch (AVD_EINVAL): everything
 * avd_fifo_shift_f32 / _hist_f32 check, then a non-null guide, known and alpha_bar, T_train > 0, 1 <= P <= 2^32, and known / mask
 * must not overlap z_out, hist_out or popped.  16-byte lanes under the shift's rule (known / mask are read as 16-byte values when they
 * are aligned too); one element per lane otherwise; the same bits either way. */
int avd_fifo_shift_guided_f32(const avd_noise_key* key, int64_t t, int64_t c, const avd_clip_guide* guide, const float* alpha_bar,
                              int T_train, int everywhere, const float* z_in, float* z_out, float* popped, const float* hist_in,
                              float* hist_out, int B, int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream);

/* ---- slot CFG control: guidance by noise level, per-slot guidance rescale and per-slot APG for the slot entries (a public contract).
 * The per-sample controls (avd_cfg_control, "adaptive projected guidance") do not carry over to slots: a sample of a queue holds S
 * slots at S noise levels, so a std ratio or a norm cap over the sample mixes nearly clean and pure-noise positions, and what a user
 * varies along a queue is the guidance along the NOISE LEVEL (Kynkaanniemi et al. 2024), which in a queue is the slot's t_now.  Here
 * every coefficient belongs to one slot, and g and phi are looked up by the slot's level inside the kernels: no host tables per
 * iteration, so the ramp, the replayed driver (rows chosen by a device cursor) and the lookahead queue (held duplicates) need nothing.
 * Levels and coefficients.  For slot (b, s), tb = b*S + s, the level is i = min(max(t_now[tb], 0), T_train - 1);
 *     g = guidance_t ? guidance_t[i] : the scalar guidance;        phi = rescale_t ? rescale_t[i] : 0.
 * The combine is cfg_combine(cond, null, g) = null + g (cond - null) in fp32 without contraction, as today: a table whose entries all
 * equal the scalar, with no rescale and no APG, gives the bits of the existing slot entries (eta == 0, seeded or guided).  A level
 * table that is 1 outside an interval is the slot form of the guidance interval (a queue has no cond-only steps: some slot is always
 * inside the interval).
 * The elements of a slot.  Video: the tokens with t' = s, Ht*Wt*D contiguous values of the token layout; per_slot = C*p0*H*W.  Audio
 * (stride == len only, as in "slot timesteps"): token s, per_slot = Ca*len; the uncovered tail f >= Na*len takes no part in the
 * moments and its eps stays 0.  per_slot >= 2.
 * Rescale (rescale_t set).  Steps 3 and 4 of avd_cfg_control with n = per_slot, c the slot's cond values and y its combined values:
 * the fp64 moments run over chunks of 1024 elements in TOKEN order counted from the slot's first element, each chunk's partial is
 * written with plain stores and the partials are summed in index order; s is rounded once to fp32 and is 1 when sigma_y == 0 or the
 * result is not finite; r(e) is avd_cfg_control's, unchanged.
 * APG (apg != 0; excludes rescale_t).  Items 1 and 3 to 5 of "adaptive projected guidance" per slot with beta = 0: d = c - u, the
 * chunks are 1024 elements in the LATENT order of the slot alone ((c, t in slot, h, w) for video, (ch, j) for audio), r caps the
 * SLOT's L2 norm of d: a threshold chosen for a whole sample of S slots corresponds to r / sqrt(S) per slot.  With momentum == 0
 * there is no buffer and nothing of item 2; a momentum is "slot APG momentum" below.
 * Partition rule.  At S == 1 the slot is the sample: both partitions, and therefore every coefficient and every output bit, are
 * those of the per-sample controlled entries (avd_denoise_step_cfg_f32 / avd_denoise_step_apg_f32) with g_b = guidance_t[t_now[b]]
 * and phi_b = rescale_t[t_now[b]] (audio: where the chunk covers the whole latent, F == len).
 * Invariance.  A slot's coefficients are a pure function of the slot's eps tokens, its g and the slot geometry: the same whatever B
 * and S are, whichever (b, s) holds the slot, whatever the other slots do, eager or replayed, under either split_streams setting.
 * Held slots (t_prev == t_now) are z bit for bit: their statistics blocks return before they load anything, the finalize pass
 * stores the neutral (1, 0, 0, 0) for them, and their tables and x0_hist elements are not read.
 * Order within a stepping slot: combine -> rescale or APG -> the solver update (DDIM, seeded DDIM with the slot key, DPM-Solver++(2M)
 * or its SDE form; x0_hist receives the x0 of the controlled eps) -> the clip guide's blend last.
 * Scratch.  Needed when rescale_t or apg is set (a guidance table alone launches no statistics pass): avd_slot_cfg_stats_bytes(B, S,
 * per_slot) bytes, 16-byte aligned; its last 16*B*S bytes hold per slot (s, g, phi, 0) after a rescale call, (s, k, w, g) after an
 * APG call.
 * Checked before any HIP call, in this order: AVD_EINVAL for a null cfg, apg together with rescale_t, r < 0 or NaN, eta_p outside
 * [0, 1] or NaN, a missing or short scratch (B*S > 65535 and per_slot < 2 count as short); AVD_EUNSUPPORTED for a misaligned
 * scratch; AVD_EINVAL for a scratch overlapping z, z_out, x0_hist or the eps tokens (the whole step: the workspace), and for
 * everything the slot entries already check.  The kernels trust the device values: table entries that are NaN or outside their range
 * are not detected there (DenoiseEngine.set_slot_cfg / schedule_utils.level_table check them before upload).
 * Limits: the per-sample avd_cfg_control / avd_apg_control stay refused under slot timesteps; overlapping audio chunks stay
 * refused.  Quality is not measured here (no trained weights): the contract is the arithmetic. */
typedef struct {
    const float* guidance_t;   /* fp32 [T_train] on the device, or NULL = the scalar guidance */
    const float* rescale_t;    /* fp32 [T_train] phi in [0, 1], or NULL = no rescale */
    int32_t apg;               /* 1: adaptive projected guidance per slot (excludes rescale_t) */
    float norm_threshold;      /* r >= 0, as avd_apg_control; read when apg */
    float eta_parallel;        /* in [0, 1], as avd_apg_control; read when apg */
    void* stats;               /* caller-owned scratch, needed when rescale_t or apg is set */
    int64_t stats_bytes;       /* its size */
} avd_slot_cfg;
/* The control with the two trailing fields of "slot APG momentum" (below).  avd_slot_cfg keeps its 48 bytes, so callers built against
 * it stay valid; a caller that wants the momentum passes &m.cfg of this struct to the same entries with cfg.apg ==
 * AVD_SLOT_APG_MOMENTUM, which tells them that the two fields follow.  Never set that value on a plain avd_slot_cfg. */
#define AVD_SLOT_APG_MOMENTUM 2
typedef struct {
    avd_slot_cfg cfg;          /* apg == AVD_SLOT_APG_MOMENTUM: per-slot APG, and the fields below are read */
    float momentum;            /* beta, finite; 0: none (momentum_buf NULL) */
    float* momentum_buf;       /* fp32 [B, per_sample], latent layout: a stepping slot's elements are read, then overwritten with d */
} avd_slot_cfg_momentum;
/* Bytes of the statistics scratch of B*slots slots of per_slot (>= 2) elements; -1 on bad arguments (B*slots outside [1, 65535]). */
int64_t avd_slot_cfg_stats_bytes(int B, int slots, int64_t per_slot);
/* The fused updates alone: avd_cfg_unpatch_ddim_slots_guided_f32 / avd_cfg_untoken_ddim_audio_slots_guided_f32 under the control.  key
 * may be NULL at eta == 0, guide may be NULL (no clip guide); t_last / x0_hist both NULL or both set, as there. */
int avd_cfg_unpatch_ddim_slots_cfg_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                       const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                       const avd_slot_key* key, const avd_clip_guide* guide, int slots, float* x0_hist, float* z_out,
                                       int B, int C, int T, int H, int W, int t, int h, int w, const avd_slot_cfg* cfg,
                                       avd_stream_t stream);
int avd_cfg_untoken_ddim_audio_slots_cfg_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                             const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                             const avd_slot_key* key, const avd_clip_guide* guide, int slots, float* x0_hist,
                                             float* z_out, int B, int Ca, int F, int len, int stride, const avd_slot_cfg* cfg,
                                             avd_stream_t stream);

/* ---- slot APG momentum: APG's momentum per slot, in a buffer that travels with its slot through the queue (a public contract).
 * The third part of "adaptive projected guidance" for the slot entries: momentum (beta) and momentum_buf (M), the two fields that
 * trail the control in avd_slot_cfg_momentum.  The entries take that struct through its first member, with cfg.apg ==
 * AVD_SLOT_APG_MOMENTUM; avd_slot_cfg itself is unchanged (any other non-zero apg is the momentum-free APG, and nothing behind the 48
 * bytes is read), so momentum without apg cannot be stated.
 * The buffer.  M is fp32 [B, per_sample] in LATENT layout, caller-owned, indexed as x0_hist is: slot (b, s) owns the elements of its
 * slot_len positions of the sliding axis.  Audio: stride == len only, as everywhere under slot timesteps; the uncovered tail f >=
 * Na*len is never read or written.
 * A stepping slot, beta != 0.  Item 2 of "adaptive projected guidance" per slot: d = d0 + beta m_prev in fp32 without contraction,
 * d0 = c - u, m_prev the slot's elements of M.  The moments S_dd, S_dc, S_cc of "slot CFG control" run over this d (the slot's
 * latent order, chunks of 1024, fp64 partials summed in index order) and give (s, k, w, g) by the same expressions.  The fused update
 * stores d back into the slot's elements of M and steps on e = c + w (d - k c).  The order within the slot is unchanged: combine ->
 * APG -> the solver update (DDIM, seeded DDIM with the slot key, DPM-Solver++(2M) or its SDE form; x0_hist receives the x0 of e) ->
 * the clip guide's blend last.  The statistics launch reads m_prev before the fused launch that overwrites it starts (one stream).
 * A held slot (t_prev == t_now) neither reads nor writes M, and is z bit for bit.
 * An entering slot's momentum is zero (avd_fifo_carry_f32 below), so a slot's first step has d = d0 + beta*0: the bits of the
 * momentum-free slot APG except where d0 is -0.0 (-0.0 + 0.0 = +0.0).
 * Invariance.  A slot's coefficients and output are a pure function of its eps tokens, its g, the slot geometry and its own elements
 * of M: the same wherever the slot sits in the batch, eager or replayed, under either split_streams setting.
 * Partition rule.  At S == 1 the step equals avd_denoise_step_apg_f32 with momentum = beta and g_b = guidance_t[t_now[b]], bit for
 * bit, output and buffer (audio: where F == len).
 * Checked before any HIP call, after the control's parameter ranges: AVD_EINVAL for a beta that is not finite and for a buffer that
 * is not set exactly when beta != 0; then, behind the scratch's checks, AVD_EUNSUPPORTED for a
 * buffer that is not 16-byte aligned and AVD_EINVAL for one that overlaps z, z_out, x0_hist, the scratch or the eps tokens (the whole
 * step: the workspace).  momentum == 0 and momentum_buf == NULL is "slot CFG control" as it was, launch for launch.
 * The carry.  avd_fifo_carry_f32 takes a slot-attached buffer of the batch's layout [B, outer, slots*slot_len, inner] through the
 * queue move, out of place (in and out must not overlap: AVD_EINVAL).  It applies exactly the map avd_fifo_lookahead_hist_f32
 * applies to its history: with h = slots - ctx, out window b position s >= ctx = the owner copy of logical slot b*h + s + shift of
 * `in` (window (q - ctx) / h, position ctx + (q - ctx) % h); the entering tail slot (shift == 1) and every context position s < ctx
 * are zero.  ctx == 0, shift == 1 is the history map of avd_fifo_shift_hist_f32; shift == 0 moves nothing and copies the stepping
 * positions.  The map reads neither a clip slot nor a cursor, so the same launch follows the eager shift, the lookahead move and the
 * cursor shift of a captured graph.  16-byte lanes when inner % 4 == 0 and both bases are 16-byte aligned, one element per lane
 * otherwise: the same bits.  It is a launch of its own beside the four shift kernels on purpose: one launch is below the loop's
 * resolution (profiles/fifo_guided_shift_e2e.txt). */
int avd_fifo_carry_f32(const float* in, float* out, int B, int64_t outer, int slots, int ctx, int shift, int slot_len, int64_t inner,
                       avd_stream_t stream);

/* ---- FIFO queue shift: the queue step of diagonal denoising (FIFO-Diffusion, Kim et al. 2024) in one out-of-place launch.
 * The batch z_in [B, outer, L, inner] ((outer, L, inner) as in "canvas-keyed noise") with L = slots*slot_len is read as a queue of
 * B*slots slots: queue slot q lives in sample q / slots at positions (q % slots)*slot_len .. + slot_len - 1 of the sliding axis.
 *   z_out slot q = z_in slot q + 1 for q < B*slots - 1, crossing sample boundaries;
 *   popped [outer, slot_len, inner] = z_in slot 0 (the finished head);
 *   z_out's tail slot = fresh noise for slot c of the clip: the canvas-keyed normals of canvas positions c*slot_len + j at timestep t,
 *     bit for bit avd_canvas_noise_f32(key {seed, sample_offset = c}, t_now = {t}, N = 1, outer, L = slot_len, hop = slot_len, inner).
 * key->sample_offset is not read: c (by value) is the window index.  A queue initialised with avd_canvas_noise_f32(key {seed, 0}, t,
 * N = B, outer, L, hop = L, inner) holds clip slots 0 .. B*slots - 1, and the shift number m (c = B*slots + m) appends the next one:
 * slot c of the clip starts from the same normals however long the clip runs.
 * Checked before the launch (AVD_EINVAL): 0 <= t < 2^32; c >= 0 and (c + 1)*slot_len <= 2^32; outer*inner < 2^34; z_in, z_out and
 * popped must not overlap one another.  16-byte lanes when inner % 4 == 0 and the three bases are 16-byte aligned, one element per
 * lane otherwise (every audio latent); same bits either way. */
int avd_fifo_shift_f32(const avd_noise_key* key, int64_t t, int64_t c, const float* z_in, float* z_out, float* popped,
                       int B, int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream);
/* FIFO queue shift with history: the same launch carries a multistep solver's per-element history (x0_hist of the slot form of
 * DPM-Solver++(2M)) along with its slot.  (z_in -> z_out, popped) is avd_fifo_shift_f32's, the same bits and the same tail noise;
 * hist_out slot q = hist_in slot q + 1 for q < B*slots - 1, and hist_out's tail slot is zero (the entering slot has no history: its
 * t_last is -1, so the zeros are never read; they keep the buffer defined).  The head's history is dropped.  Out of place for both
 * pairs; z_in, z_out, popped, hist_in and hist_out must not overlap one another (AVD_EINVAL), the other checks are avd_fifo_shift_f32's.
 * 16-byte lanes when inner % 4 == 0 and all five bases are 16-byte aligned, one element per lane otherwise; same bits either way. */
int avd_fifo_shift_hist_f32(const avd_noise_key* key, int64_t t, int64_t c, const float* z_in, float* z_out, float* popped,
                            const float* hist_in, float* hist_out, int B, int64_t outer, int slots, int slot_len, int64_t inner,
                            avd_stream_t stream);

/* ---- FIFO lookahead: overlapping queue windows with held context (lookahead denoising, the second half of FIFO-Diffusion).
 * With S = slots and a lookahead ctx in 0 .. S - 1, the first ctx slots of every sample are context only and h = S - ctx is the
 * window stride, the number of slots a sample updates.
 *   - the logical queue has Q = ctx + B*h slots: slots 0 .. ctx - 1 are the context (the most recently finished slots), slot ctx + a
 *     is active slot a, a = 0 .. n - 1, n = B*h; active slot 0 is the head, n - 1 the tail (the schedule has n steps);
 *   - window k is sample k of the batch and holds logical slots k*h .. k*h + S - 1: its first ctx slots are held by the step
 *     (t_prev == t_now, "slot timesteps"), its last h slots step, and the stepping slots of all windows tile the active queue once;
 *   - a logical slot lives in up to ceil(S / h) windows.  Its owner copy is the one in a stepping position: active slot a in window
 *     a / h at slot ctx + a % h; context slot q in window 0 at slot q.  Every other copy is a read-only duplicate.
 *   - the plan invariant (schedule_utils.fifo_lookahead_plan): a duplicate is held at the timestep its owner takes as t_now in the
 *     same call, so every copy of a slot embeds the same timestep.
 * One out-of-place launch keeps the copies coherent, pops the head and draws the tail.  Old[q], q < Q, is the owner copy of logical
 * slot q in z_in; Old[Q] is the fresh tail, bit for bit the canvas-keyed normals avd_fifo_shift_f32 draws for clip slot c at
 * timestep t.  With shift in {0, 1}:
 *   z_out window k slot s = Old[k*h + s + shift];
 *   shift == 1: popped [outer, slot_len, inner] = Old[ctx], the head the step has just finished, which is also what becomes context
 *     slot ctx - 1; Old[0] is dropped;
 *   shift == 0: nothing is popped (popped must be null) and nothing is drawn (key, t and c are not read): the launch only refreshes
 *     every duplicate from its owner, which a queue's ramp needs after each of its steps.
 * ctx == 0, shift == 1 gives the bits of avd_fifo_shift_f32.  A finished slot costs B = n/h sample-steps against n/S without
 * lookahead: a factor S/h, 2 at ctx = S/2.
 * Checked before the launch (AVD_EINVAL): 0 <= ctx < slots; shift in {0, 1}; popped null exactly when shift == 0; at shift == 1 the
 * key, t and c as in avd_fifo_shift_f32; outer*inner < 2^34; no two buffers overlap.  All index arithmetic is 64-bit.  16-byte lanes
 * when inner % 4 == 0 and every base is 16-byte aligned, one element per lane otherwise; same bits either way. */
int avd_fifo_lookahead_f32(const avd_noise_key* key, int64_t t, int64_t c, int shift, const float* z_in, float* z_out, float* popped,
                           int B, int64_t outer, int slots, int ctx, int slot_len, int64_t inner, avd_stream_t stream);
/* FIFO lookahead with history (the x0_hist of the slot form of DPM-Solver++(2M)): (z_in -> z_out, popped) as above; hist_out at the
 * stepping positions (s >= ctx) follows the same map from hist_in's owner copies, with zeros in the entering tail slot, and every
 * context position (s < ctx) of hist_out is zero: held slots neither read nor write history, the zeros keep the buffer defined.
 * ctx == 0, shift == 1 gives the bits of avd_fifo_shift_hist_f32.  The buffers must not overlap one another (AVD_EINVAL). */
int avd_fifo_lookahead_hist_f32(const avd_noise_key* key, int64_t t, int64_t c, int shift, const float* z_in, float* z_out,
                                float* popped, const float* hist_in, float* hist_out, int B, int64_t outer, int slots, int ctx,
                                int slot_len, int64_t inner, avd_stream_t stream);

/* ---- FIFO device cursors: the three host numbers of a FIFO iteration moved onto the device, so that a whole iteration is a fixed
 * chain of launches a HIP graph can hold.  A cursor is one int32 in device memory.  No entry below addresses by a cursor without the
 * clamp or the guard its contract names, so no cursor value makes a kernel leave its buffers; every entry only READS its cursor, and
 * avd_cursor_add moves it in a launch of its own, behind the last launch of the iteration that reads it. */
/* *cursor += delta, one launch of one thread on `stream`. */
int avd_cursor_add(int32_t* cursor, int delta, avd_stream_t stream);
/* Slot-table select, the slot analogue of avd_sched_advance / avd_sched_advance_ms: tab0, tab1 (and tab2, or null with out2 null) are
 * [n_rows, n] int64 tables (n = B*slots: the ramp rows of a FIFO plan, t_now / t_prev / t_last); one launch copies row
 * min(max(*cursor, 0), n_rows - 1) of each into its fixed [n] buffer out0, out1 (, out2).  The clamp is the guard: any cursor reads a
 * row of the tables.  Checked (AVD_EINVAL): n_rows >= 1, n >= 1, non-null pointers, tab2 and out2 both set or both null. */
int avd_slot_tables_select(const int64_t* tab0, const int64_t* tab1, const int64_t* tab2, int n_rows, int n, const int32_t* cursor,
                           int64_t* out0, int64_t* out1, int64_t* out2, avd_stream_t stream);
/* Prompt gather: out [B, outer, prompt_len, inner] from the prompt canvas [outer, P, inner] (audio [Ca, P]: inner = 1; video
 * [C, P, H, W]: inner = H*W).  With m = max(*cursor, 0), out[k, o, l, i] = canvas[o, (m + k*slots)*prompt_hop + l, i] where that
 * position is < P and 0 beyond the canvas end: a position is compared with P before it is read, so any cursor stays inside the canvas.
 * All index arithmetic is 64-bit.  16-byte lanes when inner % 4 == 0 and both bases are 16-byte aligned, one element per lane otherwise;
 * same bits either way.  Checked (AVD_EINVAL): positive dims, B*slots and prompt_len fit an int, out does not overlap the canvas. */
int avd_fifo_prompt_gather_f32(const float* canvas, const int32_t* cursor, float* out, int B, int slots, int prompt_hop, int64_t outer,
                               int64_t P, int64_t prompt_len, int64_t inner, avd_stream_t stream);
/* ---- fractional prompt hop (a public contract): the prompt gather for a prompt that has a rational number of positions per target
 * slot (a video prompt under an audio target: 12 * 4 / 150 = 8 / 25 at the shipped geometry).  The hop is a reduced fraction num / den
 * of prompt positions per target slot, 1 <= num, den < 2^31.  For the target slot with clip index q (any int64 with |q| < 2^31;
 * negative in the lookahead queue), in 64-bit integers:
 *     i0  = floor(q * num / den)      (a floor division, also for q < 0)
 *     rem = q * num - i0 * den        (in [0, den))
 * Row l (0 <= l < prompt_len) of the slot's prompt window is then, by `interp`:
 *   0, "nearest":  canvas position i0 + l + (2 * rem >= den ? 1 : 0): real latents only, the window lags or leads the slot by at most
 *                  half a position; a tie (2 * rem == den) rounds up.
 *   1, "linear":   with a = canvas[i0 + l] and b = canvas[i0 + l + 1] the value a + f * (b - a), evaluated in fp32 in that order
 *                  without contraction, f = (float)rem / (float)den (one correctly rounded fp32 division).  When rem == 0 the value
 *                  is a itself and b is not read (an inf or NaN neighbour does not leak).
 * In both modes a position < 0 or >= P reads as 0, in either operand, and is compared before it is loaded: no q makes the kernel leave
 * the canvas, and the last in-canvas row of a linear window blends toward 0.  den == 1 gives, in both modes, the bits of
 * avd_fifo_prompt_gather_f32.  Which mode serves a trained model better is the user's choice; it cannot be measured on synthetic
 * weights.  The pure-torch restatement is stream_infer.fifo_prompt_windows(prompt_den=, prompt_interp=).
 * avd_fifo_prompt_gather_frac_f32: out [B, outer, prompt_len, inner] from the canvas [outer, P, inner]; sample k holds clip slot
 * q = first + max(*cursor, 0) + k*stride.  `cursor` may be null and then reads as 0 (the eager drivers pass m by value in `first`);
 * `first` may be negative and `stride` below the slots of a sample, so one entry serves the plain queue (first = 0, stride = slots,
 * m off the cursor), the eager loop (first = m) and the lookahead's overlapping windows (first = m - ctx, stride = slots - ctx).  A
 * cursor from which sample 0 starts at or past P gives zeros everywhere, as every larger one does: the kernel clamps the cursor there,
 * which changes no value and keeps q * num in range whatever the cursor holds.  q, i0 and rem are computed once per lane.  16-byte
 * lanes when inner % 4 == 0 and both bases are 16-byte aligned, one element per lane otherwise (every audio prompt: inner = 1); same
 * bits either way.  Checked before the launch (AVD_EINVAL): non-null canvas and out, positive dims, num >= 1, den >= 1, interp 0 or 1,
 * |first|, B*stride and prompt_len below 2^31, the largest |q| of the call times num below 2^62, out does not overlap the canvas. */
int avd_fifo_prompt_gather_frac_f32(const float* canvas, const int32_t* cursor, float* out, int B, int64_t first, int stride, int num,
                                    int den, int interp, int64_t outer, int64_t P, int64_t prompt_len, int64_t inner,
                                    avd_stream_t stream);
/* FIFO queue shift off a device cursor: (z_in -> z_out) is avd_fifo_shift_f32's with c = c0 + *cursor, the same kernel body and the
 * same bits (c only keys the tail's noise draw, modulo 2^32: it addresses nothing).  The finished head is written straight into slot
 * *cursor of the clip canvas clip [outer, n_out*slot_len, inner] — clip[o, *cursor*slot_len + j, i] = z_in slot 0 [o, j, i], a strided
 * write, no popped buffer.  The guard: when *cursor is outside [0, n_out) the head is written nowhere; the queue still shifts.
 * Checked before the launch (AVD_EINVAL): c0 >= 0, n_out >= 1 and (c0 + n_out)*slot_len <= 2^32; z_in, z_out and the clip canvas
 * must not overlap one another; the other checks are avd_fifo_shift_f32's.  16-byte lanes when inner % 4 == 0 and all bases are
 * 16-byte aligned, one element per lane otherwise; same bits either way. */
int avd_fifo_shift_cursor_f32(const avd_noise_key* key, int64_t t, int64_t c0, const int32_t* cursor, int64_t n_out, const float* z_in,
                              float* z_out, float* clip, int B, int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream);
/* As avd_fifo_shift_cursor_f32 with the history pair of avd_fifo_shift_hist_f32 (hist_out slot q = hist_in slot q + 1, zeros in the
 * tail); the five buffers, the clip canvas among them, must not overlap one another. */
int avd_fifo_shift_cursor_hist_f32(const avd_noise_key* key, int64_t t, int64_t c0, const int32_t* cursor, int64_t n_out,
                                   const float* z_in, float* z_out, float* clip, const float* hist_in, float* hist_out, int B,
                                   int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream);

/* ---- FIFO clip batch (a public contract): K independent clips denoised as K queues in lockstep inside one batch, so that one model
 * call finishes one slot of every clip.  The slot entries allow it as they are (samples never attend to one another, the slot tables
 * are per sample, the slot CFG control is per slot); this entry is the queue step of such a batch in one out-of-place launch.
 * Layout.  The batch [B, outer, L, inner] with B = K*B_q and L = slots*slot_len is K queues: queue k is samples k*B_q .. (k+1)*B_q - 1
 * and has B_q*slots slots, slot q of it in sample k*B_q + q / slots at positions (q % slots)*slot_len ...
 *   z_out slot q of queue k = z_in slot q + 1 of queue k for q < B_q*slots - 1, crossing the sample boundaries inside the queue and
 *     never the boundary between two queues;
 *   z_out's tail slot of queue k = the canvas-keyed normals of clip slot c at timestep t under seeds[k], bit for bit what
 *     avd_fifo_shift_f32 draws with avd_noise_key{seeds[k]}.  seeds: K uint64 values in device memory (8-byte aligned); c and t are
 *     shared by the queues, which run in lockstep;
 *   the head (slot 0) of queue k is written straight into slot m of clip canvas k, clips [K, outer, n_clip*slot_len, inner]:
 *     clips[k, o, m*slot_len + j, i] = z_in[k*B_q, o, j, i], a strided write as avd_fifo_shift_cursor_f32's, with m by value.  m outside
 *     [0, n_clip) writes no head (the queues still shift): m is compared before the address is formed;
 *   riders: (hist_in, hist_out) and (carry_in, carry_out), each both NULL or both set, are buffers of z's layout that take the same
 *     map with zeros in every entering tail slot: the map of avd_fifo_shift_hist_f32's history, which avd_fifo_carry_f32 applies at
 *     ctx == 0, shift == 1.  The first carries DPM-Solver++(2M)'s x0_hist, the second the slot APG momentum; either may ride alone.
 * Equivalence.  The launch is bit for bit K calls of avd_fifo_shift_f32 (avd_fifo_shift_hist_f32 with a history) on the K slices with
 * keys {seeds[k]}, K copies of `popped` into the canvases and, with a carry pair, K avd_fifo_carry_f32 calls on its slices.  K == 1
 * gives the existing entries' bits.
 * Checked before the launch (AVD_EINVAL): everything avd_fifo_shift_f32 checks (the dims, 0 <= t < 2^32, c >= 0 and (c + 1)*slot_len
 * <= 2^32, outer*inner < 2^34); K >= 1 and K divides B; non-null seeds and clips; 1 <= n_clip and n_clip*slot_len <= 2^32; each rider
 * pair both NULL or both set; no two buffers overlap, the canvases and the seeds included.  All index arithmetic is 64-bit.  16-byte
 * lanes when inner % 4 == 0 and every base is 16-byte aligned, one element per lane otherwise (every audio latent); the same bits
 * either way.  Limits of the drivers built on it (stream_infer.fifo_denoise_clips): the plain eager queue only, and the clips share
 * n_clip; eta > 0 and a latent guide per clip ride on "clip batch keying" below. */
int avd_fifo_shift_clips_f32(const uint64_t* seeds, int64_t t, int64_t c, const float* z_in, float* z_out, float* clips, int64_t n_clip,
                             int64_t m, const float* hist_in, float* hist_out, const float* carry_in, float* carry_out, int B, int K,
                             int64_t outer, int slots, int slot_len, int64_t inner, avd_stream_t stream);

/* ---- clip batch keying (a public contract): the step noise and the latent guide of a FIFO clip batch, one seed and one canvas per
 * queue.  avd_slot_key and avd_clip_guide carry one seed, one canvas and one clip-position walk first + b*stride over the whole batch;
 * in a clip batch the K queues restart that walk and own their seeds and canvases.  A batch [B, outer, L, inner] with B = K*B_q is K
 * queues; sample b is sample b' = b mod B_q of queue k = b / B_q.  With a descriptor present the keying of "clip-keyed slot noise" and
 * "clip-keyed latent guide" changes as follows, and nothing else does.
 *   Step noise.  Element (b, o, l, i) sits on clip position p = ((first + max(*cursor, 0) + b'*stride)*slot_len + l) mod 2^32 and draws
 *     that contract's normal under seed step_seeds[k]: same counter words, same SLOT domain word, same lane rules.  key->seed is not read.
 *   Clip guide.  guide->known and guide->mask are [K, outer, P, inner] (the mask may be NULL: 1 everywhere).  Queue k reads canvas k at
 *     p = (first + max(*cursor, 0) + b'*stride)*slot_len + l, signed and unwrapped, compared with [0, P) before anything is read; its
 *     known noise is the guide stream under guide_seeds[k].  guide->seed is not read.
 * Equivalence.  A call with a descriptor is bit for bit K calls of the existing entry on the K sample slices, with
 * avd_slot_key{step_seeds[k], first, stride, cursor} and avd_clip_guide{known[k], mask[k], P, guide_seeds[k], first, stride, cursor}.
 * K == 1 gives the existing entries' bits.  A held slot, eta == 0, the final step, the all-zero mask and the "no contraction" rule are
 * unchanged.  The seeds are read on the device at every launch, so a graph driver can swap them; K is held by value.
 * Checked before any launch (AVD_EINVAL): everything the existing entries check; K >= 1 and K divides B; non-null, 8-byte aligned
 * step_seeds at eta > 0 (with a slot key) and guide_seeds with a guide; the K canvases together must not overlap z_out (out), x0_hist
 * or the seeds, and the seeds must not overlap z_out (out) or x0_hist.  All index arithmetic is 64-bit. */
typedef struct {
    int32_t K;                    /* queues; K >= 1 and K divides B */
    const uint64_t* step_seeds;   /* K uint64 on the device, 8-byte aligned; read only at eta > 0 (may be NULL at eta == 0) */
    const uint64_t* guide_seeds;  /* K uint64 on the device; read only with a clip guide (NULL without one) */
} avd_clip_queues;
/* avd_slot_noise_f32 with the descriptor: t_now int64 [B*slots]. */
int avd_slot_noise_clips_f32(const avd_slot_key* key, const avd_clip_queues* queues, const int64_t* t_now, float* out, int B,
                             int64_t outer, int L, int slots, int slot_len, int64_t inner, avd_stream_t stream);
/* avd_clip_guide_slots_f32 with the descriptor.  One in-place launch with AVD_SLOT_LEAVE everywhere except each queue's tail slot puts
 * all K entering slots on their forward paths. */
int avd_clip_guide_slots_clips_f32(const avd_clip_guide* g, const avd_clip_queues* queues, const int64_t* tau, const float* alpha_bar,
                                   int T_train, int everywhere, const float* z, float* out, int B, int64_t outer, int L, int slots,
                                   int slot_len, int64_t inner, avd_stream_t stream);
/* The fused updates alone: avd_cfg_unpatch_ddim_slots_cfg_f32 / avd_cfg_untoken_ddim_audio_slots_cfg_f32 with the descriptor.  cfg may
 * be NULL here (the scalar guidance), key may be NULL at eta == 0, guide may be NULL; a descriptor with neither an eta > 0 key nor a
 * guide changes nothing. */
int avd_cfg_unpatch_ddim_slots_clips_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                         const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                         const avd_slot_key* key, const avd_clip_guide* guide, const avd_clip_queues* queues, int slots,
                                         float* x0_hist, float* z_out, int B, int C, int T, int H, int W, int t, int h, int w,
                                         const avd_slot_cfg* cfg, avd_stream_t stream);
int avd_cfg_untoken_ddim_audio_slots_clips_f32(const float* eps2, const float* z, const int64_t* t_last, const int64_t* t_now,
                                               const int64_t* t_prev, const float* alpha_bar, int T_train, float guidance, float eta,
                                               const avd_slot_key* key, const avd_clip_guide* guide, const avd_clip_queues* queues,
                                               int slots, float* x0_hist, float* z_out, int B, int Ca, int F, int len, int stride,
                                               const avd_slot_cfg* cfg, avd_stream_t stream);

/* ---- latent guide: inpainting / outpainting and SDEdit over a known clean latent (a public contract).
 * Per sample b of a call, with x_k = known[b] and m = the mask, both in the latent's natural layout ([C,T,H,W] video, [Ca,F] audio,
 * row-major; element e as in avd_noise_key), and a(tau) = alpha_bar[clamp(tau, 0, T_train-1)] for tau >= 0, 1 for tau < 0:
 *   1. known-noise stream n_k(s, e): the avd_noise_key construction (key.seed) with counter (e >> 2, (uint32) s, 0, 0x4B4E5731)
 *      and s = key.sample_offset + b.  The counter holds no timestep: each element keeps one normal for the whole trajectory, so
 *      the known region follows one deterministic forward path.  The last word tags this use of the generator (DDIM's is 0x44444D31);
 *   2. q(tau) = A x_k + S n_k with A = sqrt(a), S = sqrt(max(1 - a, 0)), in fp32 in that order without contraction;
 *      q = x_k exactly (no arithmetic) when a == 1.0f, which includes tau < 0;
 *   3. blend(m, q, z) = z where m == 0, q where m == 1 (both selects), else (1 - m) z + m q in fp32, in that order, without
 *      contraction: an all-zero mask is bit-identical to no guide, an all-one mask bit-identical to q;
 *   4. the guided step = the step (DDIM at eta = 0, seeded DDIM at eta > 0 or DPM-Solver++(2M)) producing z_out, then
 *      z_out <- blend(m, q(t_prev[b]), z_out) in the same kernel.  DPM's x0_hist still receives the model's x0_s, not a blended
 *      value.  The final step (t_prev = -1) returns x_k bit for bit wherever m == 1. */
typedef struct {
    const float* known;          /* fp32 [B, per_sample], 16-byte aligned */
    const float* mask;           /* fp32, values in [0,1]: [per_sample] (mask_batch_stride 0) or [B, per_sample] (mask_batch_stride
                                    per_sample), 16-byte aligned; NULL = 1 everywhere */
    int64_t mask_batch_stride;   /* 0 or per_sample */
    avd_noise_key key;           /* seed / sample_offset of the known-noise stream */
} avd_latent_guide;
/* out[b] = blend(mask, q(tau[b]), z[b]); z == NULL reads as "mask is 1 everywhere" (pure forward noising: out = q).  out may be z;
 * known / mask must not overlap out.  tau: int64 [B]; z, out: fp32 [B, per_sample]. */
int avd_latent_guide_f32(const avd_latent_guide* g, const int64_t* tau, const float* alpha_bar, int T_train,
                         const float* z, float* out, int B, int64_t per_sample, avd_stream_t stream);

/* ---- canvas-keyed known noise: the second keying of the guide's stream, for windows of one canvas (a public contract; the
 * construction of "canvas-keyed noise" applied to n_k).  A batch is N consecutive windows [N, outer, L, inner] of one canvas, `hop`
 * positions apart ((outer, L, inner) as in avd_window_consensus_f32).  Window b has the global index w = guide.key.sample_offset + b;
 * its element (o, l, i) sits on canvas position
 *     p = w*hop + l                                                  (computed in 64 bits)
 * and takes the known-noise value the per-sample guide stream (step 1 of avd_latent_guide) gives for sample s = p and element
 * e' = o*inner + i: counter (e' >> 2, (uint32) p, 0, 0x4B4E5731), the element takes n[e' & 3].  In other words n_k at [b, o, l, i] has
 * the bits of the per-sample stream of key {seed, 0} over B = P samples of outer*inner elements at [p, e'].  q, blend, the a == 1
 * shortcut (no arithmetic, no generator call) and "no contraction" are exactly those of avd_latent_guide: one implementation.
 * Every window over a canvas position holds q = A x_k + S n_k(p) with the same normal there, so when the windows' known latents agree
 * on their overlaps (one canvas: avd_window_consensus_f32 of the encoded windows, once) a held region passes through the consensus
 * mean as it is, for any weights: it stays on its forward path.  Keyed per sample the mean would shrink the noise term (by 1/sqrt(k)
 * under uniform weights).  The definition does not contain the canvas length.
 * Arguments, checked before any launch (AVD_EINVAL): hop >= 1; (sample_offset + N - 1)*hop + L <= 2^32; outer*inner < 2^34; and
 * avd_latent_guide's own (per_sample = outer*L*inner).  avd_latent_guide keeps its layout: the keying is chosen by the entry. */
/* out[b] = blend(mask, q(tau[b]), z[b]) with the canvas-keyed n_k; argument order as avd_canvas_noise_f32; z == NULL reads as "mask is
 * 1 everywhere"; out may be z; known / mask must not overlap out.  When inner % 4 == 0 and z / out are 16-byte aligned a lane's four
 * values lie inside one (o, l) slice and come from one Philox call; otherwise (every audio latent) one call per element.  Same bits
 * either way, and the same bits from the fused step. */
int avd_latent_guide_canvas_f32(const avd_latent_guide* g, const int64_t* tau, const float* alpha_bar, int T_train,
                                const float* z, float* out, int N, int64_t outer, int L, int hop, int64_t inner, avd_stream_t stream);

/* ---- renoise: the forward jump z_t -> z_t' (t' > t) of RePaint resampling (Lugmayr et al. 2022; a public contract).
 * A resampling schedule (schedule_utils.resample_schedule) sends the trajectory back up the schedule after a stretch of steps and
 * denoises that stretch again, so that the free and the held region of a latent guide meet at a common noise level more than once.
 * Per sample b of a call, with a(tau) as in avd_latent_guide, a_f = a(t_from[b]) and a_t = a(t_to[b]):
 *   1. identity case: if !(a_t < a_f) then out = z bit for bit — no arithmetic and no generator call.  This covers t_to <= t_from
 *      and a_f == 0;
 *   2. jump case: otherwise rho = a_t / a_f, A = sqrt(rho), S = sqrt(max(1 - rho, 0)) and out = A z + S n_r, all in fp32, in that
 *      order, without contraction (q(z_t' | z_t) of the forward process);
 *   3. renoise stream n_r(s, e): the avd_noise_key construction with counter (e >> 2, (uint32) s, (uint32) visit, 0x52504E31) and
 *      s = key.sample_offset + b.  `visit` is one uint32 per launch, passed by value: it names the jump, so a jump taken again (with
 *      another visit) draws fresh normals.  The last word keeps the stream apart from DDIM's (0x44444D31) and the guide's known
 *      noise (0x4B4E5731);
 *   4. with a guide (g != NULL) the launch ends in the guide's blend, out <- blend(mask, q(t_to[b]), out), with the guide_coef /
 *      q / blend of avd_latent_guide, one implementation: a held region leaves the jump on its deterministic forward path, bit for
 *      bit what avd_latent_guide_f32 gives at t_to; the renoised value there is discarded;
 *   5. canvas keying (avd_renoise_canvas_f32): the batch is N consecutive windows of one canvas as in "canvas-keyed noise", window b
 *      at global index w = key.sample_offset + b; element (o, l, i) takes n_r of sample s = p = w*hop + l, element e' = o*inner + i.
 *      The guide's known noise is canvas-keyed too ("canvas-keyed known noise"), and the guide's key must carry the same
 *      sample_offset as the renoise key (AVD_EINVAL otherwise).  Windows that agree on an overlap before the call agree after it:
 *      the same linear map with the same normals.  When inner % 4 == 0 and z / out are 16-byte aligned a lane's four values come
 *      from one Philox call, otherwise (every audio latent) one call per element; same bits either way.
 * Arguments, checked before any launch: avd_noise_key's (per-sample) or those of "canvas-keyed noise" / "canvas-keyed known noise"
 * (canvas), and avd_latent_guide's when g is passed.  out may be z (in place); otherwise they must not overlap; known / mask must
 * not overlap out.  t_from, t_to: int64 [B]; z, out: fp32 [B, per_sample] / [N, outer, L, inner].
 * Limit: the step noise of an eta > 0 sampler keeps its own contract (keyed by t_now, not by visit), so a revisited timestep repeats
 * its step normals; only the renoise normals are fresh per visit. */
int avd_renoise_f32(const avd_noise_key* key, uint32_t visit, const avd_latent_guide* g, const int64_t* t_from, const int64_t* t_to,
                    const float* alpha_bar, int T_train, const float* z, float* out, int B, int64_t per_sample, avd_stream_t stream);
int avd_renoise_canvas_f32(const avd_noise_key* key, uint32_t visit, const avd_latent_guide* g, const int64_t* t_from,
                           const int64_t* t_to, const float* alpha_bar, int T_train, const float* z, float* out, int N, int64_t outer,
                           int L, int hop, int64_t inner, avd_stream_t stream);

/* ---- CFG control: per-sample guidance scales and guidance rescale (Lin et al. 2023, diffusers' rescale_noise_cfg; a public
 * contract).  For sample b of a call, with n = per_sample (>= 2):
 *   1. g_b = guidance[b] when that pointer is set, else the scalar guidance (avd_step_desc.guidance); the token-space combine is
 *      e = null + g_b (cond - null) in fp32 without contraction, as today: an array whose entries all equal g gives the scalar's bits;
 *   2. U maps tokens to the latent's natural layout: the tube un-patch (a permutation) for video, the overlap-add mean with crop /
 *      zero-pad (the loop order of the fused audio step) for audio.  c = U(cond tokens), y = U(combined tokens): y is the eps the
 *      solver consumes without control;
 *   3. moments in fp64 over the n elements, for v = c and v = y: sigma^2 = (S2 - S1^2 / n) / (n - 1) with S1 = sum v, S2 = sum v^2
 *      (the unbiased std, as torch.std); s_b = (float)(sigma_c / sigma_y), rounded once; s_b = 1 when sigma_y == 0 or s_b is not
 *      finite;
 *   4. r(e) = e where phi_b == 0, e s_b where phi_b == 1 (both selects), else phi_b (e s_b) + (1 - phi_b) e in fp32, in that
 *      order, without contraction; phi_b = rescale[b], 0 when that pointer is NULL;
 *   5. the step (DDIM, seeded DDIM or DPM-Solver++(2M)) runs on r(y) in place of y: DPM's x0_hist receives the x0 of r(y); a
 *      latent guide's blend (avd_latent_guide) still comes last.
 * s_b is a pure function of sample b's eps tokens, g_b and the geometry: the fp64 sums run over a partition of the sample fixed by
 * n alone (chunks of 1024 elements in the order of the source layout, tokens for video and the latent for audio), the chunks'
 * partials are stored with plain stores and summed in index order, no float atomics.  s_b is therefore the same at any B,
 * sample_offset, split_streams setting, eager or graph launch.  The kernels trust the device values: phi_b outside [0, 1] or NaN is
 * not detected there (DenoiseEngine / set_cfg / functional.cfg_rescale check them before upload). */
typedef struct {
    const float* guidance;     /* fp32 [B] per-sample guidance scales, or NULL (the scalar) */
    const float* rescale;      /* fp32 [B] per-sample phi in [0, 1], or NULL (phi = 0: no statistics pass, no rescale) */
    void* stats;               /* caller-owned scratch of >= avd_cfg_stats_bytes(B, per_sample) bytes, 16-byte aligned; needed
                                  when rescale is set; must not overlap z_out or x0_hist */
    int64_t stats_bytes;       /* its size */
} avd_cfg_control;
/* Bytes of the statistics scratch of B samples of per_sample (>= 2) elements; -1 on bad arguments. */
int64_t avd_cfg_stats_bytes(int B, int64_t per_sample);
/* The rescale alone, on latent-layout tensors (steps 3 and 4 with c = e_cond, y = e_cfg): out[b] = r(e_cfg[b]).  e_cond, e_cfg,
 * out: fp32 [B, per_sample]; phi: fp32 [B] on the device.  out may alias e_cfg. */
int avd_cfg_rescale_f32(const float* e_cond, const float* e_cfg, const float* phi, void* stats, int64_t stats_bytes, float* out,
                        int B, int64_t per_sample, avd_stream_t stream);

/* ---- adaptive projected guidance (APG; Sadat, Hilliges, Weber 2024; diffusers' AdaptiveProjectedGuidance / normalized_guidance; a
 * public contract).  APG splits the guidance direction cond - null into the part parallel to the conditional prediction, which it
 * damps, and the orthogonal part, which it keeps; it caps the direction's norm and optionally carries a (negative) momentum across
 * steps.  For sample b of a call, with U the token -> latent map of avd_cfg_control item 2 and n = per_sample (>= 2) latent elements:
 *   1. c = U(cond tokens) and u = U(null tokens); for audio two separate overlap-add means, each accumulated in the window order of
 *      the fused audio step; d0 = c - u in fp32;
 *   2. momentum, beta = `momentum`: d = d0 + beta m_prev in fp32 without contraction, m_prev the sample's momentum buffer: fp32
 *      [B, per_sample] in LATENT layout, caller-owned, indexed as x0_hist is; the fused kernel stores d back into it.  beta == 0 means
 *      no buffer: the pointer must then be NULL, d = d0 and nothing is read or written.  A zeroed buffer gives the first step d = d0;
 *   3. moments in fp64 over the n latent elements: S_dd = sum d^2, S_dc = sum d c, S_cc = sum c^2, over a partition fixed by n alone:
 *      chunks of 1024 consecutive LATENT-ORDER elements, for both modalities; each chunk's partial is stored with plain stores and the
 *      partials are summed in index order, no float atomics.  The coefficients are therefore the same at any B, sample_offset,
 *      split_streams setting, eager or graph launch;
 *   4. coefficients, each rounded once to fp32: s_b = (float)min(1, r / sqrt(S_dd)), 1 when r == 0 (no cap), when S_dd == 0 or when
 *      the result is not finite; r = norm_threshold >= 0 caps the whole-sample L2 norm of d, as in diffusers.
 *      k_b = (float)((1 - eta_p) S_dc / S_cc), evaluated left to right in fp64, 0 when S_cc == 0 or when the result is not finite;
 *      eta_p = eta_parallel in [0, 1] is the kept share of the parallel component.  w_b = (g_b - 1.0f) * s_b in fp32, g_b =
 *      guidance[b] when a per-sample array is set, else the scalar;
 *   5. the eps the solver consumes is e = c + w_b * (d - k_b * c) in fp32, in that order, without contraction: the paper's form, cond
 *      + (g - 1) update.  At r = 0, eta_p = 1, beta = 0 it equals plain CFG MATHEMATICALLY BUT NOT IN BITS: plain CFG is evaluated as
 *      null + g (cond - null);
 *   6. the step (DDIM, seeded DDIM, DPM-Solver++(2M) or its SDE form) runs on e in place of the combined eps: DPM's x0_hist receives
 *      the x0 of e; a latent guide's blend (avd_latent_guide) still comes last;
 *   7. scope: guidance rescale (a control whose rescale is set) together with APG is refused: its statistics would need the APG
 *      output.  A cond-only step does not apply APG and leaves the momentum buffer untouched.  Slot timesteps refuse it, as they
 *      refuse every per-sample CFG control: their form is "slot CFG control".  The kernels trust the device values (guidance[b]);
 *      the by-value parameters are range-checked here (NaN refused) and again by DenoiseEngine / functional.apg_guidance.
 * Checked before any HIP call: the scratch's size (avd_apg_stats_bytes) and 16-byte alignment; momentum_buf 16-byte aligned, NULL
 * exactly when momentum == 0, and overlapping none of z, z_out, x0_hist, the scratch and the eps tokens (for the whole step: the
 * workspace); the scratch likewise.  What the effect on sample quality is at a given guidance scale is not measured here: that
 * needs trained weights. */
typedef struct {
    float norm_threshold;      /* r >= 0; 0: no norm cap */
    float eta_parallel;        /* eta_p in [0, 1]; 1 keeps the whole parallel component (with r = 0 and no momentum: CFG) */
    float momentum;            /* beta, finite; 0: no momentum (momentum_buf NULL) */
    float* momentum_buf;       /* fp32 [B, per_sample], latent layout, read then overwritten with d; NULL exactly when momentum == 0 */
    void* stats;               /* caller-owned scratch of >= avd_apg_stats_bytes(B, per_sample) bytes, 16-byte aligned */
    int64_t stats_bytes;       /* its size */
} avd_apg_control;
/* Bytes of the APG statistics scratch of B samples of per_sample (>= 2) elements; -1 on bad arguments.  Its last 16 * B bytes hold
 * (s_b, k_b, w_b, g_b) per sample after a call. */
int64_t avd_apg_stats_bytes(int B, int64_t per_sample);
/* The combine alone, on latent-layout tensors (steps 2 to 5 with c = e_cond, u = e_null): out[b] = e.  e_cond, e_null, out: fp32
 * [B, per_sample]; guidance: fp32 [B] on the device, or NULL for guidance_scalar.  out must not overlap the inputs. */
int avd_apg_guidance_f32(const float* e_cond, const float* e_null, const float* guidance, float guidance_scalar,
                         const avd_apg_control* apg, float* out, int B, int64_t per_sample, avd_stream_t stream);

/* ---- a8 fused: CFG combine + tube un-patch + DDIM — avdiff/models/infer/sample_clip.py:381-389.
 * eps2: [2B,Nv,C*t*h*w] (cond batch then null batch); eps = null + g*(cond-null); un-patched on the fly.
 * z, z_out: [B,C,T,H,W]. */
int avd_cfg_unpatch_ddim_f32(const float* eps2, const float* z, const int64_t* t_now, const int64_t* t_prev,
                             const float* alpha_bar, int T_train, float guidance, float eta,
                             const float* noise, float* z_out,
                             int B, int C, int T, int H, int W, int t, int h, int w, avd_stream_t stream);

/* ---- a8' fused: CFG combine + audio overlap-add + DDIM — sample_clip.py:342-348.
 * eps2: [2B,Na,Ca*len]; z,z_out: [B,Ca,F]. */
int avd_cfg_untoken_ddim_audio_f32(const float* eps2, const float* z, const int64_t* t_now,
                                   const int64_t* t_prev, const float* alpha_bar, int T_train,
                                   float guidance, float eta, const float* noise, float* z_out,
                                   int B, int Ca, int F, int len, int stride, avd_stream_t stream);

/* ---- guidance interval: cond-only steps (Kynkaanniemi et al. 2024, guidance in a limited interval; a public contract).
 * A sampler that applies classifier-free guidance on part of the schedule only takes two kinds of step.  A CFG step is every entry
 * above and avd_denoise_step_*: two branches, eps = null + g (cond - null).  A cond-only step is the single-branch form:
 *   1. eps = eps_cond exactly — the conditional prediction's bits, not null + 1 (cond - null); the null half is neither assembled, nor
 *      run through the core and head, nor read;
 *   2. z_out = update(z, eps): DDIM at eta = 0, DDIM at eta > 0 on explicit or seeded noise, or DPM-Solver++(2M), each the expression of
 *      its CFG twin; then the latent guide's blend (avd_latent_guide) when a guide is passed;
 *   3. per-sample guidance scales and guidance rescale (avd_cfg_control) do not apply: with y = c the rescale is the identity, and no
 *      statistics pass runs;
 *   4. the seeded noise is keyed as in a CFG step (sample, t_now, element): a trajectory's noise does not depend on which steps are
 *      cond-only;
 *   5. DPM-Solver++(2M): x0_hist is read and written as by a CFG step, so the history carries across a boundary between the two kinds
 *      and the solver does not restart first order there.
 * Which steps are cond-only is the caller's decision (DenoiseEngine: t_now outside [t_lo, t_hi]).
 *
 * The single-branch fused updates alone: eps: [B,Nv,C*t*h*w] resp. [B,Na,Ca*len], the conditional prediction.  Optional, NULL when
 * unused: key (with eta > 0: seeded noise, `noise` is not read), t_last + x0_hist (both or neither: the DPM-Solver++(2M) update, eta
 * == 0, x0_hist must not overlap z or z_out), guide (eta > 0 then needs key).  eta > 0 needs noise or key.  Bit-identical to
 * avd_tube_unpatch_f32 / avd_audio_untokens_f32 (no window) followed by avd_ddim_step_f32 / avd_dpmpp_2m_step_f32 and
 * avd_latent_guide_f32. */
int avd_eps_unpatch_ddim_f32(const float* eps, const float* z, const int64_t* t_now, const int64_t* t_prev,
                             const float* alpha_bar, int T_train, float eta, const float* noise, float* z_out,
                             int B, int C, int T, int H, int W, int t, int h, int w, const avd_noise_key* key,
                             const int64_t* t_last, float* x0_hist, const avd_latent_guide* guide, avd_stream_t stream);
int avd_eps_untoken_ddim_audio_f32(const float* eps, const float* z, const int64_t* t_now, const int64_t* t_prev,
                                   const float* alpha_bar, int T_train, float eta, const float* noise, float* z_out,
                                   int B, int Ca, int F, int len, int stride, const avd_noise_key* key,
                                   const int64_t* t_last, float* x0_hist, const avd_latent_guide* guide, avd_stream_t stream);

/* ---- a1+a3+a4+a5 fused front end — sample_clip.py:363-371,377 (A->V) / :322-333,338 (V->A).
 * Builds the CFG-stacked sequence X2[2B, Nt+Np, d] in one pass:
 *   target rows : [ adapter(tokens(z_target)) | temb(t_now[b]) ]   (same in both halves)
 *   prompt rows : Xp[b] in the cond half, zeros in the null half (whole d-wide rows, as the reference)
 * target_kind 0 = video latent [B,C,T,H,W] with tubes (p0,p1,p2)=(t,h,w); 1 = audio latent [B,Ca,F]
 * with chunk (p0,p1)=(len,stride).  target_first != 0 puts target rows before prompt rows
 * (the reference's order is always [video ; audio]).
 * Xp: [B,Np,d] = adapter(prompt tokens) | temb(0), computed once per run by the caller.
 * tok_ws: scratch [B*Nt, tok_dim].  Wt: [d-tdim, tok_dim], bt: [d-tdim]. */
typedef struct {
    int target_kind;      /* 0 video, 1 audio */
    int target_first;
    int B, d, tdim;
    int C, T, H, W;       /* video latent dims (target_kind 0) — or Ca=C, F=T for audio */
    int p0, p1, p2;
    int Nt, Np;
    const float* temb_freqs;   /* optional device table [tdim/2], see avd_timestep_embedding_f32; may be NULL */
    int temb_add;              /* 0: concat [adapter(d-tdim) | temb(tdim)] as the sampler (sample_clip.py:59-70);
                                  1: adapter(d) + temb(d) as the trainer (train/trainer.py:45-49); needs tdim == d */
} avd_embed_desc;
/* floats of scratch `tok_ws` must hold (tokens + the [B,tdim] timestep embedding); -1 on a bad descriptor */
int64_t avd_embed_workspace_floats(const avd_embed_desc* desc);
int avd_embed_cfg_pair_f32(const avd_embed_desc* desc, const float* z_target, const float* Wt, const float* bt,
                           const int64_t* t_now, const float* Xp, float* tok_ws, float* X2,
                           avd_stream_t stream);
/* As avd_embed_cfg_pair_f32 on slot timesteps (see "slot timesteps"): t_now is int64 [B*slots] and target row n of sample b embeds
 * t_now[b, slot(n)] in both halves; prompt rows and the adapter columns are unchanged.  Concat mode only. */
int avd_embed_cfg_pair_slots_f32(const avd_embed_desc* desc, const float* z_target, const float* Wt, const float* bt,
                                 const int64_t* t_now, int slots, const float* Xp, float* tok_ws, float* X2,
                                 avd_stream_t stream);
/* The single-branch front end of a cond-only step: X1[B, Nt+Np, d], bit-identical to the cond half of avd_embed_cfg_pair_f32's X2 on
 * the same inputs; B (Nt+Np) rows are handled, no null rows are written.  ss: NULL, or [B (Nt+Np)] that receives each finished row's
 * sum of squares in concat mode (the table the core's first folded RMSNorm reads; the bits the two-branch front end leaves for its
 * cond rows inside avd_denoise_step_f32); not written with temb_add. */
int avd_embed_cond_f32(const avd_embed_desc* desc, const float* z_target, const float* Wt, const float* bt,
                       const int64_t* t_now, const float* Xp, float* tok_ws, float* X1, float* ss,
                       avd_stream_t stream);

/* ---- composites: whole modules / the whole step as one host call (stateless; weights by pointer table).
 * These enqueue exactly the kernels above in order; they exist to keep the per-step host cost at one FFI
 * call and to make a step one hipGraph-capturable unit. */
typedef struct {                       /* avdiff/models/mmdt.py:88-99 (Block) state_dict, device ptrs */
    const float* norm1_scale;          /* blocks.{i}.norm1.scale (norm="layernorm": .weight) [d] */
    const float* in_proj_weight;       /* blocks.{i}.attn.mha.in_proj_weight  [3d,d]   */
    const float* in_proj_bias;         /* blocks.{i}.attn.mha.in_proj_bias    [3d]     */
    const float* out_proj_weight;      /* blocks.{i}.attn.mha.out_proj.weight [d,d]    */
    const float* out_proj_bias;        /* blocks.{i}.attn.mha.out_proj.bias   [d]      */
    const float* norm2_scale;          /* blocks.{i}.norm2.scale              [d]      */
    const float* fc1_weight;           /* blocks.{i}.mlp.fc1.weight           [hid,d]  */
    const float* fc1_bias;             /* blocks.{i}.mlp.fc1.bias             [hid]    */
    const float* fc2_weight;           /* blocks.{i}.mlp.fc2.weight           [d,hid]  */
    const float* fc2_bias;             /* blocks.{i}.mlp.fc2.bias             [d]      */
    /* optional split3 images of the four weights above (avd_split3_f32); all four non-NULL in every block selects
     * the bf16x3 matmul path of avd_core_forward_f32 for large batches (see "bf16x3" below), NULL keeps fp32 MFMA */
    /* optional: in_proj_weight * norm1.scale[None,:] and fc1_weight * norm2.scale[None,:] (fp32, same shapes).  Both non-NULL
     * lets the fp32 path fold each RMSNorm into its neighbours: the preceding residual epilogue emits the rows' sums of
     * squares, the following Linear runs on the un-normalised stream with these weights and scales its rows by 1/rms. */
    const float* in_proj_weight_n;
    const float* fc1_weight_n;
    const void* in_proj_weight3;
    const void* out_proj_weight3;
    const void* fc1_weight3;
    const void* fc2_weight3;
    const float* norm1_bias;           /* norm="layernorm" only: blocks.{i}.norm1.bias / norm2.bias [d]; NULL for RMSNorm */
    const float* norm2_bias;
    /* split_terms == 3 ("f16x2") only: power-of-two scales of the fp16 operand images (see "f16x2" below).
     * [0..3] the weight images in_proj, out_proj, fc1, fc2 (the *_weight3 pointers then hold avd_split_f16x2_f32 images);
     * [4..7] the activation images: norm1 output, q|k|v (and the attention output), norm2 output, GELU(fc1) output.  Each
     * activation scale must satisfy scale * bound <= 2^15 for a bound on the magnitudes the image can hold. */
    float f16x2_scale[8];
    /* optional (bf16 plane modes, i.e. split_terms 6 / 9 / 1): split3 images of in_proj_weight_n and fc1_weight_n above.  Both non-NULL
     * in every block folds each RMSNorm of the split path into its neighbours: the residual epilogues of out_proj / fc2 also write the
     * stream's operand image and its rows' sums of squares, in_proj / fc1 run on that un-normalised image with these weights and scale
     * their rows by 1 / (rms + eps) before the bias — no RMSNorm kernel between the first block's input and the final norm
     * (mmdt.py:39-42, 95-99; same arithmetic up to rounding). */
    const void* in_proj_weight3n;
    const void* fc1_weight3n;
} avd_block_weights;

typedef struct {                       /* avdiff/models/mmdt.py:116-149 (MMDiT) */
    int d, n_layers, n_heads, mlp_hidden;
    float norm_eps;                    /* 1e-6 */
    const avd_block_weights* blocks;   /* HOST array [n_layers] of device-pointer tables */
    const float* final_norm_scale;     /* final_norm.scale [d] */
    int norm_kind;                     /* 0: RMSNorm (every shipped config); 1: nn.LayerNorm (build_norm, mmdt.py:44-45) — fp32 path only */
    const float* final_norm_bias;      /* final_norm.bias [d] for norm_kind 1, else NULL */
    int split_terms;                   /* bf16x3 path only: product terms kept per k — 0 or 6: default (fp32-level error), 9: strict
                                        * (nothing dropped), 1: plain bf16 operands (reduced precision, BASELINE config C2),
                                        * 3: f16x2 — two scaled fp16 planes per operand, three terms (22-bit operands, fp32
                                        * accumulation; needs avd_block_weights.f16x2_scale) */
    int attn_mode;                     /* bf16x3 path only: 0 = attention follows split_terms; 1 = fp8 (OCP e4m3) QK^T and PV with fp32
                                        * accumulation (csrc/attn_fp8.hip) — reduced precision, BASELINE config C5, reported error */
} avd_core_weights;

typedef struct {                       /* avdiff/models/heads/noise_heads.py:94-229, one modality path */
    int d_in, hidden, d_out, n_shared;
    float ln_eps;                      /* 1e-5 */
    int act;                           /* AVD_ACT_GELU */
    const float* input_proj_weight;    /* input_proj.{m}.weight [hidden,d_in] */
    const float* input_proj_bias;
    const float* const* shared_lin_weight;  /* HOST array [n_shared]: shared.{j}.0.weight [hidden,hidden] */
    const float* const* shared_lin_bias;
    const float* const* shared_ln_weight;   /* shared.{j}.1.weight [hidden] */
    const float* const* shared_ln_bias;
    const float* out_proj_weight;      /* out_proj.{m}.weight [d_out,hidden] */
    const float* out_proj_bias;
    /* optional split-operand mode of the head's Linears (same meaning as avd_core_weights.split_terms; 0 = fp32 MFMA).  Taken when
     * every image pointer below is non-NULL, d_in % 16 == 0, hidden % 256 == 0, d_out % 256 == 0 and there are >= 6144 rows. */
    int split_terms;
    const void* input_proj_weight3;    /* operand images of the weights above (avd_split3_f32, or avd_split_f16x2_f32 for terms 3) */
    const void* const* shared_lin_weight3;
    const void* out_proj_weight3;
    /* split_terms == 3 only, HOST array of 2 * (n_shared + 2) power-of-two scales: the weight images [input_proj, shared 0.., out_proj],
     * then the activation images [head input rows, input_proj output, LayerNorm+act output 0..] (the caller bounds the input rows;
     * the rest follows from the weights, see multimodal_diffusion_amd/noise_heads.py) */
    const float* f16x2_scale;
} avd_head_weights;

/* ---- "bf16x3": fp32-accurate Linear on the bf16 matrix pipe (same reference ops as avd_gemm_bias_act_f32:
 * avdiff/models/mmdt.py:60,77-83).  Every fp32 operand is split exactly into three bf16 planes (x = h + m + l); a
 * product keeps the six terms down to 2^-16 and accumulates them in fp32, so the result carries the error of an fp32
 * FMA chain (measured slightly below it) while the matrix pipe runs 2.67x fewer cycles than with fp32 MFMA.
 * Operands travel as "split3 images" (tiled, 6 bytes per element, rows padded to 256; layout in csrc/gemm_bf16x3.hip).
 * `terms` selects the product terms kept per k: 6 (or 0) the default above; 9 strict — all nine, nothing dropped; 1 — only the
 * high planes, i.e. plain bf16 operands with fp32 accumulation: the reduced-precision variant BASELINE config C2 names, whose
 * error is REPORTED against the fp32 oracle and which is never a parity path.
 * Domain: finite operands with |x| >= ~2^-110 or 0 split exactly (below that the lower planes leave bf16's range and the
 * absolute error per product is < 2^-126); +-inf / NaN in an operand row make that output row non-finite (NaN where an
 * fp32 chain would give +-inf). */
int64_t avd_split3_bytes(int64_t rows, int K);                     /* bytes of the image of a [rows,K] matrix; -1 if K % 16 */
int avd_split3_f32(const float* x, void* out, int64_t rows, int K, avd_stream_t stream);   /* x [rows,K] contiguous */
/* RMSNorm (mmdt.py:39-42) whose output is written as a split3 image (the A operand of the next Linear) */
int avd_rmsnorm_split3_f32(const float* x, const float* scale, void* out, int64_t rows, int d, float eps,
                           avd_stream_t stream);
/* LayerNorm + activation (avd_layernorm_act_f32's arithmetic; noise_heads.py:141-147) whose output is written as a split3 image: the
 * producer avd_head_forward_f32 runs between the trunk Linears in the split-operand modes.  d % 16 == 0, d <= 2048, rows > 0;
 * image rows >= rows are left untouched. */
int avd_layernorm_act_split3_f32(const float* x, const float* gamma, const float* beta, void* out, int64_t rows, int d, float eps,
                                 int act, avd_stream_t stream);
/* avd_attn_fwd_f32 whose [B*N, H*Dh] result is written as a split3 image (rows >= n_query of a sample are left untouched) */
int avd_attn_fwd_split3_f32(const float* qkv, void* out3, int B, int N, int H, int Dh, float scale, int n_query,
                            avd_stream_t stream);
/* bf16x3 attention (csrc/attn_bf16x3.hip): in_proj writes q, k, v as a "qkv3 image" (three bf16 planes per value, per
 * (part, sample, head) rows of 384 B, q pre-multiplied by qscale = softmax scale * log2 e), the attention kernel reads it.
 * Same reference op as avd_attn_fwd_f32 (mmdt.py:51-61), same fp32-level error. */
int64_t avd_qkv3_bytes(int B, int N, int H);                       /* bytes of the image for [B,N,3*H*64] */
/* qkv = A W^T + bias, A3/W3 split3 images of A [M,K] (M = B*tokens rows) and in_proj_weight [3*heads*64, K] */
int avd_gemm_bf16x3_qkv3_f32(const void* A3, const void* W3, const float* bias, void* qkv3, int64_t M, int tokens,
                             int heads, int K, float qscale, int terms, avd_stream_t stream);
/* softmax(q k^T) v from a qkv3 image; out3 == NULL: fp32 out [B,N,H*64]; else the split3 image of [B*N, H*64].
 * Rows >= n_query of every sample are not computed and left untouched. */
int avd_attn_fwd_qkv3_f32(const void* qkv3, float* out, void* out3, int B, int N, int H, int n_query, int terms,
                          avd_stream_t stream);
/* fp8 (OCP e4m3) attention from the same qkv3 image (csrc/attn_fp8.hip): both contractions on v_mfma_f32_32x32x16_fp8_fp8 with
 * fp32 accumulation and fp32 softmax.  Reduced precision — BASELINE config C5 names it; the reference has no such path
 * (infer/sample_clip.py:399-411), so its error is reported against the fp32 result, never gated as parity.
 * workspace: avd_attn_fp8_workspace_bytes(B, N, H) bytes (the quantised, tile-major Q / K / V^T images). */
int64_t avd_attn_fp8_workspace_bytes(int B, int N, int H);
int avd_attn_fwd_fp8_f32(const void* qkv3, void* workspace, int64_t workspace_bytes, float* out, void* out3, int B, int N, int H,
                         int n_query, avd_stream_t stream);
/* the same with an f16x2 q|k|v image at scale qkv_scale (avd_gemm_f16x2_qkv_f32); out2 != NULL: the result as an f16x2 image at out_scale */
int avd_attn_fwd_fp8_f16x2_f32(const void* qkv, void* workspace, int64_t workspace_bytes, float* out, void* out2, int B, int N,
                               int H, int n_query, float qkv_scale, float out_scale, avd_stream_t stream);
/* C = act(A W^T + bias) (+ residual), A3/W3 split3 images of A [M,K] and W [N,K]; N % 256 == 0, K % 16 == 0.
 * C3 == NULL: fp32 row-major C [M,N], act AVD_ACT_NONE, residual optional (may alias C).
 * C3 != NULL: the result is written as the split3 image of [M,N] instead (bias required, act AVD_ACT_NONE or AVD_ACT_GELU,
 * no residual). */
int avd_gemm_bf16x3_f32(const void* A3, const void* W3, const float* bias, const float* residual, float* C, void* C3,
                        int64_t M, int N, int K, int act, int terms, avd_stream_t stream);
/* The residual epilogue the MMDiT composite runs for out_proj / fc2 (six terms), stand-alone: C = (A W^T + bias) + residual as fp32
 * [M,N] (residual may alias C), the split3 image of C into C3, and the sums of squares of every row's 64-column chunks into
 * ss_out [M, N / 64] — the producer side of a folded RMSNorm.  N % 256 == 0, K % 16 == 0; every pointer required. */
int avd_gemm_bf16x3_res_img_f32(const void* A3, const void* W3, const float* bias, const float* residual, float* C, void* C3,
                                float* ss_out, int64_t M, int N, int K, avd_stream_t stream);

/* ---- "f16x2": the same Linear / attention (mmdt.py:51-61,77-83) with every operand held as TWO fp16 planes, x ~ (h + l) / s
 * with h = rn_f16(s x), l = rn_f16(s x - h), and three product terms hh + hl + lh accumulated in fp32 on
 * v_mfma_f32_32x32x16_f16: half the matrix-pipe work of bf16x3.  An operand carries 22 significant bits (error <= 2^-22
 * relative) and the dropped ll term is <= 2^-22 relative, so a product is accurate to ~7e-7 against fp32's 6e-8 rounding;
 * over a dot product these errors add like the fp32 accumulation rounding both modes share (measured error in DESIGN.md).
 * fp16 has 5 exponent bits, so an image is stored at a power-of-two `scale` with |scale * x| <= 2^15 for every element:
 * the CALLER supplies the scale from a bound on |x| (for the MMDiT core the bounds follow from the weights alone, see
 * multimodal_diffusion_amd/mmdt.py `_f16x2_scales`); a value past the range turns its output rows into NaN, never into a
 * silently saturated number.  Images have the split3 / qkv3 geometry (same byte counts; the third plane is unused).
 * ab_scale = (A image scale) * (W image scale); c_scale / qkv_scale / out_scale = scale of the image being written. */
/* out2[0] = max |w|, out2[1] = max over rows of ||w_row||_2 for w [rows, cols] (a vector: rows = 1) — the quantities the scale
 * bounds above are made of; exact, order-independent (integer atomic maxima); NaN in w makes both NaN. */
int avd_weight_bounds_f32(const float* w, int64_t rows, int cols, float* out2, avd_stream_t stream);
int avd_split_f16x2_f32(const float* x, void* out, int64_t rows, int K, float scale, avd_stream_t stream);
int avd_rmsnorm_split_f16x2_f32(const float* x, const float* gamma, void* out, int64_t rows, int d, float eps, float scale,
                                avd_stream_t stream);
/* avd_layernorm_act_split3_f32 writing an f16x2 image at `scale` (> 0; the head bounds the output by sqrt(d) |gamma| + |beta|) */
int avd_layernorm_act_split_f16x2_f32(const float* x, const float* gamma, const float* beta, void* out, int64_t rows, int d,
                                      float eps, int act, float scale, avd_stream_t stream);
int avd_gemm_f16x2_f32(const void* A2, const void* W2, const float* bias, const float* residual, float* C, void* C2,
                       int64_t M, int N, int K, int act, float ab_scale, float c_scale, avd_stream_t stream);
int avd_gemm_f16x2_qkv_f32(const void* A2, const void* W2, const float* bias, void* qkv, int64_t M, int tokens, int heads,
                           int K, float qscale, float ab_scale, float qkv_scale, avd_stream_t stream);
int avd_attn_fwd_qkv_f16x2_f32(const void* qkv, float* out, void* out2, int B, int N, int H, int n_query, float qkv_scale,
                               float out_scale, avd_stream_t stream);

/* bytes of scratch avd_core_forward_f32 needs for a [B,N,d] input */
int64_t avd_core_workspace_bytes(const avd_core_weights* w, int B, int N);
/* MMDiT.forward(x) -> y, x,y: [B,N,d] (y may alias x).  n_out_rows: number of leading rows per sample whose
 * output is needed (N = reference behaviour; fewer lets the last block skip dead rows when the caller only
 * consumes the first n_out_rows — the engine passes the target-row count). out_row0: first needed row.  Rows of y outside
 * [out_row0, out_row0 + n_out_rows) are unspecified: with the window at row 0 the last block's attention, out_proj, fc1, fc2 and the final
 * norm run on the window's rows only (six-term bf16-plane path).
 * key_padding_mask: NULL or bytes [B,N], see avd_attn_fwd_f32.  A mask, or norm_kind 1 (LayerNorm), keeps the whole forward on the fp32
 * MFMA kernels whatever split_terms says — the split-operand attention takes no mask and the split producers are RMSNorm's; results
 * are the fp32 path's, at its speed.  attn_mode 1 (fp8 attention) with either of them is refused (AVD_EUNSUPPORTED). */
int avd_core_forward_f32(const avd_core_weights* w, const float* x, float* y, int B, int N,
                         int out_row0, int n_out_rows, const uint8_t* key_padding_mask, void* workspace,
                         int64_t workspace_bytes, avd_stream_t stream);

int64_t avd_head_workspace_bytes(const avd_head_weights* w, int64_t rows);
/* MultiModalNoiseHead path for ONE modality over `rows` token rows taken from h with segmented addressing:
 * row r lives at h + (r / seg_rows) * seg_stride + (r % seg_rows) * ldh.  out: [rows, d_out] contiguous. */
int avd_head_forward_f32(const avd_head_weights* w, const float* h, int64_t ldh, int64_t seg_rows,
                         int64_t seg_stride, int64_t rows, float* out, void* workspace,
                         int64_t workspace_bytes, avd_stream_t stream);

typedef struct {                       /* one whole CFG denoising step (sample_clip.py:359-389 / 318-348) */
    avd_embed_desc embed;
    const avd_core_weights* core;
    const avd_head_weights* head;      /* the TARGET modality's path */
    const float* adapt_w; const float* adapt_b;   /* target adapter */
    const float* alpha_bar; int T_train;
    float guidance, eta;
    int split_streams;   /* !=0: run the cond and null CFG halves as two kernel chains on two streams (fork/join by events;
                            graph-capturable); results are bit-identical to the single-stream order.  1: both chains on the full
                            layout.  2: the null half's short layout (avd_cfg_dedup_set above) as two chains — the cond half, B
                            samples of N rows, on `stream`, the null half, B samples of Nt + 1 rows, on the second stream, both on
                            the kernels the stacked 2B x N batch takes — and the one-stream step (0) wherever that layout does not
                            apply.  The null chain starts at the fork, or, with the tune key cfg_offset (AVD_CFG_OFFSET; 0 default,
                            1 .. 3) set to k > 0, behind the cond chain's k-th launch of block 0 (in_proj, attention, out_proj): an
                            event recorded there, no waiting in kernels; measured slower than 0 at every k
                            (profiles/two_stream_dedup_e2e.txt) */
} avd_step_desc;
int64_t avd_step_workspace_bytes(const avd_step_desc* s);
/* z_out = DDIM(z, eps_cfg(z, Xp, t_now), t_now -> t_prev).  z_out must not alias z. */
int avd_denoise_step_f32(const avd_step_desc* s, const float* z, const float* Xp, const int64_t* t_now,
                         const int64_t* t_prev, const float* noise, float* z_out,
                         void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole step on slot timesteps (see "slot timesteps"): t_now, t_prev int64 [B*slots], slots == the geometry's S.  Requires
 * s->eta == 0 and the concat embedding; the workspace is avd_step_workspace_bytes'.  Fed a table that repeats one pair per sample it
 * returns avd_denoise_step_f32's bits.  Graph-capturable: the tables are read at their addresses at every launch. */
int avd_denoise_step_slots_f32(const avd_step_desc* s, const float* z, const float* Xp, const int64_t* t_now,
                               const int64_t* t_prev, int slots, float* z_out,
                               void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* As avd_denoise_step_slots_f32, ending in the slot form of the DPM-Solver++(2M) update (see "slot timesteps"): t_last int64 [B*slots],
 * x0_hist fp32 [B, per_sample], 16-byte aligned, not overlapping z or z_out.  The front end is avd_denoise_step_slots_f32's, launch for
 * launch; refusals are its own, plus those of x0_hist.  Uniform tables give avd_denoise_step_dpmpp_2m_f32's bits in z_out and x0_hist.
 * Graph-capturable: the tables and x0_hist are read at their addresses at every launch. */
int avd_denoise_step_slots_dpmpp_2m_f32(const avd_step_desc* s, const float* z, const float* Xp, const int64_t* t_last,
                                        const int64_t* t_now, const int64_t* t_prev, int slots, float* x0_hist, float* z_out,
                                        void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole step on slot timesteps at s->eta >= 0, both solvers (see "clip-keyed slot noise"): t_last and x0_hist both NULL end it in
 * the DDIM slot update, both set in the slot form of DPM-Solver++(2M) (its SDE form at eta > 0), the noise of every stepping slot
 * drawn inside the fused kernel by clip position.  The front end is avd_denoise_step_slots_f32's, launch for launch; the key is
 * checked before the model runs.  At s->eta == 0 the key is not read and the result has the bits of the two entries above.
 * Graph-capturable: the tables, x0_hist and key->cursor are read at their addresses at every launch; seed, first and stride are held
 * by value. */
int avd_denoise_step_slots_seeded_f32(const avd_step_desc* s, const avd_slot_key* key, const int64_t* t_last, float* x0_hist,
                                      const float* z, const float* Xp, const int64_t* t_now, const int64_t* t_prev, int slots,
                                      float* z_out, void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole step on slot timesteps ending in the clip guide's blend (see "clip-keyed latent guide"): avd_denoise_step_slots_seeded_f32
 * with the guide added; key may be NULL at s->eta == 0.  The front end is avd_denoise_step_slots_f32's, launch for launch; the guide
 * and the key are checked before the model runs.  Graph-capturable: the cursor is read at every launch. */
int avd_denoise_step_slots_guided_f32(const avd_step_desc* s, const avd_slot_key* key, const avd_clip_guide* guide, const int64_t* t_last,
                                      float* x0_hist, const float* z, const float* Xp, const int64_t* t_now, const int64_t* t_prev,
                                      int slots, float* z_out, void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole step on slot timesteps under a slot CFG control (see "slot CFG control"): avd_denoise_step_slots_guided_f32 with the control
 * added; key may be NULL at s->eta == 0, guide may be NULL.  The front end is avd_denoise_step_slots_f32's, launch for launch; the
 * control (the workspace standing for the eps tokens in its overlap check), the guide and the key are checked before the model runs;
 * the statistics pass of a rescale or APG control runs on the caller's stream right before the fused update.  Graph-capturable: the
 * tables are read at their addresses at every launch. */
int avd_denoise_step_slots_cfg_f32(const avd_step_desc* s, const avd_slot_cfg* cfg, const avd_slot_key* key, const avd_clip_guide* guide,
                                   const int64_t* t_last, float* x0_hist, const float* z, const float* Xp, const int64_t* t_now,
                                   const int64_t* t_prev, int slots, float* z_out, void* workspace, int64_t workspace_bytes,
                                   avd_stream_t stream);
/* The whole step of a FIFO clip batch under per-queue keys and guides (see "clip batch keying"): avd_denoise_step_slots_cfg_f32 with the
 * descriptor, both solvers.  cfg may be NULL here (the scalar guidance); the slot CFG control and the slot momentum are per slot already
 * and unchanged.  The descriptor is checked before the model runs, as the fused update's launcher checks it again.  Graph-capturable:
 * the seeds are read at their addresses at every launch. */
int avd_denoise_step_slots_clips_f32(const avd_step_desc* s, const avd_slot_cfg* cfg, const avd_slot_key* key, const avd_clip_guide* guide,
                                     const avd_clip_queues* queues, const int64_t* t_last, float* x0_hist, const float* z,
                                     const float* Xp, const int64_t* t_now, const int64_t* t_prev, int slots, float* z_out,
                                     void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* As avd_denoise_step_f32, with the eta > 0 noise drawn inside the fused CFG + DDIM kernel from the seeded stream (avd_noise_key)
 * for samples key->sample_offset .. + B - 1 at t_now: no noise buffer, graph-capturable.  With s->eta == 0 it is the plain step. */
int avd_denoise_step_seeded_f32(const avd_step_desc* s, const avd_noise_key* key, const float* z, const float* Xp,
                                const int64_t* t_now, const int64_t* t_prev, float* z_out,
                                void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* As avd_denoise_step_f32, ending in the DPM-Solver++(2M) update (avd_dpmpp_2m_step_f32) inside the fused CFG kernel instead of DDIM:
 * t_last: int64 [B] (< 0: first order); x0_hist: fp32 [B, per_sample] in the latent's natural layout, read by second-order steps and
 * overwritten with this step's x0.  Requires s->eta == 0 (eta > 0: avd_denoise_step_dpmpp_2m_sde_f32); x0_hist must not alias z or z_out.
 * Graph-capturable: x0_hist stays at its address from step to step. */
int avd_denoise_step_dpmpp_2m_f32(const avd_step_desc* s, const float* z, const float* Xp, const int64_t* t_last,
                                  const int64_t* t_now, const int64_t* t_prev, float* x0_hist, float* z_out,
                                  void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole CFG step ending in the guided update (avd_latent_guide): z_out = blend(mask, q(t_prev), step(z)).  key != NULL with
 * s->eta > 0: seeded DDIM noise (as avd_denoise_step_seeded_f32); eta > 0 without a key is refused.  t_last and x0_hist both
 * non-NULL: the DPM-Solver++(2M) update (eta == 0, as avd_denoise_step_dpmpp_2m_f32).  known / mask must not overlap z_out or
 * x0_hist.  Graph-capturable: the guide's buffers are read at their addresses at every launch. */
int avd_denoise_step_guided_f32(const avd_step_desc* s, const avd_latent_guide* g, const avd_noise_key* key,
                                const int64_t* t_last, float* x0_hist, const float* z, const float* Xp,
                                const int64_t* t_now, const int64_t* t_prev, float* z_out,
                                void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole CFG step under a CFG control (avd_cfg_control): per-sample guidance and / or guidance rescale.  With ctl->rescale set, a
 * statistics pass runs on the stream right before the fused update (after the join of split_streams).  g (the latent guide), key,
 * t_last and x0_hist are optional and mean what they mean in avd_denoise_step_guided_f32 (eta > 0 needs a key).  Graph-capturable:
 * the per-sample arrays and the scratch are read at their addresses at every launch. */
int avd_denoise_step_cfg_f32(const avd_step_desc* s, const avd_cfg_control* ctl, const avd_latent_guide* g,
                             const avd_noise_key* key, const int64_t* t_last, float* x0_hist, const float* z, const float* Xp,
                             const int64_t* t_now, const int64_t* t_prev, float* z_out,
                             void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole CFG step on the adaptive projected guidance eps (avd_apg_control; "adaptive projected guidance" above).  It takes what
 * avd_denoise_step_cfg_f32 takes plus the APG control and the two canvas hops, so that every combination the controlled step has is
 * one entry: ctl NULL (the scalar guidance) or a control with per-sample guidance (its rescale must be NULL); g, key, t_last + x0_hist
 * as there, with eta > 0 beside x0_hist being the solver's SDE form; canvas_hop != 0 keys the eta > 0 noise by canvas position
 * (avd_denoise_step_canvas_f32's rules), guide_hop != 0 the guide's known noise (avd_denoise_step_canvas_guided_f32's rules; at eta
 * > 0 canvas_hop must equal it).  The statistics pass runs on the stream right before the fused update.  Graph-capturable: the
 * scratch and the momentum buffer are read and written at their addresses at every launch; the three parameters are held by value. */
int avd_denoise_step_apg_f32(const avd_step_desc* s, const avd_apg_control* apg, const avd_cfg_control* ctl,
                             const avd_latent_guide* g, const avd_noise_key* key, int canvas_hop, int guide_hop,
                             const int64_t* t_last, float* x0_hist, const float* z, const float* Xp,
                             const int64_t* t_now, const int64_t* t_prev, float* z_out,
                             void* workspace, int64_t workspace_bytes, avd_stream_t stream);
/* The whole cond-only step (see "guidance interval" above): the single-branch front end, the core and the head on B (Nt+Np) resp. B Nt
 * rows — their kernels chosen for those row counts — and the single-branch fused update.  One kernel chain on `stream`: no second
 * stream, no fork / join, whatever s->split_streams says; s->guidance is not read.  The workspace is the CFG step's
 * (avd_step_workspace_bytes): the cond half of each region is used, and eps [B,Nt,D] lands where the cond half of eps2 does (the first
 * B Nt D floats of the trailing eps region).  g, key, t_last and x0_hist are optional and follow avd_denoise_step_guided_f32's rules
 * (t_last and x0_hist go together and need eta == 0; x0_hist must not alias z or z_out; known / mask must not overlap z_out or
 * x0_hist).  eta > 0 needs key or, without a guide, an explicit `noise` [B, per_sample]; noise with a key or with a guide is refused.
 * Graph-capturable as its twins. */
int avd_denoise_step_cond_f32(const avd_step_desc* s, const avd_latent_guide* g, const avd_noise_key* key,
                              const int64_t* t_last, float* x0_hist, const float* z, const float* Xp,
                              const int64_t* t_now, const int64_t* t_prev, const float* noise, float* z_out,
                              void* workspace, int64_t workspace_bytes, avd_stream_t stream);

/* The whole seeded eta > 0 DDIM step with canvas-keyed noise (see "canvas-keyed noise"): the B samples of s->embed are consecutive windows
 * of one canvas, `hop` positions apart along T (video) or F (audio), window 0 at global index key->sample_offset.  Requires s->eta > 0 and
 * key; the canvas-keying limits are checked before the model runs.  cond_only == 0: the CFG step, with ctl (NULL or an avd_cfg_control, as
 * avd_denoise_step_cfg_f32) and g (NULL or a latent guide, as avd_denoise_step_guided_f32; its known-noise stream stays keyed per sample:
 * the canvas keying of the guide is avd_denoise_step_canvas_guided_f32).  cond_only != 0: the cond-only step (as avd_denoise_step_cond_f32
 * with a key; ctl must be NULL).  Only the draw inside the fused update differs from those entries: fed avd_canvas_noise_f32's output as
 * explicit noise, avd_denoise_step_f32 returns the same bits.  This entry is the DDIM step: the canvas-keyed DPM-Solver++(2M) step is
 * avd_denoise_step_dpmpp_2m_sde_f32 with canvas_hop != 0.  Graph-capturable: seed, sample_offset and hop are held by value. */
int avd_denoise_step_canvas_f32(const avd_step_desc* s, const avd_noise_key* key, int hop, const avd_cfg_control* ctl,
                                const avd_latent_guide* g, int cond_only, const float* z, const float* Xp,
                                const int64_t* t_now, const int64_t* t_prev, float* z_out,
                                void* workspace, int64_t workspace_bytes, avd_stream_t stream);

/* The whole step ending in the SDE form of the DPM-Solver++(2M) update (avd_dpmpp_2m_sde_step_f32) inside the fused kernel, its noise
 * drawn from the seeded stream: one entry for every kind of SDE step.  Requires s->eta > 0, key, t_last and x0_hist (as
 * avd_denoise_step_dpmpp_2m_f32).  canvas_hop == 0: per-sample keying (as avd_denoise_step_seeded_f32); canvas_hop >= 1: the B samples
 * are consecutive windows of one canvas and the draw is keyed by canvas position (as avd_denoise_step_canvas_f32, same range checks).
 * cond_only == 0: the CFG step, with ctl (NULL or an avd_cfg_control) and g (NULL or a latent guide; its known-noise stream stays
 * keyed per sample).  cond_only != 0: the cond-only step (ctl must be NULL).  All argument checks run before the model.  The
 * workspace is the CFG step's (avd_step_workspace_bytes).  Unseeded or explicit noise is not supported here.  Graph-capturable: the
 * key and canvas_hop are held by value, x0_hist stays at its address. */
int avd_denoise_step_dpmpp_2m_sde_f32(const avd_step_desc* s, const avd_noise_key* key, int canvas_hop, const avd_cfg_control* ctl,
                                      const avd_latent_guide* g, int cond_only, const int64_t* t_last, float* x0_hist,
                                      const float* z, const float* Xp, const int64_t* t_now, const int64_t* t_prev, float* z_out,
                                      void* workspace, int64_t workspace_bytes, avd_stream_t stream);

/* The whole step ending in the canvas-keyed guided update ("canvas-keyed known noise"): one entry for every kind of step.  The B samples
 * of s->embed are consecutive windows of one canvas, `hop` positions apart along T (video) or F (audio), window 0 at global index
 * g->key.sample_offset; z_out = blend(mask, q(t_prev), step(z)) with n_k keyed by canvas position.  The step: DDIM at s->eta == 0 (key is
 * not read: pass NULL), seeded DDIM at eta > 0, or with t_last and x0_hist (both or neither) DPM-Solver++(2M) in its ODE (eta == 0) or
 * SDE (eta > 0) form; x0_hist receives the model's x0, not the blended value.  At eta > 0 the step's own noise is canvas-keyed with the
 * same hop from `key` (as avd_denoise_step_canvas_f32; key->sample_offset is the first window's global index for that stream): a
 * canvas-keyed guide with per-sample, unseeded or explicit step noise is refused (AVD_EINVAL), as is eta > 0 without a key.
 * cond_only == 0: the CFG step, with ctl NULL or an avd_cfg_control; cond_only != 0: the cond-only step (ctl must be NULL).  All
 * argument checks run before the model.  The workspace is the CFG step's.  Graph-capturable: seeds, offsets and hop are held by
 * value, the guide's buffers and x0_hist are read at their addresses at every launch. */
int avd_denoise_step_canvas_guided_f32(const avd_step_desc* s, const avd_latent_guide* g, int hop, const avd_noise_key* key,
                                       const avd_cfg_control* ctl, int cond_only, const int64_t* t_last, float* x0_hist,
                                       const float* z, const float* Xp, const int64_t* t_now, const int64_t* t_prev, float* z_out,
                                       void* workspace, int64_t workspace_bytes, avd_stream_t stream);

/* ---- a9 / next-1: VideoVAE.decode — avdiff/models/encoders/vae_video3d.py:195-214 (decode), :79-84
 * (_conv_block_3d: Conv3d 3x3x3 pad 1 -> GELU(erf) -> GroupNorm(min(8,C), eps 1e-5, affine)), :108-119.
 * z [B,Cv,Tp,Hp,Wp] NCDHW -> from_lat (1x1x1) -> trilinear upsample (align_corners=False) to (T,H,W) ->
 * n_blocks x [conv3x3x3 + GELU + GroupNorm] -> to_img (1x1x1) -> sigmoid | tanh -> out [B,out_ch,T,H,W] NCDHW.
 * Inside, activations are NDHWC in a zero-haloed buffer and the convolution is the fp32 MFMA GEMM with a
 * per-tap address shift (no im2col).  Decoder width must be 64 (the reference default). */
typedef struct {
    int B, Cv, Tp, Hp, Wp;             /* latent dims */
    int T, H, W;                       /* output size (reference default: Tp*t_down, Hp*s_down, Wp*s_down) */
    int base, n_blocks, out_ch;        /* dec_base (64), dec_blocks, in_ch of the VAE (3) */
    int out_tanh;                      /* 0 = sigmoid, 1 = tanh (cfg.out_activation) */
    float gn_eps;                      /* 1e-5 */
    const float* from_lat_w;           /* from_lat.weight  [base,Cv]   (1x1x1 kernel squeezed) */
    const float* from_lat_b;           /* from_lat.bias    [base] */
    const float* const* conv_w;        /* HOST array [n_blocks]: dec_net.{i}.0.weight re-laid as [out][kt][kh][kw][in] */
    const float* const* conv_b;        /* dec_net.{i}.0.bias [base] */
    const float* const* gn_w;          /* dec_net.{i}.2.weight [base] */
    const float* const* gn_b;          /* dec_net.{i}.2.bias   [base] */
    const float* to_img_w;             /* to_img.weight [out_ch,base] */
    const float* to_img_b;             /* to_img.bias   [out_ch] */
    const void* const* conv_w3;        /* optional HOST array [n_blocks] of avd_conv3_weight_f32 images: the convolutions then run
                                        * on the bf16 matrix pipe with exactly split operands (fp32-level error, see "bf16x3"); NULL = fp32 MFMA */
    int conv_terms;                    /* with conv_w3: 0 or 6 = bf16x3; 3 = f16x2 (images from avd_conv3_weight_f16x2_f32, see "f16x2") */
    const float* conv_w_scale;         /* conv_terms 3: HOST array [n_blocks], power-of-two scales of the weight images */
    const float* conv_a_scale;         /* conv_terms 3: HOST array [n_blocks], scales of each block's INPUT image: entry i >= 1 from the bound
                                        * |GroupNorm output| <= sqrt(n - 1) max|gamma| + max|beta| (n = elements of one group of one sample);
                                        * entry 0 is ignored — the first image's scale is derived on the device, per sample, from max |from_lat(z)| */
    /* ABI 6 — the first convolution composed with what precedes it (vae_video3d.py:205-209: from_lat -> trilinear upsample -> dec_net.0.0):
     * upsampling is linear, channel-wise and its weights sum to one, so conv(upsample(from_lat(z))) is a convolution of upsample(z) — Cv <= 16
     * input channels instead of 64, a quarter of the matrix work — plus a bias term.  With conv_w3 and conv0_lat_w3 both given the decoder
     * takes that route for block 0 (same operator up to fp32 rounding); NULL = the three separate passes. */
    const void* conv0_lat_w3;          /* avd_conv3_weight_[f16x2_]f32 image of the composite weight [out][kt][kh][kw][in], in < Cv:
                                        * sum_c conv_w[0][out][c][tap] * from_lat_w[c][in], in >= Cv zero */
    const float* conv0_lat_btab;       /* [64 border classes][base]: sum over the taps INSIDE the volume of sum_c conv_w[0][out][c][tap] * from_lat_b[c];
                                        * class bits: t-1 inside, t+1 inside, h-1, h+1, w-1, w+1 (the conv zero-pads u = from_lat(.), not its bias) */
    float conv0_lat_w_scale;           /* conv_terms 3: scale of the conv0_lat_w3 image */
    /* ABI 7 (round 5): 1 = conv0_lat_w3 is the PACKED image (Cv <= 8): "tap" s of the [out][27][base] tensor handed to avd_conv3_weight_*
     * holds the composite weights of tap 2 s in channels 0 .. 7 and of tap 2 s + 1 in channels 8 .. 15 (s = 0 .. 13; tap 27 = zeros) — the
     * kernel then runs 14 k-steps of two taps instead of 27 of one whose upper 8 channels are zero.  0 = one tap per step. */
    int conv0_lat_packed;
} avd_vae_decode_desc;
/* weight image of one 3x3x3 64->64 convolution for the split-operand decoders: w_tap_major is [out][kt][kh][kw][in] fp32 */
int64_t avd_conv3_weight_bytes(void);
int avd_conv3_weight_f32(const float* w_tap_major, void* img, avd_stream_t stream);
int avd_conv3_weight_f16x2_f32(const float* w_tap_major, void* img, float scale, avd_stream_t stream);
int64_t avd_vae_decode_workspace_bytes(const avd_vae_decode_desc* d);
int avd_vae_decode_f32(const avd_vae_decode_desc* d, const float* z, float* out, void* workspace,
                       int64_t workspace_bytes, avd_stream_t stream);

/* ---- next-1: VideoVAE.encode — avdiff/models/encoders/vae_video3d.py:164-189 (deterministic path):
 * x [B,in_ch,T,H,W] NCDHW (already cropped to multiples of t_down / s_down) -> n_blocks x [conv3x3x3 + GELU + GroupNorm]
 * -> AvgPool3d(t_down,s_down,s_down) -> to_lat (1x1x1) -> z [B,lat_ch,T/t_down,H/s_down,W/s_down] NCDHW.
 * The first conv (in_ch -> 64) runs on the same MFMA kernel with the input padded to 4 channels (K = 32 taps x 4). */
typedef struct {
    int B, in_ch, T, H, W;
    int t_down, s_down;
    int base, n_blocks, lat_ch;        /* enc_base (64), enc_blocks, latent channels */
    float gn_eps;
    const float* const* conv_w;        /* HOST array [n_blocks]: block 0: enc_net.0.0.weight re-laid as [64][32 taps][4]
                                          (27 real taps, channel 3 and taps 27..31 zero); blocks >= 1: [64][27][64] */
    const float* const* conv_b;
    const float* const* gn_w;
    const float* const* gn_b;
    const float* to_lat_w;             /* to_lat.weight (or to_mu.weight) [lat_ch,64] */
    const float* to_lat_b;
    const void* const* conv_w3;        /* optional HOST array [n_blocks] (entry 0 unused): avd_conv3_weight_f32 images of the 64->64
                                        * convolutions, which then run on the bf16 matrix pipe (as in avd_vae_decode_desc); NULL = fp32 */
    int conv_terms;                    /* as in the decode descriptor; entries 0 of the scale arrays are unused (block 0 is the fp32 4 -> 64 conv) */
    const float* conv_w_scale;
    const float* conv_a_scale;
    /* ABI 7 (round 5), optional: the FIRST convolution (in_ch <= 8 -> base) on the matrix pipe with two taps per k-step — the
     * avd_conv3_weight_f32 image of a [out][27][base] tensor whose "tap" s (s = 0 .. 13) holds enc_net.0.0.weight[out][:, tap 2 s] in
     * channels 0 .. in_ch-1 and tap 2 s + 1 in channels 8 .. 8+in_ch-1 (everything else zero).  With it set, conv_terms 0 / 6, two conv
     * blocks and pooling (4, 8, 8), avd_vae_encode_f32 writes no fp32 activation at all (folded route, avd_tune_set "vae_fold"); NULL = fp32 first conv. */
    const void* conv0_pk_w3;
} avd_vae_encode_desc;
int64_t avd_vae_encode_workspace_bytes(const avd_vae_encode_desc* d);
int avd_vae_encode_f32(const avd_vae_encode_desc* d, const float* x, float* z, void* workspace,
                       int64_t workspace_bytes, avd_stream_t stream);

/* ---- next-2: AudioCodec layers — avdiff/models/encoders/audio_codec.py:88-133, :158-214.
 * NCL conv1d (odd k <= 15, zero padding k/2, stride 1) with optional nearest-neighbour upsampling of the INPUT by
 * `upsample` folded into the indexing (decode's F.interpolate(mode="nearest") x hop), then act in {none, GELU, tanh}.
 * x [B,Cin,Lin], w [Cout,Cin,k], bias [Cout] or NULL, out [B,Cout,Lin*upsample]. */
int avd_conv1d_act_f32(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout,
                       int Lin, int upsample, int k, int act, avd_stream_t stream);
/* audio_codec.py:158-182: right-pad with zeros / crop to Fa*hop samples, then avg_pool1d(kernel = stride = hop).
 * x [rows, L] -> out [rows, Fa]. */
int avd_avgpool_frames_f32(const float* x, float* out, int rows, int L, int Fa, int hop, avd_stream_t stream);

/* ---- next-3: sliding-window stitching — avdiff/models/infer/stream_infer.py:85-116 (crossfade_audio),
 * :119-143 (crossfade_video).  N windows of L positions x `inner` values placed every `hop` positions, weighted by
 * w[L] (host-built fade table), divided by the summed weights clamped at 1e-6; out has (N-1)*hop + L positions.
 * The u8 form divides by 255 on input and clips / scales / truncates to uint8 on output like the reference. */
int avd_crossfade_f32(const float* chunks, const float* w, float* out, int N, int L, int hop, int64_t inner,
                      avd_stream_t stream);
int avd_crossfade_u8(const uint8_t* chunks, const float* w, uint8_t* out, int N, int L, int hop, int64_t inner,
                     avd_stream_t stream);

/* ---- latent window consensus (extension: MultiDiffusion-style co-denoising, Bar-Tal et al. 2023, for the windows of
 * stream_generate).  z [N, outer, L, inner] holds N consecutive windows of one canvas of (N-1)*hop + L positions along the sliding
 * axis, window k at positions k*hop .. k*hop + L - 1 (video latent [N,C,T,H,W]: outer = C, L = T, inner = H*W; audio latent
 * [N,Ca,F]: outer = Ca, L = F, inner = 1).  In place: every canvas element (o, p, j) that lies under two or more windows k = lo..hi
 * (the windows the cross-fade gathers for p) becomes
 *     m = (sum_k w[p - k*hop] * z[k, o, p - k*hop, j]) / (sum_k w[p - k*hop])
 * in every one of them: sums over k in increasing order from 0, multiply, add and divide rounded separately (no FMA contraction), so
 * the fp32 result is that of a numpy loop in the same order.  An element under one window is not touched (it keeps its bits).
 * w[L]: per-position weights on the device, all > 0 (the caller checks: the sum is not clamped).  N == 1 or hop >= L launches
 * nothing.  One thread owns one canvas element and nobody else reads or writes its z elements, so the pass is race free. */
int avd_window_consensus_f32(float* z, const float* w, int N, int64_t outer, int L, int hop, int64_t inner, avd_stream_t stream);

/* device-side sampling-schedule cursor so a captured step can be replayed without host writes:
 * t_now[b] = sched[*cursor], t_prev[b] = sched[*cursor+1] for all b, then (*cursor)++ . */
int avd_sched_advance(const int64_t* sched, int n_sched, int32_t* cursor, int64_t* t_now, int64_t* t_prev,
                      int B, avd_stream_t stream);
/* As avd_sched_advance, and t_last[b] = sched[*cursor - 1] when *cursor > 0 and sched[*cursor - 1] > sched[*cursor], else -1 (the
 * multistep solver's history step).  An entry before t_now that lies at or below it means the schedule has just jumped up (a
 * resampling schedule, "renoise"): the history does not belong to this stretch and the step is first order.  On a strictly
 * decreasing schedule the second condition always holds.  A cursor past the end repeats the last step, with its own t_last. */
int avd_sched_advance_ms(const int64_t* sched, int n_sched, int32_t* cursor, int64_t* t_last, int64_t* t_now, int64_t* t_prev,
                         int B, avd_stream_t stream);

/* ---- measurement hooks (bench.py): when enabled, every kernel launch made by this library is bracketed by
 * hipEvents recorded on the launch stream and tagged with its kernel name (template arguments included, so the
 * tags line up with rocprofv3's per-kernel rows) and its algorithmic work (FLOPs for the MFMA kernels, bytes
 * for the HBM-bound ones).  Disabled by default; zero cost when off.  Not for use during graph capture. */
int         avd_prof_enable(int on);       /* on=1 start recording (clears previous records), on=0 stop */
int         avd_prof_num_tags(void);
const char* avd_prof_tag_name(int tag);
/* synchronises the recorded events and accumulates per tag: launches, total milliseconds, algorithmic work */
int         avd_prof_report(int64_t* launches, double* total_ms, double* work, int ntags);

#ifdef __cplusplus
}
#endif
#endif /* AVDIFF_HIP_H */

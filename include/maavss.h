/* libmaavss_hip -- C-ABI of the MI355X (gfx950) kernels behind the MAAVSS training hot path.
 *
 * The reference (carlmoore256/MAAVSS) has no FFI layer: its boundary is two Python classes
 * (avse_model_final.py:14 AV_Fusion_Model_Frames, video_attention.py:24 VideoAttention) plus the
 * STFT helpers of av_dataset.py.  Each entry point below replaces the ATen/vendor-library work one
 * reference line dispatches; the citation names that line.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain pointers are DEVICE pointers unless named host_*; the library never allocates, frees
 *     or synchronises; every launch goes to `stream` (a hipStream_t, 0 = default stream);
 *   - scratch memory is caller-provided (`ws`, size documented per call);
 *   - return value 0 = ok, non-zero = error, text via maavss_last_error() (thread-local);
 *   - tensors are dense, row-major in the documented order; f32 unless stated; "bf16" = raw
 *     uint16 bfloat16 bits;
 *   - `precise` (a.k.a. mode) selects the arithmetic of MFMA-backed kernels: 0 = operands rounded to bf16,
 *     f32 accumulate (v_mfma_f32_16x16x32_bf16); 1 = exact f32 MFMA (v_mfma_f32_16x16x4_f32); 2 = operands
 *     rounded to IEEE half, f32 accumulate (v_mfma_f32_16x16x32_f16; same rate as bf16, used for forward
 *     operands whose range BatchNorm bounds).
 */
#ifndef MAAVSS_H
#define MAAVSS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ABI version = what maavss_version() of a matching library returns; bumped whenever an entry point is removed or changes
 * meaning (INTEGRATION.md "ABI history").  maavss_amd/_lib.py refuses a library whose version differs from this header's.
 *   100  rounds 1-2
 *   300  round 3: maavss_vit_attn_fp8{,_ws_bytes} removed (-> maavss_vit_attn_mx*); maavss_conv3d_c1_fwd(precise = 2) writes one
 *        stat_partials row per 8-tile workgroup (maavss_conv3d_c1_fwd_nparts), not one per tile; the Philox counter layout of
 *        maavss_stft_fwd's in-kernel noise changed (same seed, different noise)
 *   400  round 4: maavss_set_deterministic_workspace takes the stream the scratch is bound to; NULL ln_gamma / ln_beta = LayerNorm without
 *        the affine part; epilogue 4 of maavss_vit_ws_gemm (GELU in packed half); the in-kernel noise of maavss_stft_fwd draws the bin n_fft / 2
 *        from its own per-frame-pair Philox block (same seed, different noise in that bin); maavss_bn_pool_act_fwd and
 *        maavss_conv3d_c1_bn_pool_act take an out_bf16 pointer behind out16, maavss_conv3d_wgrad's dy16 became the mask in16; see INTEGRATION.md
 *   401  maavss_convt2d_{out_size,fwd,dgrad,wgrad_nchunk,wgrad} removed: the STFT decoder runs through maavss_conv2d_gen_* (<= 30 taps)
 *   402  maavss_conv2d_{fwd,dgrad,wgrad_nchunk,wgrad} removed: the STFT encoder runs through maavss_conv2d_gen_*, which launch its (3,9)
 *        kernels when the call is such a layer; the size of maavss_conv2d_gen_wgrad's ws comes from maavss_conv2d_gen_wgrad_ws_bytes */
#define MAAVSS_ABI_VERSION 402
const char* maavss_last_error(void);
int maavss_version(void);
const char* maavss_arch(void);

/* ---- K17 audio STFT + noise ------------------------------------------------------------------
 * replaces AV_Dataset.stft (av_dataset.py:157-174: torchaudio spectrogram(pad=0, hamming, n_fft,
 * hop, power=None, normalized, onesided) minus the last frame [and last bin]) and
 * gen_stft_example/add_noise (av_dataset.py:217-220, 335-342).
 * audio [batch][audio_stride] (length valid samples), window [n_fft] = periodic Hamming already
 * multiplied by the 1/sqrt(sum w^2) normalisation, y/x [batch][2][n_frames][n_bins_out].
 * x (nullable) = y + sigma * noise; noise (nullable, same layout as y) else Philox4x32-10(seed).
 * clip_absmax (nullable) [batch], pre-zeroed: receives max|y| per clip (for maavss_stft_normalise). */
int maavss_stft_fwd(const float* audio, int64_t batch, int64_t length, int64_t audio_stride, const float* window,
                    int n_fft, int hop, int n_frames, int n_bins_out, float* y, float* x, const float* noise,
                    float sigma, uint64_t seed, float* clip_absmax, void* stream);
/* normalize_output_fft=True path (av_dataset.py:339-341): y *= 1/(clip_absmax + 1e-7); x = y + sigma*noise. */
int maavss_stft_normalise(float* y, float* x, const float* noise, const float* clip_absmax, int64_t batch,
                          int n_frames, int n_bins_out, float sigma, uint64_t seed, void* stream);

/* inverse: AV_Dataset.istft (av_dataset.py:181-201) = torch.istft(n_fft, hop, win_length = n_fft, window, normalized,
 * onesided, center).  spec [batch][2][n_frames][n_bins_in] (n_bins_in = n_fft/2+1, or n_fft/2 when the Nyquist bin was
 * trimmed: read as zero), window [n_fft] = the RAW periodic Hamming window; frames_ws [batch][n_frames][n_fft] scratch;
 * audio [batch][audio_stride], hop*(n_frames-1) valid samples per clip. */
int maavss_istft(const float* spec, int64_t batch, int n_frames, int n_bins_in, const float* window, int n_fft, int hop,
                 int normalized, float* frames_ws, float* audio, int64_t audio_stride, void* stream);

/* ---- EXTENSION: mix-and-separate training examples (maavss_amd.Mixer) --------------------------------------------------
 * extends add_noise / gen_stft_example (av_dataset.py:217-220, 335-342), whose only corruption of the input is white noise on
 * the STFT coefficients: the input becomes the clip plus other clips' audio at a chosen signal-to-interferer ratio, the target
 * stays the clip's own STFT.  Added without a version bump (nothing existing changed meaning).
 *   audio [batch][audio_stride], pool [n_pool][pool_stride] (length valid samples per row; pool may be audio itself);
 *   partners [batch][k_slots] int32 on the DEVICE, 1 <= k_slots <= 4, entries in [0, n_pool) or -1 = empty slot (anything else is
 *   read as empty: the values live on the device, the caller checks them);
 *   s_b[n] = sum_k pool[partners[b][k]][n], f32, summed in slot order;
 *   g_b = snr_factor[b] * sqrt(sum_n audio_b[n]^2 / sum_n s_b[n]^2), snr_factor[b] = 10^(-snr_db_b / 20) evaluated by the host
 *   (the two mean powers' 1/length cancels); g_b = 0 exactly when clip b has no partner or either sum is 0, and also when the
 *   quotient or the product is past float's range (an interferer some 1e-19 of the clip's level): no inf or NaN reaches an output.
 * maavss_mix_gains writes gain [batch].  One workgroup per clip, sequential runs then a tree, no atomics: the bits of g_b depend on
 * the clip, its partners and length only -- not on the launch or the run. */
int maavss_mix_gains(const float* audio, int64_t batch, int64_t length, int64_t audio_stride, const float* pool, int64_t n_pool,
                     int64_t pool_stride, const int* partners, int k_slots, const float* snr_factor, float* gain, void* stream);
/* mixture [batch][mixture_stride] = audio_b + g_b * s_b (the waveform behind x: for listening, or as Enhancer input).  mixture must
 * not overlap audio or pool (refused): other workgroups still read the rows one workgroup writes. */
int maavss_mix_wave(const float* audio, int64_t batch, int64_t length, int64_t audio_stride, const float* pool, int64_t n_pool,
                    int64_t pool_stride, const int* partners, int k_slots, const float* gain, float* mixture, int64_t mixture_stride,
                    void* stream);
/* x = y + (g_b * c_b) * STFT(s_b) + sigma * noise, with window / n_fft / hop / n_frames / n_bins_out / noise / seed as in
 * maavss_stft_fwd and y [batch][2][n_frames][n_bins_out] READ: the output of maavss_stft_fwd(audio, x = NULL), after
 * maavss_stft_normalise(x = NULL) when the clips are normalised -- the target is the plain call's, bit for bit.
 * clip_absmax NULL: c_b = 1 and the in-kernel noise (noise = NULL) is maavss_stft_fwd's, element for element, for the same seed;
 * clip_absmax [batch] (what maavss_stft_fwd wrote): c_b = 1 / (clip_absmax[b] + 1e-7) and the noise is maavss_stft_normalise's.
 * x must not overlap y, noise or pool (refused); for a clip whose g_b * c_b is 0 or not finite
 * x = y + sigma * noise.  Frames are paired inside a clip, so clip b's x depends on the launch through y alone. */
int maavss_stft_mix_fwd(const float* pool, int64_t n_pool, int64_t length, int64_t pool_stride, const int* partners, int k_slots,
                        int64_t batch, const float* window, int n_fft, int hop, int n_frames, int n_bins_out, const float* y, float* x,
                        const float* noise, float sigma, uint64_t seed, const float* gain, const float* clip_absmax, void* stream);

/* ---- generic f32 GEMM on MFMA -----------------------------------------------------------------
 * C[M,N] = act(alpha * op(A)[M,K] . op(B)[N,K]^T) (+ C when beta = 1).  Replaces the nn.Linear forwards
 * of avse_model_final.py:141-146,203-213,244-249,264-268, the LSTM input projection (:132,242) and the
 * gradients autograd derives from them.  transA=0: A[m*lda+k], 1: A[k*lda+m]; transB=0: B[n*ldb+k]
 * (torch Linear weight layout), 1: B[k*ldb+n]; transC=0: C[m*ldc+n], 1: C[n*ldc+m].
 * act: 0 none, 1 tanh, 2 sigmoid.  split_k: 0 = auto, n>1 = split K over n blocks (f32 atomics). */
/* Process-wide switch (default 0).  1: maavss_gemm_f32 takes no path that accumulates with f32 atomics (the split-K forms of the
 * M = batch Linear layers and the automatic split-K of the generic kernel) -- bit-identical results run to run, at the price of
 * slower weight streaming on those shapes.  Everything else in the library is deterministic already (conv weight gradients:
 * partial + reduce).  No reference counterpart (torch on one device is deterministic for these layers). */
int maavss_set_deterministic(int on);   /* returns the previous setting */
int maavss_get_deterministic(void);
/* Optional device scratch (16-byte aligned; the library never allocates) that lets deterministic mode keep the K split of the
 * M = batch Linear forms: slices write partial sums [slices][32][cols], a second kernel adds them in slice order.  8.4 MB covers the
 * reference shapes (fc1 8192 -> 4096 at 512-wide slices); shapes that need more fall back to one slice per output element.  One
 * scratch per process, bound to `stream`: Linear kernels launched on any other stream do not use it (single-slice path), so
 * two streams cannot race on it (ABI 400; before: no stream argument and no guard).  NULL removes it. */
int maavss_set_deterministic_workspace(float* ws, int64_t bytes, void* stream);
int maavss_gemm_f32(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                    int64_t ldc, int transC, int64_t M, int64_t N, int64_t K, float alpha, int beta, int act,
                    int split_k, int precise, void* stream);

/* ---- K7/K8 Conv3d(k=(3,5,5), stride 1, pad (1,p,p), bias=False) -- avse_model_final.py:34,39,44,49,54 ----
 * Activations channels-last [B][T][H][W][C] f32.  Weights in the reference layout [Co][Ci][3][5][5].
 * maavss_conv3d_kp(c_in): padded K of the re-laid weight image; prep writes wt[3][n][KP] in bf16 (precise=0)
 * or f32 (precise=1): mode 0 = forward (n=Co), mode 1 = input gradient (n=Ci; flipped taps, use pad 4-p).
 * igemm: y[B][T][Ho][Wo][c_out], Ho = H+2*pad-4; stat_partials (nullable) [grid blocks][2][c_out] receives
 * per-block (sum, sum^2) for BatchNorm, grid blocks = ceil(Wo/16)*ceil(Ho/16)*B*T.
 * wgrad: dw[Co][Ci][3][5][5] (+= when beta=1); ws of maavss_conv3d_wgrad_ws_bytes(c_in,c_out,nchunk) bytes.
 * x16 / dy16 = 1: that operand is already stored in the MFMA format of `precise` (IEEE half x from
 * maavss_bn_pool_act_fwd's out16 for the forward pass, bf16 dy from maavss_bn_pool_act_bwd for the two backward passes):
 * the producer rounded once, the kernels copy instead of converting -- bit-identical results, half the bytes. */
int maavss_conv3d_kp(int c_in);
int maavss_conv3d_prep_weights(const float* w, void* wt, int c_out, int c_in, int mode, int precise, void* stream);
int maavss_conv3d_igemm(const void* x, const void* wt, float* y, float* stat_partials, int B, int T, int H, int W,
                        int c_in, int c_out, int pad, int precise, int x16, void* stream);
int64_t maavss_conv3d_wgrad_ws_bytes(int c_in, int c_out, int nchunk);
/* in16: bit 0 = dy is bf16 (precise = 0), bit 1 = x is bf16 as well (needs bit 0 and one of the shapes 16->32, 32->64, 64->64: both operand
 * images then go global -> LDS by DMA, no conversion); any combination gives the same dw bit for bit. */
int maavss_conv3d_wgrad(const void* x, const void* dy, float* dw, float* ws, int nchunk, int B, int T, int H, int W,
                        int c_in, int c_out, int pad, int beta, int precise, int in16, void* stream);
/* first layer (C_in = 1, pad 2): x [B][T][H][W], w [16][1][3][5][5], w16_ws 1200 floats scratch,
 * y [B][T][H][W][16]; stat_partials [maavss_conv3d_c1_fwd_nparts(...)][2][16] (one row per workgroup: the MFMA form walks
 * 8 tiles per workgroup); wgrad ws = nchunk*1200 floats. */
int64_t maavss_conv3d_c1_fwd_nparts(int B, int T, int H, int W, int precise);
int maavss_conv3d_c1_fwd(const float* x, const float* w, float* w16_ws, float* y, float* stat_partials, int B, int T,
                         int H, int W, int precise /* 1: exact-f32 VALU convolution; 2: IEEE-half operands on the MFMA
                         (25 taps of a kd plane = one 32-deep step), f32 accumulation */, void* stream);
int maavss_conv3d_c1_wgrad(const float* x, const float* dy, float* dw, float* ws, int nchunk, int B, int T, int H,
                           int W, int beta, void* stream);
/* The same with the first layer's BatchNorm / max-pool / LeakyReLU backward folded into the loader: y is the conv output,
 * dout / out / argmax [B*T][H/pool][W/pool][16] the pooled gradient, output and window argmax, coef [3][16] the
 * coefficients maavss_bn_pool_act_bwd leaves at ws + 2*C*maavss_bn_stats_nblk(rows) when called with dy = NULL. */
int maavss_conv3d_c1_wgrad_bn(const float* x, const float* y, const float* dout, const float* out, const void* argmax,
                              const float* mean, const float* invstd, const float* coef, int pool, float* dw, float* ws,
                              int nchunk, int B, int T, int H, int W, int beta,
                              int precise /* 1: exact-f32 VALU; 0: bf16 operands on the MFMA (positions = K dimension) */, void* stream);

/* The 16-bit first layer WITHOUT its conv output (avse_model_final.py:34-37: Conv3d(1,16,(3,5,5)) -> BatchNorm3d -> MaxPool3d((1,2,2))
 * -> LeakyReLU): y [B][T][H][W][16] is the largest tensor of the step (1.6 GB at 32 x 16 x 224^2) and the layer is 59 GFLOP on
 * an idle matrix pipe, so the convolution is run three times instead of stored once and read twice:
 *   maavss_conv3d_c1_stats          conv (IEEE-half MFMA) -> stat_partials [maavss_conv3d_c1_fwd_nparts(.., 2)][2][16] only; `y` is
 *                                   written ONLY if some |gamma[c]| < 1e-2 (the BatchNorm backward reduction then gathers from it);
 *   maavss_conv3d_c1_bn_pool_act    conv again -> gamma (y - mean) invstd + beta -> 2x2 max pool -> LeakyReLU(0.01): out f32 and out16
 *                                   (IEEE half, may be NULL) [B*T][H/2][W/2][16], argmax one byte per element (window position
 *                                   dy * 2 + dx); bit-identical to maavss_conv3d_c1_fwd(.., 2) + maavss_bn_pool_act_fwd;
 *   maavss_conv3d_c1_wgrad_bn_recompute   maavss_conv3d_c1_wgrad_bn(.., precise 0) with w [16][1][3][5][5] in place of y and the
 *                                   BatchNorm bias bn_beta [16] in place of the pooled output: the tile's y is recomputed from the
 *                                   staged halo and the LeakyReLU slope from its sign; bit-identical gradient. */
int maavss_conv3d_c1_stats(const float* x, const float* w, const float* gamma, float* y, float* stat_partials, int B, int T, int H,
                           int W, void* stream);
int maavss_conv3d_c1_bn_pool_act(const float* x, const float* w, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, float* out, void* out16, void* out_bf16 /* nullable, as maavss_bn_pool_act_fwd's */,
                                 void* argmax, int B, int T, int H, int W, void* stream);
int maavss_conv3d_c1_wgrad_bn_recompute(const float* x, const float* w, const float* dout, const void* argmax, const float* mean,
                                        const float* invstd, const float* bn_beta, const float* coef, int pool, float* dw, float* ws,
                                        int nchunk, int B, int T, int H, int W, int beta, void* stream);

/* ---- K9 BatchNorm (train mode) + MaxPool(1,p,p) + LeakyReLU / BatchNorm2d + Tanh -----------------
 * avse_model_final.py:35-37,...,55-57 (pool before activation) and :103-104 (pool = 1, act = 1).
 * y channels-last [B*T][H][W][C]; the pooled output (and its gradient) are addressed with element strides
 * b*os_b + t*os_t + (py*Wp+px)*os_p + c*os_c so the last stage can write the [B,16,T,S] / LSTM-sequence
 * layout directly (avse_model_final.py:58,239-240).  act: 0 LeakyReLU(0.01), 1 Tanh.
 * bn_finalize: count = B*T*H*W; updates running stats with `momentum` and the unbiased variance and
 * increments num_batches_tracked (int64) like torch.nn.BatchNorm (pointers nullable).
 * bwd ws: (2*C*nblk + 3*C) floats, nblk = maavss_bn_stats_nblk(B*T*Hp*Wp). */
int maavss_bn_stats_nblk(int64_t rows);
int maavss_bn_stats(const float* y, float* partials, int64_t rows, int C, void* stream);
int maavss_bn_finalize(const float* partials, int nblk, int C, double count, float eps, float momentum, float* mean,
                       float* invstd, float* running_mean, float* running_var, void* num_batches_tracked,
                       float* ws /* nullable; 256*2*C floats enable the two-level reduction */, void* stream);
/* eval mode (model.eval()): mean / invstd from the running statistics instead of the batch */
int maavss_bn_eval_stats(const float* running_mean, const float* running_var, float eps, float* mean, float* invstd, int C,
                         void* stream);
int maavss_bn_pool_act_fwd(const float* y, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, float* out, void* argmax, int B, int T, int H, int W, int C, int pool,
                           int act, int64_t os_b, int64_t os_t, int64_t os_p, int64_t os_c,
                           void* out16 /* nullable: IEEE-half copy of the pooled activation, contiguous channels-last
                                          [B][T][Hp][Wp][C] -- the operand format of the next Conv3d's forward MFMA */,
                           void* out_bf16 /* nullable: the same as bf16 -- the x operand of the next Conv3d's weight gradient
                                             (maavss_conv3d_wgrad, in16 bit 1) */,
                           void* stream);
/* beta (nullable): with it, LeakyReLU layers recover the normalised input at the pooled maximum from `out` instead of
 * gathering it from y (xhat = (leaky^-1(out) - beta) / gamma; channels with |gamma| < 1e-2 still gather).  dy NULL: only
 * dgamma / dbeta and the coefficients (see maavss_conv3d_c1_wgrad_bn). */
int maavss_bn_pool_act_bwd(const float* dout, const float* out, const void* argmax, const float* y,
                           const float* mean, const float* invstd, const float* gamma, const float* beta, void* dy, float* dgamma,
                           float* dbeta, int accumulate, float* ws, int B, int T, int H, int W, int C, int pool,
                           int act, int64_t os_b, int64_t os_t, int64_t os_p, int64_t os_c,
                           int dy_bf16 /* 1: dy is written as bf16 (what both of its MFMA consumers round it to), 0: f32 */,
                           void* stream);

/* Global-batch BatchNorm under data parallelism (the reference normalises over the WHOLE batch on one device,
 * avse_model_final.py:35,40,45,50,55,103): split forms whose per-channel sums -- double sums[2*C + 1] = {sum, sum^2 (or
 * sum g, sum g*z), element count} -- are all-reduced by the host (RCCL) between the two halves.  bwd_finish takes this
 * rank's sums for dgamma / dbeta (the gradient all-reduce adds the ranks) and the reduced ones for the dx coefficients;
 * coef: 3*C floats (as left by maavss_bn_pool_act_bwd in its ws). */
int maavss_bn_partials_to_sums(const float* partials, int nblk, int C, double count, double* sums,
                               float* ws /* nullable, as bn_finalize */, void* stream);
int maavss_bn_finalize_sums(const double* sums, int C, float eps, float momentum, float* mean, float* invstd,
                            float* running_mean, float* running_var, void* num_batches_tracked, void* stream);
int maavss_bn_pool_act_bwd_sums(const float* dout, const float* out, const void* argmax, const float* y, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, float* ws, double* sums, int B,
                                int T, int H, int W, int C, int pool, int act, int64_t os_b, int64_t os_t, int64_t os_p,
                                int64_t os_c, void* stream);
int maavss_bn_pool_act_bwd_finish(const float* dout, const float* out, const void* argmax, const float* y, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, void* dy, float* dgamma,
                                  float* dbeta, int accumulate, const double* sums_local, const double* sums_global,
                                  float* coef, int B, int T, int H, int W, int C, int pool, int act, int64_t os_b,
                                  int64_t os_t, int64_t os_p, int64_t os_c, int dy_bf16, void* stream);

/* ---- K19 Conv2d / ConvTranspose2d (bias nullable): the phasegram variant avse_model.AV_Fusion_Model
 * (avse_model.py:433,452,494,591): kernels (1,9) and (5,5), any stride / padding, <= 30 taps, the
 * STFT decoder (avse_model_final.py:155-193: ConvTranspose2d (3,9) / (3,10), padding (1,4), bias=False; formerly K11) and the
 * STFT encoder (K10; avse_model_final.py:98-102: Conv2d (3,9), stride in {1,2}^2, padding (1,pw), bias=False).
 * A small map S [B][Hs][Ws][Cs] and a big map G [B][Hb][Wb][Cb] with by = sy*sh - ph + kh, bx = sx*sw - pw + kw and a
 * weight w[cs][cb][kh][kw] (= Conv2d's [Co][Ci] and ConvTranspose2d's [Ci][Co]):
 *   gen_small: S = bias + G (*) w   -- Conv2d forward, ConvTranspose2d input gradient (bias NULL)
 *   gen_big:   G = bias + S (*)^T w -- ConvTranspose2d forward, Conv2d input gradient (bias NULL)
 *   gen_wgrad: dw = S (x) G         -- both; ws: maavss_conv2d_gen_wgrad_ws_bytes(the same geometry) bytes
 * A call without bias that is an encoder layer -- kernel (3,9), ph = 1, pw <= 8, strides in {1,2}^2, S dense NHWC of the size the
 * convolution arithmetic gives, G dense NHWC (gen_small, gen_wgrad: or dense NCHW), Cs in {4,8,16} with Cb <= 16 (gen_small), Cs in
 * {4,8,12,16} with Cb in {2,4,8,16} (gen_big), Cs in {4,8,16} (gen_wgrad) -- launches one-thread-per-position kernels and a weight
 * gradient of one partial per >= 1024 positions; every other call one-thread-per-element kernels and one partial per
 * maavss_conv2d_gen_wgrad_nchunk(B,Hs,Ws) = 4096 positions.  Which of the two runs is part of the result's last bits.
 * small_strides / big_strides: HOST arrays of 4 element strides {batch, y, x, channel} (NCHW and channels-last, also
 * channel-padded, without copies).  channel_sum: out[c] (+)= sum_rows x[row*row_stride + c*chan_stride] (bias gradients). */
int maavss_conv2d_gen_small(const float* big, const float* w, const float* bias, float* small, int B, int Cs, int Hs, int Ws,
                            int Cb, int Hb, int Wb, int kh, int kw, int sh, int sw, int ph, int pw,
                            const int64_t* small_strides, const int64_t* big_strides, void* stream);
int maavss_conv2d_gen_big(const float* small, const float* w, const float* bias, float* big, int B, int Cs, int Hs, int Ws,
                          int Cb, int Hb, int Wb, int kh, int kw, int sh, int sw, int ph, int pw,
                          const int64_t* small_strides, const int64_t* big_strides, void* stream);
int maavss_conv2d_gen_wgrad_nchunk(int B, int Hs, int Ws);
int64_t maavss_conv2d_gen_wgrad_ws_bytes(int B, int Cs, int Hs, int Ws, int Cb, int Hb, int Wb, int kh, int kw, int sh, int sw, int ph,
                                         int pw, const int64_t* small_strides, const int64_t* big_strides);
int maavss_conv2d_gen_wgrad(const float* small, const float* big, float* dw, float* ws, int B, int Cs, int Hs, int Ws, int Cb,
                            int Hb, int Wb, int kh, int kw, int sh, int sw, int ph, int pw, const int64_t* small_strides,
                            const int64_t* big_strides, int beta, void* stream);
int maavss_channel_sum(const float* x, float* out, int64_t rows, int C, int64_t row_stride, int64_t chan_stride, int beta,
                       void* stream);
/* Linear bias + LeakyReLU(slope) (avse_model.py:613-621,660-663): z = act(z + bias) in place over [rows][n], act 0 = none,
 * 3 = LeakyReLU; leaky_bwd: dz = dout * (out > 0 ? 1 : slope). */
int maavss_bias_act_fwd(float* z, const float* bias, int64_t rows, int n, int act, float slope, void* stream);
int maavss_leaky_bwd(const float* dout, const float* out, float* dz, int64_t n, float slope, void* stream);

/* ---- K20 utilities.video_phasegram (utilities.py:206-228; train_av_net.py:122-125) ----
 * frames [batch][T][P][P] (attention maps, P in {32, 64}); out [batch][T][P*P] (= the reference's [B,1,T,P*P]):
 * fft2 -> fftshift over ALL axes, batch and frame included (the reference passes no dim) -> angle -> (cumulative ? cumsum / (2 pi P*P) : (angle + pi) / 2 pi) -> (diff ? temporal difference with a
 * zero first row) -> (normalize ? / max |.| over the whole batch tensor).  p_ws [batch][T][P*P] and absmax_ws [1] are scratch. */
int maavss_video_phasegram(const float* frames, int64_t batch, int T, int P, int diff, int cumulative, int normalize, float* p_ws,
                           float* absmax_ws, float* out, void* stream);

/* bilinear resize in front of the phasegram (utilities.py:208-209: torchvision resize of a tensor =
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False), no antialias): in [n][H][W] -> out [n][h][w]. */
int maavss_resize_bilinear(const float* in, float* out, int64_t n, int H, int W, int h, int w, void* stream);

/* ---- K12 bidirectional LSTM recurrence (hidden 256, no bias) -- avse_model_final.py:132-133,242 ----
 * gx [B][L][2][4][256] = X.W_ih^T (both directions, gate order i,f,g,o); av [B][L][512]; hp [B][L][2][256];
 * gs [B][L][2][4][256]; cs [B][L][2][256]; bwd: dav [B][L][512] -> dgx (same shape as gx), dc scratch [2][B][256]. */
int maavss_lstm_fwd(const float* gx, const float* whh_f, const float* whh_b, float* av, float* hp, float* gs,
                    float* cs, int B, int L, void* stream);
int maavss_lstm_bwd(const float* dav, const float* whh_f, const float* whh_b, const float* gs, const float* cs,
                    float* dgx, float* dc, int B, int L, void* stream);

/* ---- K15/K16 loss, activation backward, Adam ---------------------------------------------------
 * act_bwd: dz = dout * act'(out), act 1 tanh / 2 sigmoid (avse_model_final.py:246-249,264-268).
 * mse_pair: losses[0..2] = a_loss, v_loss, (a_loss + coeff*v_loss)*inv_num_seq and (nullable) the gradients
 * of losses[2] w.r.t. the predictions (train_avse_frames.py:166-170); ws = 1024 floats.
 * adam_step: torch.optim.Adam semantics (train_avse_frames.py:92,180) on flat 16-byte-aligned buffers;
 * `step` is the 1-based step count, grad_scale multiplies g (1/world_size for data parallel). */
int maavss_act_bwd(const float* dout, const float* out, float* dz, int64_t n, int act, void* stream);
int maavss_mse_pair(const float* a_pred, const float* a_tgt, int64_t na, const float* v_pred, const float* v_tgt,
                    int64_t nv, float coeff, float inv_num_seq, float* d_a, float* d_v, float* losses, float* ws,
                    void* stream);
int maavss_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, int64_t step, float grad_scale, void* stream);
/* adam_step_dscale: maavss_adam_step with the gradient scale read from device memory (one f32, 4-byte aligned) by the same kernel
 * body -- the clip scale maavss_tensor_stats wrote earlier on the stream, so that clipping costs no host synchronisation.  Same
 * arithmetic: with *grad_scale_dev == grad_scale the results are bit-identical to maavss_adam_step's. */
int maavss_adam_step_dscale(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                            float eps, int64_t step, const float* grad_scale_dev, void* stream);

/* ---- EXTENSION: AdamW decay, weight average and non-finite step skip in the optimizer kernel (maavss_amd.FusedAdam) --------------
 * NOT in the reference, whose optimizer is torch.optim.Adam at one fixed rate (train_avse_frames.py:92): decoupled weight decay per
 * tensor (torch.optim.AdamW's update), an exponential moving average of the weights (lerp(ema, p, 1 - d)) and the skip of a step whose
 * gradient norm is not finite, in one launch per contiguous run of stepped parameters.  Added without a version bump; maavss_adam_step
 * and maavss_adam_step_dscale are unchanged (they are compiled with contraction and are not bit-compatible with this entry point).
 * adamw_ema_step: p, g, m, v and (nullable) ema are f32 [n], 16-byte aligned.  Per element, every operation an IEEE f32 operation
 * rounded on its own (the file is compiled without contraction; tests/optim_twin.py restates it):
 *     gr = g * gscale                                   gscale = *scale_dev when scale_dev is given (4-byte aligned), else grad_scale
 *     m  = beta1 * m + (1.f - beta1) * gr
 *     v  = beta2 * v + ((1.f - beta2) * gr) * gr
 *     p  = p * decay_s                                  decay_s = (float)(1.0 - (double)lr * (double)wd_s), s = the element's segment
 *     p  = p - (lr_bc1 * m) / (sqrtf(v) * inv_sqrt_bc2 + eps)
 *     e  = ema_decay * e + one_m_d * p                  only with ema; one_m_d = (float)(1.0 - (double)ema_decay), 0 <= ema_decay < 1
 * with lr_bc1 = (float)(lr / (1 - beta1^step)) and inv_sqrt_bc2 = (float)(1 / sqrt(1 - beta2^step)) formed in double as maavss_adam_step
 * forms them; `step` is the 1-based step count.  wd_s = 0 gives decay_s == 1.0f and p * 1 == p: undecayed tensors take no branch.
 * Decay table (HOST arrays, copied into the launch arguments: no device table, no staging copy): host_seg_end [n_seg] = the segment
 * ends in elements relative to p, ascending, multiples of 4, the last one >= n; host_seg_wd [n_seg] = the weight decay of each segment,
 * finite and >= 0; 1 <= n_seg <= 64 -- the caller splits a run with more (maavss_amd.trainer.plan_launches).
 * Skip: with skip_nonfinite != 0 the kernel reads *norm_dev (f32, what maavss_tensor_stats left on the stream) and, when it is NaN or
 * an infinity, every thread returns before its first store: p, m, v and ema keep their bytes.  With count_skip != 0 (needs
 * skip_nonfinite and skipped) thread 0 of workgroup 0 then adds 1 to *skipped with a plain load and store: exactly one launch of a step
 * carries the flag and launches on a stream are ordered.  Deviation from torch.cuda.amp.GradScaler, which leaves a skipped step out of
 * the optimizer's step count: `step` is the caller's count, and maavss_amd.FusedAdam advances it (and its learning-rate schedule) on a
 * skipped step too -- the bias correction moves on by one step while the moments do not move.
 * Every argument is checked before the launch.  No float atomics: two runs give identical bytes.
 * swap_f32: exchanges a [n] and b [n] in place (16-byte aligned, not overlapping): the weights and their average around a validation
 * pass, without a third buffer. */
int maavss_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                          float eps, int64_t step, float grad_scale, const float* scale_dev, const float* norm_dev,
                          int skip_nonfinite, int* skipped, int count_skip, const int64_t* host_seg_end, const float* host_seg_wd,
                          int n_seg, float ema_decay, void* stream);
int maavss_swap_f32(float* a, float* b, int64_t n, void* stream);

/* ---- EXTENSION: per-tensor statistics of a flat f32 buffer (maavss_amd.TensorStats, gradient-norm clipping, ModelWatch) ------
 * What torch.nn.utils.clip_grad_norm_ and wandb.watch(model, log="all") (train_avse_frames.py:108) compute through autograd hooks,
 * for the autograd-free step: one segmented reduction over the flat gradient (or parameter) buffer.  Added without a version bump.
 *   segment s = one tensor, elements [host_seg_offset[s], + host_seg_numel[s]) of buf [n] (buf 16-byte aligned; numel < 2^31);
 *   chunks [n_chunks][3] int64 on the DEVICE: (segment, first element, length) -- every segment cut, in buffer order, into
 *   ceil(numel / CH) pieces of at most CH = maavss_tensor_stats_chunk() elements; seg_first [n_segments + 1] int32 on the device:
 *   the rows of segment s are seg_first[s] .. seg_first[s + 1].  A row outside the buffer is read as empty.
 *   seg_mask [n_segments] int32 (nullable = all): the segments that count towards total_sumsq / norm / scale.
 * Per segment: sumsq f64 = sum of the squares of the FINITE elements (squares exact, accumulated in f64 in a fixed order: within
 * (numel - 1) * 2^-53 relative of the exact sum), seg_min / seg_max f32 over the finite elements (NaN when there is none),
 * nonfinite [n_segments][3] int32 = counts of NaN, +inf, -inf.
 * max_norm >= 0 requests a clip: total_sumsq f64 = sum of sumsq over the selected segments; with
 *   norm64 = sqrt(total_sumsq) * grad_scale (f64), norm = (float)norm64, scale = (float)(grad_scale * min(1, max_norm / (norm64 + 1e-6)))
 * -- clip_grad_norm_'s coefficient for the gradient after grad_scale, times grad_scale: what maavss_adam_step_dscale multiplies g by.
 * A NaN in a selected segment makes norm and scale NaN, otherwise an inf makes norm +inf and scale 0 (error_if_nonfinite=False).
 * max_norm < 0: total_sumsq / norm / scale are not written (and may be null).
 * hist (nullable) [n_segments][bins] int32, 1 <= bins <= 1024: torch.histc(x, bins) of the finite elements of each segment between
 * its min and max ([lo - 1, hi + 1] when they are equal): element x counts in bin (int)((x - lo) * (float)bins / (hi - lo)) evaluated
 * in f32 with one rounding per operation, bins -> bins - 1.
 * ws: maavss_tensor_stats_ws_bytes(n_chunks, n_segments, bins) bytes, 8-byte aligned =
 *   round256(32 * n_chunks) [one {f64 sumsq, f32 min, f32 max, int32 nan, +inf, -inf, pad} per chunk] + round256(8 * n_segments)
 *   [the selected sums]; `bins` is range-checked only (0 for an invalid argument): the counts are accumulated in hist itself.
 * Launches: pass 1 (one workgroup per chunk), finalize (one workgroup), and with hist a second pass over buf.  No floating-point
 * atomics: every output is bit-identical from run to run. */
int maavss_tensor_stats_chunk(void);
int64_t maavss_tensor_stats_ws_bytes(int64_t n_chunks, int64_t n_segments, int bins);
int maavss_tensor_stats(const float* buf, int64_t n, const int64_t* chunks, int64_t n_chunks, const int* seg_first,
                        const int64_t* host_seg_offset, const int64_t* host_seg_numel, int64_t n_segments, const int* seg_mask,
                        double* sumsq, float* seg_min, float* seg_max, int* nonfinite, int* hist, int bins, double max_norm,
                        float grad_scale, double* total_sumsq, float* norm, float* scale, void* ws, int64_t ws_bytes, void* stream);

/* ---- EXTENSION: quality metrics of held-out data (maavss_amd.quality: wave_metrics, spectrum_metrics, Validator) ---------------
 * The reference validates: train_avse_frames.py:55-65 splits off a validation set, train_av_net.py:147-181 averages the loss over
 * val_steps batches under model.eval() + torch.no_grad() and saves a checkpoint when it improves (:174-181).  These entry points are the
 * reductions of that pass, plus the waveform measures an enhanced recording is judged by.  Added without a version bump.  Every sum is
 * f64 over the f32 inputs, in a fixed order (partials in the workspace, combined in index order): no floating-point atomics, two runs
 * give identical bytes.  No epsilon anywhere.
 *
 * maavss_wave_metrics: per row of est [B][L] against ref [B][L]; strides in elements, >= 0, rows may overlap (stride < L), ignored when
 * B = 1; the pointers need 4-byte alignment only.  out [B][9] f64:
 *   0 Sxx = sum ref^2   1 Syy = sum est^2   2 Sxy = sum ref est   3 See = sum (est - ref)^2
 *   4 Srr = sum (est - alpha ref)^2, alpha = Sxy / Sxx, summed directly in a second pass over the rows
 *   5 snr_db = 10 log10(Sxx / See) (+inf when est == ref; NaN when Sxx = 0: without a reference there is no ratio)
 *   6 si_sdr_db = 10 log10(alpha^2 Sxx / Srr) (+inf when est = c ref, -inf when Sxy = 0, NaN when Sxx = 0)
 *   7 seg_snr_db = mean over the floor(L / seg_len) complete frames with Sxx_f > 0 of clamp(10 log10(Sxx_f / See_f), -10, 35); a trailing
 *     partial frame is dropped; NaN when no frame counts      8 the number of frames that counted
 * A non-finite sample in est or ref makes columns 0-7 of that row NaN and column 8 zero.  1 <= seg_len <= CH = maavss_wave_metrics_chunk():
 * a row is cut into ceil(L / CL) chunks of CL = floor(CH / seg_len) * seg_len samples (whole frames; the last chunk takes the rest), one
 * workgroup each, so a single long row uses the whole device.  ws: maavss_wave_metrics_ws_bytes(B, L, seg_len) bytes, 8-byte aligned =
 * round256(48 * B * chunks) [{Sxx, Syy, Sxy, See, frame sum, frame count} per chunk] + round256(8 * B * chunks) [Srr] + round256(8 * B)
 * [alpha]; 0 for invalid arguments.  Four launches: pass 1, finalize, pass 2, finalize. */
int maavss_wave_metrics_chunk(void);
int64_t maavss_wave_metrics_ws_bytes(int64_t B, int64_t L, int seg_len);
int maavss_wave_metrics(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t B, int64_t L, int seg_len,
                        double* out, void* ws, int64_t ws_bytes, void* stream);
/* maavss_spectrum_metrics: per row of pred [B][2][T][F] against tgt (contiguous; F may be odd).  out [B][2] f64:
 *   0 the squared-error sum over the 2 T F elements -- the numerator of the reference's MSE (train_avse_frames.py:166)
 *   1 lsd_db = mean over T of sqrt(mean over F of (10 log10(max(P_pred, floor)) - 10 log10(max(P_tgt, floor)))^2), P = re^2 + im^2 in f64;
 *     lsd_floor > 0 is a power.  A NaN power stays a NaN.
 * ws: maavss_spectrum_metrics_ws_bytes(B, T) = round256(16 * B * T) bytes [{squared error, frame distance} per (b, t)].
 * maavss_sqerr_rows: out [B] f64 = sum over n of (pred - tgt)^2 per row of two contiguous [B][n] arrays (the attention term of the loss,
 * train_avse_frames.py:167); ws: maavss_sqerr_rows_ws_bytes(B, n) = round256(8 * B * ceil(n / maavss_sqerr_rows_chunk())) bytes. */
int64_t maavss_spectrum_metrics_ws_bytes(int64_t B, int64_t T);
int maavss_spectrum_metrics(const float* pred, const float* tgt, int64_t B, int64_t T, int64_t F, double lsd_floor, double* out, void* ws,
                            int64_t ws_bytes, void* stream);
int maavss_sqerr_rows_chunk(void);
int64_t maavss_sqerr_rows_ws_bytes(int64_t B, int64_t n);
int maavss_sqerr_rows(const float* pred, const float* tgt, int64_t B, int64_t n, double* out, void* ws, int64_t ws_bytes, void* stream);
/* The Validator's additive f64 accumulator (sums and counts only: the mean over val_steps batches of train_av_net.py:160-172 is a
 * quotient taken on the host at the end), updated on the device, one wave, fixed order.
 * add_sum: acc[0] += sum_i vals[i * stride], acc[1] += n * weight (the number of elements behind the n values).
 * add_classes: for each column c < cols, v_i = vals[i * stride + c] - minus[i * stride + c] (minus nullable: v_i = vals[...]);
 * acc[5 c + 0..4] += {sum of the finite v_i, count of finite, +inf, -inf, NaN}. */
int maavss_metric_add_sum(const double* vals, int64_t n, int64_t stride, double weight, double* acc, void* stream);
int maavss_metric_add_classes(const double* vals, const double* minus, int64_t n, int64_t stride, int cols, double* acc, void* stream);

/* ---- EXTENSION: power-law compressed spectral loss and its gradient (maavss_amd.SpectralLoss, TrainStep(audio_loss=...)) -------
 * An audio objective beside the plain MSE of mse_pair: compressed magnitudes plus compressed complex coefficients, per bin, on any
 * number of frames and without an inverse STFT.  Added without a version bump.  tests/spectral_loss_twin.py is the float64 restatement.
 * pred, tgt: f32 contiguous [B][2][T][F], plane 0 real and plane 1 imaginary (F may be odd; 4-byte alignment only).  Parameters:
 * compress c in (0, 1], mix lambda in [0, 1], eps > 0 (a power).  Everything is evaluated in f64 on the exactly converted f32 inputs,
 * every operation rounded on its own.  Per bin, for pred (p) and tgt (t):
 *   r  = re^2 + im^2 + eps          M = pow(r, c / 2)          g = pow(r, (c - 1) / 2)      (two pows: c = 1 gives g = 1 exactly)
 *   e_r = p_r g_p - t_r g_t         e_i = p_i g_p - t_i g_t
 *   mag term = (M_p - M_t)^2        complex term = e_r^2 + e_i^2
 *   S_mag[b], S_cplx[b] = the sums over the T F bins of row b: a wave per (b, t) frame (lane l adds bins l, l + 64, ..., then a butterfly),
 *   then the row's frames in index order
 *   a_loss = ((1 - lambda) sum_b S_mag[b] + lambda sum_b S_cplx[b]) / (2 B T F)
 * The denominator is the number of real elements: compress = 1, mix = 1 is the MSE a_loss of mse_pair (the mag term times an exact 0).
 * The gradient with respect to pred, each element rounded once to f32:
 *   s = e_r p_r + e_i p_i      q = (c - 1) g_p / r_p      k = (1 - lambda) (M_p - M_t) c M_p / r_p
 *   d/dp_r = 2 grad_scale (k p_r + lambda (e_r g_p + q s p_r))      d/dp_i = 2 grad_scale (k p_i + lambda (e_i g_p + q s p_i))
 * A bin that is zero on both sides has gradient 0; pred == tgt gives sums 0 and gradient 0 exactly; a non-finite input makes its row's
 * sums non-finite and the gradient non-finite in the bins where this arithmetic says so.  No floating-point atomics: two runs give
 * identical bytes, and a row of a batch has the bytes of a call of its own.
 * maavss_spectral_loss: rows [B][2] f64 = {S_mag, S_cplx} per row; d_pred (nullable: the forward-only form writes no gradient) f32 of
 * pred's shape.  ws: maavss_spectral_loss_ws_bytes(B, T) = round256(16 B T) bytes, 8-byte aligned [{mag, complex} per (b, t)]; 0 for
 * invalid sizes.  Two launches.
 * maavss_spectral_loss_pair: mse_pair with this audio term.  losses [3] f32 in mse_pair's positions: a_loss as above, v_loss and
 * d_v (nullable) by mse_pair's own kernel and arithmetic (bit-identical to maavss_mse_pair's on the same operands),
 * (a_loss + coeff v_loss) inv_num_seq; d_a (nullable) = the gradient above with grad_scale = inv_num_seq / (2 B T F); parts [2] f64 =
 * sum_b S_mag / (2 B T F), sum_b S_cplx / (2 B T F).  ws: maavss_spectral_loss_pair_ws_bytes(B, T) bytes, 8-byte aligned. */
int64_t maavss_spectral_loss_ws_bytes(int64_t B, int64_t T);
int maavss_spectral_loss(const float* pred, const float* tgt, int64_t B, int64_t T, int64_t F, double compress, double mix, double eps,
                         double grad_scale, float* d_pred, double* rows, void* ws, int64_t ws_bytes, void* stream);
int64_t maavss_spectral_loss_pair_ws_bytes(int64_t B, int64_t T);
int maavss_spectral_loss_pair(const float* a_pred, const float* a_tgt, int64_t B, int64_t T, int64_t F, double compress, double mix,
                              double eps, const float* v_pred, const float* v_tgt, int64_t nv, float coeff, float inv_num_seq, float* d_a,
                              float* d_v, float* losses, double* parts, void* ws, int64_t ws_bytes, void* stream);

/* ---- EXTENSION: clip-level waveform loss through the inverse STFT (maavss_amd.WaveformLoss, TrainStep(wave_loss=...)) -----------
 * SI-SDR or SNR of istft(pred) against istft(tgt), in dB with the sign of a loss (lower is better), and its gradient with respect to
 * pred.  Added without a version bump.  tests/wave_loss_twin.py is the float64 restatement.  pred, tgt: f32 contiguous [B][2][T][F],
 * F = n_bins = N/2 + 1 or N/2 (trimmed), N = n_fft in {256, 512, 1024}, T >= 2, 0 < hop <= N: the conditions of maavss_istft.
 * window = the synthesis window w of maavss_istft.  L = hop (T - 1), c = (normalized ? sqrt N : 1) / N.
 *   waves     x = istft(pred), s = istft(tgt), f32 [B][L], by maavss_istft's own kernels: bit-identical to what that entry returns
 *   sums      Sxx = sum x^2, Sss = sum s^2, Sxs = sum x s, D = sum (x - s)^2: f64 sums over the exactly converted f32 samples in a
 *             fixed order, the chunk passes of maavss_wave_metrics.  No mean is subtracted.
 *   snr       kind 1: l = 10 log10(D + eps) - 10 log10(Sss + eps), E = D
 *   si_sdr    kind 0: alpha = Sxs / (Sss + eps), E = sum (x - alpha s)^2 summed directly in a second pass,
 *             l = 10 log10(E + eps) - 10 log10(alpha^2 Sss + eps)
 *   rows      [B][5] f64 = (l, Sxx, Sss, Sxs, E).  eps > 0: every finite input has a finite loss and gradient; a row with a NaN or an
 *             infinity in either wave has five NaNs and a NaN gradient, and no other row is touched.
 *   gradient  g[n] = d(sum_b l_b) / dx[n] = a_b x[n] + b_b s[n] with k = 10 / ln 10:
 *             snr      a = 2 k / (D + eps), b = -a
 *             si_sdr   a = 2 k / (E + eps), b = -2 k alpha ((1 + eps / (Sss + eps)) / (E + eps) + Sss / ((Sss + eps) (alpha^2 Sss + eps)))
 *             carried to the STFT planes by the adjoint of maavss_istft: den[p] = sum_t w[p - t hop]^2 over the frames that cover
 *             position p of the centre-padded signal; u[p] = g[p - N/2] / den[p] for N/2 <= p < N/2 + L and 0 elsewhere;
 *             q_t[j] = c w[j] u[t hop + j] (formed in f64, rounded once to f32);
 *             d/dRe X_t[k] = grad_scale m_k sum_j q_t[j] cos(2 pi j k / N), d/dIm X_t[k] = -grad_scale m_k sum_j q_t[j] sin(2 pi j k / N),
 *             m_k = 2 for 0 < k < N/2 and 1 for k = 0, N/2; the imaginary gradients of DC and Nyquist are 0 (irfft drops those inputs).
 * d_pred (nullable: the forward-only form writes no gradient): block t / d_frames of the destination takes frame t of the clip; a block
 * is a contiguous [B][2][d_frames][F] and blocks lie d_block_stride elements apart (d_frames = T: one block, pred's own layout;
 * d_frames must divide T).  accumulate != 0 adds the gradient, rounded to f32, to what the destination holds.
 * ws: maavss_wave_loss_ws_bytes(B, T, n_fft, hop) bytes, 8-byte aligned; 0 for invalid sizes.  It starts with the two waves,
 * x [B][L] then s [B][L] f32, followed by the iSTFT frame buffer, the envelope and the chunk partials.  No floating-point atomics: two
 * runs give identical bytes.  Launches only; nothing waits for the device. */
int64_t maavss_wave_loss_ws_bytes(int64_t B, int64_t T, int n_fft, int hop);
int maavss_wave_loss(const float* pred, const float* tgt, int64_t B, int64_t T, int n_bins, const float* window, int n_fft, int hop,
                     int normalized, int kind, double eps, double grad_scale, float* d_pred, int64_t d_frames, int64_t d_block_stride,
                     int accumulate, double* rows, void* ws, int64_t ws_bytes, void* stream);

/* ---- EXTENSION: intelligibility scores (maavss_amd.stoi_metrics, Validator(intelligibility_sr=...)) -----------------------------
 * maavss_stoi: short-time objective intelligibility (STOI, Taal et al. 2011) and its extended form (ESTOI, Jensen & Taal 2016) of est
 * [rows][n] against ref [rows][n], f32 sampled at 10 kHz, per row.  Samples are widened to f64 on load and every operation from there on is
 * f64 in a fixed order: no floating-point atomics, two runs give identical bytes.  Added without a version bump.  Row strides in elements,
 * >= 0, rows may overlap, ignored when rows = 1; the pointers need 4-byte alignment only.  tests/stoi_twin.py is the float64 restatement.
 *   window    w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i < 256
 *   frames    a signal of L samples has nf(L) = len(range(0, L - 256, 128)) frames, frame k = samples [128 k, 128 k + 256): one frame fewer
 *             than fit when L - 256 is a multiple of 128 (the convention of the widely used Python implementation, kept)
 *   silence   E[k] = sum_i (w[i] ref[128 k + i])^2; frame k is kept iff E[k] 1e4 > max E (40 dB under the loudest frame).  The silence-free
 *             ref and est are the overlap-add at hop 128 of their kept windowed frames (one mask, the reference's): n_kept frames
 *   bands     the silence-free signals are framed again (M = n_kept - 1 frames), windowed again, zero-padded to 512 and transformed;
 *             X[j][k] (ref) and Y[j][k] (est) = sqrt of the summed powers of bins [lo[j], hi[j]), 15 third-octave bands from 150 Hz:
 *             lo = 7 9 11 14 17 22 27 34 43 55 69 87 109 138 174, hi = lo[1:], 219
 *   segments  columns [m - 30, m) for m = 30 .. M: M - 29 segments (384 ms each)
 *   STOI      per band of a segment: y' = min(alpha y, x (1 + 10^(15/20))), alpha = |x| / (|y| + eps); x and y' minus their means, each
 *             divided by (its norm + eps), dot product.  The score is the mean over the 15 bands and all segments.  eps = 2^-52
 *   ESTOI     per segment, x and y alike: each band minus its mean over time, divided by (its norm + eps); then each frame minus its mean
 *             over bands, divided by (its norm + eps); sum(xn yn) / 30.  The score is the mean over segments
 * Two deviations from that Python implementation: (1) the mask compares squared norms directly, without its eps inside a logarithm; (2) a
 * row without a segment (M < 30: too short, too much silence, an all-silent reference, max E = 0) scores NaN with n_segments = 0 where the
 * package returns 1e-5 and warns.  A non-finite sample anywhere in est or ref gives NaN, NaN, 0, 0 for that row only (an explicit flag).
 * out [rows][4] f64: stoi, estoi, n_kept, n_segments.  n < 2^31.  ws: maavss_stoi_ws_bytes(rows, n) bytes (0 for invalid arguments), 8-byte
 * aligned: the window and twiddle tables, per (row, frame) E, the flag and src[], per row the counts, X and Y [rows][2][15][nf - 1] and
 * per (row, segment) the two partial scores.  Launches: tables, energies, select, [bands, segments when nf(n) > 30], finalize; the
 * silence-free waveform is never written. */
int64_t maavss_stoi_ws_bytes(int64_t rows, int64_t n);
int maavss_stoi(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t rows, int64_t n, double* out, void* ws,
                int64_t ws_bytes, void* stream);

/* ---- EXTENSION: BSS-eval SDR, SIR and SAR against known sources (maavss_amd.bss_eval_metrics, Validator(bss_filter=...)) ----------
 * maavss_bss_eval: per row, the estimate e[0..n), the target s_0[0..n) (ref) and K >= 0 other sources s_1..s_K (others), all f32, and a
 * time-invariant distortion filter of L taps (Vincent, Gribonval & Fevotte 2006).  T = n + L - 1; every signal is zero outside [0, n).
 * Everything is f64 over the f32 data in a fixed order: no floating-point atomics, two runs give identical bytes, and a row's bytes do not
 * depend on the other rows of the call.  Added without a version bump.  tests/bss_twin.py is the float64 restatement.
 *   live      the target is live; another source is live when the f64 sum of its exact squares is not 0 (an all-zero source, an empty
 *             Mixer slot, is left out exactly).  J = the number of live sources
 *   lags      A_j[m, t] = s_j[m - t], m in [0, T), t in [0, L); A = [A_0 .. A_{J-1}] over the live sources in their order
 *   target    c_t solves (A_0^T A_0) c_t = A_0^T e; p_t = A_0 c_t
 *   full      c solves (A^T A) c = A^T e; p = A c.  With J = 1 the second solve is not run and p is p_t itself
 *   Gram      every entry of A^T A and of A^T e is an f64 sum of exact products of f32 samples, the auto- and cross-correlations at the
 *             lags -(L-1)..L-1; the matrix is block Toeplitz and is built from them.  It is factored by Cholesky (one factorisation:
 *             the leading L x L block of the factor is the factor of A_0^T A_0)
 *   sums      over m in [0, T), e zero-extended, each accumulated directly from the materialised projections, never as a difference of
 *             quadratic forms:  S_tt = sum p_t^2, S_ee = sum (e - p_t)^2, S_ii = sum (p - p_t)^2, S_aa = sum (e - p)^2, S_pp = sum p^2
 *   scores    sdr_db = 10 log10(S_tt / S_ee), sir_db = 10 log10(S_tt / S_ii), sar_db = 10 log10(S_pp / S_aa).  No epsilon: with J = 1
 *             S_ii is exactly 0, sir_db is +inf and sar_db equals sdr_db bit for bit
 *   status    0 ok; 1 a sample of e or of any source is non-finite; 2 the target is silent; 3 a Cholesky pivot is not positive or not
 *             finite.  With a status the five sums and the three scores are NaN; n_sources is 0 for 1 and 2, J for 3.  A Gram matrix that
 *             is rank-deficient without an exactly silent source (two identical sources) gives status 3 or whatever the arithmetic gives
 * Deviations from the usual Python package (bss_eval_sources), stated: the silent-source rule; NaN and a status where the package falls
 * back to a least-squares solve; no permutation search (the target is known); no framewise variant.
 * out [rows][10] f64: S_tt, S_ee, S_ii, S_aa, S_pp, sdr_db, sir_db, sar_db, n_sources, status.
 * 0 <= K <= 3, 1 <= L <= 512, n >= (K + 1) L (otherwise there are more unknowns than equations), n < 2^31, rows <= 65535.  Strides in
 * elements, >= 0, rows may overlap; the row strides are ignored when rows = 1, others_src_stride (between the sources of one row) when
 * K < 2; others may be null when K = 0; samples are contiguous and the pointers need 4-byte alignment only.
 * ws: maavss_bss_eval_ws_bytes(rows, n, K, L) bytes (0 for invalid arguments), 8-byte aligned: per row 8 ints, per (signal, chunk of 2048
 * samples) two doubles, per (ordered pair, chunk) and per ordered pair L lags, the matrix of (64 nbt + 64) x 64 nbt doubles with
 * nbt = ceil((K + 1) L / 64) (34.6 MB at 2048 unknowns), the nbt factored diagonal tiles (32 KB each), 2 x 64 nbt coefficients and
 * 5 doubles per 1024 outputs.
 * Launches: screen, plan, corr, corr_sum, gram, per tile column {panel, update}, backsolve, fir, finalize = 7 + 2 nbt. */
int64_t maavss_bss_eval_ws_bytes(int64_t rows, int64_t n, int K, int L);
int maavss_bss_eval(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, const float* others,
                    int64_t others_row_stride, int64_t others_src_stride, int K, int64_t rows, int64_t n, int L, double* out, void* ws,
                    int64_t ws_bytes, void* stream);

/* K18 helper, EXTENSION (the reference is single-device): bf16 wire format of the data-parallel gradient all-reduce -- a bucket of
 * the flat f32 gradient buffer is rounded to bf16 (round-to-nearest-even) for the collective and widened back into the f32 master
 * buffer afterwards (trainer.GradSync(wire_dtype="bf16")).  n a multiple of 8, buffers 16-byte aligned. */
int maavss_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int maavss_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);

/* ---- K1-K6 DINO ViT-S/8 and ViT-B/8 attention-frame extractor ---------------------------------------
 * What VideoAttention._inference (video_attention.py:38-103) obtains from dino's
 * VisionTransformer.get_last_selfattention (external module, call site video_attention.py:52), batched
 * over frames.  rows = frames * ntok, ntok = (H/8)*(W/8) + 1.
 * dtype    : the 16-bit storage / MFMA operand format of the activations and weights, raw uint16 bits: 0 = bf16,
 *            2 = IEEE half (same MFMA rate, 3 more mantissa bits; the LayerNorm-ed / softmax-bounded activations of the
 *            extractor fit its range).  "bf16" below stands for whichever is selected; accumulation, residual stream,
 *            LayerNorm and softmax are always f32.
 * patchify : frames [F][3][H][W] f32 -> a [rows][192] bf16 (CLS rows zero).
 * gemm     : C = epilogue(A[M][K] bf16 . W[N][K]^T bf16); N % 128 == 0, K % 64 == 0.  epilogue 0: +bias,
 *            columns < qscale_cols times qscale -> bf16;  1: +bias, exact GELU -> bf16;  2: C(f32) += acc + bias
 *            (residual, in place);  3: C(f32) = acc + table[row % period][N] (cls/pos-embed/conv-bias table).
 * layernorm: x [rows][dim] f32 -> bf16, dim 384 (ViT-S) or 768 (ViT-B) (eps as given, 1e-6 for DINO).
 * attn     : qkv [rows][ld_qkv] bf16 (q | k | v, heads x 64 each, q pre-scaled) -> out [rows][ld_out] bf16.
 * cls_attn : last block: softmax of the CLS query over all tokens, CLS column dropped -> att [F][heads][ntok-1] f32.
 * attn_maps: video_attention.py:80-96 + av_dataset.py:328: head sum, x(1/frame max), nearest x8 upsample,
 *            x(1/clip max over groups of clip_frames frames; 0 = skip) -> out [F][1][H][W] f32 (zero outside the
 *            patch grid); ws = F * ((H/8)*(W/8) + 1) floats. */
int maavss_vit_patchify(const float* frames, void* a, int64_t n_frames, int H, int W, int dtype, void* stream);
int maavss_vit_gemm(const void* A, int lda, const void* W, const float* bias, const float* table, int period, void* C,
                    int ldc, int64_t M, int N, int K, int epilogue, int qscale_cols, float qscale, int dtype, void* stream);
int maavss_vit_layernorm(const float* x, const float* gamma, const float* beta, void* y, int64_t rows, int dim,
                         float eps, int dtype, void* stream);
/* panel GEMM for the K = 384 layers with the preceding LayerNorm fused (dino Block: norm1->attn.qkv, attn.proj,
 * norm2->mlp.fc1): C = epilogue(LN(X)[M][384] . W[N][384]^T) when X (f32) is given, or A (bf16, [M][lda]) . W^T
 * otherwise; exactly one of X / A is non-null.  epilogue 0 / 1 / 2 as in maavss_vit_gemm (bf16+q-scale, bf16+GELU,
 * f32 residual in place).  N % 128 == 0, N <= 2048, ldc % 8 == 0, qscale_cols % 8 == 0.  C must be ALLOCATED with
 * c_rows >= ceil(M/128)*128 rows: the register epilogue stores whole 128-row panels unguarded (rows >= M receive
 * don't-care values) so that its counted DMA waits stay exact. */
int maavss_vit_panel_gemm(const float* X, const void* A, int lda, const float* ln_gamma, const float* ln_beta,
                          float ln_eps, const void* W, const float* bias, void* C, int ldc, int64_t c_rows, int64_t M,
                          int N, int epilogue, int qscale_cols, float qscale, int dtype, void* stream);
/* weight-stationary GEMM for the same K = 384 layers (attn.qkv, attn.proj, mlp.fc1 of dino's Block; call site
 * video_attention.py:52): C = epilogue(A[M][384] (16-bit, dense rows) . W[N][384]^T), the weights held in registers, the
 * activation rows streamed through LDS in 64-row panels.  epilogue 0 / 1 / 2 as in maavss_vit_gemm; epilogue 4 (ABI 400, dtype 2
 * only) = epilogue 1 with the GELU polynomial evaluated in packed IEEE half instead of f32 (mlp.fc1: 7 % faster, twice the
 * rounding error of the stored value -- VideoAttention(gelu="half"), never the default).  N % 384 == 0 (one
 * workgroup per 384 columns; the N / 384 workgroups of a row range share one XCD's L2), ldc % 8 == 0, qscale_cols % 384 == 0.
 * A and C must be ALLOCATED with a_rows, c_rows >= ceil(M/64)*64 rows (whole panels are read and stored; rows >= M hold
 * don't-care values).  xn_out (epilogue 2 with N = 384 only, may be null): additionally LayerNorm(ln_gamma, ln_beta, ln_eps)
 * of every updated row of C -> 16-bit [c_rows][384], so that the consumer GEMM needs no LayerNorm pass.  ln_gamma = ln_beta = NULL
 * (ABI 400; here and in maavss_vit_ws_gemm_ln / _ln_mx): the LayerNorm WITHOUT its affine part, (x - mean) * rstd -- for callers that
 * have folded gamma / beta into the consumer's frozen weights (W' = W diag(gamma), b' = b + W beta).  maavss_amd.VideoAttention does NOT fold by
 * default: measured +0.3 % clips/s for another rounding realisation of the weights (end-to-end mask-MSE 4.0e-6 ... 8.4e-6 instead of 5.4e-6 ...
 * 6.5e-6 over the three gated cases: same mean, thinner worst-case margin to 1e-5; HISTORY.md H4). */
int maavss_vit_ws_gemm(const void* A, int lda, int64_t a_rows, const void* W, const float* bias, void* C, int ldc,
                       int64_t c_rows, int64_t M, int N, int epilogue, int qscale_cols, float qscale, void* xn_out,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, int dtype, void* stream);
/* norm1 -> attn.qkv without a LayerNorm pass: X f32 [x_rows][384] is normalised on the way into LDS (epilogue 0: +bias,
 * q-scale -> 16-bit).  row_stats [M][3][2] = (mean, sum of squared deviations) of the three 128-column thirds of every row of X,
 * as left by maavss_vit_gemm_stats when it wrote X. */
int maavss_vit_ws_gemm_ln(const float* X, int64_t x_rows, const float* row_stats, const float* ln_gamma, const float* ln_beta,
                          float ln_eps, const void* W, const float* bias, void* C, int ldc, int64_t c_rows, int64_t M, int N,
                          int qscale_cols, float qscale, int dtype, void* stream);
/* The same layer with the LayerNorm applied AFTER the product (round 4): the rows of X are only rounded to the storage format on the way in,
 * W is the gamma-folded weight W diag(gamma) (storage format), col_sums[n] = sum over k of that ROUNDED W's row n (f32), bias = b + W beta, and the
 * epilogue computes  rstd_r (x W^T - mean_r col_sums[n]) + bias[n]  (then the q-scale).  Equal to maavss_vit_ws_gemm_ln in exact arithmetic;
 * in 16 bits another rounding realisation (raw rows rounded instead of normalised ones).  No per-element LayerNorm arithmetic in the loader. */
int maavss_vit_ws_gemm_ln_post(const float* X, int64_t x_rows, const float* row_stats, const float* col_sums, float ln_eps, const void* W,
                               const float* bias, void* C, int ldc, int64_t c_rows, int64_t M, int N, int qscale_cols, float qscale, int dtype,
                               void* stream);
/* maavss_vit_gemm with the f32 epilogues (2, 3) additionally writing, for every row and every 128-column tile, (mean, sum of
 * squared deviations from that mean) of the values it stored: row_stats [M][N / 128][2] (null = maavss_vit_gemm). */
int maavss_vit_gemm_stats(const void* A, int lda, const void* W, const float* bias, const float* table, int period, void* C,
                          int ldc, int64_t M, int N, int K, int epilogue, int qscale_cols, float qscale, float* row_stats,
                          int dtype, void* stream);
int maavss_vit_attn(const void* qkv, void* out, int frames, int ntok, int heads, int ld_qkv, int ld_out, int dtype,
                    void* stream);
int maavss_vit_cls_attn(const void* qkv, float* att, int frames, int ntok, int heads, int ld_qkv, int dtype, void* stream);
/* Block-scaled fp8 attention, BASELINE config "fp8 MFMA attention QK^T / AV" (round 3; replaces round 2's non-scaled fp8 kernel) --
 * same call site (video_attention.py:52) and the out tensor / layout of maavss_vit_attn: Q K^T and P V on v_mfma_scale_f32_32x32x64_f8f6f4 (OCP MX:
 * e4m3 elements, one e8m0 scale per 32-element K block; f32 accumulation -- the config's "bf16 accumulate" is f32 here, wider).
 * `ws` (maavss_vit_attn_mx_ws_bytes(rows) bytes, 256-byte aligned, rows = frames * ntok) holds the operand images laid out in
 * csrc/vit_mx.h: q8 / k8 [rows_alloc][384] with per-(token, head, 32 d) scales, V transposed [384][rows_alloc] with per-(d row,
 * 32-token block) scales.  They are written either by maavss_vit_qkv_mx from a 16-bit qkv tensor, or directly by the attn.qkv
 * GEMM (maavss_vit_ws_gemm_ln_mx: no 16-bit qkv, no quantisation pass).  `dtype` = the 16-bit format of out (and of qkv). */
int64_t maavss_vit_attn_mx_ws_bytes(int64_t rows);
int maavss_vit_qkv_mx(const void* qkv, void* ws, int64_t rows, int ld_qkv, int dtype, void* stream);
int maavss_vit_attn_mx(const void* ws, void* out, int frames, int ntok, int heads, int ld_out, int dtype, void* stream);
/* attn.qkv (N = 1152) with norm1 applied on the way in, exactly as maavss_vit_ws_gemm_ln, but the epilogue writes the images above
 * into `mx_ws` (maavss_vit_attn_mx_ws_bytes(M) bytes; bytes past the stored panels must be zero -- allocate zeroed once) instead
 * of a 16-bit qkv tensor: no quantisation pass, half the output bytes.  `dtype` = the 16-bit format of W. */
int maavss_vit_ws_gemm_ln_mx(const float* X, int64_t x_rows, const float* row_stats, const float* ln_gamma, const float* ln_beta,
                             float ln_eps, const void* W, const float* bias, void* mx_ws, int64_t M, int qscale_cols, float qscale,
                             int dtype, void* stream);
int maavss_vit_attn_maps(const float* att, float* out, float* ws, int64_t n_frames, int heads, int H, int W,
                         int clip_frames, int attn_diff /* av_dataset.py:323-326, needs clip_frames > 0 */, void* stream);
/* Same, and sets *nonfinite_flag (device int32, sticky, never cleared here; null = no check) to 1 when any CLS-attention value
 * is inf or NaN.  This is the range guard of the IEEE-half storage format (dtype 2) of the extractor: the reference computes in
 * fp32 (video_attention.py:52), where |activation| > 65504 is harmless; here such a value becomes inf in a 16-bit store,
 * poisons that frame's residual stream and arrives in this row as NaN -- one check on 6 x n values per frame covers every
 * upstream store.  The host side (maavss_amd/video_attention.py) raises and names act_dtype="bf16". */
int maavss_vit_attn_maps_checked(const float* att, float* out, float* ws, int64_t n_frames, int heads, int H, int W,
                                 int clip_frames, int attn_diff, int32_t* nonfinite_flag, void* stream);
/* Per-head thresholded attention masks, DINO's segmentation read-out (video_attention.py:59-78): for every (frame, head) row a[0..n) of
 * att [n_frames][heads][n] f32 (what maavss_vit_cls_attn wrote; values >= 0), n = (H / patch) * (W / patch) <= 4096: sort ascending by
 * value, ties by ascending patch index (torch.sort(stable=True)); v = sorted / sum(a); c = inclusive cumsum(v) in f32; a patch is
 * kept <=> its c > 1 - threshold; the kept flags are written back at each patch's own position.  The kept set is always a suffix
 * of the sorted order (everything from the first position with c > 1 - threshold on).  A row whose sum is 0 gives an all-zero mask.
 * out: values 0 / 1, out_dtype 0 = uint8, 1 = float32 (the reference's .float() at :68); upsample = 0: [n_frames][heads][H / patch]
 * [W / patch]; upsample = 1: [n_frames][heads][H][W], every patch value repeated patch x patch times (nearest, :70-75), pixels
 * outside the patch grid (H or W not a multiple of patch) written 0, as in maavss_vit_attn_maps.  threshold in [0, 1].
 * *nonfinite_flag (device int32, sticky, never cleared here; null = no check) is set to 1 when an input value is inf or NaN, as in
 * maavss_vit_attn_maps_checked; that row's output is then unspecified (the kernel still terminates and stays in bounds).
 * One launch, no atomics, deterministic; 16-byte stores when out is 16-byte aligned and the row length (W, or n without upsample)
 * is a multiple of 16 (uint8) / 4 (float32), element stores otherwise.  Additive in ABI 400. */
int maavss_vit_attn_masks(const float* att, void* out, int out_dtype, int64_t n_frames, int heads, int H, int W, int patch,
                          int upsample, float threshold, int32_t* nonfinite_flag, void* stream);

/* ---- EXTENSION (no reference counterpart): AdaptiveAvgPool2d closing the STFT encoder for frame sizes the
 * reference constructor cannot build (224^2, 384^2; SURVEY.md finding 2).  x NHWC [B][H][W][C]; out/dout
 * addressed b*os_b + (oy*Wo+ox)*os_p + c*os_c. */
int maavss_adaptive_pool_fwd(const float* x, float* out, int B, int H, int W, int C, int Ho, int Wo, int64_t os_b,
                             int64_t os_p, int64_t os_c, void* stream);
int maavss_adaptive_pool_bwd(const float* dout, float* dx, int B, int H, int W, int C, int Ho, int Wo, int64_t os_b,
                             int64_t os_p, int64_t os_c, void* stream);

/* ---- frame transform of the data path (no GPU form in the reference) ----------------------------------------------------
 * AV_Dataset's clip transform (av_dataset.py:108-112 RandomResizedCrop(framesize, scale=(0.6, 1.0)) + Normalize, applied at
 * av_dataset.py:315-319 and :346-350 after permute(0,3,1,2).float() / 255, followed by torchvision autocontrast when the
 * dataset's `autocontrast` flag is set).  src uint8 [F][H0][W0][3] (the decoder's HWC frames); boxes int32 [F / clip_frames][4]
 * = (top, left, height, width) on the DEVICE, one box shared by the clip_frames consecutive frames of a clip; host_boxes = the
 * same values in host memory, checked (inside the frame, h, w >= 1) before any launch -- the kernels clamp to the frame as well.
 * out f32 [F][3][S][S] = (interpolate(crop / 255, (S, S), bilinear, align_corners=False, antialias) - mean_c) / std_c, then with
 * autocontrast = 1 per (frame, channel) plane (x - min) / (max - min) clamped to [0, 1] (a constant plane: clamp(x, 0, 1)).
 * antialias = 1 is the separable triangle filter of torch's antialiased bilinear resize (support grows with the downscale
 * factor, per axis).  S >= 8, a multiple of 4.  ws: maavss_video_transform_ws_bytes(...) bytes (16-byte aligned), or -1 when
 * the arguments are invalid.  Additive in ABI 400. */
int64_t maavss_video_transform_ws_bytes(int64_t F, int clip_frames, int H0, int W0, int S, int antialias, int autocontrast);
int maavss_video_transform(const void* src, const int32_t* boxes, const int32_t* host_boxes, float* out, void* ws, int64_t ws_bytes,
                           int64_t F, int clip_frames, int H0, int W0, int S, float mean0, float mean1, float mean2, float std0,
                           float std1, float std2, int antialias, int autocontrast, void* stream);

/* ---- audio transform of the data path (no GPU form in the reference) ----------------------------------------------------------
 * AV_Dataset.audio_transforms (av_dataset.py:203-215): channel downmix (every channel / C, summed in channel order), with
 * normalize = 1 the clip TIMES its own max |x| (av_dataset.py:209 as written), torchaudio's sinc_interp_hann Resample(orig -> new)
 * and with contrast = 1 torchaudio.functional.contrast(x, 75) = sin(x pi/2 + 0.1 sin(4 x pi/2)).
 * src [B][C][L0] addressed b * stride_b + c * stride_c + i (elements); src_dtype 0 = f32, 1 = int16 (scaled by 2^-15).
 * orig_rate, new_rate: the two rates divided by their gcd.  orig_rate == new_rate: no resampling (taps / first_tap may be null, L <= L0),
 * samples pass through unchanged.  Otherwise the COMPRESSED polyphase table of the host (maavss_amd/audio_transform.py): taps f32
 * [S][new_rate] (tap-major), taps[k][p] = dense tap first_tap[p] + k of phase p, first_tap int32 [new_rate]; `width` as torchaudio
 * defines it (ceil(lowpass_filter_width * orig / base)).  The signal is zero-padded; output n = j * new_rate + p of a clip is
 * sum_k taps[k][p] * x[j * orig_rate - width + first_tap[p] + k], k ascending in one f32 FMA chain.  first_tap must be the first tap of
 * the window's support (floor(a + p * orig / new) + 1 for one a): the kernel stages ceil(255 orig / new) + S + 2 input samples per 256
 * outputs and clamps every read into them, so another table gives wrong samples but no access out of bounds; that span is limited to
 * 16384 samples (orig / new up to about 60) and new_rate * S to 2^22.
 * out f32, row b at out + b * ld_out, L <= ceil(new_rate * L0 / orig_rate) samples per clip (a shorter L crops).
 * ws: maavss_audio_transform_ws_bytes(...) bytes (0 without normalize: ws may then be null), -1 when the arguments are invalid.
 * At most two launches (one without normalize).  Additive in ABI 400. */
int64_t maavss_audio_transform_ws_bytes(int64_t B, int C, int64_t L0, int normalize);
int maavss_audio_transform(const void* src, int src_dtype, int64_t B, int C, int64_t L0, int64_t stride_b, int64_t stride_c,
                           const float* taps, const int32_t* first_tap, int orig_rate, int new_rate, int S, int width, int normalize,
                           int contrast, float* out, int64_t L, int64_t ld_out, void* ws, int64_t ws_bytes, void* stream);

/* ---- whole-recording inference (maavss_amd.Enhancer; train_avse_frames.py:139-176,196-200 done over every clip) --------------
 * Pass 1 of maavss_vit_attn_maps_checked alone (video_attention.py:80-95): small [n_frames][n] = head sum of att [n_frames][heads][n]
 * times 1 / its frame max, fmax [n_frames] = max of the scaled map, *nonfinite_flag as there.  The clip normalisation is left to
 * the window gather, so the ViT runs once per recording frame, not once per (overlapping) clip.  Additive in ABI 400. */
int maavss_vit_attn_maps_pass1(const float* att, float* small, float* fmax, int64_t n_frames, int heads, int n,
                               int32_t* nonfinite_flag, void* stream);
/* Per clip c of clip_frames frames from recording frame clip_start[c] (device int32 [n_clips], clamped into [0, n_frames -
 * clip_frames]): clip_rcp[c] = 1 / (clip max) of av_dataset.py:328 -- over fmax (nullable; the pass-1 frame maxima) or else over
 * the clip's maps [n_frames][frame_elems]; attn_diff = 1: over the zero-padded temporal difference, av_dataset.py:323-326. */
int maavss_av_clip_scale(const float* maps, const float* fmax, const int32_t* clip_start, int64_t n_clips, int64_t n_frames,
                         int clip_frames, int64_t frame_elems, int attn_diff, float* clip_rcp, void* stream);
/* Attention windows of train_avse_frames.py:152 (x_attn[:, :, j:j+num_frames]) for windows w0 .. w0 + n_win - 1, window
 * w = c * num_seq + j: out [n_win][win_frames][H][W] (16-byte aligned) = clip frames j .. j + win_frames - 1 of clip c, normalised
 * as attention_frames(clip, clip_frames, attn_diff) does (bit for bit: same f32 operations).  upsample = 1: maps = pass-1 maps
 * [n_frames][H/8][W/8], nearest x8 with zeros outside the patch grid (video_attention.py:80-96); 0: full-resolution maps
 * [n_frames][H][W] (16-byte aligned), e.g. the reference's attention-frame cache (av_dataset.py:251-278). */
int maavss_av_attn_windows(const float* maps, const float* clip_rcp, const int32_t* clip_start, int64_t n_clips, int64_t n_frames,
                           int clip_frames, int num_seq, int win_frames, int64_t w0, int64_t n_win, int H, int W, int upsample,
                           int attn_diff, float* out, void* stream);
/* STFT windows of train_avse_frames.py:157-163: y [n_clips][2][clip_rows][n_bins] (one maavss_stft_fwd over overlapping rows) ->
 * out [n_win][2][hops_per_frame * win_frames][n_bins], window w = c * num_seq + j = STFT frames hops_per_frame * j + [0, hops_per_frame *
 * win_frames) of clip c. */
int maavss_av_stft_windows(const float* y, int64_t n_clips, int clip_rows, int n_bins, int hops_per_frame, int num_seq, int win_frames,
                           int64_t w0, int64_t n_win, float* out, void* stream);
/* Stitch of train_avse_frames.py:172-174 over all clips: pred [n_win][2][hops_per_frame][n_bins] (the model's audio output) ->
 * out [2][hops_per_frame * n_clips * num_seq][n_bins], rows hops_per_frame * w + [0, hops_per_frame) of window w = w0 + i = pred[i]
 * times g_c = clip_absmax[c] + 1e-7 (the divisor of maavss_stft_normalise, av_dataset.py:339-340; clip_absmax null: g_c = 1). */
int maavss_av_stitch(const float* pred, const float* clip_absmax, int64_t n_clips, int num_seq, int hops_per_frame, int n_bins,
                     int64_t w0, int64_t n_win, float* out, void* stream);

/* ---- EXTENSION: device-resident clip bank (maavss_amd.ClipBank) -----------------------------------------------------------------
 * The reference trains from cached attention frames and one audio memmap of the whole dataset (av_dataset.py:251-268, 285-294:
 * attn_frames_path, use_audio_memmap).  Here both stay in HBM: per-frame maps at patch resolution, [n_frames_total][(H/8) * (W/8)]
 * as maavss_vit_attn_maps_pass1 writes them (each frame divided by its own maximum), stored as f32 (storage 0) or as 16-bit
 * integers (storage 1), and every recording's samples in one f32 buffer.  A batch is cut from them by device tables of start
 * positions.  The library does not allocate and does not synchronise; no atomics; additive symbols (nothing existing changed meaning).
 * Pack: q = rint(min(max(v, 0), 1) * 65535), the product one f32 product, rounded half to even; NaN packs to 0.  Unpack: the
 * correctly rounded f32 quotient q / 65535 (65535 gives exactly 1).  |unpack(pack(v)) - v| <= 1 / 131070 (half a step) + 2^-23 (the f32 roundings of the product and of the quotient) for v in [0, 1]. */
int maavss_bank_pack_u16(const float* maps, void* out, int64_t n, void* stream);
int maavss_bank_unpack_u16(const void* q, float* out, int64_t n, void* stream);
/* out [n_clips][clip_frames][H][W] (16-byte aligned): frame t of clip b = bank frame clip_start[b] + t (device int32 [n_clips], clamped
 * into [0, n_frames_total - clip_frames]), nearest x8 with zeros outside the patch grid, times clip_rcp[b] = 1 / (clip max) of
 * av_dataset.py:328 over the clip's (unpacked) map values; attn_diff = 1: the zero-padded temporal difference of av_dataset.py:323-326
 * and its maximum, clip frame 0 being 0 * clip_rcp[b] -- the frame in front of a clip is never read.  The f32 operations of
 * maavss_av_clip_scale + maavss_av_attn_windows (num_seq = 1, win_frames = clip_frames), so storage 0 gives attention_frames(clip,
 * clip_frames, attn_diff) bit for bit and storage 1 the same expression on the unpacked maps.  clip_rcp: n_clips floats of workspace.
 * Two launches; n_clips * clip_frames * ceil(H / 8) * (W / 4) must stay below 2^31.  16-byte stores throughout. */
int maavss_bank_attn_clips(const void* maps, int storage, const int32_t* clip_start, int64_t n_clips, int64_t n_frames_total,
                           int clip_frames, int H, int W, int attn_diff, float* clip_rcp, float* out, void* stream);
/* Row gather from the audio bank [n_samples]: out[b * ld_out + i] = bank[clip_start[b] + i], i < L; clip_start device int64 [n_clips]
 * (8-byte aligned), clamped into [0, n_samples - L]; 64-bit offsets.  16-byte stores when out is 16-byte aligned and ld_out % 4 == 0
 * (the source rows start anywhere and are read as dwords), element stores otherwise.  out must not overlap the bank. */
int maavss_bank_audio_clips(const float* bank, int64_t n_samples, const int64_t* clip_start, int64_t n_clips, int64_t L, float* out,
                            int64_t ld_out, void* stream);
/* Per-clip random resized crop and flip of the stored maps, at patch resolution (maavss_amd.ClipBank.batch(boxes=, flip=), warp_maps;
 * csrc/bank_warp.hip; tests/bank_warp_twin.py restates every operation).  A crop of the attention map is not the attention of the
 * cropped frame (the ViT would re-attend): this is a geometric augmentation of the tensor the fusion network reads.
 * Inputs.  S % 8 == 0, hp = S / 8, n = hp * hp.  Per clip b: clip_start[b] as above; boxes[b] = (top, left, height, width), device int32
 * [n_clips][4], in pixels of the S x S frame, 0 <= top, 1 <= height, top + height <= S and likewise for the columns (the layout of
 * VideoTransform.sample_boxes; the caller checks its host copy, the kernel clamps what it reads into those bounds); flips[b], device
 * uint8 [n_clips], non-zero = mirror the columns (flips null: no clip is flipped).
 * Resampling.  Output patch row i of a clip reads source patch rows a and b, all in integers:
 *     D = 16 hp,  N = 2 top hp + (2 i + 1) height - 8 hp,  y0 = floor(N / D),  r = N - y0 D  (in [0, D)),
 *     wy = (double)r / (double)D  (one f64 division),  lo = top / 8,  hi = (top + height - 1) / 8,
 *     a = clamp(y0, lo, hi),  b = clamp(y0 + 1, lo, hi)
 * -- N / D is the centre of output patch i in crop coordinates, in source-patch units: bilinear with align_corners = False, clamped to
 * the patches the box touches.  Columns likewise from left / width: c, d, wx.  With m the stored map of the clip's frame t (storage 0:
 * f32; 1: the correctly rounded f32 quotient q / 65535), converted exactly to f64:
 *     r0 = (1 - wx) * m[a][c] + wx * m[a][d],   r1 = (1 - wx) * m[b][c] + wx * m[b][d],   v = (float)((1 - wy) * r0 + wy * r1)
 * every f64 operation rounded on its own, v rounded once to f32.  A flipped clip writes v to column hp - 1 - j instead of j.
 * The whole-frame box gives wy = wx = 0 and v = m exactly, flip alone the mirrored map exactly (finite maps).
 * Frame normalisation (frame_norm != 0), the arithmetic of maavss_vit_attn_maps_pass1: mx = fmaxf over the frame's n values v from
 * -1e30f, rcp = 1.f / mx, the value stored is v * rcp in f32; frame_norm = 0 stores v.  There is no guard: a frame that is all zero
 * inside the box gives 0 * inf = NaN, as an all-zero map does in the extractor.
 * out [n_clips * clip_frames][n] f32, frame t of clip b at row b * clip_frames + t: the maps maavss_bank_attn_clips then reads with
 * storage = 0 and clip_start[b] = b * clip_frames (clip maximum, attn_diff and the x8 stores are that entry point's, unchanged).
 * One launch, one workgroup per (clip, frame); no atomics, no float sum: two runs give identical bytes, and a clip's rows do not depend
 * on the other clips of the call.  A clip reads only its own clip_frames frames.  n_clips * clip_frames must stay below 2^31.
 * Additive symbol (nothing existing changed meaning). */
int maavss_bank_warp_maps(const void* maps, int storage, const int32_t* clip_start, const int32_t* boxes, const void* flips,
                          int64_t n_clips, int64_t n_frames_total, int clip_frames, int S, int frame_norm, float* out, void* stream);

/* ---- EXTENSION: per-clip activity statistics of the clip bank (maavss_amd.ClipBank.activity, maavss_amd.ClipSampler) ------------
 * Which clips of a bank are silent, still or cut (the reference's to_do.txt: "audio thresholding", "video reject"), from one read of
 * the bank.  T = clip_frames, P = frame_elems, hop, J = hops_per_frame * T segments of hop samples that tile a clip of n = J * hop
 * samples exactly; clip b starts at bank frame v = clip_frame[b] and bank sample s = clip_sample[b] and belongs to recording
 * r = clip_rec[b].  Every sum is f64 over the exactly converted f32 data (a square of an f32 is exact in f64), in the ONE order
 * stated here; no atomics; two runs give identical bytes, and a clip's row does not depend on which other clips or recordings the
 * tables hold.  tests/select_twin.py restates all of it.  The library does not allocate and does not synchronise.  Every table exists
 * twice: on the device for the kernels, which clamp what they read from it, and in host memory (host_*), which the entry point checks
 * entry by entry before any launch.  Additive symbols (nothing existing changed meaning).
 *
 * Recording level.  rec_tab int64 [3][n_rec]: first bank sample, samples N_r, first partial slot (the running count of
 * maavss_bank_level_chunks(N_q), q < r) of each recording.  A chunk is 16384 consecutive samples from the recording's first (the last
 * one shorter).  Chunk partial: "thread" t of 256 adds the squares of the chunk's samples t, t + 256, ... in index order, a NON-FINITE
 * sample counting as 0 (so that a bad sample disturbs only the clips that hold it); the 64 sums of each of the four "waves" (threads
 * 64 w .. 64 w + 63) go through the butterfly v[l] += v[l ^ o], o = 32, 16, 8, 4, 2, 1; the four results as (w0 + w1) + (w2 + w3).
 * level[r] = the recording's partials added in index order, from 0.  partials: n_partials doubles of workspace.  Two launches.
 * At most 65535 chunks (1.07e9 samples) per recording. */
int64_t maavss_bank_level_chunks(int64_t samples);
int maavss_bank_recording_level(const float* audio, int64_t n_samples, const int64_t* rec_tab, const int64_t* host_rec_tab,
                                int64_t n_rec, double* partials, int64_t n_partials, double* level, void* stream);
/* D [n_frames - 1] f64: D[f] = (sum_e |m[f+1][e] - m[f][e]|) / P over the stored maps [n_frames][P] as the bank's batches read them
 * (storage 0: f32; 1: the correctly rounded f32 quotient q / 65535), for every pair of consecutive bank frames, once each (the pair
 * that straddles two recordings too: no clip uses it).  Difference and absolute value in f64; "lane" l of 64 adds the terms
 * e = l, l + 64, ... in index order, the 64 sums through the butterfly above, then one division.  One launch, one wave per pair. */
int maavss_bank_frame_motion(const void* maps, int storage, int64_t n_frames, int64_t frame_elems, double* D, void* stream);
/* Per clip b (one workgroup each), all outputs [n_clips]:
 *   E_j       segment j = samples s + j hop .. s + (j + 1) hop - 1: lane l adds the squares of the segment's samples l, l + 64, ... in
 *             index order (non-finite samples included: IEEE decides), the 64 sums through the butterfly above
 *   energy    E_0 + E_1 + ... + E_{J-1} added in index order, from 0
 *   rms_db    10 * log10(energy / n): -inf for silence
 *   rel_db    10 * log10((energy / n) / (level[r] / N_r)): NaN in a recording whose level is 0
 *   peak      max |x_i| in f32 over the clip's samples that are not NaN (fmaxf from 0), exact
 *   n_bad     the number of samples that are inf or NaN
 *   n_active  the number of segments with   E_j / (double)hop >= (level[r] / (double)N_r) * floor_factor   (three f64 operations and
 *             one comparison, as written; a NaN on either side is not active; in a recording whose level is 0 every segment is),
 *             floor_factor = 10^(-range_db / 10) formed by the caller, in [0, 1]
 *   motion_mean  (D[v] + D[v+1] + ... + D[v+T-2]) / (T - 1), added in index order from 0;  motion_peak  the largest of those D, from 0,
 *             by `d > m` (a NaN is passed over); both 0 when T = 1 (D may then be null).  Only pairs inside the clip's frames are read.
 * level, D: what the two entry points above wrote.  J is limited to maavss_bank_max_segments() = 2048 (the E_j stay in LDS): a larger
 * J, a clip outside the bank or a recording number outside [0, n_rec) in the host tables is refused before any launch.  One launch. */
int maavss_bank_max_segments(void);
int maavss_bank_clip_activity(const float* audio, int64_t n_samples, const double* D, int64_t n_frames, const double* level,
                              const int64_t* rec_tab, int64_t n_rec, const int64_t* clip_sample, const int32_t* clip_frame,
                              const int32_t* clip_rec, const int64_t* host_clip_sample, const int32_t* host_clip_frame,
                              const int32_t* host_clip_rec, int64_t n_clips, int clip_frames, int hops_per_frame, int hop,
                              double floor_factor, double* energy, double* rms_db, double* rel_db, double* motion_mean,
                              double* motion_peak, float* peak, int32_t* n_bad, int32_t* n_active, void* stream);
/* reasons uint8 [n_clips]: bit 0 too quiet (rms_db < min_rms_db), 1 too quiet for its recording (rel_db < min_rel_db), 2 too few active
 * segments ((double)n_active < min_active; the caller passes min_active_fraction * J), 3 static (motion_mean < min_motion), 4 scene cut
 * (motion_peak > max_motion_peak), 5 clipped (peak >= max_peak, in f32), 6 non-finite (n_bad > 0); and-ed with `enabled` (bit k: reason
 * k is tested; the threshold of a reason that is not is ignored).  A comparison with a NaN statistic is false.  One launch. */
int maavss_bank_clip_select(const double* rms_db, const double* rel_db, const int32_t* n_active, const double* motion_mean,
                            const double* motion_peak, const float* peak, const int32_t* n_bad, int64_t n_clips, int enabled,
                            double min_rms_db, double min_rel_db, double min_active, double min_motion, double max_motion_peak,
                            float max_peak, void* reasons, void* stream);

/* ---- the training callback's images (maavss_amd.figures; train_avse_frames.py:191-215) ----------------------------------------------
 * RGBA bytes made on the device, defined pixel for pixel by matplotlib's colour mapping; tests/figures_twin.py restates every definition
 * below in float64.  No entry point allocates, synchronises or uses an atomic; two runs give the same bytes.  Additive symbols (nothing
 * existing changed meaning).
 *
 * What imshow does to an array (utilities.py:336-350 plt.imshow(y_stft_ex[0].T), :316 imshow(y_img, vmin=-1, vmax=1), and the image
 * Axes.specgram makes, :398, :409): cm.viridis(Normalize(vmin, vmax)(np.ma.masked_invalid(x.astype(float64))), bytes=True).
 * x: n_img images of H x W, dtype 0 = float32, 1 = float64, element (n, r, c) at x[n * sn + r * sh + c * sw] (element strides >= 0: a
 * view needs no copy).  maavss_viridis_range: range[2 n], range[2 n + 1] = minimum and maximum over the finite elements of image n
 * (+inf, -inf when it has none), f64.  maavss_viridis_image: per element u = (double(x) - vmin) / (vmax - vmin) in f64 (u = 0 when
 * vmax == vmin), pixel = LUT[clamp(trunc(256 u), 0, 255)] with alpha 255, LUT = matplotlib's viridis as bytes (csrc/viridis_lut.h); a
 * non-finite element gives (0, 0, 0, 0).  vmin / vmax of image n are range[2 n], range[2 n + 1] (device memory, e.g. what
 * maavss_viridis_range wrote) unless bit 0 / bit 1 of `fixed` takes them from the arguments (fixed = 3: range may be null).
 * transpose = 1: the image is x's transpose (W rows of H); flip_rows = 1: its rows from the last to the first; then every pixel is
 * repeated sy x sx times (nearest, integers in 1 .. 64).  out uint8 [n_img][Hi sy][Wi sx][4], 4-byte aligned; four pixels per
 * 16-byte store when it is 16-byte aligned (pixel by pixel otherwise, and for the last pixels of an output whose count is no multiple
 * of four).  One launch each. */
int maavss_viridis_range(const void* x, int dtype, int64_t n_img, int64_t H, int64_t W, int64_t sn, int64_t sh, int64_t sw,
                         double* range, void* stream);
int maavss_viridis_image(const void* x, int dtype, int64_t n_img, int64_t H, int64_t W, int64_t sn, int64_t sh, int64_t sw,
                         const double* range, int fixed, double vmin, double vmax, int transpose, int flip_rows, int sy, int sx,
                         void* out, void* stream);
/* The two arrays utilities.plot_waveform_specgram (utilities.py:386-416) hands to imshow through Axes.specgram(x, mode='magnitude') and
 * (mode='phase') with matplotlib's defaults, in f64 throughout.  wave: rows x L f32, row r at wave + r * stride (stride >= 0, rows may
 * overlap; 4-byte aligned).  nfft a power of two in 32 .. 1024, 0 <= noverlap < nfft.  A row shorter than nfft is zero-padded to it;
 * n = (max(L, nfft) - noverlap) / (nfft - noverlap) segments (maavss_specgram_segments; 0 for arguments maavss_specgram refuses),
 * segment i from sample i (nfft - noverlap), times np.hanning(nfft) (the symmetric window), no detrending, one-sided transform F.
 * mag_db = 20 log10(|F| / sum(w)); phase = np.unwrap(angle(F)) along frequency: dd = diff(p), m = mod(dd + pi, 2 pi) - pi with m = pi
 * where m == -pi and dd > 0, the correction m - dd zeroed where |dd| < pi, its cumulative sum (in bin order) added.  Both
 * [rows][nfft / 2 + 1][n] f64 with row 0 the Nyquist bin (specgram flips before imshow).  A silent segment gives -inf dB and phase 0;
 * a non-finite sample makes its segments NaN; samples equal to -0.0 are outside the contract (angle(-0) = pi).  One launch, one
 * workgroup per (row, segment). */
int64_t maavss_specgram_segments(int64_t rows, int64_t L, int nfft, int noverlap);
int maavss_specgram(const float* wave, int64_t stride, int64_t rows, int64_t L, int nfft, int noverlap, double* mag_db, double* phase,
                    void* stream);
/* utilities.video_frames_image with generate_filmstrip(..., resize=False) (utilities.py:286-326, 230-245) as one image.  y_attn, yh_attn
 * [T][H][W] f32, video [3][T][H][W] f32 or null, all contiguous.  Per tensor, in f32 as the reference forms it: s = 1 / (max + 1e-7),
 * v s, clipped to [0, 1]; the inputs are NOT modified (the reference scales its arguments in place).  max is the tensor's maximum
 * with NaNs ignored (torch.max would return the NaN); a NaN element gives the pixel (0, 0, 0, 0).  Attention pixels: the colour map
 * with vmin = -1, vmax = 1 (the reference's imshow arguments), so the maps use its upper half; video pixels: (trunc(255 r),
 * trunc(255 g), trunc(255 b), 255), what imshow does with float RGB.  out uint8 [R H][T W][4], 4-byte aligned (16-byte stores when 16-byte aligned): frame t at columns
 * t W .. t W + W - 1 (frames may be rectangular; the reference's indexing is right for square ones only), strips from the top: video,
 * y, yh (R = 3), or y, yh (R = 2, video null).  maxes: 192 floats of workspace (64 partial maxima per tensor).  Two launches. */
int maavss_filmstrip(const float* y_attn, const float* yh_attn, const float* video, int T, int H, int W, float* maxes, void* out,
                     void* stream);

/* ---- EXTENSION: reverberation (maavss_amd.Reverb) ---------------------------------------------------------------------------------
 * The reference's only corruption is white noise on the STFT coefficients (av_dataset.py:217-220) and the mixer adds dry clips; this
 * changes the acoustics of a source: a synthetic room response, and its convolution with audio whose past is read from where it lies
 * (a clip bank's recording), not assumed silent.  tests/reverb_twin.py restates both definitions in float64.  No entry point allocates,
 * synchronises or uses an atomic; two runs give identical bytes.  Additive symbols (nothing existing changed meaning).
 *
 * Room response of K taps (1 <= K <= maavss_rir_max_taps() = 32768), row r of params f64 [n_rirs][3] = (lam, D, k0):
 * lam = ln(1000) / (rt60 * sr) (60 dB of amplitude decay per rt60), D = 10^(drr_db / 10), both formed by the caller in f64; k0 the
 * predelay in samples, read as 1 below 1 (or NaN) and as K above K.
 *   h[0] = 1 (the direct path at lag 0: wet = dry + tail, aligned with the dry signal);  h[k] = 0.0 for 1 <= k < k0;
 *   h[k] = f32(s * t_k) for k0 <= k < K,  t_k = (double)g[k] * exp((-lam) * (double)k),  s = sqrt(1.0 / (D * E)),  E = sum t_k^2,
 * every operation in f64 and rounded on its own (t_k^2 is rounded before it is added), each tap rounded once to f32, so that
 * 10 log10(1 / sum_{k >= k0} (s t_k)^2) = drr_db over the truncated tail as stored.  E in ONE order: "thread" t of 256 takes the quads
 * (taps 4 q .. 4 q + 3) q = t, t + 256, ... in index order and adds each quad's squares in tap order, from +0.0 (a tap in front of k0
 * adds nothing); the 64 sums of each of the four "waves" (threads 64 w .. 64 w + 63) go through the butterfly v[l] += v[l ^ o],
 * o = 32, 16, 8, 4, 2, 1; the four results as (w0 + w1) + (w2 + w3).  When E > 0 is false (k0 >= K, silent noise, a NaN) or s = 0,
 * every tap behind h[0] is +0.0: h = [1, 0, ...].  exp is the device library's (a few ulp): tests/reverb_twin.py derives what that
 * allows a tap to differ from the twin's.
 * g: noise[r * ld_noise + k] (f32) when noise is given; otherwise the four taps of quad q of row r are the four deviates of
 * philox_normal4(seed, idx) in order, idx = 0x52455642 << 32 | (row0 + r) << 13 | q (row0 + n_rirs <= 2^19): a row's bytes depend on
 * (seed, row0 + r, its parameters, K) only, not on n_rirs or on the launch.  rirs [n_rirs][ld_rir], ld_rir >= K; the padding is not
 * written.  rirs must not overlap noise.  One launch, one workgroup per row. */
int maavss_rir_max_taps(void);
int maavss_rir_synth(const double* params, const float* noise, int64_t ld_noise, uint64_t seed, int64_t row0, int64_t n_rirs, int K,
                     float* rirs, int64_t ld_rir, void* stream);
/* out[b * ld_out + n] = f32( sum over k = 0 .. K - 1 with p >= floor[b] of (double)h[k] * (double)src[p] ),  p = start[b] + n - k,
 * 0 <= n < L, h = rirs + rir_index[b] * ld_rir.  src: one flat f32 buffer of n_src samples; rows start[b] .. start[b] + L - 1 may begin
 * at any sample and may overlap; the samples floor[b] .. start[b] - 1 are row b's history (floor = start: from zero state).  A term with
 * p < floor[b] is left out of the sum, not added as a zero, and no tap is skipped for being zero: IEEE decides what an inf or NaN
 * sample does, and it reaches the K outputs from its own position on and no others.
 * Every product of two f32 values is exact in f64, so only the order of the additions matters, and it is ONE order: per output, S = 4
 * partial sums, each from +0.0; tap k goes to partial k mod 4, taps ascending; out = f32((a0 + a1) + (a2 + a3)).  The tiling does not
 * enter: a row in a batch has the bytes of a call of its own.
 * start, floor: device int64 [B] (8-byte aligned), rir_index: device int32 [B]; the kernel clamps what it reads from them (start into
 * [0, n_src - L], floor into [0, start], the index into [0, n_rirs)).  host_*: the same tables in host memory, checked entry by entry
 * before the launch: start[b] + L > n_src, floor[b] > start[b], a negative entry or an index outside [0, n_rirs) is refused.
 * 64-bit offsets; 1 <= K <= 32768, L >= 1, ld_out >= L, ld_rir >= K.  out must overlap neither src nor rirs.  One launch: a workgroup
 * per 1024 consecutive outputs of a row, the taps staged through LDS 1024 at a time. */
int maavss_reverb(const float* src, int64_t n_src, const int64_t* start, const int64_t* floor, const int64_t* host_start,
                  const int64_t* host_floor, int64_t B, int64_t L, const float* rirs, int64_t n_rirs, int64_t ld_rir, int K,
                  const int32_t* rir_index, const int32_t* host_rir_index, float* out, int64_t ld_out, void* stream);

/* ---- EXTENSION: image-source room responses (maavss_amd.Reverb.make_room_rirs) ----------------------------------------------------
 * A second way to fill the table maavss_reverb convolves with: the image-source model of a shoebox room (Allen & Berkley 1979), one
 * microphone, one source per row; rows that share dimensions, microphone and walls are sources of one room.  tests/room_twin.py
 * restates the definition in float64 and the kernel gives its bytes.  Additive symbol (nothing existing changed meaning).
 *
 * Row r of geom f64 [n_rows][15] = (L[3], m[3], s[3], beta[6]): room dimensions in metres, microphone, source (both strictly inside
 * the room and not on each other), pressure reflection coefficients of the walls x0 x1 y0 y1 z0 z1 in [0, 1].  Row r of bounds int32
 * [n_rows][3] = (Nx, Ny, Nz).  Per axis a, lattice index n in [-N_a, N_a] and parity p in {0, 1}:
 *   u_a = ((2 n) L_a + (1 - 2 p) s_a) - m_a,  reflected |n - p| times off wall a0 and |n| times off wall a1;
 *   d = sqrt((ux ux + uy uy) + uz uz);  d0 the same for n = 0, p = 0 on all axes (the direct path);
 *   A = (((((x0^e1 * x1^e2) * y0^e3) * y1^e4) * z0^e5) * z1^e6) * d0) / d,  integer powers by
 *       r = 1; while (e) { if (e & 1) r = r * b; b = b * b; e >>= 1; }   (0^0 = 1: a wall of beta = 0 is anechoic, the direct path stays);
 *   tau = (d - d0) * (sr / c),  k0 = floor(tau),  f = tau - k0:  a response is normalised to its own direct path and starts at it,
 *       so the direct path adds exactly 1 to h[0] (wet = dry + reflections, aligned with the dry signal as maavss_rir_synth's is);
 *   for m = -H + 1 .. H, tap k = k0 + m with 0 <= k < K (others are dropped, not folded) receives A * w,
 *       pos = ((m - f) + H) * R,  i = min(floor(pos), 2 H R - 1),  t = pos - i,  w = T[i] + t * (T[i + 1] - T[i]);
 *   T = table, f64 [2 H R + 1], the caller's: a windowed sinc sampled at x = i / R - H with exact zeros at the integers and an exact 1
 *       at x = 0 keeps an image that falls on a sample a clean impulse (T[2 H R] = 0 makes w = 0 exactly at pos = 2 H R).  No device
 *       sin or cos enters.
 *   Fixed point: q = llrint((A * w) * 2^40) (ties to even) as int64; a tap is the integer sum of its q; h[k] = f32((double)sum * 2^-40).
 * Every f64 operation is rounded on its own in the order written (the file is compiled without contraction; sqrt and / are the
 * correctly rounded ones).  Integer addition is associative: the order of the images, the tiling and the launch cannot change a bit, no
 * float atomic is involved, and a row in a table has the bytes of a table of its own.  |A w| <= 1 and a row has at most 2^31 images
 * (8 (2 Nx + 1)(2 Ny + 1)(2 Nz + 1), refused above that), so the sum stays below 2^62.
 * Which images are evaluated: those of the lattice box.  With 2 N_a L_a >= d0 + (K + H) c / sr on every axis no image outside the box
 * reaches a tap below K, and any larger box gives the same bytes; a smaller one truncates the response.
 * geom, bounds, table: device memory (8-, 4-, 8-byte aligned); host_geom, host_bounds: the same tables in host memory, checked row by
 * row before the launch (a NaN fails every check).  1 <= K <= 32768, 1 <= H <= 32, 1 <= R <= 256, n_rows <= 2^19, ld_rir >= K; the
 * padding of rirs is not written.  No allocation, no synchronisation, no workspace.  One launch: a workgroup per (row, 1024 taps)
 * accumulates its taps as int64 in LDS from the shell of images that can reach them and writes them once. */
int maavss_room_rir(const double* geom, const int32_t* bounds, const double* host_geom, const int32_t* host_bounds, int64_t n_rows,
                    const double* table, int H, int R, double sr, double c, int K, float* rirs, int64_t ld_rir, void* stream);

/* ---- EXTENSION: room-acoustic figures of a response table (maavss_amd.Reverb.measure) ---------------------------------------------
 * What a stored response IS, whichever way the table was filled: row r of out f64 [n_rows][6] = (energy, edt, t20, t30, c50_db,
 * drr_db) of h = rirs + r * ld_rir (f32, K taps).  tests/rir_measure_twin.py restates the definition in float64.  Additive symbol
 * (nothing existing changed meaning).
 *
 * Backward energy (the Schroeder integral): E[k] = sum_{j >= k} (double)h[j] * (double)h[j]; every product is exact in f64, so only the
 * order of the additions matters, and it is ONE order.  The taps form blocks of 32 (block b = taps 32 b .. 32 b + 31, the last one
 * cut at K):
 *   s[k] = s[k + 1] + h[k]^2 inside a block, from its last tap towards its first, from +0.0;   T[b] = s[32 b];
 *   C[B - 1] = +0.0,  C[b] = C[b + 1] + T[b + 1], from the last block towards the first;        E[k] = s[k] + C[k / 32].
 * energy = E[0].  No atomic; two runs give identical bytes, and a row in a table has the bytes of a table of its own.
 * Crossing of level l in (-5, -10, -25, -35) dB with threshold c_l = thresholds[l] (host memory, n_thresholds = 4; the caller forms
 * 10^(l / 10) in f64, so no device pow enters a decision; they must descend inside (0, 1)): the first j >= 1 with
 * E[j] <= E[0] * c_l, a plain f64 comparison.  Its time in samples:
 *   t_l = (double)(j - 1) + (d[j - 1] - l) / (d[j - 1] - d[j]),   d[i] = 10.0 * log10(E[i] / E[0])
 * (IEEE decides what E[j] = 0 gives: d[j] = -inf, t_l = j - 1); NaN when no tap crosses.
 *   edt = (6.0 * t_-10) / sr,   t20 = (3.0 * (t_-25 - t_-5)) / sr,   t30 = (2.0 * (t_-35 - t_-5)) / sr      seconds.
 * Early and late energy at a boundary tap kb: late = E[kb], +0.0 when kb >= K; early = the sum over k < kb in a forward order of its
 * own (NOT E[0] - E[kb], which rounds where the direct path alone is exact): per block f[b] = the squares of its taps below kb, first
 * tap towards last, from +0.0; early = ((f[0] + f[1]) + f[2]) + ..., from +0.0, over the blocks that hold a tap below kb.
 *   c50_db = 10.0 * log10(early / late) at kb = k_early (the caller's round(0.050 sr)),   drr_db the same at kb = k_direct.
 * An all-zero row gives energy 0 and NaN elsewhere; a non-finite tap makes its own row's figures what IEEE gives and touches no other
 * row.  log10 is the device library's (1 ulp): tests/rir_measure_twin.py derives what that allows a figure to differ from the twin's.
 * 1 <= K <= 32768, 1 <= n_rows <= 2^19, ld_rir >= K, k_direct, k_early >= 0; rirs 4-byte aligned, out 8-byte, contiguous.  No
 * allocation, no workspace, no synchronisation.  One launch on `stream`: a workgroup per row, the row staged through LDS 8192 taps at
 * a time (twice: totals, then crossings). */
int maavss_rir_measure(const float* rirs, int64_t n_rows, int K, int64_t ld_rir, double sr, int k_direct, int k_early,
                       const double* thresholds, int n_thresholds, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

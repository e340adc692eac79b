/*
 * bigcodec.h — C ABI of libbigcodec_hip.so, the MI355X (gfx950) BigCodec tokenization hot path.
 *
 * The reference (hoyso48/AudioTokenization, BigCodec_SSL/) is pure PyTorch and has no FFI: its
 * boundary is the nn.Module call surface of vq/codec_encoder.py, vq/codec_decoder.py and the
 * modules they compose.  Each entry point below replaces one aten call chain behind one of those
 * modules (cited per function).  The Python package audiotokenization_amd binds them with ctypes
 * (INTEGRATION.md shows the binding) and mirrors the reference modules on top.
 *
 * Conventions
 *   - every pointer argument named x/y/z/... is DEVICE memory (fp32 unless stated) and contiguous in
 *     the stated layout; pointers named *_host are host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all launches are
 *     stream-ordered and asynchronous; no function allocates, frees or synchronises;
 *   - return value: 0 = ok, 1 = bad argument, 2 = HIP launch error, 3 = unsupported shape.
 *   - activations are [B][C][T] (batch, channel, time) as in the reference's Conv1d tensors.
 */
#ifndef BIGCODEC_H
#define BIGCODEC_H

#ifdef __cplusplus
extern "C" {
#endif

#define BC_ABI_VERSION 18

int bc_abi_version(void);
/* bc_build_digest: sha256 (64 hex characters) of the sources, headers and compiler flags this library was built
 * from (ABI 16).  build_lib.py compiles it in and rebuilds when it differs from the tree's; bench.py reports a
 * committed PMC profile's traffic only when the profile was taken on a library with the running one's digest. */
const char* bc_build_digest(void);

/* ---- Conv1d (weight-normed, fused residual / tanh / next-Snake epilogue) --------------------------
 * Replaces: F.pad + conv1d of CausalConv1d.forward (vq/module.py:45-48) and weight_norm(nn.Conv1d)
 * (vq/module.py:59-65), followed by ResidualUnit's `x + ...` (vq/module.py:88-89) when
 * residual != NULL, by nn.Tanh (vq/codec_decoder.py:80) when epilogue == 1, and by the SnakeBeta of
 * the NEXT Activation1d (vq/activations.py:107-118) when out_snake_alpha_exp != NULL:
 *   v[b,co,n] = residual[b,co,n] + bias[co] + sum_{ci,k} W[co,ci,k] * x[b,ci, n*stride + k*dilation - pad_left]
 *   y = snake_co(v) (y2 == NULL)   or   y = v, y2 = snake_co(v) (dual output)   or   y = v / tanh(v)
 * Out-of-range input samples read as 0 (zero padding).  Non-causal: pad_left = padding; causal:
 * pad_left = (K - stride) * dilation (vq/module.py:43).  The input x is the already-activated
 * tensor (the Snake that precedes every reference conv runs in the producer's epilogue or in
 * bc_snake_fwd).  W is the FOLDED weight g*v/||v|| [Cout][Cin][K] packed by bc_conv1d_pack for
 * cfg = bc_conv1d_select_cfg(Cout, Cin, K, stride, dilation, mode) (any other valid tile id also
 * runs — tuning — with weights packed for that same cfg; a tile the shape does not fit returns 3).
 * mode 0: fp32 MFMA (v_mfma_f32_16x16x4_f32).  mode 1 (the package default): fp32-accurate "x6" MFMA — both operands
 * split exactly into three bf16 terms, six bf16 products per pair accumulated in fp32 — for the
 * shapes where it applies (Cin >= 16), else the fp32 kernel.  Its error against fp64 is at or below
 * the fp32 kernel's.  mode 2: plain bf16 products with fp32 accumulation (one MFMA
 * per pair; BASELINE config 5's "bf16 encoder conv stack"; activations stay fp32 in memory) where
 * Cin >= 16, else fp32.  bc_reslstm_fwd runs mode 2 as mode 3 (the recurrence stays fp32-class; its
 * input projection is packed with cfg = bc_conv1d_select_cfg(..., 3)).
 * mode 3 ("h3", opt-in; 22-bit operands, narrower than the reference's fp32): block-scaled 2 x fp16 split — each operand block is
 * scaled by a power of two from its maximum (weights per output row, packed by bc_conv1d_pack;
 * activations per staged 32-channel chunk) and split v*S = hi + lo (two fp16 terms, 22 significant
 * bits); a*b accumulates hi*hi + hi*lo + lo*hi in fp32 on v_mfma_f32_16x16x32_f16 (the dropped lo*lo
 * term is below 2^-22 |ab|), 3 MFMAs per pair, where Cin >= 16, else fp32.  Error against fp64 at or
 * below the native fp32 kernel's.
 * out_snake_alpha_exp[c] = exp(alpha[c]); out_snake_inv_beta[c] = 1/(exp(beta[c]) + 1e-9).
 * Limits: Cin*Tin*4 < 2^31 bytes per clip. */
int bc_conv1d_select_cfg(int Cout, int Cin, int K, int stride, int dilation, int mode);
/* bc_conv1d_select_cfg_n: the same choice for a launch of B clips with Tout output columns each: a stride-1
 *   multi-tap conv with Tout <= 128 (a streaming chunk, a small batch) may take a narrower tile than the shape
 *   table's (ABI 15; x6 / bf16 results are the same on either tile, h3 agrees to fp32 rounding).  The packed
 *   weights must be packed for the returned cfg. */
int bc_conv1d_select_cfg_n(int Cout, int Cin, int K, int stride, int dilation, int mode, int B, int Tout);
long long bc_conv1d_packed_floats(int Cout, int Cin, int K, int cfg);
int bc_conv1d_pack(const float* w_host, float* packed_host, int Cout, int Cin, int K, int cfg);
int bc_conv1d_fwd(const float* x, const float* w_packed, const float* bias, const float* residual,
                  const float* out_snake_alpha_exp, const float* out_snake_inv_beta,
                  float* y, float* y2, int B, int Cin, int Tin, int Cout, int Tout,
                  int K, int stride, int dilation, int pad_left, int epilogue, int cfg,
                  void* stream);

/* ---- ResidualUnit in one launch (modes 1 "x6", 2 bf16 and 3 "h3"; C in {16, 32, 48, 64, 96}) -------
 * Replaces ResidualUnit.forward (vq/module.py:88-89) after its first Activation1d:
 *   v = x_raw + conv1(snake_mid(conv7_d(x_act)))      (x_act = snake1(x_raw), from the producer)
 *   y = v, or snake_out(v), or y = v and y2 = snake_out(v)  (epilogue as bc_conv1d_fwd)
 * x_raw, x_act, y, y2: [B][C][T]; the k=7 conv keeps length T (pad_left = 3*dilation non-causal,
 * 6*dilation causal; the rest on the right).  w7_packed / w1_packed = bc_conv1d_pack(folded weight,
 * K = 7 / 1, cfg) with cfg = bc_resunit_select_cfg(C, dilation, mode); that returns -1 where the
 * unit does not fit one workgroup, or mode is 0 (then run the two bc_conv1d_fwd calls).  Another
 * candidate tile of the same mode whose rows cover C is accepted too (same results, A/B timing); any
 * other cfg returns BC_ERR_ARG.  The
 * activated k=7 output stays in LDS (never written to memory).  mid_snake_*: the unit's second
 * Activation1d. */
int bc_resunit_select_cfg(int C, int dilation, int mode);
int bc_resunit_fwd(const float* x_raw, const float* x_act, const float* w7_packed, const float* b7,
                   const float* mid_snake_alpha_exp, const float* mid_snake_inv_beta,
                   const float* w1_packed, const float* b1, const float* out_snake_alpha_exp,
                   const float* out_snake_inv_beta, float* y, float* y2, int B, int C, int T,
                   int dilation, int pad_left, int cfg, void* stream);
/* bc_resunit_fwd_snake_in: the same unit with its FIRST Activation1d applied while the k=7 input is
 *   staged (x_act = snake_in(x_raw) is never materialised: the producer writes only x_raw). */
int bc_resunit_fwd_snake_in(const float* x_raw, const float* in_snake_alpha_exp, const float* in_snake_inv_beta,
                            const float* w7_packed, const float* b7, const float* mid_snake_alpha_exp,
                            const float* mid_snake_inv_beta, const float* w1_packed, const float* b1,
                            const float* out_snake_alpha_exp, const float* out_snake_inv_beta, float* y, float* y2,
                            int B, int C, int T, int dilation, int pad_left, int cfg, void* stream);

/* ---- ConvTranspose1d (weight-normed, fused next-Snake epilogue) -------------------------------
 * Replaces: weight_norm(nn.ConvTranspose1d) (vq/module.py:67-72) and CausalConvTranspose1d
 * (vq/module.py:50-57, crop of the last `stride` samples) inside DecoderBlock (vq/module.py:
 * 115-141) (DecoderBlock uses K = 2*stride).  Run as `stride` polyphase convolutions with
 * Kp = bc_convT1d_phase_taps(K, stride) = ceil(K/stride) taps: phase r has
 * W_r[co][ci][j'] = W[ci][co][r + stride*(Kp-1-j')] (0 where that tap index >= K), packed with
 * bc_conv1d_pack(..., K=Kp, cfg), cfg = bc_conv1d_select_cfg(Cout, Cin, Kp, 1, 1, mode).  w_phases is
 * a HOST array of `stride` device pointers.  Output length Tout = (Tin-1)*stride - 2*padding + K +
 * output_padding (the caller passes Tout, which carries output_padding); DecoderBlock non-causal:
 * padding = stride/2 + stride%2, output_padding = stride%2.  Causal (crop of the last `stride`
 * samples): padding = 0, Tout = (Tin-1)*stride + K - stride.  Epilogue as bc_conv1d_fwd.
 * padding > stride * (Kp - 1) (e.g. K = stride = 4, padding = 1) returns BC_ERR_UNSUPPORTED from both
 * entry points, with nothing written. */
int bc_convT1d_phase_taps(int K, int stride);
int bc_convT1d_fwd(const float* x, const float* const* w_phases, const float* bias,
                   const float* out_snake_alpha_exp, const float* out_snake_inv_beta, float* y,
                   float* y2, int B, int Cin, int Tin, int Cout, int Tout, int K, int stride,
                   int padding, int cfg, void* stream);
/* bc_convT1d_fwd_ws (ABI 11): the same transposed convolution and the same values bit for bit, with a
 * workspace of bc_convT1d_workspace_floats(B, Cout, Tout, K, stride, padding, dual) device floats
 * (dual = y2 != NULL): each phase writes its outputs contiguously (16-byte stores) into the workspace
 * and one interleave pass writes y (and y2) in order.  bc_convT1d_fwd writes every phase straight into
 * y with stride-`stride` scalar stores (each output line written in `stride` partial passes); the
 * decoder's stride-5 upsampler ran 2x slower that way.  workspace NULL: as
 * bc_convT1d_fwd. */
long long bc_convT1d_workspace_floats(int B, int Cout, int Tout, int K, int stride, int padding, int dual);
int bc_convT1d_fwd_ws(const float* x, const float* const* w_phases, const float* bias,
                      const float* out_snake_alpha_exp, const float* out_snake_inv_beta, float* y,
                      float* y2, int B, int Cin, int Tin, int Cout, int Tout, int K, int stride,
                      int padding, int cfg, float* workspace, void* stream);

/* ---- SnakeBeta / anti-aliased Activation1d -------------------------------------------------------
 * bc_snake_fwd replaces SnakeBeta.forward (vq/activations.py:107-118).
 * bc_aa_snake_fwd replaces Activation1d.forward with antialias=True (vq/alias_free_torch/act.py:
 * 25-32): UpSample1d (resample.py:25-33) -> SnakeBeta -> DownSample1d (resample.py:47-49,
 * filter.py:86-95).  up_filter / down_filter: the 12-tap buffers `upsample.filter` and
 * `downsample.lowpass.filter` (device, 12 floats each). */
int bc_snake_fwd(const float* x, const float* snake_alpha_exp, const float* snake_inv_beta,
                 float* y, int B, int C, long long T, void* stream);
int bc_aa_snake_fwd(const float* x, const float* snake_alpha_exp, const float* snake_inv_beta,
                    const float* up_filter, const float* down_filter, float* y,
                    int B, int C, int T, void* stream);
/* bc_aa_snake_fwd_ex: the same for Activation1d(up_ratio, down_ratio, up_kernel_size, down_kernel_size)
 * (act.py:8-23; resample.py:10-33 geometry for any ratio): up_filter has up_taps floats, down_filter
 * down_taps; ratios 1..16, taps up to 256 (up_taps >= up_ratio), else 3.  y: [B][C][Tout] with
 * Tout = bc_aa_snake_out_len(T, up_ratio, down_ratio, down_taps) (= T when the ratios are equal and
 * down_taps is even).  (2, 12, 2, 12) runs bc_aa_snake_fwd's kernel. */
long long bc_aa_snake_out_len(int T, int up_ratio, int down_ratio, int down_taps);
int bc_aa_snake_fwd_ex(const float* x, const float* snake_alpha_exp, const float* snake_inv_beta,
                       const float* up_filter, const float* down_filter, float* y, int B, int C, int T, int up_ratio,
                       int up_taps, int down_ratio, int down_taps, void* stream);

/* Diagnostics (bench.py's roofline attribution, no compute): the kernel symbol a bc_conv1d_fwd launch with
 * this cfg (K = the conv's kernel size, before any phase decomposition) or a bc_resunit_fwd launch runs, as
 * rocprofv3 prints it without "void bc::" and the argument list; decided by the launchers' own code.
 * Returns the name's length (written NUL-terminated, truncated to buflen), or -1 for an invalid cfg. */
int bc_conv1d_kernel_name(int cfg, int K, int stride, int dilation, char* buf, int buflen);
int bc_resunit_kernel_name(int cfg, int C, int dilation, char* buf, int buflen);

/* bc_tanh_fwd: nn.Tanh (vq/codec_decoder.py:80) called on its own (decoder.model used as the
 * reference's nn.Sequential); the fused decoder runs it in the last conv's epilogue (epilogue = 1). */
int bc_tanh_fwd(const float* x, float* y, long long n, void* stream);

/* ---- ResLSTM ----------------------------------------------------------------------------------------
 * Replaces ResLSTM.forward (vq/module.py:156-167): rearrange b f t -> b t f, nn.LSTM(H, H,
 * num_layers, batch_first=True) (unidirectional), + skip, rearrange back.  x, out: [B][H][T].
 * Per layer l: w_ih_packed[l] = bc_conv1d_pack(weight_ih_l{l} as [4H][H][1], cfg =
 * bc_conv1d_select_cfg(4H, H, 1, 1, 1, mode)); bias[l] = bias_ih_l{l} + bias_hh_l{l} ([4H], device);
 * w_hh_packed[l] = bc_lstm_pack_hh(weight_hh_l{l}, mode) (same mode as the forward call).  The three
 * pointer arrays are HOST arrays of device pointers.  out = snake(y + x) when out_snake_alpha_exp !=
 * NULL (the Activation1d that follows the ResLSTM in both stacks), else y + x.  workspace:
 * bc_lstm_workspace_floats(B, H, T) device floats.  H % 16 == 0.
 * Modes 1, 2 (= 3) and 3 with H in {256, 512, 1024, 1536}: the recurrence runs as ONE persistent launch per
 * layer (H/8 workgroups that must all be resident at once — checked against the kernel's occupancy,
 * else 3 — W_hh register-resident; mode 1 3xbf16-split, mode 3 2xfp16-split MFMA); otherwise one
 * launch per step (fp32 MFMA).
 * TIMEOUT STATUS: the call zeroes ((int*)workspace)[0] on the stream, and every persistent
 * workgroup that gives up waiting for a neighbour (bounded spin; never in a correct run) adds 1 to it
 * and leaves, so `out` is then WRONG.  The caller must read that int after the call completes and
 * treat nonzero as an error before consuming `out` (the Python package raises BigCodecLibraryError).
 * bc_lstm_status(reset) returns the same count summed over the process's calls (diagnostic),
 * synchronising the device. */
long long bc_lstm_hh_packed_floats(int H, int mode);
int bc_lstm_pack_hh(const float* w_hh_host, float* packed_host, int H, int mode);
long long bc_lstm_workspace_floats(int B, int H, int T);
int bc_lstm_status(int reset);

/* Diagnostic (not on the codec path; bench.py's roofline): nwg workgroups of 4 waves, each wave
 * issuing 16 * iters v_mfma_f32_16x16x32_bf16 on random register operands (16384 FLOP each); out:
 * nwg * 4 device floats.  Timed by the caller, it gives the dense-BF16 rate the device sustains
 * under its clock management, the practical ceiling beside the spec peak. */
int bc_mfma_probe(float* out, int nwg, int iters, void* stream);
int bc_reslstm_fwd(const float* x, float* out, int B, int H, int T, int num_layers,
                   const float* const* w_ih_packed, const float* const* bias,
                   const float* const* w_hh_packed, const float* out_snake_alpha_exp,
                   const float* out_snake_inv_beta, float* workspace, int mode, void* stream);
/* bc_reslstm_fwd_state: bc_reslstm_fwd with carried state for streaming (nn.LSTM's (h0, c0) in, (h_n, c_n)
 *   out): h0 / c0 / hT / cT are [num_layers][H][B] device buffers (unit-major; NULL h0 and c0 = zero
 *   state, NULL hT and cT = not returned).  Runs on the persistent kernel only (modes 1 and 3, H a
 *   multiple of 128 up to 1536); other shapes return 3. */
int bc_reslstm_fwd_state(const float* x, float* out, int B, int H, int T, int num_layers,
                         const float* const* w_ih_packed, const float* const* bias,
                         const float* const* w_hh_packed, const float* out_snake_alpha_exp,
                         const float* out_snake_inv_beta, float* workspace, int mode, const float* h0,
                         const float* c0, float* hT, float* cT, void* stream);
/* bc_reslstm_fwd_state_lens: bc_reslstm_fwd_state with a step count per clip (a streaming session pool whose sessions
 *   deliver chunks of different lengths in one push, streaming.py StreamPool; like streaming itself it stands in for
 *   no reference behaviour, each session's whole-sequence causal pass defines its result).  lens is a DEVICE array
 *   int32[B]: hT[l][u][b] / cT[l][u][b] are the state of every layer after step clamp(lens[b], 1, T) - 1 of clip b.
 *   out is unchanged, all T steps of every clip: the steps past a clip's own length run on and are the caller's to
 *   ignore.  lens NULL, or every entry == T, is bc_reslstm_fwd_state bit for bit (the same launches; lens only
 *   selects the step whose state is stored).  Returns 3 before any launch for a shape the per-step kernels serve. */
int bc_reslstm_fwd_state_lens(const float* x, float* out, int B, int H, int T, int num_layers,
                              const float* const* w_ih_packed, const float* const* bias,
                              const float* const* w_hh_packed, const float* out_snake_alpha_exp,
                              const float* out_snake_inv_beta, float* workspace, int mode, const float* h0,
                              const float* c0, float* hT, float* cT, const int* lens, void* stream);

/* bc_reslstm_bidir_fwd: ResLSTM(dimension = D, bidirectional=True) (vq/module.py:150-152: nn.LSTM(D, D / 2,
 *   num_layers, batch_first=True, bidirectional=True)), + skip.  x, out: [B][D][T], H = D / 2, D % 32 == 0.
 *   The pointer arrays hold TWO entries per layer, [2l] = forward and [2l + 1] = backward direction
 *   (torch's weight_ih_l{l} / weight_ih_l{l}_reverse ...), each packed as above but with Cin = D:
 *   w_ih_packed = bc_conv1d_pack(weight_ih as [4H][D][1], cfg = bc_conv1d_select_cfg(4H, D, 1, 1, 1, mode)),
 *   w_hh_packed = bc_lstm_pack_hh(weight_hh, H, mode).  Layer outputs are [forward h | backward h]
 *   (torch's concatenation order); the backward direction runs the forward recurrence over the
 *   time-reversed sequence.  workspace: bc_reslstm_bidir_workspace_floats(B, D, T) floats, same timeout
 *   status contract as bc_reslstm_fwd.  No carried state (streaming models are unidirectional). */
long long bc_reslstm_bidir_workspace_floats(int B, int D, int T);
int bc_reslstm_bidir_fwd(const float* x, float* out, int B, int D, int T, int num_layers,
                         const float* const* w_ih_packed, const float* const* bias,
                         const float* const* w_hh_packed, const float* out_snake_alpha_exp,
                         const float* out_snake_inv_beta, float* workspace, int mode, void* stream);

/* ---- Factorized VQ (codebook_dim == 8) ---------------------------------------------------------
 * bc_vq_prepare_codebook: F.normalize(codebook) and its row sums of squares
 *   (vq/factorized_vector_quantize.py:99,105).
 * bc_vq_fwd: FactorizedVectorQuantize.forward in eval mode (factorized_vector_quantize.py:29-76):
 *   z [B][D][T] -> in_proj (folded WN Linear, w_in [8][D], b_in [8]) -> decode_latents (:93-108) ->
 *   idx [B][T] int64; z_e_out [B][8][T] (optional, may be NULL); post_out [B][D][T] = out_proj of
 *   the straight-through z_q (optional, may be NULL; w_out [D][8], b_out [D]).
 * bc_vq_argmin: decode_latents' search alone: z_e rows [N][8] -> idx [N] int64.  Given the same
 *   z_e the indices equal the reference's ("VQ exactness").
 * bc_vq2emb: FactorizedVectorQuantize.vq2emb (:78-81): idx[n*idx_stride] -> emb [N][D] (= (B,T,D)
 *   as the reference returns); w_out == NULL means proj=False (emb = codebook rows, D == dim);
 *   accumulate != 0 adds into emb (ResidualVQ.vq2emb sum, residual_vq.py:42-48); an index outside
 *   [0, n_codes) gives NaN, never an out-of-range read.
 * bc_rvq_update: ResidualVQ bookkeeping (residual_vq.py:31-33): residual -= q; out (+)= q. */
int bc_vq_prepare_codebook(const float* codebook, float* codebook_norm, float* codebook_sq,
                           int n_codes, int dim, void* stream);
int bc_vq_fwd(const float* z, const float* w_in, const float* b_in, const float* codebook,
              const float* codebook_norm, const float* codebook_sq, const float* w_out,
              const float* b_out, long long* idx, float* z_e_out, float* post_out,
              int B, int D, int T, int n_codes, int dim, void* stream);
int bc_vq_argmin(const float* z_e, const float* codebook_norm, const float* codebook_sq,
                 long long* idx, long long N, int n_codes, int dim, void* stream);
int bc_vq2emb(const long long* idx, long long idx_stride, const float* codebook,
              const float* w_out, const float* b_out, float* emb, long long N, int D, int n_codes,
              int dim, int accumulate, void* stream);
int bc_rvq_update(float* residual, float* out, const float* q, long long n, int first,
                  void* stream);
/* bc_vq2emb_ct: the token -> audio entry (codec_decoder.py:96-99 vq2emb, then the caller's
 *   transpose(1, 2) before decoder(x, vq=False)): idx[B][T][nq] int64 -> emb[B][D][T], summed over the
 *   nq quantizers in the reference's order.  Quantizer parameters stacked: codebooks [nq][n_codes][dim],
 *   w_out [nq][D][dim] (folded weight norm), b_out [nq][D].  1 <= nq <= 8, dim == 8.  An index outside
 *   [0, n_codes) gives NaN in its column (never an out-of-range read). */
int bc_vq2emb_ct(const long long* idx, int nq, const float* codebooks, const float* w_out,
                 const float* b_out, float* emb, int B, int T, int D, int n_codes, int dim, void* stream);

/* bc_fsq_fwd: FSQ.forward (vendored lucidrains finite_scalar_quantization.py:205-262; the decoder's
 *   fsq=True quantizer, codec_decoder.py:41-47, 85-92), eval, channel_first: z[B][D][T] ->
 *   idx[B][T] int32 and (optional) post[B][D][T] = project_out(codes).  w_in [d][D], b_in [d], w_out [D][d],
 *   b_out [D]; consts[5][d] = half_l, offset, shift, half_width, basis (float32, from the reference's own
 *   expressions); 1 <= d <= 8. */
int bc_fsq_fwd(const float* z, const float* w_in, const float* b_in, const float* w_out, const float* b_out,
               const float* consts, int* idx, float* post, int B, int D, int T, int d, void* stream);

/* bc_fsq_codes: FSQ.indices_to_codes (finite_scalar_quantization.py:159-192), channel_first, one codebook: the
 *   fsq=True decoder's token -> latent step (its vq2emb raises AttributeError in the reference: FSQ has no vq2emb,
 *   codec_decoder.py:96-99).  idx[B][T] (idx_bits 32: int32, 64: int64) -> post[B][D][T] = project_out(codes),
 *   codes[j] = ((idx // basis[j]) % levels[j] - levels[j] // 2) / (levels[j] // 2) with torch's floor // and %
 *   (any integer maps to a grid point, as in the reference), basis = cumprod([1] + levels[:-1]).  levels is a
 *   HOST array of d ints >= 2; w_out [D][d], b_out [D] as in bc_fsq_fwd, whose post it reproduces bit for bit
 *   for the indices it returned.  1 <= d <= 8. */
int bc_fsq_codes(const void* idx, int idx_bits, const int* levels, const float* w_out, const float* b_out,
                 float* post, int B, int D, int T, int d, void* stream);

/* bc_stream_window: one step of a causal stream's carried state (audiotokenization_amd/streaming.py; the reference has
 *   no streaming mode, its whole-sequence causal convs, vq/module.py:11-48, define the result): for each row (b, c)
 *   win[b][c][j] = j < P ? ctx[b][c][j] : act(x[b][c][j - P]) for j < P + n, and ctx_out[b][c][i] = win[b][c][n + i]
 *   for i < P.  act = SnakeBeta with (snake_alpha_exp, snake_inv_beta) as bc_snake_fwd takes them, or the identity
 *   when both are NULL; ctx NULL reads zeros (a stream's start).  x is read at x + b * x_batch_stride + c *
 *   x_row_stride + t (floats), so a strided view works; win is [B][C][P + n], ctx / ctx_out [B][C][P] (ctx_out may be
 *   NULL only when P == 0) and must not overlap ctx. */
int bc_stream_window(const float* x, long long x_batch_stride, long long x_row_stride, const float* ctx,
                     const float* snake_alpha_exp, const float* snake_inv_beta, float* win, float* ctx_out, int B, int C,
                     int n, int P, void* stream);

/* bc_stream_window_la: bc_stream_window for a look-ahead stream (streaming.py LookaheadEncoder / LookaheadDecoder,
 *   DESIGN.md §23; the reference has no streaming mode: its whole-sequence non-causal convs, vq/module.py:59-72 with
 *   symmetric padding, define the result).  A stage of such a stream is a lazy valid conv whose carried input grows and
 *   shrinks and whose right zero padding arrives at the flush, so the carry read (Pin columns) and the carry stored
 *   (Pout columns) differ and R zero columns may follow: for each row (b, c), with S = Pin + n,
 *   win[b][c][j] = j < Pin ? ctx[b][c][j] : j < S ? act(x[b][c][j - Pin]) : 0.0f for j < S + R, and
 *   ctx_out[b][c][i] = win[b][c][S - Pout + i] for i < Pout, Pout <= S (it may reach back into ctx, never into the
 *   zeros).  act, ctx NULL (zeros) and the strides as in bc_stream_window; win is [B][C][S + R], ctx [B][C][Pin],
 *   ctx_out [B][C][Pout], NULL exactly when Pout == 0, and must not overlap ctx.  n == 0 is legal when Pin + R > 0 (a
 *   flush without new input; x is then not read and may be NULL).  Pin == Pout, R == 0 reproduces bc_stream_window bit
 *   for bit.  Returns 1 for a null pointer or inconsistent sizes (an empty window, Pout > Pin + n, a ctx_out that
 *   disagrees with Pout), 3 when B * C or Pin + n + R exceeds 2^31 - 1, 0 without a launch when B == 0. */
int bc_stream_window_la(const float* x, long long x_batch_stride, long long x_row_stride, const float* ctx,
                        const float* snake_alpha_exp, const float* snake_inv_beta, float* win, float* ctx_out, int B,
                        int C, int n, int Pin, int R, int Pout, void* stream);

/* bc_stream_window_slots: bc_stream_window for a pool of independent streaming sessions (streaming.py StreamPool).  It
 *   stands in for no reference behaviour: the reference has no streaming, and its whole-sequence causal pass defines
 *   each session's result, as for bc_stream_window.  The contexts live in pool[pool_rows][C][P]; the DEVICE arrays
 *   src[B] / dst[B] give, for entry b of the push, the pool row its context is read from (src[b] < 0: a fresh session,
 *   zeros) and the row the next context (the window's last P columns) is stored to (dst[b] < 0: not stored, a
 *   padding entry).  win [B][C][P + n], x, the Snake and the strides as in bc_stream_window (bit-identical values);
 *   P >= 1 (a stage without history has no state: bc_stream_window).  With n < P a row's elements are read and
 *   overwritten by different workgroups, so the CALLER guarantees that no row is both in src and in dst of one call
 *   and that dst names no row twice; slot values are not checked by the launcher (they are on the device; the debug
 *   build skips and counts a row >= pool_rows).  Returns 1 for a null pointer or inconsistent sizes, 3 when B * C,
 *   P + n or pool_rows * C exceeds 2^31 - 1, 0 without a launch when B == 0.
 * bc_lstm_state_gather / bc_lstm_state_scatter: the pool's ResLSTM state around bc_reslstm_fwd_state (which still sees
 *   a dense batch).  h_pool / c_pool are [num_layers][H][pool_rows], h0 / c0 / hT / cT [num_layers][H][B].  Gather:
 *   h0[l][u][b] = src[b] < 0 ? 0 : h_pool[l][u][src[b]] (c likewise); scatter: h_pool[l][u][dst[b]] = hT[l][u][b] for
 *   dst[b] >= 0 (dst without duplicates).  One launch serves h and c.  Same status codes. */
int bc_stream_window_slots(const float* x, long long x_batch_stride, long long x_row_stride, float* pool, const int* src,
                           const int* dst, const float* snake_alpha_exp, const float* snake_inv_beta, float* win, int B,
                           int C, int n, int P, int pool_rows, void* stream);
/* bc_stream_window_slots_lens: bc_stream_window_slots with a chunk length per entry.  lens is a DEVICE array int32[B]
 *   in hops and unit the columns per hop at this stage (n / n_hops of the push): entry b delivers L_b =
 *   clamp(lens[b] * unit, 0, n) columns, left-aligned in its row of x.  win[b][c][j] is bc_stream_window_slots' value
 *   for j < P + L_b and 0.0f for P + L_b <= j < P + n; x is never read at or past column L_b (it may hold NaN there);
 *   the context stored to row dst[b] is win[b][c][L_b + i], i < P: the last P columns of [context | chunk[:L_b]],
 *   which with L_b < P reach back into the old context.  Every lens[b] * unit == n reproduces bc_stream_window_slots
 *   bit for bit.  Same src / dst contract and status codes; unit < 1 or a null lens returns 1. */
int bc_stream_window_slots_lens(const float* x, long long x_batch_stride, long long x_row_stride, float* pool,
                                const int* src, const int* dst, const int* lens, int unit, const float* snake_alpha_exp,
                                const float* snake_inv_beta, float* win, int B, int C, int n, int P, int pool_rows,
                                void* stream);
/* bc_stream_window_slots_la: the window of a pool of look-ahead streams (streaming.py LookaheadPool):
 *   bc_stream_window_la's carry in / carry out of different lengths and zeros behind, over bc_stream_window_slots_lens'
 *   pool rows and length per entry, plus an input offset per entry.  It stands in for no reference behaviour (the
 *   reference has no streaming; its whole-sequence non-causal pass defines each session's result).  src, dst, cin, n,
 *   xoff, keep, cout are DEVICE arrays int32[B]; pool is [pool_rows][C][Pmax], Pmax the row pitch (the largest carry the
 *   stage can hold); win is [B][C][W]; x has x_cols columns per row, read at x + b * x_batch_stride + c *
 *   x_row_stride + t (floats), so a strided view works (x may be NULL when x_cols == 0).  For each row (b, c), j < W:
 *     win[b][c][j] = j < cin[b] ? pool[src[b]][c][j] : j - cin[b] < n[b] ? act(x[b][c][xoff[b] + j - cin[b]]) : 0.0f
 *     pool[dst[b]][c][i] = win[b][c][keep[b] + i]   for i < cout[b]   (dst[b] >= 0)
 *   Every row is left-aligned: the zeros behind an entry are a short entry's tail and, at a flush, the layer's own
 *   right zero padding alike.  src[b] < 0 reads the cin[b] carried columns as zeros (a fresh session's left zero
 *   padding; a caller without one passes cin[b] == 0); dst[b] < 0 or cout[b] == 0 stores nothing.  cin and cout are
 *   clamped to [0, Pmax], xoff to [0, x_cols] and n to [0, min(W - cin, x_cols - xoff)], on the device, so no array
 *   value takes an access out of x, win or a pool row, and x is never read outside [xoff[b], xoff[b] + n[b]) (it may
 *   hold NaN there).  The CALLER guarantees keep[b] + cout[b] <= cin[b] + n[b] (the carry never reaches into the
 *   zeros), and, as for bc_stream_window_slots, that no pool row is both in src and in dst of one call and that dst
 *   names no row twice: a row's elements are read and overwritten by different workgroups, and the kernel cannot check
 *   it.  Slot values are not checked by the launcher (the debug build skips and counts a row >= pool_rows, and a carry
 *   that reaches into the zeros).  act and the Snake pointers as in bc_stream_window.  Every cin == cout == Pmax, n ==
 *   W - Pmax, xoff == 0, keep == n reproduces bc_stream_window_slots bit for bit; one entry with src < 0 or a dense
 *   carry in its pool row reproduces bc_stream_window_la.  Returns 1 for a null pointer or inconsistent sizes (W < 1,
 *   Pmax < 1, pool_rows < 1, x_cols < 0, strides that do not hold x_cols columns), 3 when B * C or pool_rows * C
 *   exceeds 2^31 - 1, 0 without a launch when B == 0. */
int bc_stream_window_slots_la(const float* x, long long x_batch_stride, long long x_row_stride, int x_cols, float* pool,
                              const int* src, const int* dst, const int* cin, const int* n, const int* xoff,
                              const int* keep, const int* cout, const float* snake_alpha_exp,
                              const float* snake_inv_beta, float* win, int B, int C, int W, int Pmax, int pool_rows,
                              void* stream);
int bc_lstm_state_gather(const float* h_pool, const float* c_pool, const int* src, float* h0, float* c0, int num_layers,
                         int H, int B, int pool_rows, void* stream);
int bc_lstm_state_scatter(float* h_pool, float* c_pool, const int* dst, const float* hT, const float* cT, int num_layers,
                          int H, int B, int pool_rows, void* stream);

/* bc_zero_tail (ABI 18): ragged batches (clips of different lengths zero-padded into one batch; the reference encodes
 *   each file alone, extract_indices.py:497-561, and its convs zero-pad at the clip's end, vq/module.py:45-48, 59-72).
 *   For y[B][C][T], the optional y2 of the same shape (NULL: none) and the DEVICE array lens[B], stores 0.0f at every
 *   t in [clamp(lens[b], 0, T), T) of every row (b, c): stores, not a product with a mask, so Inf / NaN in a tail
 *   become zero.  tail_max = T - min(lens) is computed by the host and only sizes the launch to the padding (a larger
 *   value costs idle threads, a smaller one nothing but time); tail_max <= 0 launches nothing.  Returns 1 for a null
 *   y or lens or a non-positive B, C or T. */
int bc_zero_tail(float* y, float* y2, const int* lens, int B, int C, long long T, long long tail_max, void* stream);

/* ---- Real-audio ingest ------------------------------------------------------------------------
 * bc_resample_sinc: torchaudio.transforms.Resample(orig, new) as extract_indices.py:129-132 and
 *   data_module.py:95-98 call it: x[B][Lin] -> y[b * y_pitch + o], o < Lout = ceil(new * Lin / orig)
 *   (y_pitch >= Lout leaves room for extract_indices.py:135-137's pad_to_stride zeros), with
 *   orig / new already divided by their gcd and kern[new][taps] the host-built sinc-Hann filters
 *   (audiotokenization_amd/ingest.py sinc_resample_kernel, taps = 2 * width + orig). */
int bc_resample_sinc(const float* x, float* y, const float* kern, int B, long long Lin, long long Lout,
                     long long y_pitch, int orig, int new_freq, int taps, int width, void* stream);

/* ---- FLAC decoding (host code, no device memory) -----------------------------------------------
 * Replaces soundfile's read of the reference's LibriTTS / LibriSpeech .flac utterances
 * (extract_indices.py:98-106: sf.SoundFile(...).read(dtype='float32', always_2d=True)).  RFC 9639 streams:
 * all subframe types, Rice / escaped residuals, wasted bits, stereo decorrelations, 4-32 bit samples.
 * bc_flac_info: STREAMINFO of an in-memory stream (total_samples 0 = unknown); returns 0, 1 (bad argument),
 *   2 (not FLAC / corrupt), 3 (unsupported).
 * bc_flac_decode: every frame into out[channel * max_samples + i] (HOST memory), int32 when out_int32 != 0,
 *   else float32 = sample * 2^-(bits - 1) (libsndfile's normalised float read); check_crc verifies the
 *   frame-header CRC-8 and frame CRC-16.  Returns samples per channel, or -1 bad argument, -2 corrupt,
 *   -3 unsupported, -4 CRC mismatch, -5 more than max_samples samples. */
int bc_flac_info(const unsigned char* data, long long n, int* sample_rate, int* channels, int* bits,
                 long long* total_samples);
long long bc_flac_decode(const unsigned char* data, long long n, void* out, int out_int32, long long max_samples,
                         int check_crc);

/* ---- Layout helpers & synthetic input --------------------------------------------------------
 * bc_btc_to_ctb: x[B][C][T] -> y[C][T][B];  bc_ctb_to_btc_add: out = transpose(y) + skip.
 * bc_synth_clips: x[B][T] white noise, clip i = clip0 + b (SURVEY.md §8(d) spec). */
int bc_btc_to_ctb(const float* x, float* y, int B, int C, int T, void* stream);
int bc_ctb_to_btc_add(const float* y, const float* skip, float* out, int B, int C, int T,
                      void* stream);
int bc_synth_clips(float* x, int B, long long T, long long clip0, void* stream);

/* ---- Round-trip quality metrics (added under ABI 18: additive, no existing entry point changes) -----------------
 * What inference_full.py:570-604, 644-647, 723-737 reports of a reconstruction, where the waveforms already are
 * (PESQ excepted: DESIGN.md section 16; STOI: section 21).  ref / rec are [B][T] fp32; lens[b] (int32, device; NULL = every
 * clip fills T) is clip b's own length: samples at or beyond it are never read, and clip b's result is bit for bit
 * what the clip alone gives.
 * bc_si_snr: out[b] = torchmetrics' ScaleInvariantSignalNoiseRatio(preds = rec, target = ref) in dB over clip b:
 *   t' = ref - mean, p' = rec - mean, eps = 2^-23, alpha = (sum p't' + eps) / (sum t't' + eps), s = alpha t',
 *   10 log10((sum s^2 + eps) / (sum (s - p')^2 + eps)); three passes with fp64 accumulators (NaN for lens[b] <= 0).
 * bc_logmel_l1: one resolution of criterions/mel_loss.py:22-31, 44-49 (torchaudio MelSpectrogram: periodic Hann
 *   window of n_fft, hop n_fft / 4, center=True with reflect padding at the clip's own ends, one-sided magnitude,
 *   mel matrix, clamp, log10): out[b] = mean over n_mels x (1 + lens[b] / hop) cells of
 *   |log10 max(mel_ref, clamp_eps) - log10 max(mel_rec, clamp_eps)|.  basis[2 * bins][n_fft] (bins = n_fft / 2 + 1;
 *   rows [0, bins) the windowed cosines, rows [bins, 2 bins) the windowed negative sines; 16-byte aligned) and
 *   mel[n_mels][bins] are built on the host (audiotokenization_amd/metrics.py).  n_fft a multiple of 16,
 *   n_mels <= 320 (else 3).  workspace: bc_logmel_workspace_doubles(B, T, n_fft) doubles (-1: bad arguments), one
 *   partial sum per tile of bc_logmel_tile_frames() frames; no spectrogram is written to memory.  A clip shorter
 *   than n_fft / 2 + 1 samples (reflect padding undefined) gives NaN.  Native fp32 MFMA operands.
 * bc_code_hist: counts[c] (int64[n_codes], accumulated) += the number of codes[b][t] == c, t < lens[b] (in frames;
 *   NULL = all T); codes (code_bits 32 or 64, signed) outside [0, n_codes) are ignored.  n_codes <= 16384 (else 3). */
int bc_si_snr(const float* ref, const float* rec, const int* lens, float* out, int B, long long T, void* stream);
int bc_logmel_tile_frames(void);
long long bc_logmel_workspace_doubles(int B, long long T, int n_fft);
int bc_logmel_l1(const float* ref, const float* rec, const int* lens, const float* basis, const float* mel, float* out,
                 double* workspace, int B, long long T, int n_fft, int n_mels, float clamp_eps, void* stream);
int bc_code_hist(const void* codes, int code_bits, const int* lens, long long* counts, int B, long long T, int n_codes,
                 void* stream);

/* ---- STOI (additive under ABI 18) ----------------------------------------------------------
 * The short-time objective intelligibility measure of Taal et al. 2011 (non-extended, as the pystoi package computes
 * it; the written definition is tests/stoi_ref.py): both signals to 10 kHz, the frames (256 / 128, Hann) of the
 * CLEAN signal more than 40 dB below its loudest dropped from both, STFT (n = 512) of the signals rebuilt from the
 * kept frames, 15 third-octave band magnitudes from 150 Hz, and per 30-frame segment and band the clipped (-15 dB),
 * centred, normalised correlation; out[b] is their mean.  clean / proc are [B][T] fp32 and lens as above: samples at
 * or beyond lens[b] are never read, and clip b's result is bit for bit what the clip alone gives.
 * bc_stoi: up / down = 10000 / sample rate, reduced (16 kHz: 5 / 8; 1 / 1: no resampling, filt may be NULL).
 *   filt[2 half_len + 1]: the taps of y[n] = sum_m x[m] filt[down n - up m + half_len], n < ceil(lens[b] up / down)
 *   (scipy.signal.resample_poly's effective filter); basis[2 * 224][256], 16-byte aligned: rows [0, 224) are
 *   w[n] cos(2 pi (7 + r) n / 512), rows [224, 448) are -w[n] sin(...), w the 256-point Hann window without its zero
 *   end points (both built on the host: audiotokenization_amd/metrics.py).  kept[b] (int32): the frames kept; the
 *   signal rebuilt from them has kept[b] - 1 STFT frames.  out[b] = 1e-5 with fewer than 30 STFT frames, NaN for
 *   lens[b] <= 0.  workspace: bc_stoi_workspace_bytes(B, T, up, down) bytes (-1: bad or unsupported arguments),
 *   16-byte aligned: the 10 kHz samples, the frame energies, the kept list and the [2][B][15][frames] band
 *   magnitudes; no spectrogram is written to memory.  Returns 1 for a null pointer or a non-positive size, 3 for
 *   up or down above 64 or not reduced, more than 4096 taps, B > 65535 or B T > 2^36, before anything is launched.
 *   Native fp32 MFMA operands for the DFT; the resampling sums, the frame energies and the correlations are fp64. */
long long bc_stoi_workspace_bytes(int B, long long T, int up, int down);
int bc_stoi(const float* clean, const float* proc, const int* lens, const float* filt, int up, int down, int half_len,
            const float* basis, float* out, int* kept, void* workspace, int B, long long T, void* stream);

/* ---- Conformer-STFT codec family (additive under ABI 18) -----------------------------------
 * Everything of ConformerEncoderSTFT / ConformerDecoderISTFT that is not a Linear or a 1x1 conv (those run on
 * bc_conv1d_fwd).  Activations are [B][C][T] fp32; the arithmetic is fp32 VALU in every precision mode, the long sums
 * fold 16-term fp32 partial sums into an fp64 total.  Each call checks its arguments on the host (1 / 3) before it
 * launches.
 * bc_stft_frames: vq/codec_encoder.py:108-122 (F.pad by (win - hop) / 2 per side, torch.stft center=False) and the
 *   real / imaginary concatenation of :188-192.  x[B][T]; basis_t[n_fft][n_fft + 2], column c < bins = n_fft / 2 + 1:
 *   w[n] cos(2 pi c n / n_fft), column bins + c: -w[n] sin(...), w the periodic Hann window (built in float64 on the
 *   host: audiotokenization_amd/conformer.py); y[B][n_fft + 2][F], F = (T + 2 ((win - hop) / 2) - n_fft) / hop + 1.
 *   3 for win != n_fft or an odd n_fft.
 * bc_rmsnorm_fwd: vq/module.py:357-370 over the channels of every (b, t): (x * rsqrt(mean_c x^2 + eps)) * w[c], in that
 *   order; w may be NULL (no gain); silu != 0 applies x * sigmoid(x) to the result (module.py:490-491).
 * bc_dwconv_glu_fwd: nn.GLU(dim=1) and the depthwise conv of ConformerConvModule (vq/module.py:476-480, 488-489).
 *   x[B][2 C][T] (pointwise_conv1's output), w[C][K], bias[C] or NULL, y[B][C][T]:
 *   y[c][t] = bias[c] + sum_k w[c][k] g[c][t + k - pad_left], g = x[c] * sigmoid(x[C + c]), zero outside [0, T).
 *   pad_left = (K - 1) / 2 is padding='same' (the right pad is K - 1 - pad_left), K - 1 the CausalConv1d.  K <= 63.
 * bc_swiglu_fwd: F.silu(w1 x) * (w3 x) of FeedForward (vq/module.py:468) over h[B][2 H][T], the output of w1 and w3
 *   stacked into one conv; y[B][H][T].
 * bc_attention_fwd: SelfAttention.forward's manual branch between qkv_proj and out_proj (vq/module.py:421-449).
 *   qkv[B][3 n_head D][T], channel s n_head D + h D + d (s: q, k, v); rope[>= T][D / 2][2]: torch.view_as_real of
 *   precompute_freqs_cis (module.py:372-377); y[B][n_head D][T].  q and k are RMS-normalised over D (eps 1e-6) and
 *   rotated, then softmax(q k^T / sqrt(D)) v with the keys <= the query when causal.  Keys and values pass through LDS
 *   in tiles and the softmax is online: no T x T array exists.  head_dim 32 or 64 (3 otherwise).
 *   bc_attention_tiles: the queries per workgroup and the keys per LDS tile (the tests' edge lengths).
 * bc_istft_head: ISTFTHead.forward after self.out and ISTFT.forward with padding="same" (vq/codec_decoder.py:171-213,
 *   261-274).  x_pred[B][n_fft + 2][F]: rows [0, bins) log-magnitudes, rows [bins, 2 bins) phases;
 *   S = min(exp(.), 100) (cos p + i sin p) (own range reduction up to |p| < 39000, libm beyond); basis[n_fft + 2][n_fft]:
 *   the inverse real DFT (backward norm, DC and Nyquist imaginary rows zero) times the window, built in float64 on
 *   the host; window[n_fft].  y[B][(F - 1) hop + n_fft - 2 ((n_fft - hop) / 2)]: the overlap-add cropped by
 *   (n_fft - hop) / 2 per side and divided by the sum of window^2 over the frames that overlap each sample. */
int bc_stft_frames(const float* x, const float* basis_t, float* y, int B, long long T, int n_fft, int hop, int win,
                   void* stream);
int bc_rmsnorm_fwd(const float* x, const float* w, float* y, int B, int C, int T, float eps, int silu, void* stream);
int bc_dwconv_glu_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int T, int K,
                      int pad_left, void* stream);
int bc_swiglu_fwd(const float* h, float* y, int B, int H, long long T, void* stream);
int bc_attention_tiles(int* q_tile, int* kv_tile);
int bc_attention_fwd(const float* qkv, const float* rope, float* y, int B, int n_head, int head_dim, int T, int causal,
                     void* stream);
int bc_istft_head(const float* x_pred, const float* basis, const float* window, float* y, int B, int F, int n_fft,
                  int hop, void* stream);

/* ---- Bounds-checked debug build (no reference counterpart: SURVEY.md §5 row 2) ------------------------------
 * libbigcodec_hip.so built with -DBC_DEBUG (build_lib.build(debug=True) -> audiotokenization_amd/_debug/, loaded by
 * the Python package when BIGCODEC_DEBUG=1) checks the indices of the kernels' computed global accesses (conv /
 * ResidualUnit epilogue stores and residual reads, weight copies, ResLSTM output stores); a failed check is counted
 * and its access skipped, so a bad launch reports instead of faulting the GPU.
 * bc_debug_status(out[2]): out[0] = failed checks since the last call, out[1] = the first failing source line
 *   (0 = none); reads and clears; synchronises the device.  Returns 3 (unsupported) in the product build.
 * bc_debug_selftest(n, stream): a kernel whose n lanes fail one check each on purpose, touching no memory
 *   outside the debug words (the mechanism's own test).  Returns 3 in the product build. */
int bc_debug_status(unsigned int* out);
int bc_debug_selftest(int n, void* stream);

/* ---- Launch timer of the composite calls (ABI 17; no reference counterpart: the measurement row SURVEY.md §8(d)) --
 * The Python layer times every conv / ResidualUnit launch it makes itself; the kernels that bc_reslstm_fwd[_state],
 * bc_reslstm_bidir_fwd and bc_vq_fwd launch inside one call (the layout transposes, the ResLSTM input projection and
 * its pre-split planes, the persistent recurrence, the VQ) are only visible to the library.  While enabled, each of
 * those launches is bracketed by HIP events recorded on the stream it is launched on.
 * bc_launch_timer_enable(on): 1 starts a fresh recording (stale records are dropped), 0 stops it (records kept).
 * bc_launch_timer_read(max, names, ms, flops, bytes): with max <= 0 or a null array, returns the number of records
 *   and keeps them; otherwise synchronises the recorded events, copies the first max records (names: max x 64 bytes,
 *   NUL-terminated kernel symbols; ms: event-timed duration; flops / bytes: the launch's algorithmic work), clears
 *   all of them and returns their number (-1 on a HIP error). */
int bc_launch_timer_enable(int on);
int bc_launch_timer_read(int max, char* names, float* ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* BIGCODEC_H */

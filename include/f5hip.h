/* libf5hip — C ABI of the MI355X-native F5-TTS inference hot path.
 *
 * Plain C, plain pointers and sizes, no torch types.  Pointers named *_dev are HIP device pointers
 * (e.g. torch tensor .data_ptr() on a ROCm device), all other pointers are host memory.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Every function returns 0 on success and a negative
 * code on failure; f5hip_last_error() gives the message.  Nothing here falls back to the CPU.
 *
 * Streams.  A handle (f5hip_dit, f5hip_vocos, f5hip_bigvgan) has one call in flight: issue its next call on the same stream, or
 * after the caller has ordered the two.  The calls that take no handle (the mel front-ends, f5hip_ref_*, f5hip_flac_decode,
 * f5hip_wave_*, f5hip_watermark_*) keep their request tables and scratch in one workspace per device and kind of call.  They are
 * issued one at a time per device from the host (no two threads inside such calls on one device at once) and may be issued on any
 * streams: a call whose workspace was last used on another stream makes its own stream wait for that use on the device
 * (hipStreamWaitEvent, no host wait), so a call's result does not depend on which stream the next call uses.  On one stream that
 * costs one event record per call.
 *
 * Each entry point names the reference interface it replaces (F/ = src/server/f5_tts/ of
 * dwani-ai/tts-indic-server-f5); INTEGRATION.md shows the ctypes binding a maintainer would add.
 */
#ifndef F5HIP_H
#define F5HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F5HIP_ABI_VERSION 1

int f5hip_abi_version(void);
const char* f5hip_last_error(void);

/* ---------------------------------------------------------------- DiT backbone + CFM sampler ---------- */

/* model.arch of F/configs/F5TTS_*_train.yaml:24-30 (+ mel_dim, vocab size: F/infer/utils_infer.py:240-242). */
typedef struct f5hip_dit_config {
    int32_t dim, depth, heads, ff_mult, text_dim, conv_layers, mel_dim, text_num_embeds;
    int32_t gemm_planes; /* GEMM operand precision, all with fp32 accumulation:
                            2 = split-bf16 "bf16x3" everywhere (strictest: 1.1e-4 mel RMS vs the fp32 reference at C2);
                            3 = mixed: fp16 operands for the transformer-block GEMMs (QKV, out, FF1, FF2), bf16x3 for every GEMM that
                                touches the ODE state / embeddings / U-skips (3.1e-4 mel RMS for F5-Base at 32 NFE, 4.9e-4 for E2-Base
                                at 64 NFE, against the reference's own CFM.sample outputs: inside the 1e-3 bound);
                            1 = plain bf16 (fast, ~8e-3 mel RMS: outside the bound) */
    int32_t arch;        /* 0 = DiT (F5-TTS, F/model/backbones/dit.py), 1 = UNetT (E2-TTS, F/model/backbones/unett.py: text_dim = mel_dim, conv_layers = 0),
                            2 = MMDiT (F/model/backbones/mmdit.py: text_dim = dim, conv_layers = 0; state_dict keys transformer.audio_embed.*,
                                transformer.transformer_blocks.{i}.attn_norm_{c,x} / attn.to_{q,k,v}[_c] / attn.to_out[_c] / ff_{c,x}) */
} f5hip_dit_config;

typedef struct f5hip_dit f5hip_dit;

/* Replaces DiT.__init__ (F/model/backbones/dit.py:94-128). */
f5hip_dit* f5hip_dit_create(const f5hip_dit_config* cfg);
void f5hip_dit_destroy(f5hip_dit* m);

/* Replaces model.load_state_dict (F/infer/utils_infer.py:195-209): one call per tensor, `name` is the
 * reference checkpoint key with the "ema_model." prefix stripped ("transformer.time_embed.time_mlp.0.weight", ...),
 * `data` is host fp32 in the tensor's own row-major layout. */
int f5hip_dit_load_param(f5hip_dit* m, const char* name, const float* data, int64_t numel);
/* Checks that every parameter arrived, packs the weights for the MFMA kernels (split bf16, padded, fused QKV /
 * AdaLN matrices) and uploads them.  Must be called once before any forward/sample call. */
int f5hip_dit_finalize(f5hip_dit* m);

/* One evaluation of DiT.forward (F/model/backbones/dit.py:130-163) for n_seq independent sequences.
 *   seq_len[i]   frames of sequence i (rows of x/cond/out belonging to it, packed back to back)
 *   kv_len[i]    valid keys (== seq_len[i] for mask=None; < seq_len reproduces the reference's padded-batch
 *                key-padding mask and zeroed attention rows, F/model/modules.py:429-447)
 *   x_dev, cond_dev  fp32 [sum(seq_len)][mel_dim];  text: int32 [n_seq][nt_max], -1 padded;  time: scalar t
 *   drop_audio_cond[i], drop_text[i]: the two CFG switches of the reference signature
 *   n_blocks     -1 = whole network (out_dev = [sum(seq_len)][mel_dim]); k >= 0 = stop after k transformer
 *                blocks and return the residual stream in h_out_dev [sum(seq_len)][dim] (parity taps)
 */
int f5hip_dit_forward(f5hip_dit* m, int32_t n_seq, const int32_t* seq_len, const int32_t* kv_len,
                      const float* x_dev, const float* cond_dev, const int32_t* text, int32_t nt_max, float time,
                      const uint8_t* drop_audio_cond, const uint8_t* drop_text, int32_t n_blocks,
                      float* out_dev, float* h_out_dev, void* stream);

/* Copies an internal fp32 activation of the last forward for parity taps: "text_embed" -> [sum(seq_len)][text_dim]; "text_rows" (MMDiT) ->
 * the text stream's embedding as laid out, [text rows][text_dim] with every sequence's nt_max tokens padded to a multiple of 128 rows;
 * "text_stream" (MMDiT) -> the text residual stream behind the blocks that forward ran (n_blocks; its embedding for 0), [text rows][dim] in the
 * same layout.  Behind the last, context-pre-only block the stream is dropped: the rows then still hold what the block before it left. */
int f5hip_dit_read_tap(f5hip_dit* m, const char* tap, float* dst_dev, int64_t numel, void* stream);

/* The ODE loop of CFM.sample (F/model/cfm.py:160-204): Euler over t_grid with classifier-free guidance,
 * each utterance sampled with the reference's batch-1 semantics (mask=None).
 *   dur[u]          total frames of utterance u (already max(lens+1, duration) clamped, cfm.py:136-137)
 *   cond_dev        fp32 [sum(dur)][mel_dim] mel conditioning, zero padded to dur (cfm.py:144)
 *   cond_mask       uint8 [sum(dur)] 1 where the frame is conditioning (cfm.py:129-131,145-146)
 *   text            int32 [n_utt][nt_max] token ids, -1 padded (cfm.py:116-121)
 *   y0_dev          fp32 [sum(dur)][mel_dim] initial noise (cfm.py:181-186)
 *   t_grid          float [steps+1] (cfm.py:196-198)
 *   cfg_strength    < 1e-5 skips the unconditional branch (cfm.py:170-171)
 *   out_dev         fp32 [sum(dur)][mel_dim] = where(cond_mask, cond, x_1) (cfm.py:204)
 */
int f5hip_cfm_sample(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const float* cond_dev,
                     const uint8_t* cond_mask, const int32_t* text, int32_t nt_max, const float* y0_dev,
                     const float* t_grid, int32_t steps, float cfg_strength, float* out_dev, void* stream);

/* The same loop with the reference's PADDED-BATCH semantics (what CFM.sample does for batch > 1: F/model/cfm.py:151-154, mask =
 * lens_to_mask(duration); F/model/modules.py:429-447): every item is laid out with dur[u] = the batch maximum, kv_len[u] = its own
 * duration; keys >= kv_len[u] are masked in every attention, the attention output rows >= kv_len[u] are zeroed, and everything
 * else (text / conv embeddings, feed-forward, the ODE update of the padded rows) runs over all dur[u] rows exactly like the
 * reference's padded tensors.  kv_len == NULL is f5hip_cfm_sample. */
int f5hip_cfm_sample_masked(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev,
                            const uint8_t* cond_mask, const int32_t* text, int32_t nt_max, const float* y0_dev,
                            const float* t_grid, int32_t steps, float cfg_strength, float* out_dev, void* stream);

/* f5hip_cfm_sample_masked with one CFG strength per unit: cfg_strength is a host array of n_utt floats.  A unit whose strength is
 * < 1e-5 gets no unconditional sequence at all (the reference's early-out, cfm.py:162-175, per unit: its rows are neither laid out nor
 * run through the backbone); every other unit gets its unconditional sequence and v = p + (p - p_uncond) * cfg_strength[u].  The
 * strengths travel with the per-row metadata (no host sync).  A unit's result is what f5hip_cfm_sample_masked gives it with its own
 * strength as the scalar, with every ODE method and backbone. */
int f5hip_cfm_sample_units(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev,
                           const uint8_t* cond_mask, const int32_t* text, int32_t nt_max, const float* y0_dev,
                           const float* t_grid, int32_t steps, const float* cfg_strength, float* out_dev, void* stream);

/* f5hip_cfm_sample_units with one time grid per unit as well: unit u takes steps[u] >= 1 steps over its own grid, the steps[u] + 1 floats
 * of t_grids that follow the grids of units 0..u-1 (sum(steps) + n_utt floats in all), and its own CFG strength cfg_strength[u].  With
 * every ODE method and backbone, a unit's result is what f5hip_cfm_sample_units (or _masked) gives it alone with its grid and strength as
 * the call's; when all units share one grid, the call IS f5hip_cfm_sample_units.  The union of the units' time points (Euler: steps[u]
 * per unit, midpoint: 2 steps[u], RK4: 3 steps[u] + 1; equal values once) may hold at most 256 points -- checked before anything is
 * launched.  The call runs the forwards of the unit with the most steps; a unit whose steps are done is frozen and leaves the layout
 * (counter "dit_rows": the summed backbone rows of the forwards). */
int f5hip_cfm_sample_grids(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev,
                           const uint8_t* cond_mask, const int32_t* text, int32_t nt_max, const float* y0_dev,
                           const int32_t* steps, const float* t_grids, const float* cfg_strength, float* out_dev, void* stream);

/* One SPAN of the ODE loop of CFM.sample (F/model/cfm.py:160-204): f5hip_cfm_sample_grids that can stop at a step boundary and be
 * resumed by a later call.  The library keeps nothing between spans: a span is one more stateless sampler call.
 *   y0_dev     per unit its CURRENT ODE state [dur, mel]: the noise (cfm.py:181-186) for its first span, else the rows the previous span
 *              returned for it
 *   steps[u], t_grids   this span only: steps[u] >= 1 steps over steps[u] + 1 points, a contiguous slice of the unit's whole grid
 *              (cfm.py:196-198) with the whole grid's fp32 values.  Midpoint and RK4 spans end on step boundaries too; RK4's fourth
 *              stage of the span's last step is evaluated at the slice's last point.
 *   last[u]    host uint8 [n_utt].  != 0: the unit ends with this span and receives where(cond_mask, cond, x) (cfm.py:204) like every
 *              other sampler call; 0: it receives the raw fp32 state of all its frames after its last step of the span, prompt frames
 *              included -- what the next span takes as y0_dev.  Chosen per frame on the device by the final select kernel; the flags
 *              ride in the per-call metadata upload.  Nothing else about the step loop depends on `last`.
 * Units of a span may be at different points of grids of different lengths; everything f5hip_cfm_sample_grids says about layout, limits
 * (256 distinct time points) and dispatch holds: equal span grids make it the one-grid call, and a span over every unit's whole grid with
 * `last` all 1 launches the kernels of f5hip_cfm_sample_grids and returns its bits.  With the shape-invariant attention mode a unit
 * sampled in spans, among any other units, equals the unit sampled alone in one call, bit for bit.  Every refusal (null `last`,
 * steps[u] < 1, the dur / kv_len / time-point limits) comes before the first launch. */
int f5hip_cfm_sample_span(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev,
                          const uint8_t* cond_mask, const int32_t* text, int32_t nt_max, const float* y0_dev,
                          const int32_t* steps, const float* t_grids, const float* cfg_strength, const uint8_t* last,
                          float* out_dev, void* stream);

/* f5hip_cfm_sample_span with one ODE method per unit as well: unit u is stepped by solver method[u] (host int32 [n_utt]: 0 euler, 1 midpoint,
 * 2 rk4, the codes of f5hip_dit_set_ode_method) over its steps[u] >= 1 steps.  The handle's own method is ignored by this call and left
 * unchanged.  `last` as in f5hip_cfm_sample_span; NULL = every unit ends (f5hip_cfm_sample_grids' result).
 *   Unit u takes F_u = steps[u] * (1, 2 or 4) backbone forwards.  The units are laid out by F_u, descending, and the call runs max F_u
 *   forwards: before forward f the layout shrinks to the units with F_u > f (counter "dit_rows"), and after it ONE launch steps every frame
 *   by the rule and stage its unit is at -- the one update kernel of every sampler call, here with op and step size per unit.
 *   The union of the units' time points, each by its own rule (Euler steps[u], midpoint 2 steps[u], RK4 3 steps[u] + 1; equal values once),
 *   may hold at most 256 points.  RK4's fourth stage of a unit's last step is evaluated at its slice's last point.
 * When all method[u] are equal the call IS f5hip_cfm_sample_span / _grids on a handle set to that method: same kernels, same bits.  With
 * the shape-invariant attention mode a unit's result is what f5hip_cfm_sample_span / _grids gives it alone on a handle set to its method,
 * bit for bit.  Every refusal (null `method`, a value outside 0..2, steps[u] < 1, the dur / kv_len / time-point limits) comes before the
 * first launch. */
int f5hip_cfm_sample_methods(f5hip_dit* m, int32_t n_utt, const int32_t* dur, const int32_t* kv_len, const float* cond_dev,
                             const uint8_t* cond_mask, const int32_t* text, int32_t nt_max, const float* y0_dev,
                             const int32_t* steps, const float* t_grids, const float* cfg_strength,
                             const int32_t* method /* host [n_utt], 0 euler / 1 midpoint / 2 rk4 */,
                             const uint8_t* last /* as f5hip_cfm_sample_span; NULL = every unit ends */,
                             float* out_dev, void* stream);

/* The fixed-grid solver both sample calls use: replaces CFM(odeint_kwargs=dict(method=...)) (F/model/cfm.py:37-41,72,200; set from
 * load_model(ode_method=...), F/infer/utils_infer.py:251).  0 = "euler" (default): x += dt * v(t_i, x).  1 = "midpoint":
 * x += dt * v(t_i + dt / 2, x + dt / 2 * v(t_i, x)), two backbone evaluations per step, at most 64 steps per call.  2 = "rk4": torchdiffeq's
 * fixed-grid rule (rk4_alt_step_func, the 3/8 rule), four backbone evaluations per step, at most 42 steps per call:
 *   k1 = v(t_i, x), k2 = v(t_i + dt / 3, x + dt * k1 / 3), k3 = v(t_i + 2 dt / 3, x + dt * (k2 - k1 / 3)), k4 = v(t_{i+1}, x + dt * (k1 - k2 + k3)),
 *   x += (k1 + 3 (k2 + k3) + k4) * dt / 8.
 * `steps` is the number of grid intervals for every method. */
int f5hip_dit_set_ode_method(f5hip_dit* m, int32_t method);

/* Attention kernel choice.  0 (default): the fastest form per launch shape -- a launch with 192-query tiles (e.g. one 10 s utterance) runs
 * the SIMD-balanced kernel, in which a third of the query blocks accumulate the two key halves of every tile separately and merge them at
 * the end: the same sums in a different fp32 association, so a sequence's output can differ in the last bits from what it gets inside a
 * larger batch (the softmax offsets and the fp16 probabilities are the same in every variant).  In the mixed GEMM mode any last-bit
 * difference grows to that mode's rounding-noise floor over a forward pass (profiles/r03_attn_mode_tapdiff.txt).  1: shape-invariant arithmetic -- every variant adds every query's terms in one order, so a
 * sequence's output does not depend on what it is batched with (bit-identical); ~3 % slower at batch 1.
 * f5hip_set_attention_shape_invariant sets the PROCESS DEFAULT; f5hip_dit_set_attention_shape_invariant sets it for one handle
 * (1 / 0, or -1 = follow the process default again), so two handles in one process -- a serving handle that promises batch-independent
 * results next to a latency-bound one -- do not share the setting. */
int f5hip_set_attention_shape_invariant(int32_t on);
int f5hip_dit_set_attention_shape_invariant(f5hip_dit* m, int32_t on);
/* Per-handle profiling: like f5hip_set_profiling / f5hip_get_profile below, but the HIP-event spans, their pool and the totals belong to this
 * handle alone (a handle that never called it records into the process-wide state when that is enabled).  Calls on one handle are still one
 * at a time; calls on different handles may come from different threads. */
int f5hip_dit_set_profiling(f5hip_dit* m, int32_t enabled);
int f5hip_dit_get_profile(f5hip_dit* m, const char* kernel_class, double* total_ms, int64_t* launches);
/* Per-kernel timing of the last f5hip_cfm_sample call when profiling was enabled with
 * f5hip_set_profiling(1): average milliseconds per launch of the named kernel class
 * ("gemm", "attn", "ln", "other") measured with HIP events on the launch stream, and launch counts. */
int f5hip_set_profiling(int32_t enabled);
int f5hip_get_profile(const char* kernel_class, double* total_ms, int64_t* launches);
/* Launch counters of the GEMM dispatcher since the last reset (test instrumentation: proves which kernel a config exercised):
 * "gemm5_rb11" / "gemm5_rb8" (exact-fit tile heights 176 / 128), "gemm5_wide" (128- and 192-column tiles), "gemm5_cb12" (192-column
 * tiles only), "gemm3_wide" (fp16 128 x 256 tiles), "gemm3" (every gemm3 launch, wide or not), "conv5", "gemm6" (ping-pong tiles
 * of 256 columns: the batch-mode shapes), "gemm6_r176" / "gemm6_r256" (gemm6 by tile height), "gemm_reg_bn64" / "gemm_reg_bn128"
 * (every gemm.h launch by column-tile width, convolutions included);
 * and of the attention dispatcher, one per attn3 instance: "attn_bal8" (SIMD-balanced 8-wave, 9-stage ring), "attn_nw8_deep" /
 * "attn_nw8" (8 waves, 9- / 5-stage ring), "attn_nw6_deep" / "attn_nw6" (6 waves, shape-invariant mode only), "attn_nw4", plus
 * "attn_seg2" (every two-range launch, whatever its instance), and "dit_rows" (the summed audio rows M of every backbone forward);
 * "gemm3_thin" (the gemm3 launches, counted in "gemm3" too, that took the 32-row instance) and "time_table_builds" (sampler calls and
 * forwards that built the handle's time tables: a whole-grid sampler call on the time points of the handle's last build reuses them);
 * the audio calls' counters are named where each call is described;
 * name "reset" zeroes all of them (value may be NULL). */
int f5hip_get_counter(const char* name, int64_t* value);

/* ---------------------------------------------------------------- per-kernel unit ops ----------------- */
/* One production kernel each, fp32 device tensors in and out, through the same dispatcher the sampler uses (SURVEY section 8(b)-4:
 * "per-kernel ops for unit parity").  They allocate their operand planes per call: test / tooling entry points, not the hot path.
 *
 * f5hip_op_gemm: out = (act(A W^T + bias), rows with row_keep == 0 zeroed) * mul + res   -- nn.Linear + the fused epilogue of
 *   Attention.to_out / FeedForward (F/model/modules.py:324-328,441-447,566-571).
 *   a_dev [M][K], w_dev [N][K] (nn.Linear layout), bias_dev [N] | NULL, mul_dev [N] | NULL (AdaLN gate), res_dev [M][N] | NULL,
 *   row_keep_host uint8 [M] | NULL (host); prec 1 = bf16, 2 = split bf16 (bf16x3), 3 = fp16 operands, fp32 accumulate;
 *   act 0 none, 1 GELU(tanh), 2 GELU(erf), 3 Mish, 4 SiLU.  out_dev fp32 [M][N], or out16_dev: one fp16 plane [M][N] (the operand the
 *   next fp16 GEMM reads; saturates at +-65504).  iters > 0: also times `iters` launches with HIP events on `stream`, cycling through
 *   w_copies copies of the packed weights (a pool larger than the Infinity Cache makes them HBM-cold as in the real forward).
 *   bn: the column-tile width the call site asks for where the dispatcher picks the register-staged gemm.h kernel (bf16 / split-bf16
 *   operands, many tiles): 0 or 128 (the projection / FF1 call sites), or 64 (the residual and UNetT skip call sites); the other
 *   kernels ignore it. */
int f5hip_op_gemm(int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev, const float* bias_dev, int32_t prec,
                  int32_t act, const float* mul_dev, const float* res_dev, const uint8_t* row_keep_host, float* out_dev,
                  uint16_t* out16_dev, int32_t w_copies, int32_t iters, double* avg_us, void* stream, int32_t bn);
/* f5hip_op_gemm_rowmul: f5hip_op_gemm with the multiplier taken per ROW, out = ((A W^T + bias), rows with row_keep == 0 zeroed) *
 *   mul[row_mod[r]] + res -- the gated residual projections of a mixed-grid sampler call, whose rows sit at different time points.
 *   mul_dev points into a table fp32 [n_mod_rows][mod_ld] at a column offset (16-byte aligned; mod_ld >= N, mod_ld % 4 == 0): row r reads
 *   mul_dev + row_mod_host[r] * mod_ld .. + N.  row_mod_host int32 [M] (host).  These kernels are the (no activation, residual, fp32
 *   output) epilogue only: res_dev and out_dev are required.  Everything else as in f5hip_op_gemm. */
int f5hip_op_gemm_rowmul(int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev, const float* bias_dev, int32_t prec,
                         const float* mul_dev, const int32_t* row_mod_host, int32_t mod_ld, int32_t n_mod_rows, const float* res_dev,
                         const uint8_t* row_keep_host, float* out_dev, void* stream, int32_t bn);
/* f5hip_op_qkv: fused to_q | to_k | to_v projection with its epilogue: bias, rotary embedding on channels 0..63 (head 0, interleaved
 *   pairs) of q and k, q * log2(e) / 8 (the attention kernel's scores are base-2 exponents), V transposed (F/model/modules.py:409-426).  a_dev [M][D], w_dev [3 D][D], bias_dev [3 D], row_pos host
 *   int32 [M] (rotary position of every row, 0..4096); outputs fp16 (saturated): qk_dev [ceil128(M)][2 D], vt_dev [D][ceil128(M)] with the tokens of
 *   every aligned group of 16 in the order 0-3, 8-11, 4-7, 12-15 (the order the attention kernel's PV fragments read them in). */
int f5hip_op_qkv(int32_t M, int32_t D, const float* a_dev, const float* w_dev, const float* bias_dev, const int32_t* row_pos,
                 int32_t prec, uint16_t* qk_dev, uint16_t* vt_dev, int32_t iters, double* avg_us, void* stream);
/* f5hip_op_attention: softmax(q k^T / 8 + key-padding mask) v per (sequence, head), head dim 64 -- F.scaled_dot_product_attention with the
 *   reference's [b, 1, 1, n] key mask (F/model/modules.py:424-436).  q_dev / k_dev / v_dev / out_dev fp32 [sum(seq_len)][64 heads], sequences
 *   packed back to back; kv_len[i] <= seq_len[i] valid keys (NULL: all).  Operands are rounded to fp16 (saturated) like the QKV epilogue's outputs.
 *   impl must be 3 (the production kernel, attn3); any other value fails.  shape_invariant: the launch's attention arithmetic, as
 *   f5hip_set_attention_shape_invariant (1 / 0, or -1 = the process default).  out_format: what the kernel writes, read back into out_dev
 *   as fp32 -- 0 split-bf16 planes (hi + lo), 1 one fp16 plane (the blocks' fp16 GEMM mode), 2 the bf16 hi plane alone (bf16 GEMM mode). */
int f5hip_op_attention(int32_t n_seq, const int32_t* seq_len, const int32_t* kv_len, int32_t heads, const float* q_dev, const float* k_dev,
                       const float* v_dev, float* out_dev, int32_t impl, int32_t iters, double* avg_us, void* stream, int32_t shape_invariant,
                       int32_t out_format);
/* f5hip_op_joint_attention: the joint attention of the MMDiT blocks (JointAttnProcessor, F/model/modules.py:496-522): per sequence the
 *   queries and the keys are its audio rows followed by its text rows; only audio keys can be padding (x_kvlen[i] <= x_len[i] valid; NULL:
 *   all).  q_dev / k_dev / v_dev / out_dev fp32 [sum(x_len) + sum(c_len)][64 heads]: all audio frames sequence by sequence, then all
 *   text tokens sequence by sequence.  Operands are rounded to fp16 (saturated) like the QKV epilogue's outputs.  shape_invariant and
 *   out_format as in f5hip_op_attention. */
int f5hip_op_joint_attention(int32_t n_seq, const int32_t* x_len, const int32_t* x_kvlen, const int32_t* c_len, int32_t heads,
                             const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, void* stream, int32_t shape_invariant,
                             int32_t out_format);
/* f5hip_op_layernorm: y = LN(x) * (gain_off + scale) + shift (AdaLN: gain_off 1; affine LN: gain_off 0; F/model/modules.py:285-290),
 *   rms = 1: x-transformers RMSNorm y = x / max(|x|_2, 1e-12) * sqrt(D) * scale.  All fp32 [M][D] / [D]. */
int f5hip_op_layernorm(int32_t M, int32_t D, const float* x_dev, const float* scale_dev, const float* shift_dev, float gain_off, float eps,
                       int32_t rms, float* out_dev, void* stream);
/* f5hip_op_layernorm_planes: f5hip_op_layernorm (no RMSNorm) through the 16-bit outputs the GEMMs read: out_format 0 = split-bf16 planes
 *   (hi = bf16(y), lo = bf16(y - hi)), 1 = one fp16 plane (saturated); out_dev fp32 [M][D] receives hi + lo, or the fp16 values.
 *   row_mod_host NULL: scale_dev / shift_dev [D].  Else int32 [M] (host): row r takes its vectors from scale_dev / shift_dev +
 *   row_mod_host[r] * mod_ld, two column offsets (16-byte aligned) into one table fp32 [n_mod_rows][mod_ld], mod_ld >= D, mod_ld % 4 == 0
 *   -- the per-row AdaLN of a mixed-grid sampler call. */
int f5hip_op_layernorm_planes(int32_t M, int32_t D, const float* x_dev, const float* scale_dev, const float* shift_dev,
                              const int32_t* row_mod_host, int32_t mod_ld, int32_t n_mod_rows, float gain_off, float eps, int32_t out_format,
                              float* out_dev, void* stream);
/* f5hip_op_cfg_step: one launch of the sampler's CFG combine + ODE update (cfg_step_kernel), v = p_c + (p_c - p_u) cfg (v = p_c for a
 *   frame without an unconditional row), on the caller's buffers.  U frames of mel channels; pred_dev fp32 [rows][128] the backbone output, urow_c_host /
 *   urow_u_host int32 [U] (host) the conditional / unconditional row of every frame (urow_u -1: none).
 *   method 0: xout = xbase + dt v (xout_dev == xbase_dev: the Euler step in place; distinct: the midpoint rule's half step, xbase
 *   untouched); method 2: stage `stage` + 1 (stage 0..3) of the fixed-grid RK4 step (3/8 rule) in place on xbase_dev, stage slopes in
 *   k1_dev / k2_dev / k3_dev fp32 [U][mel]; method -1: no step (final select only).
 *   Strength: cfg, or cfg_frame_dev fp32 [U] per frame.  Step size: dt, or (frame_unit_host not NULL, with cfg_frame_dev) per unit --
 *   frame_unit_host int32 [U], unit_dt_host fp32 [n_units] (host) -- and the frames of units >= n_act are left as they are.
 *   xs_dev fp32 [rows][128]: the split-bf16 copy of x; it is split into planes, the launch writes split(x_next) at both rows of every
 *   frame it steps, and the planes come back as hi + lo.
 *   final_flags_host uint8 [U] (host) not NULL: then out_dev [U][mel] = flag ? cond_dev : xbase_dev, the sampler's final select. */
int f5hip_op_cfg_step(int32_t method, int32_t stage, int32_t U, int32_t mel, int32_t rows, float* xout_dev, float* xbase_dev,
                      const float* pred_dev, const int32_t* urow_c_host, const int32_t* urow_u_host, float cfg, const float* cfg_frame_dev,
                      float dt, const int32_t* frame_unit_host, const float* unit_dt_host, int32_t n_units, int32_t n_act, float* k1_dev,
                      float* k2_dev, float* k3_dev, float* xs_dev, const uint8_t* final_flags_host, const float* cond_dev, float* out_dev,
                      void* stream);
/* f5hip_op_cfg_mixed: one launch of the same kernel as a sampler call with per-unit grids or methods launches it (f5hip_cfm_sample_grids,
 *   _span, _methods), in which every frame is stepped by this forward's op of its unit.  Buffers as in f5hip_op_cfg_step (strengths per
 *   frame: cfg_frame_dev [U]; in place on xstate_dev).  frame_unit_host int32 [U]; unit_op_host int32 / unit_dt_host fp32 [n_units] (host): per unit the op code and step size --
 *   0 none (frame untouched), 1 Euler step, 2 midpoint half step (unit_dt holds dt / 2; xstate untouched, the next input goes to xs and
 *   to the frame's rows of k1_dev), 3 midpoint full step, 4..7 RK4 stage 1..4 (slopes in k1_dev / k2_dev / k3_dev [U][mel]).  The
 *   frames of units >= n_act are left as they are.  Per op code the result is f5hip_op_cfg_step's of that method / stage, bit for bit. */
int f5hip_op_cfg_mixed(int32_t U, int32_t mel, int32_t rows, float* xstate_dev, const float* pred_dev, const int32_t* urow_c_host,
                       const int32_t* urow_u_host, const float* cfg_frame_dev, const int32_t* frame_unit_host, const int32_t* unit_op_host,
                       const float* unit_dt_host, int32_t n_units, int32_t n_act, float* k1_dev, float* k2_dev, float* k3_dev, float* xs_dev,
                       void* stream);
/* f5hip_op_row_tp: the time point of every row of a mixed-grid call, row_tp_host[r] = unit_tp_host[row_unit_host[r]] (all host int32;
 *   R rows, n_units units), computed by the sampler's kernel. */
int f5hip_op_row_tp(int32_t R, const int32_t* row_unit_host, int32_t n_units, const int32_t* unit_tp_host, int32_t* row_tp_host,
                    void* stream);
/* f5hip_op_time_table: the per-call time precompute of a finalized handle over n_t <= 256 time points t_host (host), and what it leaves in
 *   the handle's tables: sinus_dev fp32 [n_t][256] = the sinusoid embedding as the time MLP reads it (split bf16, hi + lo); mod_dev fp32
 *   [n_t][mod_cols] = the AdaLN modulation rows (DiT / MMDiT; mod_cols must be the model's row width, 6 dim per block + 2 dim for DiT)
 *   or NULL; temb_dev fp32 [n_t][dim] = the time embeddings (UNetT) or NULL. */
int f5hip_op_time_table(f5hip_dit* m, const float* t_host, int32_t n_t, float* sinus_dev, float* mod_dev, int32_t mod_cols, float* temb_dev,
                        void* stream);
/* f5hip_op_conv1d: one nn.Conv1d(c_in, c_out, k, dilation = dil, padding = dil (k - 1) / 2) + bias + res of the BigVGAN generator (its
 *   AMPBlock1 convolutions: k 3 / 7 / 11, dilation 1 / 3 / 5) over channel-last rows: `batch` sequences of pitch P rows (P % 128 == 0), T valid,
 *   zero padding at the sequence bounds.  x_dev fp32 [batch P][c_in], w_host [c_out][c_in][k] (the module's weight layout), bias_host [c_out]
 *   or NULL, res_dev fp32 [batch P][c_out] or NULL, out_dev fp32 [batch P][c_out] (rows >= T of a sequence are unspecified).
 *   prec 2 = split bf16, 3 = one fp16 plane.  impl 0 = implicit GEMM (gemm.h), 5 = sliding-window kernel (conv5.h; fails if it does not
 *   cover the shape).  iters > 0: average microseconds per launch in *avg_us.  stamps_host (optional, impl 5): [stamp_blocks][16] cycle
 *   stamps of a diagnostics launch (layout: csrc/conv5.h). */
int f5hip_op_conv1d(int32_t batch, int32_t P, int32_t T, int32_t c_in, int32_t c_out, int32_t k, int32_t dil, const float* x_dev,
                    const float* w_host, const float* bias_host, const float* res_dev, float* out_dev, int32_t prec, int32_t impl,
                    int32_t iters, double* avg_us, uint64_t* stamps_host, int32_t stamp_blocks, void* stream);
/* f5hip_op_bigvgan_snake: the generator's Activation1d(SnakeBeta) (2x Kaiser-sinc up-sampling with replicate padding, x + sin^2(x e^alpha) /
 *   (e^beta + 1e-9), 2x low-pass down-sampling) over channel-last rows: `batch` sequences of pitch P rows, T valid (C % 4 == 0).  x_dev fp32
 *   [batch P][C], alpha_log_dev / beta_log_dev fp32 [C] (the log-scale parameters).  out_format: 0 = fp32, 1 = split-bf16 planes, 2 = one fp16
 *   plane (saturated); out_dev fp32 [out_rows][C] (out_rows >= batch P) receives the output as fp32.  Formats 1 / 2 run through planes
 *   of out_rows rows loaded from out_dev, so rows the kernel does not write (t >= T, and rows past batch P) come back rounded to the format. */
int f5hip_op_bigvgan_snake(int32_t batch, int32_t P, int32_t T, int32_t C, const float* x_dev, const float* alpha_log_dev,
                           const float* beta_log_dev, int32_t out_format, float* out_dev, int64_t out_rows, void* stream);
/* f5hip_op_bigvgan_upsample: one up-sampler of the generator, nn.ConvTranspose1d(c_in, c_out, 2 r, stride r, padding r / 2) + bias with
 *   r even, run as its 3-tap implicit GEMM (phase-major columns) by the generator's convolution dispatch.  x_dev fp32 [batch P][c_in]
 *   (P % 128 == 0, T valid, c_in % 4 == 0), w_host [c_in][c_out][2 r] (the module's weight layout), bias_host [c_out] or NULL; out_dev fp32
 *   [batch P r][c_out] (rows >= r T of a sequence are unspecified).  prec 2 = split bf16, 3 = one fp16 plane. */
int f5hip_op_bigvgan_upsample(int32_t batch, int32_t P, int32_t T, int32_t c_in, int32_t c_out, int32_t r, const float* x_dev,
                              const float* w_host, const float* bias_host, float* out_dev, int32_t prec, void* stream);
/* f5hip_op_bigvgan_conv_post: the generator's conv_post, nn.Conv1d(C, 1, 7, padding 3, no bias), then clamp(-1, 1).  a_dev fp32 [batch P][C]
 *   (T valid rows per sequence), w_dev fp32 [C][7] (device), wave_dev fp32 [batch][T].  variant 0 = the kernel the generator picks, 1 = the
 *   LDS-tiled kernel (fails when its tile exceeds 48 KB, C > 44), 2 = the kernel without the tile. */
int f5hip_op_bigvgan_conv_post(int32_t batch, int32_t P, int32_t T, int32_t C, const float* a_dev, const float* w_dev, int32_t variant,
                               float* wave_dev, void* stream);
/* Ragged forms of the four ops above: the layouts of f5hip_bigvgan_forward_ragged, in which every kernel of the generator finds an item's
 *   rows through a small table instead of a uniform pitch.  The caller describes the layout in rows of the stage the op runs at (host int32
 *   arrays of n_items entries); the op builds and uploads the kernel's table and launches as the generator does.  A layout the kernels'
 *   contracts exclude is refused (nothing is launched).
 * f5hip_op_conv1d_ragged: f5hip_op_conv1d over M rows (x_dev [M][c_in], res_dev / out_dev [M][c_out]) holding n_items items: item i owns
 *   rows [item_row0[i], + item_rows[i]), the first item_valid[i] of them valid (item_rows NULL: valid rounded up to the alignment below).
 *   The kernels read one [start, end) per block of blk rows (blk % 128 == 0, M % blk == 0).  Rules: every item starts at, and spans, a
 *   multiple of blk rows; no block belongs to two items or to none; 1 <= valid <= rows.  impl 5 (conv5.h) takes the bounds of a 256-row
 *   tile from the tile's first row, so there M % 256 == 0, blk is 128 or a multiple of 256, and with blk 128 every item starts at, and
 *   spans, a multiple of 256 rows.  ups_rate > 0: the 3-tap form of an up-sampler as in f5hip_op_bigvgan_upsample (w_host [c_in][c_out]
 *   [2 ups_rate], out_dev [M ups_rate][c_out], res_dev NULL; k and dil are not read).  impl 0 = gemm.h, 5 = conv5.h, never a fallback. */
int f5hip_op_conv1d_ragged(int32_t n_items, const int32_t* item_row0, const int32_t* item_rows, const int32_t* item_valid, int32_t M,
                           int32_t blk, int32_t c_in, int32_t c_out, int32_t k, int32_t dil, int32_t ups_rate, const float* x_dev,
                           const float* w_host, const float* bias_host, const float* res_dev, float* out_dev, int32_t prec, int32_t impl,
                           void* stream);
/* f5hip_op_bigvgan_snake_ragged: f5hip_op_bigvgan_snake over x_dev [M][C] with item i = rows [item_row0[i], + item_valid[i]) (grid z = item,
 *   the grid covers the longest item).  The kernel takes int4 items in first-stage rows and `scale` = the up-sampling so far: the op stores
 *   row0 / scale and valid / scale, so both must be multiples of scale (>= 1), and every item must lie inside the M rows.  n_items <= 65535.
 *   out_dev / out_rows (>= M) / out_format as in the uniform op: only the valid rows of the items are written. */
int f5hip_op_bigvgan_snake_ragged(int32_t n_items, const int32_t* item_row0, const int32_t* item_valid, int32_t scale, int32_t M, int32_t C,
                                  const float* x_dev, const float* alpha_log_dev, const float* beta_log_dev, int32_t out_format,
                                  float* out_dev, int64_t out_rows, void* stream);
/* f5hip_op_bigvgan_conv_post_ragged: f5hip_op_bigvgan_conv_post over a_dev [M][C] with items as above; item i writes samples
 *   [item_wave_off[i], + item_valid[i]) of wave_dev (wave_len samples; the op writes nothing else).  Offsets are multiples of scale too,
 *   and every item's samples lie inside wave_len; the order of the offsets is free. */
int f5hip_op_bigvgan_conv_post_ragged(int32_t n_items, const int32_t* item_row0, const int32_t* item_valid, const int32_t* item_wave_off,
                                      int32_t scale, int32_t M, int32_t C, const float* a_dev, const float* w_dev, int32_t variant,
                                      float* wave_dev, int64_t wave_len, void* stream);
/* f5hip_op_bigvgan_mean3: the generator's mean of the three AMP blocks of a stage, (y0 + y1 + y2) / 3 (n_in 3; n_in 1: the conversion of
 *   y0 alone), fp32 [rows][C] (C % 4 == 0).  out_f32_dev [rows][C] or NULL receives fp32 rows.  mode 0: nothing else (out_f32_dev required);
 *   1 / 2 / 3: split-bf16 planes / one fp16 plane (saturated) / the round-to-nearest bf16 hi plane, of pitch ldo >= C (ldo % 4 == 0).
 *   The planes are loaded from planes_dev fp32 [rows][ldo] and read back into it as fp32, so the padding channels c >= C come back as
 *   they were, up to the format's rounding. */
int f5hip_op_bigvgan_mean3(int64_t rows, int32_t C, int32_t n_in, const float* y0_dev, const float* y1_dev, const float* y2_dev, int32_t mode,
                           int32_t ldo, float* out_f32_dev, float* planes_dev, void* stream);
/* f5hip_op_bigvgan_mel_rows: the generator's first operand planes, mel -> rows of 128 channels (C = num_mels <= 128; rows past an item's
 *   frames and channels >= C are zero).  item_row0 NULL: n uniform sequences, mel_dev [n][C][T], pitch M0 / n >= T rows.  Else the ragged
 *   kernel: item i has item_frames[i] <= T frames from row item_row0[i] (a multiple of 128; it owns ceil128(frames) rows; every 128-row
 *   block of the M0 rows belongs to exactly one item), mel_dev [n][C][T] with T the column stride; columns past an item's frames are not
 *   read.  f16 0 = split bf16 (out = hi + lo), 1 = the fp16 plane (saturated).  out_dev fp32 [M0][128]. */
int f5hip_op_bigvgan_mel_rows(int32_t n, const int32_t* item_row0, const int32_t* item_frames, int32_t T, int32_t M0, int32_t C,
                              const float* mel_dev, int32_t f16, float* out_dev, void* stream);
/* f5hip_op_conv_pos_embed: the backbone's ConvPositionEmbedding, x + Mish(conv2(Mish(conv1(x)))) with two nn.Conv1d(D, D, 31, padding 15,
 *   groups 16), over n_seq sequences of seq_len[s] frames (zero padding at the sequence bounds) laid out as the backbone lays them out.
 *   x_dev fp32 [frames][D] (packed, D % 128 == 0, D <= 1024), w*_host [D][D / 16][31], b*_host [D].  lead = 1: a time-token row heads every
 *   sequence (UNetT).  impl 5 = conv5.h (prec 2, lead 0 only), 0 = gemm.h; prec 2 = split bf16, 1 = bf16.  pad_nan = 1: padding rows, time-token
 *   rows and the slack behind the last row of the internal buffers hold NaN instead of 0.  out_dev fp32 [frames][D]; c1_dev (or NULL) fp32
 *   [frames][D] receives stage 1 as the second convolution reads it (hi + lo planes, the hi plane alone at prec 1). */
int f5hip_op_conv_pos_embed(int32_t n_seq, const int32_t* seq_len, int32_t lead, int32_t D, const float* x_dev, const float* w1_host,
                            const float* b1_host, const float* w2_host, const float* b2_host, int32_t impl, int32_t prec, int32_t pad_nan,
                            float* out_dev, float* c1_dev, void* stream);
/* f5hip_op_convnext_block: one ConvNeXtV2 text block (depthwise conv k 7 + LayerNorm, pwconv1 + GELU, GRN over each sequence, pwconv2 +
 *   residual) as the backbone runs it, in split bf16, over n_seq sequences of seq_len[s] tokens.  x_dev fp32 [tokens][Td] (packed,
 *   Td % 32 == 0); params_host: 10 host fp32 arrays dwconv.weight, dwconv.bias, norm.weight, norm.bias, pwconv1.weight, pwconv1.bias,
 *   grn.gamma, grn.beta, pwconv2.weight, pwconv2.bias (module layouts).  pad_nan as above.  out_dev fp32 [tokens][Td]; each tap (or NULL)
 *   receives a stage as the next kernel reads it: tap_ln_dev [tokens][Td] dwconv + LayerNorm, tap_ty_dev [tokens][2 Td] pwconv1 + GELU,
 *   tap_grn_dev [tokens][2 Td] GRN. */
int f5hip_op_convnext_block(int32_t n_seq, const int32_t* seq_len, int32_t Td, const float* x_dev, const float* const* params_host,
                            int32_t pad_nan, float* out_dev, float* tap_ln_dev, float* tap_ty_dev, float* tap_grn_dev, void* stream);
/* f5hip_op_convnext_block_gx: the same, with one more tap: tap_gx_dev [n_seq][2 Td] (or NULL), the GRN column norms of every sequence. */
int f5hip_op_convnext_block_gx(int32_t n_seq, const int32_t* seq_len, int32_t Td, const float* x_dev, const float* const* params_host,
                               int32_t pad_nan, float* out_dev, float* tap_ln_dev, float* tap_ty_dev, float* tap_grn_dev, float* tap_gx_dev,
                               void* stream);

/* ---------------------------------------------------------------- Vocos vocoder ----------------------- */

typedef struct f5hip_vocos_config {
    int32_t in_channels, dim, intermediate_dim, num_layers, n_fft, hop_length;
    int32_t gemm_planes;
} f5hip_vocos_config;
typedef struct f5hip_vocos f5hip_vocos;

/* Replaces Vocos.from_hparams + load_state_dict (F/infer/utils_infer.py:104-115); names are vocos 0.1.0 keys
 * ("backbone.embed.weight", "backbone.convnext.0.dwconv.weight", ..., "head.out.weight"). */
f5hip_vocos* f5hip_vocos_create(const f5hip_vocos_config* cfg);
void f5hip_vocos_destroy(f5hip_vocos* v);
int f5hip_vocos_load_param(f5hip_vocos* v, const char* name, const float* data, int64_t numel);
int f5hip_vocos_finalize(f5hip_vocos* v);
/* Replaces vocoder.decode(mel) (F/infer/utils_infer.py:472): mel_dev fp32 [batch][in_channels][frames] ->
 * wave_dev fp32 [batch][hop_length * (frames - 1)]. */
int f5hip_vocos_decode(f5hip_vocos* v, int32_t batch, int32_t frames, const float* mel_dev, float* wave_dev,
                       void* stream);
/* vocoder.decode(mel) (F/infer/utils_infer.py:472) over n mels of their own lengths in ONE call: frames host int32 [n], each >= 2;
 * mel_dev fp32 [n][in_channels][T_max] (T_max = max frames[i]; item i valid for t < frames[i], the rest is not read) ->
 * wave_dev fp32 packed, item i at offset hop_length * sum_{j<i} (frames[j] - 1), hop_length * (frames[i] - 1) samples long.
 * Item i's wave equals f5hip_vocos_decode of that item alone, bit for bit. */
int f5hip_vocos_decode_ragged(f5hip_vocos* v, int32_t n, const int32_t* frames, const float* mel_dev, float* wave_dev,
                              void* stream);
/* Parity taps: f5hip_vocos_decode_ragged's own launch sequence (same arguments n, frames, mel_dev), stopped behind n_blocks ConvNeXt blocks, with
 * the valid rows of its workspace copied out packed, item after item without the 128-row padding of the library's row layout:
 *   n_blocks   0 .. num_layers: stop behind that many blocks (0: embed conv + backbone.norm only); -1: the whole decode
 *   x_dev      fp32 [sum frames][dim]: the residual stream where the call stopped (for -1 behind the last block, in front of the final norm)
 *   n_blocks = -1 also fills (they may be null otherwise, and are then left alone)
 *   y_dev      fp32 [sum frames][n_fft + 2]: the head output, log-magnitude | phase
 *   fw_dev     fp32 [sum frames][n_fft]: the windowed inverse-FFT frames in front of the overlap-add
 *   wave_dev   as f5hip_vocos_decode_ragged, and the same bits
 * n items of equal length give f5hip_vocos_decode's layout.  Refused before any launch: n_blocks outside -1 .. num_layers, a null pointer
 * among the buffers the call fills, an item of fewer than 2 frames. */
int f5hip_vocos_decode_taps(f5hip_vocos* v, int32_t n, const int32_t* frames, const float* mel_dev, int32_t n_blocks,
                            float* x_dev, float* y_dev, float* fw_dev, float* wave_dev, void* stream);

/* ---------------------------------------------------------------- BigVGAN vocoder --------------------- */

/* BigVGAN v2 generator hyper-parameters (config.json of nvidia/bigvgan_v2_24khz_100band_256x: F/infer/utils_infer.py:122-126).
 * Supported family: upsample_kernel_sizes[i] == 2 * upsample_rates[i] (even), resblock "1" with three kernel sizes x three
 * dilations, snakebeta with log-scale parameters, no tanh / no bias at the final conv. */
typedef struct f5hip_bigvgan_config {
    int32_t num_mels, num_upsamples;
    int32_t upsample_rates[8], upsample_kernel_sizes[8];
    int32_t upsample_initial_channel;
    int32_t resblock_kernel_sizes[3];
    int32_t resblock_dilations[9];   /* [kernel index][dilation index] */
    int32_t gemm_planes;             /* conv operand precision, fp32 accumulation: 2 = split bf16, three MFMAs per product (the parity
                                        mode: 1.5e-5 max on the waveform); 3 = one fp16 plane (fast mode, NOT within the 1e-4 parity
                                        bound: ~1e-3 max / 2e-4 rms measured); 1 = plain bf16 */
} f5hip_bigvgan_config;
typedef struct f5hip_bigvgan f5hip_bigvgan;

/* Replaces bigvgan.BigVGAN.from_pretrained + remove_weight_norm (F/infer/utils_infer.py:116-129); names are the generator's
 * state_dict keys after remove_weight_norm ("conv_pre.weight", "ups.0.0.weight", "resblocks.0.convs1.0.weight",
 * "resblocks.0.activations.0.act.alpha", ..., "activation_post.act.beta", "conv_post.weight"). */
f5hip_bigvgan* f5hip_bigvgan_create(const f5hip_bigvgan_config* cfg);
void f5hip_bigvgan_destroy(f5hip_bigvgan* v);
int f5hip_bigvgan_load_param(f5hip_bigvgan* v, const char* name, const float* data, int64_t numel);
int f5hip_bigvgan_finalize(f5hip_bigvgan* v);
/* Replaces vocoder(mel) (F/infer/utils_infer.py:474): mel_dev fp32 [batch][num_mels][frames] ->
 * wave_dev fp32 [batch][frames * prod(upsample_rates)] (the reference's [batch, 1, n] squeezed), clamped to [-1, 1]. */
int f5hip_bigvgan_forward(f5hip_bigvgan* v, int32_t batch, int32_t frames, const float* mel_dev, float* wave_dev, void* stream);
/* vocoder(mel) (F/infer/utils_infer.py:474, which the reference runs once per chunk) over n mels of their own lengths in ONE call:
 * frames host int32 [n], each >= 1; mel_dev fp32 [n][num_mels][T_max] (T_max = max frames[i]; item i valid for t < frames[i], the
 * rest is not read) -> wave_dev fp32 packed, item i at offset total_up * sum_{j<i} frames[j], total_up * frames[i] samples long
 * (total_up = prod(upsample_rates)).  Every stage is one launch for all items: the launch count does not depend on n.
 * Item i's wave equals f5hip_bigvgan_forward of that item alone, bit for bit.  The (small) length tables are copied on `stream`,
 * which the call waits for once before it launches. */
int f5hip_bigvgan_forward_ragged(f5hip_bigvgan* v, int32_t n, const int32_t* frames, const float* mel_dev, float* wave_dev,
                                 void* stream);

/* ---------------------------------------------------------------- mel front-end ------------------------ */

/* Replaces MelSpec.forward with mel_spec_type="vocos" (F/model/modules.py:75-101,130-143): wave_dev fp32
 * [batch][n_samples] -> mel_dev fp32 [batch][n_mels][1 + n_samples / hop] (log of clamp(mel, 1e-5)).
 * Accepted: n_fft = 1024, 1 <= hop_length <= n_fft, 1 <= n_mels <= 256, sample_rate >= 2, n_samples > n_fft / 2 (the BigVGAN variant below:
 * n_samples >= n_fft); anything else returns an error before a launch. */
int f5hip_mel_spectrogram(int32_t batch, int32_t n_samples, const float* wave_dev, float* mel_dev, int32_t n_fft,
                          int32_t hop_length, int32_t n_mels, int32_t sample_rate, void* stream);

/* Replaces MelSpec.forward with mel_spec_type="bigvgan" (get_bigvgan_mel_spectrogram, F/model/modules.py:30-72): reflect pad
 * (n_fft - hop) / 2, STFT center=False, sqrt(re^2 + im^2 + 1e-9), librosa Slaney mel filterbank (fmax = sr / 2),
 * log(clamp(., 1e-5)): wave_dev fp32 [batch][n_samples] -> mel_dev fp32 [batch][n_mels][1 + (n_samples - hop) / hop]. */
int f5hip_mel_spectrogram_bigvgan(int32_t batch, int32_t n_samples, const float* wave_dev, float* mel_dev, int32_t n_fft,
                                  int32_t hop_length, int32_t n_mels, int32_t sample_rate, void* stream);

/* Both mel front-ends for n clips of their own lengths in one launch: the reference mels of the new voices of a batch (a multi-voice script
 * brings several), straight from f5hip_ref_frontend's packed output.
 *   n_samples[i]           host, samples of clip i: > n_fft / 2 (variant 0), >= n_fft (variant 1), as in the two calls above
 *   wave_dev[i]            host array of device pointers: clip i's fp32 samples (4-byte aligned); the clips need not be contiguous
 *   mel_dev                fp32 [sum T][n_mels], frame-major and packed: clip i owns rows sum_{j<i} T_j .. + T_i, the layout the sampler's cond
 *                          has; T_i = 1 + n_samples[i] / hop (variant 0) or (n_samples[i] + 2 pad - n_fft) / hop + 1, pad = (n_fft - hop) / 2
 *   variant                0: f5hip_mel_spectrogram's front-end (vocos), 1: f5hip_mel_spectrogram_bigvgan's
 * Each clip is reflect-padded at its own bounds, and its rows equal its own single-clip call's (transposed) bit for bit: the same frame
 * code, FFT and filterbank summation order.  One launch whatever n (counters mel_ragged_launches, mel_ragged_items); the clip table is
 * copied on `stream`, which the call waits for once before it launches.
 * Refused before the launch: n < 1, a null pointer, a clip too short for its variant, an unknown variant, the geometry the calls above refuse. */
int f5hip_mel_spectrogram_ragged(int32_t n, const int32_t* n_samples, const float* const* wave_dev, float* mel_dev, int32_t n_fft, int32_t hop_length,
                                 int32_t n_mels, int32_t sample_rate, int32_t variant, void* stream);

/* ---------------------------------------------------------------- reference-audio front-end ------------ */

/* Prologue of infer_batch_process (F/infer/utils_infer.py:423-433) for n clips of one sample-rate pair, in one call:
 * mono mix (mean over channels), rms = sqrt(mean(x^2)) of the mono clip, gain x * rms_floor / rms when rms < rms_floor,
 * torchaudio.transforms.Resample(orig_freq, new_freq) (sinc_interp_hann, width 6, rolloff 0.99).
 *   n_in[i], channels[i]  host; clip i = channels[i] planes of n_in[i] fp32 samples (load_wav's layout), clips packed back to back in wave_dev
 *   taps_dev              fp32 [nf][2*width+of]: the table infer.resample_taps builds (the values resample_sinc_hann convolves with)
 *   out_dev               packed mono fp32; clip i holds n_out[i] = ceil(nf * n_in[i] / of) samples
 *   rms_dev               fp32 [n]: the measured rms BEFORE the gain (what the output path restores)
 * orig_freq == new_freq: no taps, out = the gained mono clip.
 * Two launches, no host sync between them (the length tables are copied on `stream`, which the call waits for once before it launches);
 * the sum of squares is accumulated in fp64 in a fixed order, so a clip's samples and rms do not depend on what else is in the call.
 * Refused before the first launch: n < 1, n_in[i] < 1, channels[i] < 1, a null table when the rates differ, sum(n_out) above 2^31 - 1. */
int f5hip_ref_frontend(int32_t n, const int32_t* n_in, const int32_t* channels, const float* wave_dev, int32_t orig_freq, int32_t new_freq,
                       const float* taps_dev, float rms_floor, float* out_dev, float* rms_dev, void* stream);

/* ---------------------------------------------------------------- waveform back-end ------------------ */

/* Tail of infer_batch_process (F/infer/utils_infer.py:485-519: the cross-fade join of a request's chunk waves) and
 * remove_silence_for_generated_wav (F/infer/utils_infer.py:530-539) for n requests in one call: chunk waves in, finished 16-bit PCM out.
 *   chunks_per_request[i]  host, >= 1; the chunks of all requests follow each other in chunk_dev / chunk_len, in request and chunk order
 *   chunk_dev[c]           host array of device pointers: chunk c's fp32 samples (4-byte aligned), the rms gain already applied
 *   chunk_len[c]           host, samples of chunk c (>= 1)
 *   fade                   cross-fade length in samples; 0: plain concatenation
 *   remove_silence[i]      host (or null: none), non-zero: pauses of 1 s or more below -50 dBFS are cut down to 500 ms on each side
 *   pcm_dev                int16, 16-byte aligned; request i starts at sum_{j<i} ((N_j + 7) & ~7) with N = sum(len) - (k - 1) fade joined samples
 *   len_dev                int32 [n]: the samples request i ends up with (N_i without silence removal)
 * Joined sample j is a chunk sample, or in a fade prev[len - F + t] * ramp[F - 1 - t] + next[t] * ramp[t] in fp64 (ramp = np.linspace(0, 1, F),
 * products and sum rounded one by one), rounded to fp32; the PCM is rint(x * 32768), half to even, clipped to [-32768, 32767].  With every
 * chunk at least 2 * fade samples long this equals the reference's nested cross-fade bit for bit; the silence rule is pydub's
 * split_on_silence(min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10) on integers.
 * One launch, three when a request asks for silence removal (counters wave_finish_launches, wave_finish_requests); the length tables are
 * copied on `stream`, which the call waits for once before it launches.  A request's samples do not depend on what else is in the call.
 * Refused before the first launch: n < 1, a request without chunks, an empty chunk, fade < 0, with fade > 0 a chunk shorter than 2 * fade
 * in a request of several chunks, sample_rate != 24000, more than 2^31 - 1 samples in or out. */
int f5hip_wave_finish(int32_t n, const int32_t* chunks_per_request, const float* const* chunk_dev, const int32_t* chunk_len, int32_t fade,
                      const uint8_t* remove_silence, int32_t sample_rate, int16_t* pcm_dev, int32_t* len_dev, void* stream);

/* f5hip_wave_finish with a choice per join: the pieces of a multi-voice script (F/infer/infer_cli.py:181-208) are cross-faded inside a
 * voice's piece and concatenated between pieces, so a request's chunks are joined as infer.join_segments joins them.
 *   chunk_fade[c]          host, one per chunk of the call (or null): non-zero: chunk c cross-fades into the chunk before it in its request over
 *                          `fade` samples; 0: it butts against it.  A request's first chunk is ignored.  A gap is a chunk that points at zeros.
 * Request i then has N = sum(len) - fade * (its fading joins) joined samples.  Everything else is f5hip_wave_finish's contract: the fade
 * arithmetic, the quantisation, the output offsets ((N_j + 7) & ~7), len_dev, the silence rule, one launch or three, the same counters, a
 * request's samples independent of the call.  With chunk_fade == null this IS f5hip_wave_finish (which is that call).
 * Refused before the first launch: what f5hip_wave_finish refuses (its 2 * fade rule only with chunk_fade == null), and with fade > 0 a chunk
 * shorter than (fade if it fades in) + (fade if its successor fades in): exactly where the host's nested cross-fade would take fewer than
 * `fade` samples or touch a sample twice.  With that the result equals infer.join_segments + quantise_pcm16 bit for bit. */
int f5hip_wave_finish_joins(int32_t n, const int32_t* chunks_per_request, const float* const* chunk_dev, const int32_t* chunk_len, int32_t fade,
                            const uint8_t* chunk_fade, const uint8_t* remove_silence, int32_t sample_rate, int16_t* pcm_dev, int32_t* len_dev,
                            void* stream);

/* The delivery format of n finished requests, in one call: their 24 kHz int16 PCM (f5hip_wave_finish's pcm_dev, still on the device) resampled
 * to new_freq and encoded.  Not in the reference, whose route always answers with 24 kHz PCM; the definition is infer.resample_pcm16 /
 * infer.encode_g711, which this call equals bit for bit.
 *   pcm_dev, in_off[i]     request i's samples start at pcm_dev + in_off[i] (host array, in samples; any sign: separate allocations work)
 *   max_len[i]             host, >= 0: an upper bound of request i's length, which sizes its blocks and its part of out_dev
 *   len_dev                device int32 [n] or null: the actual lengths (f5hip_wave_finish's len_dev; clamped to [0, max_len[i]]); null:
 *                          max_len
 *   new_freq               output rate; 24000: no resampling
 *   encoding               0: int16 PCM, 1: G.711 mu-law, 2: G.711 A-law (CPython's audioop.lin2ulaw / lin2alaw at width 2), one byte per sample
 *   taps_dev               fp32 [nf][2*width+of]: the table infer.resample_taps(24000, new_freq) builds; null when new_freq == 24000
 *   out_dev, out_off[i]    16-byte aligned; request i's samples / code bytes start at byte out_off[i] (host array, multiples of 16), its part
 *                          at least ceil(nf * max_len[i] / of) samples long
 *   out_len_dev            int32 [n]: ceil(nf * len_i / of), the samples request i ends up with
 * Output j = q nf + p is rint(sum_k (double)taps[p][k] * (double)xpad[q of + k]), k ascending, half to even, clipped to [-32768, 32767], with
 * xpad the request's samples between zeros (`width` in front): integer samples times fp32 taps are exact in fp64, so the sum has the bits of
 * numpy's multiply-then-add.  One launch whatever n (counters wave_encode_launches, wave_encode_requests), no atomics, a request's bytes
 * depend on that request alone; the request table is copied on `stream`, which the call waits for once before it launches.
 * Refused before the launch: n < 1, a null pointer (len_dev and, at 24000, taps_dev excepted), an unknown encoding, a null table when the
 * rates differ, a negative max_len, a misaligned pointer or output offset, more than 2^31 - 1 samples in or out, a rate whose window and tap
 * table do not fit the LDS together (the seven rates of infer.OUTPUT_SAMPLE_RATES all fit). */
int f5hip_wave_encode(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, int32_t new_freq,
                      int32_t encoding, const float* taps_dev, uint8_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream);

/* Input samples one block of f5hip_wave_encode owns at new_freq (a whole number of polyphase blocks); 0 for a rate it refuses.  For tests,
 * which place request lengths around it. */
int f5hip_wave_encode_tile(int32_t new_freq);

/* Lossless delivery: the int16 PCM of n requests at the delivery rate, still on the device (f5hip_wave_finish's pcm_dev, or the output of
 * f5hip_wave_encode with encoding 0 when the rate is not 24000), -> each request's complete native FLAC stream (RFC 9639), byte for byte
 * infer.encode_flac of its samples.  Not in the reference.  The format, with no freedom left:
 *   stream     "fLaC", one STREAMINFO block (last-block flag, length 34): min = max block size 4096, the true min / max frame size and total
 *              sample count, MD5 zero ("not computed"); 42 bytes, alone for an empty request (total 0, frame sizes 0); then the frames
 *   frame      mono, 16 bits, fixed block size 4096 (sync 0xFFF8, the frame number coded; block-size code 1100, for the short last frame 0111
 *              with a 16-bit b - 1), the rate's code, CRC-8; one subframe, no wasted bits; zero padding to a byte; CRC-16
 *   subframe   CONSTANT when all samples of the block are equal; else the fixed-predictor order o in 0..4, o < b, with the fewest bits (ties:
 *              the lower order); VERBATIM only when strictly smaller than that
 *   residual   coding method 00, never the escape code; partition order 4 for a full block and 0 for the short last one; per partition the
 *              Rice parameter k in 0..14 that minimises sum(u >> k) + n (1 + k) (ties: the smaller k), u = 2 r for r >= 0, else -2 r - 1
 *   pcm_dev, in_off[i], max_len[i], len_dev    as in f5hip_wave_encode
 *   sample_rate            one of 8000, 16000, 22050, 24000, 32000, 44100, 48000: only the streams' rate fields depend on it
 *   out_dev, out_off[i]    16-byte aligned; request i's stream starts at byte out_off[i] (host array, multiples of 16), its part at least
 *                          f5hip_wave_flac_bound(max_len[i]) bytes long
 *   out_len_dev            int32 [n]: the bytes of request i's stream
 * At most three launches whatever n (frames into a fixed-stride scratch buffer; a scan of the frame sizes per request, which writes the
 * stream header; the frames packed behind it), no host sync between them (counters wave_flac_launches, wave_flac_requests); a request's
 * bytes depend on that request alone; the request table is copied on `stream`, which the call waits for once before it launches.
 * Refused before the first launch: n < 1, a null pointer (len_dev excepted), a rate outside the table, a negative max_len, a misaligned
 * pointer or output offset, more than 2^31 - 1 samples in or bytes out. */
int f5hip_wave_flac(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, int32_t sample_rate,
                    uint8_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream);

/* f5hip_wave_flac with a FLAC level per request: byte for byte wave_codec.encode_flac(samples, sample_rate, level[i]).  Not in the reference.
 *   level                  host int32 [n], each 0 or 1; NULL: all 0, which is f5hip_wave_flac (the same kernels, launches and counters)
 * Level 0 is the format above.  Level 1 adds LPC subframes to the candidates of every full block of 4096 that is not constant; the short
 * last block, the headers, the CONSTANT test, coding method 00, partition order 4 and the Rice parameter rule stay.  The candidates in
 * order are FIXED 0 .. 4, then LPC order 6, 8, 10, 12 (precision 12), made so:
 *   window     w[i] = (32768 (4095^2 - (2 i - 4095)^2)) / 4095^2 in integers; xw[i] = (x[i] w[i]) >> 15
 *   autocorr   R[j] = sum_{i >= j} xw[i] xw[i - j], j in 0 .. 12, exact in int64; R[0] == 0: no LPC candidates
 *   Levinson   fp64, every step one correctly rounded operation in the written order, nothing fused: err = R[0]; for m = 1 .. 12:
 *              acc = R[m]; acc = acc - a[j] * R[m-1-j] for j = 0 .. m-2; k = acc / err; a'[j] = a[j] - k * a[m-2-j], a'[m-1] = k;
 *              err = err * (1.0 - k * k); !(err > 0): order m and every higher order are no candidates
 *   quantise   e = frexp(max |a[j]|)'s exponent (0 for 0), shift = min(11 - e, 15), negative: no candidate; q[j] = clip(rint(a[j] 2^shift),
 *              -2048, 2047), half to even
 *   residual   r[i] = x[i] - ((sum_j q[j] x[i-1-j]) >> shift), the sum inside int32; an order with any zigzag u >= 2^21 is no candidate
 *              (every partition sum then stays below 2^29)
 *   bits       8 + 16 o + 4 + 5 + 12 o + 2 + 4 + sum over partitions (4 + S_k); the fewest bits win, ties to the earlier candidate, VERBATIM
 *              only when strictly smaller -- so a level-1 frame is never larger than the level-0 frame and f5hip_wave_flac_bound holds
 *   on wire    subframe header (0x20 | (o - 1)) << 1, o warm-up samples, 0b1011, the shift in 5 bits, o coefficients of 12 bits, the residual
 * A call in which no request asks for level 1 launches the level-0 kernel; otherwise one kernel serves both levels, block by block.  Three
 * launches and no host sync either way.  Refused before the first launch, beside f5hip_wave_flac's list: a level outside {0, 1}. */
int f5hip_wave_flac_levels(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                           int32_t sample_rate, const int32_t* level, uint8_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream);

/* Upper bound of the bytes of a stream of max_len samples: 42 + 2 max_len + 16 ceil(max_len / 4096) (no frame is larger than its samples as
 * VERBATIM plus 16 bytes); 0 for a negative length. */
int64_t f5hip_wave_flac_bound(int32_t max_len);

/* Loudness target: the 24 kHz int16 PCM of n requests, still on the device (f5hip_wave_finish's pcm_dev), moved IN PLACE to each flagged
 * request's programme loudness (ITU-R BS.1770-4, mono), bit for bit wave_codec.normalise_loudness_pcm16.  Not in the reference.  It runs
 * behind f5hip_wave_finish and before f5hip_wave_encode / f5hip_wave_flac.  The arithmetic, integers up to one sqrt:
 *   K-weighting  y[j] = sum_k h[k] x[j - k], zeros in front; h = 1024 integer taps, rint(2^16 k_true[k]) of the two K-weighting biquads designed
 *                for 24 kHz (csrc/loudness_taps.inc = wave_codec.loudness_taps(); sum |h| = 212 915, so |y| < 2^33); z[j] = y[j] >> 14, floor
 *   sub-blocks   e[s] = sum of z^2 over the 2400 samples of sub-block s (< 2^50); only whole sub-blocks count
 *   blocks       E[b] = (e[b] + e[b+1] + e[b+2] + e[b+3]) >> 8: 400 ms, 75 % overlap, floor(len / 2400) - 3 of them
 *   gates        E[b] > 75535 = floor(10^((-70 + 0.691) / 10) 9600 2^26); then E[b] > floor(S1 / (10 n1)) over the blocks that pass the first;
 *                n2, S2 = count and sum of the blocks that pass both (int64: exact for any request below 2^31 samples)
 *   gain         g = sqrt(K_T n2 / S2), then min(g, 29203 / peak) with peak = max |x| (a sample-peak ceiling of -1 dBFS); x <- clip(rint(x g)),
 *                half to even: int -> fp64, *, /, sqrt, /, min, *, rint, one correctly rounded fp64 operation each.  n2 == 0 (shorter than
 *                400 ms, or nothing above the gates): g = 1 and the samples are not written
 *   pcm_dev, in_off[i], max_len[i], len_dev    as in f5hip_wave_encode, pcm_dev writable
 *   gain_k                 host double [n]: K_T = 10^((target + 0.691) / 10) 9600 2^26 of request i's target in LUFS; <= 0: the request is left
 *                          alone (neither its samples nor its stats row are written)
 *   stats_dev              int64 [n][4], 8-byte aligned: n2, S2, peak, the bits of g, for each flagged request
 * Three launches whatever n (the K-weighting FIR in exact fp64 FMAs with the sub-block sums and tile peaks; one workgroup per flagged request
 * for the gates and g; the gain), none when no request is flagged, no host sync between them (counters wave_loudness_launches,
 * wave_loudness_requests); no atomics, vector stores; a request's bytes depend on that request alone, and neither an unflagged request nor
 * the bytes between requests are written; the request table is copied on `stream`, which the call waits for once before it launches.
 * Refused before the first launch: n < 1, a null pointer (len_dev excepted), a negative max_len or offset, a misaligned pointer, a
 * non-finite gain_k, more than 2^31 - 1 samples. */
int f5hip_wave_loudness(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, const double* gain_k,
                        int64_t* stats_dev, void* stream);

/* Samples one block of f5hip_wave_loudness's first launch owns (two sub-blocks).  For tests, which place request lengths around it. */
int f5hip_wave_loudness_tile(void);

/* Prosody: the 24 kHz int16 PCM of n requests, still on the device (f5hip_wave_finish's pcm_dev), time-scale modified per request -- its
 * `tempo` and `pitch` --, bit for bit wave_codec.shift_pcm16.  Not in the reference.  It runs behind f5hip_wave_finish and before
 * f5hip_wave_loudness / f5hip_wave_encode / f5hip_wave_flac, which read its output, bounds and lengths as they read f5hip_wave_finish's.  The
 * arithmetic, integers up to the resampler's exact fp64 sums (csrc/wave_prosody_core.h, which tools/wave_prosody_check.cpp runs on the CPU
 * under sanitizers):
 *   WSOLA        n samples -> m = ceil(n P / Q) at the same pitch.  L = 960, H = 480, D = 240; xt[j] = x[j] inside the request, else 0;
 *                K = ceil(m / H) + 1 frames, nominal starts p_k = floor(k H Q / P) - H (64-bit products), s_0 = -H; for k >= 1, with
 *                t = s_{k-1} + H: c(d) = sum_{i < L} |xt[p_k + d + i] - xt[t + i]| (< 2^26), d_k = the d in -D .. D that minimises it, ties
 *                to the smaller |d|, then to the negative one; s_k = p_k + d_k
 *   window       W[i] = rint(32768 sin^2(pi (2 i + 1) / (2 L))) for i < H (csrc/wsola_window.inc = wave_codec.wsola_window()), W[H + i] =
 *                32768 - W[i]
 *   output       y[j] = (W[H + i] xt[s_k + H + i] + W[i] xt[s_{k+1} + i] + 16384) >> 15, a floor shift, k = j / H, i = j - k H; the
 *                numerator stays within 2^30 + 2^14 and y inside int16: no clip.  P == Q: the samples themselves
 *   pitch        s semitones, s != 0: the m samples -> ceil(q m / p) by f5hip_wave_encode's polyphase arithmetic with the pair p : q in the
 *                place of 24000 : new_freq (output j = b q + r is rint(sum_k (double)taps[r][k] * (double)ypad[b p + k]), half to even,
 *                clipped); p / q = 18/17, 46/41, 44/37, 29/23, 4/3, 41/29 for s = 1 .. 6, the reciprocal for -s.  The caller has chosen
 *                P / Q = (p / q) / tempo, so the duration is the tempo's alone
 *   pcm_dev, in_off[i], max_len[i], len_dev    as in f5hip_wave_encode
 *   stretch_p, stretch_q   host int32 [n]: P and Q of request i, 1 .. 2^20 each, 1/2 <= P / Q <= 2
 *   pitch                  host int32 [n]: -6 .. 6
 *   taps_dev               fp32, 16-byte aligned: the twelve tables wave_codec.resample_taps(p, q) of s = -6 .. -1, 1 .. 6, table s at float
 *                          f5hip_wave_prosody_tap_offset(s); may be null when no request has a pitch
 *   out_dev, out_off[i]    int16, 16-byte aligned: request i's samples at out_dev + out_off[i] (a multiple of 8), room for the length that
 *                          max_len[i] gives
 *   out_len_dev            int32 [n]: its samples
 * Two launches whatever n, one when no request has a pitch (wave_wsola_kernel: one workgroup per request, frames in sequence, the 481
 * candidates of a frame across the workgroup as packed 16-bit absolute differences, ONE min-reduction over the key cost * 2^9 + tie rank, so
 * the choice cannot depend on lane order; wave_pitch_kernel: one block per tile of a pitched request, which reads the stretched PCM from the
 * call's workspace), no host sync between them (counters wave_prosody_launches, wave_prosody_requests: the requests with P != Q or a pitch);
 * no atomics, vector stores; a request's bytes depend on that request alone, and the input is not written; the request table is copied on
 * `stream`, which the call waits for once before it launches.
 * Refused before the first launch: n < 1, a null pointer (len_dev excepted, and taps_dev without a pitch), a negative max_len or offset, a
 * misaligned pointer or output offset, P or Q < 1, a stretch outside [1/2, 2] or with a term above 2^20, a pitch outside -6 .. 6, more than
 * 2^31 - 1 samples in or out. */
int f5hip_wave_prosody(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                       const int32_t* stretch_p, const int32_t* stretch_q, const int32_t* pitch, const float* taps_dev, int16_t* out_dev,
                       const int64_t* out_off, int32_t* out_len_dev, void* stream);

/* First float of pitch step s's tap table in f5hip_wave_prosody's taps_dev (tables in the order -6 .. -1, 1 .. 6, each padded to a multiple
 * of 4 floats); s = 0: the floats of the whole table; -1 for a step outside -6 .. 6. */
int64_t f5hip_wave_prosody_tap_offset(int32_t pitch);

/* f5hip_wave_prosody with a per-request `keep_formants`: a flagged request's fundamental moves by its pitch step while its spectral envelope
 * stays (time-domain pitch-synchronous overlap-add), bit for bit wave_codec.shift_pcm16(..., keep_formants=True) = wsola_pcm16 by the
 * request's (P, Q) -- the caller passes the tempo's stretch alone, reduce(100, T) -- and then wave_codec.psola_pcm16, whose definition is
 * written down above wave_codec.psola_window (csrc/wave_formant_core.h holds its rules; tools/wave_formant_check.cpp runs them on the CPU
 * under sanitizers).  Integers only.  On the m = ceil(n P / Q) stretched samples x, xt = x inside the request and 0 elsewhere:
 *   track        frame f at t = 120 f, ceil(m / 120) frames: d[l] = sum_{i < 480} |xt[t + i] - xt[t + l + i]|, l = 48 .. 400, E = sum_{i < 480}
 *                |xt[t + i]|; lag = the smallest l with 8 d[l] <= 8 dmin + E, then upwards while d[l + 1] < d[l]; voiced iff E >= 30720 and
 *                2 d[lag] <= E
 *   marks        one chain from t = 0 while t < m, in the frame t / 120.  Unvoiced: a = t, T = 120.  Voiced, T = lag: a = the position of the
 *                largest sample in [t, t + T) after an unvoiced mark or first, in [max(t - T / 8, a_prev + 24), t + T / 8] after a voiced
 *                one; inside the wave, ties to the earlier position.  t = a + T
 *   synthesis    u_0 = a_0; u takes the nearest analysis mark i, ties to the earlier; voiced: u += (T_i q + rem) / p, rem = (T_i q + rem) % p
 *                (p / q as in f5hip_wave_prosody); unvoiced: u += 120; while u < m
 *   output       over the marks with |j - u| <= T_i: w = M[(|j - u| 1024) / T_i] (csrc/psola_window.inc = wave_codec.psola_window()), num +=
 *                w xt[a_i + j - u], den += w; y[j] = clip(floor((2 num + den) / (2 den))), y[j] = x[j] where den = 0.  m samples
 *   keep_formants   host uint8 [n]: non-zero flags request i, which must have a pitch; every other argument as in f5hip_wave_prosody
 * A call without a flagged request launches what f5hip_wave_prosody launches.  Otherwise THREE more launches whatever n
 * (f5hip_wave_prosody_formants_launches), behind the WSOLA launch, which leaves the flagged requests' stretched samples in the workspace
 * (wave_period_kernel: one block per tile of 5 frames of a flagged request, its 1360 samples in LDS biased by 32768 and twice, one sample
 * apart, the 5 x 354 sums across the threads as packed 16-bit absolute differences, two min-reductions per frame; wave_marks_kernel: one
 * wavefront per flagged request chains the analysis marks, the peak search across the lanes by a keyed maximum, and hands out the synthesis
 * marks as it goes, the counts stay on the device; wave_psola_kernel: one block per 2048 outputs, the at most 87 marks around the tile by
 * binary search, 8 samples a thread in a 16-byte store); the resampler launch only when another request has a plain pitch.  No atomics, no
 * accumulator buffer, no host sync; a request's bytes depend on that request alone (counters wave_formant_launches, wave_formant_requests).
 * Refused before the first launch: what f5hip_wave_prosody refuses, a null keep_formants, a flagged request without a pitch. */
int f5hip_wave_prosody_formants(int32_t n, const int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev,
                                const int32_t* stretch_p, const int32_t* stretch_q, const int32_t* pitch, const uint8_t* keep_formants,
                                const float* taps_dev, int16_t* out_dev, const int64_t* out_off, int32_t* out_len_dev, void* stream);

/* Launches f5hip_wave_prosody_formants adds for a call with a flagged request (3).  For tests. */
int f5hip_wave_prosody_formants_launches(void);

/* FLAC in: n native FLAC streams (RFC 9639) -- uploaded reference clips and recordings, which the reference reads with torchaudio.load
 * (F/infer/utils_infer.py:376) -- packed at arbitrary byte offsets in one device buffer -> each stream's samples as int32 planes
 * [channels, total], bit for bit wave_codec.read_flac, which defines the format accepted: every subframe type, LPC order 1 .. 32, both Rice
 * methods with escapes, every stereo mode, fixed and variable blocking; both CRCs of every frame, every reserved code, the numbering, block
 * sizes, sample size, rate and channel count against STREAMINFO, samples inside their bit depth, residuals inside 32 bits, the total.  The
 * caller parses the metadata (STREAMINFO, where the frames begin), applies the cap on the declared length and checks the MD5 afterwards.
 *   data_dev, nbytes       the packed buffer; no alignment is asked of it or of the streams in it
 *   begin[i], end[i]       stream i's frames are bytes [begin[i], end[i]) (host arrays): ascending, not overlapping
 *   info                   host int32 [n][8]: channels, bits, rate, STREAMINFO's min and max block size (0: not named), cap (samples per channel
 *                          its output has room for: f5hip_flac_decode_bound), needs_host (non-zero: do not decode it), 0
 *   total[i]               STREAMINFO's total samples, 0: unknown;  max_samples[i]: the most the stream may decode to
 *   out_dev, out_off[i]    int32: channel c of stream i at out_dev + out_off[i] + c * cap
 *   status_dev             int32 [n][2]: status (0 decoded; 1 refused; 2 needs the host; 3 both were found) and the samples per channel
 * The device takes 1 .. 2 channels, 8 .. 24 bits and block sizes up to 16 384; a stream outside that has status 2 before any launch, and a
 * stream whose frames outrun the slot pool, the record table or its output gets it on the way.  The caller decodes every stream whose status
 * is not 0 with the host definition, which either returns its samples or raises: a refusal's text never comes from the device.
 * FIVE launches whatever n (scan: one thread per byte offset finds candidate frame headers; offsets: candidate ids and slot addresses by prefix
 * sums; frame: one wavefront per candidate, false ones included; chain: one wave per stream follows end offset -> next frame from the first
 * byte, so a false sync is never visited; pack: stereo reconstruction into the output), no host sync between them (counters
 * flac_decode_launches, flac_decode_streams); nothing depends on the order of atomics; every read is bounded by the stream's end and every
 * write by the candidate's slot (csrc/flac_in_core.h, which tools/flac_in_check.cpp runs on the CPU under sanitizers); the stream table is
 * copied on `stream`, which the call waits for once before it launches.
 * Refused before the first launch: n < 1, a null pointer, nbytes outside 1 .. 2^31 - 1025, streams that overlap or leave the buffer, a
 * STREAMINFO field out of range, a misaligned output. */
int f5hip_flac_decode(int32_t n, const uint8_t* data_dev, int64_t nbytes, const int64_t* begin, const int64_t* end, const int32_t* info,
                      const int64_t* total, const int64_t* max_samples, int32_t* out_dev, const int64_t* out_off, int32_t* status_dev, void* stream);

/* Samples per channel a stream's output needs: STREAMINFO's total or, when it names none, 2 * stream_bytes + 16 384 (a stream that packs more
 * into its bytes gets status 2); never more than 64 * stream_bytes + 16 384, so that memory stays in proportion to the upload whatever
 * STREAMINFO declares, and never more than max_samples. */
int64_t f5hip_flac_decode_bound(int64_t total, int64_t stream_bytes, int64_t max_samples);

/* The reference-clip pre-step (F/infer/utils_infer.py:282-350 between reading the clip and writing the temporary WAV) for n uploaded clips
 * of ONE sample rate in one call, bit for bit audio_prep.preprocess_ref_segment: clip at a pause (windows of 1000 ms below -50 dBFS, else of
 * 100 ms below -40 dBFS, kept silence 1000 ms, seek step 10 ms, the "more than 6 s so far and more than 15 s with this chunk" stop, overlapping
 * padded ranges split at their midpoint, else a hard cut at 15 000 ms), strip the silent edges (-42 dBFS: leading in 10 ms windows, trailing
 * millisecond by millisecond with the reference's running subtraction), append 50 ms of silence.
 *   n_in[i], channels[i]   host; clip i = n_in[i] frames (0 is valid) of channels[i] interleaved int16 samples, clips packed back to back
 *   clip_short[i]          host; zero: the clip is not clipped at a pause (edges and tail only)
 *   frames_dev, n_samples  the packed int16 samples and their count, which must equal sum(n_in * channels)
 *   out_dev                fp32, room for f5hip_ref_prestep_bound samples: clip i as channels[i] planes of its output length, x / 32768,
 *                          the clips packed back to back by their OUTPUT lengths -- f5hip_ref_frontend's `wave_dev` as it stands
 *   info_dev               int32 [n][2]: the output frames of clip i (its 50 ms tail included) and whether any output sample is non-zero
 * Every rms comparison is made on exact int64 sums of squares (rms = floor(sqrt(S / n)) >= r  <=>  S >= r^2 n for the thresholds 104, 328
 * and 261 and fewer than 2^23 samples per window); fp64 appears only in the frame of a millisecond, the length in milliseconds and the
 * running subtraction, each a single IEEE operation as on the host (csrc/ref_prestep_core.h, which tools/ref_prestep_check.cpp runs on the
 * CPU under sanitizers).  THREE launches whatever n and whatever the clips hold (cells: the sum of squares of every millisecond; rule: one
 * block per clip -- prefix sums, both parameter sets, the choice, the hard cut, the edges; gather: ranges to planar fp32, tail, flag), no
 * host synchronisation once its workspace has grown to the call's size: the clip table goes through pinned staging on `stream` (counters
 * ref_prestep_launches, ref_prestep_clips).  Clip i's output equals its own single-clip call's bit for bit.
 * Refused before the first launch: n < 1, rate < 11 025, a negative frame count, channels[i] < 1, rate x channels[i] >= 2^23, counts that
 * do not add up to n_samples, more than 2^31 - 1 samples in or out, a null pointer. */
int f5hip_ref_prestep(int32_t n, const int32_t* n_in, const int32_t* channels, const uint8_t* clip_short, const int16_t* frames_dev, int64_t n_samples,
                      int32_t rate, float* out_dev, int32_t* info_dev, void* stream);

/* Samples out_dev needs: sum((n_in[i] + 50 ms of frames) * channels[i]); -1 for arguments f5hip_ref_prestep refuses. */
int64_t f5hip_ref_prestep_bound(int32_t n, const int32_t* n_in, const int32_t* channels, int32_t rate);

/* The per-voice denoiser of uploaded reference clips for n clips in one call, IN PLACE on mono 24 kHz fp32 samples (f5hip_ref_frontend's
 * packed output): audio_prep.denoise_reference in fp32 -- quantile-based noise estimation (Stahl, Fischer, Bippus 2000) with power spectral
 * subtraction.  F = ceil((len + 768) / 256) frames of 1024 samples at hop 256 under w[i] = sin(pi i / 1024), frame m = samples
 * 256 m - 768 .. 256 m + 255 (zeros outside the clip); P = |rfft|^2; floor[k] = the ((F - 1) / 5)-th smallest of the clip's P[.][k], no
 * interpolation; S = the mean of P over the 3 x 3 cells around (m, k), indices clamped; G = max(1/8, (S - 6.75 floor[k]) / S), 1/8 where
 * S = 0; out = overlap_add(irfft(G X) w) / 2.  The length is kept, a silent clip stays silent.
 *   offset[i], n_samples[i]   host; clip i is n_samples[i] samples at wave_dev + offset[i]; the ranges are disjoint and need not be adjacent:
 *                             samples between them and clips left out of the table are not touched
 *   wave_dev                  fp32, read and written
 * FOUR launches whatever n (stft: one block per frame row of the packed batch, X float2 [rows][513], P [rows][516]; floor: the exact order
 * statistic of the device's own P, bit by bit over the float's bit pattern, integer counts; gain: S, G, the Hermitian fill and the inverse
 * transform, times w / 1024; ola: one thread per sample, its four frames in ascending order, halved), no host synchronisation once its
 * workspace has grown to the call's size: the clip table goes through pinned staging on `stream` (counters ref_denoise_launches,
 * ref_denoise_clips; geometry csrc/ref_denoise_core.h, which tools/ref_denoise_check.cpp walks on the CPU under sanitizers).  Clip i's
 * output equals its own single-clip call's bit for bit.
 * Refused before the first launch: n < 1, a length below 1 or above 1 440 000 (60 s), a negative offset, overlapping ranges, a null pointer,
 * more than 2^31 - 1 frame rows. */
int f5hip_ref_denoise(int32_t n, const int64_t* offset, const int32_t* n_samples, float* wave_dev, void* stream);

/* Provenance watermark, embedding: the 24 kHz int16 PCM of n requests, still on the device (f5hip_wave_finish's or f5hip_wave_prosody's
 * buffer), IN PLACE, with the mark of each flagged request's key added -- bit for bit wave_codec.mark_pcm16.  Not in the reference.  It runs
 * behind f5hip_wave_prosody and before f5hip_wave_loudness / f5hip_wave_encode / f5hip_wave_flac, which read the marked samples.  The
 * arithmetic is integers only (csrc/wave_mark_core.h, which tools/wave_mark_check.cpp runs on the CPU under sanitizers):
 *   carrier      c [16384] int16 of a key (f5hip_watermark_carrier): its SplitMix64 chips through the 129 band taps of
 *                csrc/watermark_taps.inc, circularly, >> 3
 *   block sums   A[b] = sum |x[j]| over block b of 240 samples of the request (the last one may be partial): below 2^23
 *   envelope     E[b] = max(A[b-1], A[b], A[b+1]), a missing neighbour counting 0
 *   output       y[j] = clip(x[j] + ((E[j / 240] c[j mod 16384]) >> 23), -32768, 32767): a 64-bit product, a floor shift; |y - x| < 4066
 *   pcm_dev, in_off[i], max_len[i], len_dev    as in f5hip_wave_loudness: samples past a request's device length are not read or written
 *   key_index      host int32 [n]: the row of carriers_dev for request i, or -1 to leave the request alone
 *   carriers_dev   int16 [n_keys][16384], 16-byte aligned; may be null when no request is flagged
 *   n_keys         0 .. 16
 * TWO launches whatever n, none when no request is flagged (wave_mark_sum_kernel: one block per tile of 32 x 240 samples, the block sums into
 * the call's workspace; wave_mark_add_kernel: one block per tile, 8 samples per 16-byte load and store), no host synchronisation once the
 * workspace has grown to the call's size: the request table goes through pinned staging on `stream` (counters wave_mark_launches,
 * wave_mark_requests: the flagged requests); no atomics, vector stores; a request's bytes depend on that request alone; unflagged requests
 * and the bytes between requests are not written.
 * Refused before the first launch: n < 1, a null pointer (len_dev excepted, and carriers_dev when nobody is flagged), a negative max_len or
 * offset, misaligned samples, lengths or carriers, n_keys outside 0 .. 16, a key_index outside -1 .. n_keys - 1, more than 2^31 - 1
 * samples. */
int f5hip_wave_mark(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, const int32_t* key_index,
                    const int16_t* carriers_dev, int32_t n_keys, void* stream);

/* Samples one block of f5hip_wave_mark's second launch owns (32 blocks of 240).  For tests, which place request lengths around it. */
int f5hip_wave_mark_tile(void);

/* The carrier of a key (1 .. 2^48 - 1) into carrier [16384] on the HOST: wave_codec.watermark_carrier(key), what a row of carriers_dev
 * holds.  No device work.  Refused: a null pointer, a key outside the range. */
int f5hip_watermark_carrier(uint64_t key, int16_t* carrier);

/* Provenance watermark, detection: n mono 24 kHz fp32 clips of their own lengths scored against each of n_keys carriers in one call --
 * wave_codec.detect_watermark in fp32.  Per clip: F = ceil((len + 768) / 256) frames of 1024 samples at hop 256 under w[i] = sin(pi i /
 * 1024) (f5hip_ref_denoise's framing and FFT); U[k] = X[k] / sqrt(|X[k]|^2 + 1e-10) for bins 22 .. 136, 0 elsewhere; u = overlap_add(irfft(U)
 * w) over the clip; Z[m] = sum of u[j] over j = m mod 16384; r[o] = sum_m Z[m] c[(m + o) mod 16384]; o* = the smallest argmax of r;
 * z = (r[o*] - mean r) / (population deviation of r), 0 where that is 0.  A clip below 12 000 samples scores zeros.
 *   wave_dev                  fp32, read only
 *   offset[i], n_samples[i]   host; clip i is n_samples[i] samples at wave_dev + offset[i], disjoint ranges
 *   carriers_dev              int16 [n_keys][16384], 16-byte aligned (f5hip_watermark_carrier)
 *   scores_dev                fp32 [n][n_keys][4]: z, o*, r[o*], the deviation.  detected is z >= 7.0
 * FOUR launches whatever n and n_keys (f5hip_watermark_detect_launches; frame: one block per frame row, forward FFT, unit-modulus band,
 * Hermitian fill, inverse FFT, times w / 1024; fold: one thread per (clip, residue), samples and their four frames in ascending order;
 * correlate: one block per (4 clips, key, 512 offsets), the clips' Z and the carrier window staged in LDS, residues ascending from 0;
 * score: one block per (clip, key), fixed trees, moments in fp64), no host synchronisation once the workspace has grown to the call's size
 * (counters watermark_detect_launches, watermark_detect_clips).  Every sum runs in an order fixed by the clip alone: clip i's row equals
 * its own single-clip call's bit for bit.
 * Refused before the first launch: n < 1, n_keys outside 1 .. 16, a length below 1 or above 1 440 000 (60 s), a negative offset,
 * overlapping ranges, a null or misaligned pointer, more than 2^31 - 1 frame rows. */
int f5hip_watermark_detect(int32_t n, const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int32_t n_keys,
                           const int16_t* carriers_dev, float* scores_dev, void* stream);

/* Kernels one f5hip_watermark_detect call launches (4). */
int f5hip_watermark_detect_launches(void);

/* Provenance watermark with trace ids, embedding: f5hip_wave_mark for requests whose mark also carries a 30-bit id -- bit for bit
 * wave_codec.mark_pcm16 of a WatermarkTag(key, id).  Not in the reference.  The id is three symbols of 10 bits, s_d = (id >> 10 d) & 1023,
 * each the rotation by 16 s_d samples of the carrier of one of the key's three sub-keys (wave_codec.watermark_subkey: ordinary keys, their
 * carriers by f5hip_watermark_carrier) relative to the key's own (code-shift keying):
 *   combined     C[m] = 2 c_K[m] + sum_d c_d[(m - 16 s_d) mod 16384]: |C| <= 5 * 4336
 *   output       y[j] = clip(x[j] + ((E[j / 240] C[j mod 16384]) >> 24), -32768, 32767), A and E as f5hip_wave_mark's: |y - x| <= 10163.
 *                Without an id the sum over d is absent and (2 c E) >> 24 == (c E) >> 23: f5hip_wave_mark's bytes
 *   pcm_dev, in_off, max_len, len_dev, key_index   as f5hip_wave_mark's
 *   id             host int32 [n]: -1, or the request's id, 0 .. 2^30 - 1
 *   carriers_dev   int16 [n_keys][4][16384], 16-byte aligned: per key its own carrier, then its sub-keys' 0 .. 2
 *   n_keys         0 .. 16
 * TWO launches whatever n: wave_mark_sum_kernel, then wave_mark_id_add_kernel with wave_mark_add_kernel's tile geometry: per group of 8
 * samples one 16-byte load of x and of the key's row and, for a request with an id, three of the rotated sub-key rows (rotations are
 * multiples of 16 samples, so a group keeps its 16-byte alignment in all four rows and never straddles the wrap); unaligned requests and
 * tails sample by sample; no atomics, vector stores; unflagged requests and the bytes between requests are not written (counters
 * wave_mark_id_launches, wave_mark_id_requests: the flagged requests).  A call in which nobody has an id runs f5hip_wave_mark's two kernels
 * and counts on its counters.
 * Refused before the first launch: what f5hip_wave_mark refuses, a null id, an id outside -1 .. 2^30 - 1, an id on a request whose
 * key_index is -1. */
int f5hip_wave_mark_ids(int32_t n, int16_t* pcm_dev, const int64_t* in_off, const int32_t* max_len, const int32_t* len_dev, const int32_t* key_index,
                        const int32_t* id, const int16_t* carriers_dev, int32_t n_keys, void* stream);

/* Provenance watermark with trace ids, reading: f5hip_watermark_detect, and per (clip, key) the three symbols of the id its mark carries --
 * wave_codec.read_watermark in fp32.  Z, r_K, o* and z as f5hip_watermark_detect's; r_d = the correlation of Z with sub-key d's carrier by the
 * same formula; candidate s takes r_d[(o* - 16 s) mod 16384]; s_d = the smallest argmax over s = 0 .. 1023; z_d = (r_d there - mean r_d) /
 * (population deviation of r_d), 0 where that is 0.  The id (sum_d s_d << 10 d) stands when z >= 7.0 and every z_d >= 6.0
 * (ops.watermark_reads decides).  A clip below 12 000 samples gets zeros.
 *   wave_dev, offset, n_samples   as f5hip_watermark_detect's
 *   n_keys                    1 .. 4
 *   carriers_dev              int16 [n_keys][4][16384], 16-byte aligned: f5hip_wave_mark_ids' layout
 *   rows_dev                  fp32 [n][n_keys][10]: z, o*, r[o*], the deviation -- f5hip_watermark_detect's row of that clip and key bit
 *                             for bit --, then s_0, z_0, s_1, z_1, s_2, z_2
 * FOUR launches whatever n and n_keys (f5hip_watermark_read_ids_launches): f5hip_watermark_detect's frame, fold and correlate kernels over
 * the 4 n_keys rows, then watermark_id_score_kernel, one block per (clip, key): the key's row by the detector's fixed trees and fp64 moments,
 * each sub-key's row the same way with the maximum over its 1024 candidates, ties to the smaller symbol (counters
 * watermark_read_ids_launches, watermark_read_ids_clips).  A clip's rows are bit-identical alone, in any batch and in any order; the
 * input is never written.
 * Refused before the first launch: what f5hip_watermark_detect refuses, with n_keys outside 1 .. 4. */
int f5hip_watermark_read_ids(int32_t n, const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int32_t n_keys,
                             const int16_t* carriers_dev, float* rows_dev, void* stream);

/* Kernels one f5hip_watermark_read_ids call launches (4). */
int f5hip_watermark_read_ids_launches(void);

/* Provenance watermark, the scan of ONE long or spliced recording: f5hip_watermark_detect's (with_ids = 0) or f5hip_watermark_read_ids'
 * (with_ids = 1) row for any number of ranges of the recording -- the device half of wave_codec.scan_watermark, where the definition is
 * written down.  Not in the reference.  The recording's n_samples samples are S = ceil(n_samples / 16384) segments of 16384, the last one
 * zero-filled; range i is segments first_segment[i] .. first_segment[i] + n_segments[i] - 1.  u = the whitened band of the WHOLE recording
 * (f5hip_watermark_detect's framing: 768 zeros in front, frames of 1024 at hop 256); a range's row is Z[m] = sum over its segments s,
 * ascending, of u[16384 s + m] -- the fold of those samples by their absolute index, so a reported offset refers to sample 0 of the
 * recording --, then correlated and scored as a clip's Z is.  A range that holds fewer than 12 000 of the recording's samples
 * (min(n_samples, (first + count) 16384) - first 16384) gets zeros.
 *   wave_dev                  fp32 [n_samples], mono 24 kHz, 4-byte aligned, read only; n_samples 1 .. 14 400 000 (600 s)
 *   first_segment, n_segments host int32 [n_ranges], n_ranges 1 .. 4096: 0 <= first, 1 <= count, first + count <= S; ranges may overlap,
 *                             repeat and come in any order
 *   with_ids = 0              carriers_dev int16 [n_keys][16384], n_keys 1 .. 16; rows_dev fp32 [n_ranges][n_keys][4]: f5hip_watermark_detect's row
 *   with_ids = 1              carriers_dev int16 [n_keys][4][16384] (f5hip_wave_mark_ids' layout), n_keys 1 .. 4; rows_dev fp32
 *                             [n_ranges][n_keys][10]: f5hip_watermark_read_ids' row, its first four words the with_ids = 0 row bit for bit
 * Launches: wd_frame_kernel once over the ceil((n_samples + 768) / 256) frames of the recording; ws_range_fold_kernel once, one thread per
 * (range, residue): the range's segments ascending, each sample's four frames ascending, as f5hip_watermark_detect folds a clip (a range of
 * all S segments of a recording of at most 1 440 000 samples gives that call's row bit for bit); then the detector's correlate kernel and
 * wd_score_kernel / watermark_id_score_kernel once per SLAB of ranges.  With R = n_keys (4 n_keys with ids) carrier rows a slab is
 * floor(4096 / R) ranges, taken in the call's order, so a call launches 2 + 2 ceil(n_ranges / floor(4096 / R)) kernels -- a function of
 * (n_ranges, n_keys, with_ids) alone, FOUR whenever n_ranges R <= 4096 (f5hip_watermark_scan_launches; f5hip_watermark_scan_slabs gives the
 * slab count): every window of 600 s against four keys is one slab, against sixteen keys four.  Every sum runs in an order fixed by the range
 * alone, so a range's rows are bit-identical alone, with any other ranges, in any order of ranges and whichever slab they fall in.
 * Workspace (the detector's buffers, grown and kept): frames 4 KiB per frame (230 MB at 600 s), Z 64 KiB per range (at most 256 MiB), r 64 KiB
 * per (range of a slab, carrier row) and never more than 4096 rows (256 MiB): below 0.8 GiB at every admitted size, by construction.
 * Counters watermark_scan_launches, watermark_scan_ranges.  The input is never written.
 * Refused before the first launch: n_samples outside 1 .. 14 400 000; n_ranges outside 1 .. 4096; a range that is empty or not inside the
 * S segments; with_ids other than 0 and 1; n_keys outside 1 .. 16 (1 .. 4 with ids); a null pointer; carriers not 16-byte aligned, samples
 * or rows not 4-byte aligned. */
int f5hip_watermark_scan(const float* wave_dev, int64_t n_samples, int32_t n_ranges, const int32_t* first_segment, const int32_t* n_segments,
                         int32_t n_keys, int32_t with_ids, const int16_t* carriers_dev, float* rows_dev, void* stream);

/* Kernels an f5hip_watermark_scan call of one slab launches (4); a call of s slabs launches 2 + 2 s. */
int f5hip_watermark_scan_launches(void);

/* Slabs of an f5hip_watermark_scan call: ceil(n_ranges / floor(4096 / R)), R = n_keys or 4 n_keys with ids; -1 for a bad argument. */
int f5hip_watermark_scan_slabs(int32_t n_ranges, int32_t n_keys, int32_t with_ids);

/* Reference-clip report: is an uploaded clip fit to clone from?  The measures of audio_prep.assess_reference (the definition, written down
 * above it) for n clips in one call, on the two buffers a front-end call holds.  Not in the reference.
 *   raw_dev                   fp32, read only: the packed raw clips as f5hip_ref_frontend is handed them; clip i is channels[i] channels of
 *                             raw_len[i] samples, channel after channel, at raw_dev + raw_offset[i] (host tables; disjoint ranges)
 *   wave_dev                  fp32, read only: f5hip_ref_frontend's packed output (mono, 24 kHz); clip i is n_samples[i] samples at
 *                             wave_dev + offset[i] (host tables; disjoint ranges): the caller passes min(length, 1 440 000)
 *   rows_dev                  int64 [n][10], 8-byte aligned: clipped, the bit pattern of peak (fp32), the speech frames, k* (-1: an all-zero
 *                             clip), then as fp64 bit patterns N, S, noise_db, snr_db, speech_ratio, bandwidth_hz
 * peak = max |x| of the raw clip; a sample is hot when |x| >= peak * (1 - 2^-10) in fp32; clipped = the hot samples in runs of at least 3
 * within one channel, 0 when peak < 0.25 or every sample is hot.  The spectrum is f5hip_ref_denoise's framing, P and floor (its stft and floor
 * kernels, launched as they stand); over bins 3 .. 341: E[f] = sum_k P[f][k], N = -1 / ln(0.8) * sum_k floor[k], S = mean_f E[f];
 * noise_db = 10 log10 N; snr_db = 10 log10(max(S - N, 0) / N); speech_ratio = the share of frames with E >= 4 N and > 0; m[k] = the mean
 * over frames of the mean of P[f][k .. k + 7]; k* = the largest k with m[k] >= 1e-5 max m; bandwidth_hz = (k* + 8) * 24000 / 1024.
 * peak and the counts are exact (integer atomics, order-free); the sums over frames run in fp64 in an order fixed by the clip alone (E in
 * ascending frame order; m over tiles of 16 frame rows, rows and tiles ascending).
 * SIX launches whatever n (f5hip_ref_assess_launches: peak, runs, stft, floor, frame sums per tile of 16 rows, per clip) behind one memset of the n accumulator
 * cells, no host synchronisation once the workspace has grown to the call's size (counters ref_assess_launches, ref_assess_clips; geometry
 * and run rule csrc/ref_assess_core.h, which tools/ref_assess_check.cpp runs on the CPU under sanitizers).  Clip i's row depends on clip i
 * alone: it equals its own single-clip call's bit for bit.
 * Refused before the first launch: n outside 1 .. 4096, channels outside 1 .. 8, a length below 1, a prepared length above 1 440 000, more
 * than 2^31 - 1 raw samples in a clip, a negative offset, overlapping ranges on either side, a null or misaligned pointer, more than
 * 2^31 - 1 frame rows. */
int f5hip_ref_assess(int32_t n, const float* raw_dev, const int64_t* raw_offset, const int32_t* channels, const int32_t* raw_len,
                     const float* wave_dev, const int64_t* offset, const int32_t* n_samples, int64_t* rows_dev, void* stream);

/* Kernels one f5hip_ref_assess call launches (6). */
int f5hip_ref_assess_launches(void);

#ifdef __cplusplus
}
#endif
#endif /* F5HIP_H */

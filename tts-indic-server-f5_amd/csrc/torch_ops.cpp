// TORCH_LIBRARY registration of the hot path (north_star: "host Python calling HIP through PyTorch-ROCm custom ops"): thin operators over the
// C ABI of libf5hip (include/f5hip.h) -- torch tensors in, torch tensors out, the current HIP stream of the tensors' device, errors as
// c10::Error.  Handles are the opaque pointers the *_create functions of the ABI return, carried as int64.  Host C++ only (no kernels here):
// built by build.py into csrc/libf5hip_torch.so next to libf5hip.so, loaded with torch.ops.load_library (tts_indic_server_f5_amd/torch_ops.py).
//   torch.ops.f5hip.cfm_sample(handle, dur, kv_len?, cond, cond_mask, text, y0, t_grid, cfg_strength) -> Tensor   F/model/cfm.py:160-204
//   torch.ops.f5hip.cfm_sample_units(handle, dur, kv_len?, cond, cond_mask, text, y0, t_grid, cfg_strength) -> Tensor  (one strength per unit)
//   torch.ops.f5hip.cfm_sample_grids(handle, dur, kv_len?, cond, cond_mask, text, y0, steps, t_grids, cfg_strength) -> Tensor  (one grid per unit)
//   torch.ops.f5hip.cfm_sample_span(handle, dur, kv_len?, cond, cond_mask, text, y0, steps, t_grids, cfg_strength, last) -> Tensor  (resumable span)
//   torch.ops.f5hip.cfm_sample_methods(handle, dur, kv_len?, cond, cond_mask, text, y0, steps, t_grids, cfg_strength, method, last?) -> Tensor  (one ODE method per unit)
//   torch.ops.f5hip.vocos_decode(handle, mel) -> Tensor                                                          F/infer/utils_infer.py:472
//   torch.ops.f5hip.vocos_decode_ragged(handle, mel, frames, channels, hop_length) -> Tensor (packed)                F/infer/utils_infer.py:472
//   torch.ops.f5hip.bigvgan_forward(handle, mel, total_upsample) -> Tensor                                       F/infer/utils_infer.py:474
//   torch.ops.f5hip.bigvgan_forward_ragged(handle, mel, frames, channels, total_upsample) -> Tensor (packed)         F/infer/utils_infer.py:474
//   torch.ops.f5hip.ref_frontend(wave, n_in, channels, orig_freq, new_freq, taps?, rms_floor) -> (Tensor packed, Tensor rms)   F/infer/utils_infer.py:423-433
//   torch.ops.f5hip.wave_finish(chunks[], chunks_per_request, fade, remove_silence, sample_rate) -> (Tensor pcm int16, Tensor lengths int32)   F/infer/utils_infer.py:485-519,530-539
//   torch.ops.f5hip.wave_finish_joins(chunks[], chunks_per_request, fade, chunk_fade, remove_silence, sample_rate) -> (Tensor pcm int16, Tensor lengths int32)   F/infer/infer_cli.py:181-208
//   torch.ops.f5hip.mel_spectrogram_ragged(waves[], n_fft, hop_length, n_mels, sample_rate, variant) -> Tensor mel [sum T, n_mels]   F/model/modules.py:30-143
//   torch.ops.f5hip.wave_encode(pcm[], in_off, max_len, len_dev?, new_freq, encoding, taps?) -> (Tensor bytes uint8, Tensor lengths int32, Tensor offsets int64 host)
//   torch.ops.f5hip.wave_flac(pcm[], in_off, max_len, len_dev?, sample_rate) -> (Tensor streams uint8, Tensor lengths int32, Tensor offsets int64 host)
//   torch.ops.f5hip.wave_flac_levels(pcm[], in_off, max_len, len_dev?, sample_rate, level int32 host) -> the same, each request at its FLAC level
//   torch.ops.f5hip.flac_decode(data, begin, end, info, total, max_samples) -> (Tensor statuses and planes int32, Tensor offsets int64 host)
//   torch.ops.f5hip.ref_prestep(frames, n_in, channels, clip_short, rate) -> (Tensor planes fp32, Tensor info int32 [n, 2])   F/infer/utils_infer.py:282-350
//   torch.ops.f5hip.wave_loudness(pcm, in_off, max_len, len_dev?, gain_k) -> Tensor stats int64 [n, 4]; pcm is normalised in place
//   torch.ops.f5hip.wave_prosody(pcm, in_off, max_len, len_dev?, stretch_p, stretch_q, pitch, taps?) -> (Tensor pcm int16, Tensor lengths int32, Tensor offsets int64 host, Tensor bounds int32 host)
//   torch.ops.f5hip.wave_prosody_formants(pcm, in_off, max_len, len_dev?, stretch_p, stretch_q, pitch, keep_formants, taps?) -> the same four
//   torch.ops.f5hip.ref_denoise(wave, offset, n_samples) -> ()   the flagged clips of wave (f5hip_ref_frontend's packed output) are denoised in place
//   torch.ops.f5hip.wave_mark(pcm, in_off, max_len, len_dev?, key_index, carriers?) -> ()   the flagged requests of pcm get their key's provenance mark in place
//   torch.ops.f5hip.ref_assess(raw, raw_offset, channels, raw_len, wave, offset, n_samples) -> Tensor rows int64 [n, 10]: the reference-clip report
//   torch.ops.f5hip.watermark_detect(wave, offset, n_samples, carriers) -> Tensor scores fp32 [n, n_keys, 4]: z, offset, r at the offset, the deviation
//   torch.ops.f5hip.wave_mark_ids(pcm, in_off, max_len, len_dev?, key_index, id, carriers?) -> ()   wave_mark whose marks also carry each request's trace id
//   torch.ops.f5hip.watermark_read_ids(wave, offset, n_samples, carriers) -> Tensor rows fp32 [n, n_keys, 10]: watermark_detect's four, then (s_d, z_d) x 3
//   torch.ops.f5hip.watermark_scan(wave, first_segment, n_segments, carriers) -> Tensor rows fp32 [n_ranges, n_keys, 4 or 10]: segment ranges of ONE recording
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <tuple>
#include <vector>

#include "../../include/f5hip.h"
#include "rate_pair.h"
#include "wave_prosody_core.h"
#include "wave_mark_core.h"
#include "ref_denoise_core.h"
#include "ref_assess_core.h"

namespace {

void* stream_of(const at::Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check_dev_f32(const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), "f5hip: ", name, " must be a contiguous fp32 tensor on the HIP device");
}
void check_host(const at::Tensor& t, at::ScalarType ty, const char* name) {
    TORCH_CHECK(!t.is_cuda() && t.scalar_type() == ty && t.is_contiguous(), "f5hip: ", name, " must be a contiguous host tensor of the documented dtype");
}
template <class T>
const T* opt_ptr(const c10::optional<at::Tensor>& t) { return t.has_value() ? t->data_ptr<T>() : nullptr; }

// ---- the steps the audio operators share (ops.py holds the same helpers for the ctypes binding); `op` names the operator in the messages

// The request table (pcm, in_off, max_len, len_dev) of the wave operators, checked: in_off [n] int64 host, max_len [n] int32 host; pcm one
// contiguous 1-D int16 device tensor that holds every request or, where the operator allows `several`, one per request on one device;
// len_dev None or [n] int32 on that device
struct PcmRequests {
    int64_t n;
    const int64_t* io;
    const int32_t* ml;
    const int32_t* len_dev;   // or null
    c10::Device device;
};
PcmRequests check_pcm_requests(const char* op, at::TensorList pcm, const at::Tensor& in_off, const at::Tensor& max_len, const c10::optional<at::Tensor>& len_dev,
                               bool several) {
    check_host(in_off, at::kLong, "in_off"); check_host(max_len, at::kInt, "max_len");
    const int64_t n = max_len.numel();
    TORCH_CHECK(max_len.dim() == 1 && n > 0 && in_off.numel() == n, "f5hip::", op, ": in_off and max_len need one value per request");
    TORCH_CHECK(pcm.size() == 1 || (several && (int64_t)pcm.size() == n), "f5hip::", op, ": pcm is one tensor", several ? " or one per request" : "", " (got ",
                pcm.size(), " for ", n, ")");
    for (const at::Tensor& t : pcm)
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kShort && t.is_contiguous() && t.dim() == 1 && t.device() == pcm[0].device(), "f5hip::", op,
                    ": pcm must be contiguous 1-D int16 tensors on one HIP device");
    if (len_dev.has_value())
        TORCH_CHECK(len_dev->is_cuda() && len_dev->scalar_type() == at::kInt && len_dev->is_contiguous() && len_dev->numel() == n &&
                    len_dev->device() == pcm[0].device(), "f5hip::", op, ": len_dev must be a contiguous int32 tensor with one value per request on the pcm's device");
    return {n, in_off.data_ptr<int64_t>(), max_len.data_ptr<int32_t>(), opt_ptr<int32_t>(len_dev), pcm[0].device()};
}

// Where a request table is read from: request i reads samples [io[i], io[i] + ml[i]) of its tensor (the one tensor, or tensor i), which must
// hold them.  anchor: the first tensor that has an address -- the library's `pcm` --, rel[i]: request i's first sample relative to it
struct PcmSources {
    at::Tensor anchor;
    std::vector<int64_t> rel;
    int16_t* base() const { return anchor.data_ptr<int16_t>(); }
};
PcmSources pcm_sources(const char* op, at::TensorList pcm, const PcmRequests& rq) {
    PcmSources s{at::Tensor(), std::vector<int64_t>(rq.n)};
    for (const at::Tensor& t : pcm)
        if (t.numel() && !s.anchor.defined()) s.anchor = t;
    if (!s.anchor.defined()) s.anchor = at::zeros({8}, pcm[0].options());
    for (int64_t i = 0; i < rq.n; i++) {
        const at::Tensor& t = pcm[pcm.size() == 1 ? 0 : i];
        TORCH_CHECK(rq.ml[i] >= 0 && rq.io[i] >= 0 && rq.io[i] + rq.ml[i] <= t.numel(), "f5hip::", op, ": request ", i, " reads samples [", rq.io[i], ", ",
                    rq.io[i] + rq.ml[i], ") of a tensor of ", t.numel());
        s.rel[i] = rq.ml[i] ? (t.data_ptr<int16_t>() - s.base()) + rq.io[i] : 0;   // (an empty tensor has no address to speak of)
    }
    return s;
}

// A Tensor[] argument the library reads through a pointer table: every `what` a contiguous 1-D fp32 tensor on the first one's device (views
// of a packed buffer as they are).  The length rules are the caller's
struct PointerTable {
    std::vector<const float*> ptrs;
    std::vector<int32_t> lens;
};
PointerTable pointer_table(const char* op, at::TensorList tensors, const char* what) {
    PointerTable tb{std::vector<const float*>(tensors.size()), std::vector<int32_t>(tensors.size())};
    for (size_t i = 0; i < tensors.size(); i++) {
        const at::Tensor& t = tensors[i];
        check_dev_f32(t, what);
        TORCH_CHECK(t.dim() == 1 && t.numel() <= INT32_MAX && t.device() == tensors[0].device(), "f5hip::", op, ": ", what, " ", i,
                    " must be a 1-D tensor on the first ", what, "'s device");
        tb.ptrs[i] = t.data_ptr<float>(); tb.lens[i] = (int32_t)t.numel();
    }
    return tb;
}

// The arguments of the ragged vocoder operators: mel [n, channels, T_max] fp32 device, frames [n] int32 host with min_frames <= frames[i] <= T_max.
// Returns sum(frames)
int64_t check_ragged_frames(const char* op, const at::Tensor& mel, const at::Tensor& frames, int64_t channels, int64_t min_frames) {
    check_dev_f32(mel, "mel"); check_host(frames, at::kInt, "frames");
    TORCH_CHECK(mel.dim() == 3 && mel.size(1) == channels, "f5hip::", op, ": mel [n, ", channels, ", T_max]");
    TORCH_CHECK(frames.dim() == 1 && frames.numel() == mel.size(0) && frames.numel() > 0, "f5hip::", op, ": frames.numel() == mel.size(0)");
    const int32_t* f = frames.data_ptr<int32_t>();
    int64_t sum = 0;
    for (int64_t i = 0; i < frames.numel(); i++) {
        TORCH_CHECK(f[i] >= min_frames && f[i] <= mel.size(2), "f5hip::", op, ": frames[", i, "] = ", f[i], " outside [", min_frames, ", mel.size(2) = ", mel.size(2), "]");
        sum += f[i];
    }
    return sum;
}

// The ODE loop of CFM.sample over packed rows: dur [b] int32 host (rows laid out per item), kv_len [b] int32 host or None (valid frames per item:
// the reference's padded-batch semantics), cond [sum(dur), mel] fp32 device, cond_mask [sum(dur)] uint8 host, text [b, nt] int32 host (-1 padded),
// y0 [sum(dur), mel] fp32 device.  The three sampler operators differ in the time grid and the CFG strength only.
struct SampleArgs {
    const at::Tensor &dur, &cond, &cond_mask, &text, &y0;
    const c10::optional<at::Tensor>& kv_len;
    const int32_t* kv() const { return opt_ptr<int32_t>(kv_len); }
};

// The checks the sampler operators share; `op` names the operator in the messages
void check_sample_args(const char* op, const SampleArgs& a) {
    check_host(a.dur, at::kInt, "dur"); check_host(a.cond_mask, at::kByte, "cond_mask"); check_host(a.text, at::kInt, "text");
    check_dev_f32(a.cond, "cond"); check_dev_f32(a.y0, "y0");
    TORCH_CHECK(a.text.dim() == 2 && a.text.size(0) == a.dur.numel() && a.cond.sizes() == a.y0.sizes(), "f5hip::", op, ": shapes");
    if (a.kv_len.has_value()) {
        check_host(*a.kv_len, at::kInt, "kv_len");
        TORCH_CHECK(a.kv_len->numel() == a.dur.numel(), "f5hip::", op, ": kv_len needs one value per unit");
    }
    const int64_t rows = a.dur.sum().item<int64_t>();
    TORCH_CHECK(a.cond.dim() == 2 && a.cond.size(0) == rows && a.cond_mask.numel() == rows, "f5hip::", op, ": cond / y0 / cond_mask need sum(dur) = ", rows, " rows");
}
// a host fp32 / int32 array with one value per unit
void check_per_unit(const char* op, const at::Tensor& t, at::ScalarType ty, const char* name, const SampleArgs& a) {
    check_host(t, ty, name);
    TORCH_CHECK(t.numel() == a.dur.numel(), "f5hip::", op, ": ", name, " needs one value per unit (", t.numel(), " for ", a.dur.numel(), ")");
}
void check_t_grid(const char* op, const at::Tensor& t_grid) {
    check_host(t_grid, at::kFloat, "t_grid");
    TORCH_CHECK(t_grid.numel() >= 2, "f5hip::", op, ": shapes");
}

// Calls the entry point `fn` of the C ABI: the arguments all of them share, `tail` (its time grid and strength), then the output and the stream
template <class Fn, class... Tail>
at::Tensor run_sample(const char* name, Fn fn, int64_t handle, const SampleArgs& a, Tail... tail) {
    at::Tensor out = at::empty_like(a.y0);
    const int rc = fn((f5hip_dit*)handle, (int32_t)a.dur.numel(), a.dur.data_ptr<int32_t>(), a.kv(), a.cond.data_ptr<float>(), a.cond_mask.data_ptr<uint8_t>(),
                      a.text.data_ptr<int32_t>(), (int32_t)a.text.size(1), a.y0.data_ptr<float>(), tail..., out.data_ptr<float>(), stream_of(a.y0));
    TORCH_CHECK(rc == 0, name, ": ", f5hip_last_error());
    return out;
}

// t_grid [steps + 1] fp32 host.  Returns the sampled mel rows [sum(dur), mel].
at::Tensor cfm_sample(int64_t handle, const at::Tensor& dur, const c10::optional<at::Tensor>& kv_len, const at::Tensor& cond, const at::Tensor& cond_mask,
                      const at::Tensor& text, const at::Tensor& y0, const at::Tensor& t_grid, double cfg_strength) {
    const SampleArgs a{dur, cond, cond_mask, text, y0, kv_len};
    check_sample_args("cfm_sample", a);
    check_t_grid("cfm_sample", t_grid);
    return run_sample("f5hip_cfm_sample", f5hip_cfm_sample_masked, handle, a, t_grid.data_ptr<float>(), (int32_t)t_grid.numel() - 1, (float)cfg_strength);
}

// cfm_sample with cfg_strength [b] fp32 host: one strength per unit (f5hip_cfm_sample_units; < 1e-5 drops that unit's unconditional rows).
at::Tensor cfm_sample_units(int64_t handle, const at::Tensor& dur, const c10::optional<at::Tensor>& kv_len, const at::Tensor& cond, const at::Tensor& cond_mask,
                            const at::Tensor& text, const at::Tensor& y0, const at::Tensor& t_grid, const at::Tensor& cfg_strength) {
    const SampleArgs a{dur, cond, cond_mask, text, y0, kv_len};
    check_sample_args("cfm_sample_units", a);
    check_t_grid("cfm_sample_units", t_grid);
    check_per_unit("cfm_sample_units", cfg_strength, at::kFloat, "cfg_strength", a);
    return run_sample("f5hip_cfm_sample_units", f5hip_cfm_sample_units, handle, a, t_grid.data_ptr<float>(), (int32_t)t_grid.numel() - 1, cfg_strength.data_ptr<float>());
}

// The checks of the operators with one grid per unit: steps, t_grids and cfg_strength against the units
void check_unit_grids(const char* op, const SampleArgs& a, const at::Tensor& steps, const at::Tensor& t_grids, const at::Tensor& cfg_strength) {
    check_sample_args(op, a);
    check_host(t_grids, at::kFloat, "t_grids");
    check_per_unit(op, cfg_strength, at::kFloat, "cfg_strength", a);
    check_per_unit(op, steps, at::kInt, "steps", a);
    const int32_t* sp = steps.data_ptr<int32_t>();
    int64_t points = 0;
    for (int64_t u = 0; u < steps.numel(); u++) {
        TORCH_CHECK(sp[u] >= 1, "f5hip::", op, ": steps[", u, "] = ", sp[u], " (need >= 1)");
        points += sp[u] + 1;
    }
    TORCH_CHECK(t_grids.numel() == points, "f5hip::", op, ": t_grids needs sum(steps) + n = ", points, " values (got ", t_grids.numel(), ")");
}

// cfm_sample_units with one time grid per unit (f5hip_cfm_sample_grids): steps [b] int32 host (each >= 1), t_grids fp32 host, the b grids of
// steps[u] + 1 points one after the other (sum(steps) + b floats).
at::Tensor cfm_sample_grids(int64_t handle, const at::Tensor& dur, const c10::optional<at::Tensor>& kv_len, const at::Tensor& cond, const at::Tensor& cond_mask,
                            const at::Tensor& text, const at::Tensor& y0, const at::Tensor& steps, const at::Tensor& t_grids, const at::Tensor& cfg_strength) {
    const SampleArgs a{dur, cond, cond_mask, text, y0, kv_len};
    check_unit_grids("cfm_sample_grids", a, steps, t_grids, cfg_strength);
    return run_sample("f5hip_cfm_sample_grids", f5hip_cfm_sample_grids, handle, a, steps.data_ptr<int32_t>(), t_grids.data_ptr<float>(), cfg_strength.data_ptr<float>());
}

// One resumable span of cfm_sample_grids (f5hip_cfm_sample_span): y0 is every unit's current ODE state, steps / t_grids describe this span (a
// contiguous slice of the unit's whole grid), last [b] uint8 host: 1 = the unit ends here and gets where(cond_mask, cond, x), 0 = it gets
// its raw state, prompt frames included, to be handed back as y0 of its next span.
at::Tensor cfm_sample_span(int64_t handle, const at::Tensor& dur, const c10::optional<at::Tensor>& kv_len, const at::Tensor& cond, const at::Tensor& cond_mask,
                           const at::Tensor& text, const at::Tensor& y0, const at::Tensor& steps, const at::Tensor& t_grids, const at::Tensor& cfg_strength,
                           const at::Tensor& last) {
    const SampleArgs a{dur, cond, cond_mask, text, y0, kv_len};
    check_unit_grids("cfm_sample_span", a, steps, t_grids, cfg_strength);
    check_per_unit("cfm_sample_span", last, at::kByte, "last", a);
    return run_sample("f5hip_cfm_sample_span", f5hip_cfm_sample_span, handle, a, steps.data_ptr<int32_t>(), t_grids.data_ptr<float>(), cfg_strength.data_ptr<float>(),
                      last.data_ptr<uint8_t>());
}

// cfm_sample_span with one ODE method per unit (f5hip_cfm_sample_methods): method [b] int32 host, 0 euler / 1 midpoint / 2 rk4; the handle's own
// method is not read.  last [b] uint8 host as in cfm_sample_span, or None: every unit ends with the call.
at::Tensor cfm_sample_methods(int64_t handle, const at::Tensor& dur, const c10::optional<at::Tensor>& kv_len, const at::Tensor& cond, const at::Tensor& cond_mask,
                              const at::Tensor& text, const at::Tensor& y0, const at::Tensor& steps, const at::Tensor& t_grids, const at::Tensor& cfg_strength,
                              const at::Tensor& method, const c10::optional<at::Tensor>& last) {
    const SampleArgs a{dur, cond, cond_mask, text, y0, kv_len};
    check_unit_grids("cfm_sample_methods", a, steps, t_grids, cfg_strength);
    check_per_unit("cfm_sample_methods", method, at::kInt, "method", a);
    if (last.has_value()) check_per_unit("cfm_sample_methods", *last, at::kByte, "last", a);
    return run_sample("f5hip_cfm_sample_methods", f5hip_cfm_sample_methods, handle, a, steps.data_ptr<int32_t>(), t_grids.data_ptr<float>(),
                      cfg_strength.data_ptr<float>(), method.data_ptr<int32_t>(), opt_ptr<uint8_t>(last));
}

at::Tensor vocos_decode(int64_t handle, const at::Tensor& mel, int64_t hop_length) {
    check_dev_f32(mel, "mel");
    TORCH_CHECK(mel.dim() == 3, "f5hip::vocos_decode: mel [b, 100, T]");
    at::Tensor wave = at::empty({mel.size(0), hop_length * (mel.size(2) - 1)}, mel.options());
    const int rc = f5hip_vocos_decode((f5hip_vocos*)handle, (int32_t)mel.size(0), (int32_t)mel.size(2), mel.data_ptr<float>(), wave.data_ptr<float>(), stream_of(mel));
    TORCH_CHECK(rc == 0, "f5hip_vocos_decode: ", f5hip_last_error());
    return wave;
}

// mel [n, channels, T_max] fp32 device, frames [n] int32 host (item i valid for t < frames[i], each >= 2) -> packed wave
// [hop_length * sum(frames[i] - 1)], item i at hop_length * sum_{j<i} (frames[j] - 1)
at::Tensor vocos_decode_ragged(int64_t handle, const at::Tensor& mel, const at::Tensor& frames, int64_t channels, int64_t hop_length) {
    const int64_t total = hop_length * (check_ragged_frames("vocos_decode_ragged", mel, frames, channels, 2) - frames.numel());
    const c10::DeviceGuard guard(mel.device());   // allocation and stream on the mel's device
    at::Tensor wave = at::empty({total}, mel.options());
    const int rc = f5hip_vocos_decode_ragged((f5hip_vocos*)handle, (int32_t)frames.numel(), frames.data_ptr<int32_t>(), mel.data_ptr<float>(),
                                             wave.data_ptr<float>(), stream_of(mel));
    TORCH_CHECK(rc == 0, "f5hip_vocos_decode_ragged: ", f5hip_last_error());
    return wave;
}

at::Tensor bigvgan_forward(int64_t handle, const at::Tensor& mel, int64_t total_upsample) {
    check_dev_f32(mel, "mel");
    TORCH_CHECK(mel.dim() == 3, "f5hip::bigvgan_forward: mel [b, 100, T]");
    at::Tensor wave = at::empty({mel.size(0), 1, total_upsample * mel.size(2)}, mel.options());
    const int rc = f5hip_bigvgan_forward((f5hip_bigvgan*)handle, (int32_t)mel.size(0), (int32_t)mel.size(2), mel.data_ptr<float>(), wave.data_ptr<float>(), stream_of(mel));
    TORCH_CHECK(rc == 0, "f5hip_bigvgan_forward: ", f5hip_last_error());
    return wave;
}

// mel [n, channels, T_max] fp32 device, frames [n] int32 host (item i valid for t < frames[i], each >= 1) -> packed wave
// [total_upsample * sum(frames[i])], item i at total_upsample * sum_{j<i} frames[j]
at::Tensor bigvgan_forward_ragged(int64_t handle, const at::Tensor& mel, const at::Tensor& frames, int64_t channels, int64_t total_upsample) {
    const int64_t total = total_upsample * check_ragged_frames("bigvgan_forward_ragged", mel, frames, channels, 1);
    const int32_t* f = frames.data_ptr<int32_t>();
    const int64_t t_max = *std::max_element(f, f + frames.numel());
    TORCH_CHECK(t_max == mel.size(2), "f5hip::bigvgan_forward_ragged: mel.size(2) = ", mel.size(2), " must be the longest item's frames (", t_max, ")");
    const c10::DeviceGuard guard(mel.device());   // allocation and stream on the mel's device
    at::Tensor wave = at::empty({total}, mel.options());
    const int rc = f5hip_bigvgan_forward_ragged((f5hip_bigvgan*)handle, (int32_t)frames.numel(), f, mel.data_ptr<float>(), wave.data_ptr<float>(), stream_of(mel));
    TORCH_CHECK(rc == 0, "f5hip_bigvgan_forward_ragged: ", f5hip_last_error());
    return wave;
}

// wave fp32 device, the clips packed back to back (clip i = channels[i] planes of n_in[i] samples); n_in / channels [n] int32 host; taps fp32
// device [nf][2 width + of] (infer.resample_taps) or None when the rates are equal -> (packed mono clips at new_freq, clip i holding
// ceil(nf n_in[i] / of) samples; rms [n] fp32 device, measured before the gain)
std::tuple<at::Tensor, at::Tensor> ref_frontend(const at::Tensor& wave, const at::Tensor& n_in, const at::Tensor& channels, int64_t orig_freq, int64_t new_freq,
                                                const c10::optional<at::Tensor>& taps, double rms_floor) {
    check_dev_f32(wave, "wave"); check_host(n_in, at::kInt, "n_in"); check_host(channels, at::kInt, "channels");
    TORCH_CHECK(n_in.dim() == 1 && n_in.numel() > 0 && channels.numel() == n_in.numel(), "f5hip::ref_frontend: n_in and channels need one value per clip");
    TORCH_CHECK(orig_freq >= 1 && new_freq >= 1 && orig_freq <= INT32_MAX && new_freq <= INT32_MAX, "f5hip::ref_frontend: sample rates");
    if (taps.has_value()) check_dev_f32(*taps, "taps");
    const RatePair rp = rate_pair((int)orig_freq, (int)new_freq);
    const int64_t of = rp.of, nf = rp.nf;
    const int32_t *ni = n_in.data_ptr<int32_t>(), *ch = channels.data_ptr<int32_t>();
    int64_t total_in = 0, total_out = 0;
    for (int64_t i = 0; i < n_in.numel(); i++) {
        TORCH_CHECK(ni[i] >= 1 && ch[i] >= 1, "f5hip::ref_frontend: clip ", i, " has ", ni[i], " samples in ", ch[i], " channels");
        total_in += (int64_t)ni[i] * ch[i];
        total_out += (nf * ni[i] + of - 1) / of;
    }
    TORCH_CHECK(wave.numel() == total_in, "f5hip::ref_frontend: wave needs sum(n_in * channels) = ", total_in, " samples (got ", wave.numel(), ")");
    TORCH_CHECK(total_out <= INT32_MAX, "f5hip::ref_frontend: the outputs of the call exceed 2^31 - 1 samples");
    if (orig_freq != new_freq) {
        TORCH_CHECK(taps.has_value(), "f5hip::ref_frontend: ", orig_freq, " -> ", new_freq, " Hz needs the tap table");
        // the library derives the row length itself (rate_pair.h): a table of any other shape would be read with the wrong stride
        TORCH_CHECK(taps->dim() == 2 && taps->size(0) == nf && taps->size(1) == rp.L, "f5hip::ref_frontend: taps must be [nf = ", nf,
                    "][2 * width + of = ", rp.L, "] (rate_pair.h: torchaudio's defaults); got ", taps->sizes());
    }
    const c10::DeviceGuard guard(wave.device());   // allocations and stream on the wave's device
    at::Tensor out = at::empty({total_out}, wave.options()), rms = at::empty({n_in.numel()}, wave.options());
    const int rc = f5hip_ref_frontend((int32_t)n_in.numel(), ni, ch, wave.data_ptr<float>(), (int32_t)orig_freq, (int32_t)new_freq,
                                      taps.has_value() && orig_freq != new_freq ? taps->data_ptr<float>() : (const float*)nullptr, (float)rms_floor,
                                      out.data_ptr<float>(), rms.data_ptr<float>(), stream_of(wave));
    TORCH_CHECK(rc == 0, "f5hip_ref_frontend: ", f5hip_last_error());
    return {out, rms};
}

// chunks: the chunk waves of all requests in request and chunk order, each a contiguous 1-D fp32 device tensor (views of the vocoder's packed
// output as they are: the library reads them through a pointer table); chunks_per_request [n] int32 host; fade in samples; remove_silence [n]
// uint8 host -> (pcm int16 device, request i at sum_{j<i} ((N_j + 7) & ~7); lengths [n] int32 device)
// chunk_fade: null (every join fades: f5hip_wave_finish), or one byte per chunk of the call (f5hip_wave_finish_joins)
static std::tuple<at::Tensor, at::Tensor> wave_finish_impl(at::TensorList chunks, const at::Tensor& chunks_per_request, int64_t fade, const uint8_t* chunk_fade,
                                                           const at::Tensor& remove_silence, int64_t sample_rate) {
    check_host(chunks_per_request, at::kInt, "chunks_per_request"); check_host(remove_silence, at::kByte, "remove_silence");
    const int64_t n = chunks_per_request.numel();
    TORCH_CHECK(chunks_per_request.dim() == 1 && n > 0 && remove_silence.numel() == n, "f5hip::wave_finish: chunks_per_request and remove_silence need one value per request");
    TORCH_CHECK(fade >= 0 && fade <= INT32_MAX, "f5hip::wave_finish: the fade length must not be negative (got ", fade, ")");
    TORCH_CHECK(sample_rate == 24000, "f5hip::wave_finish: the sample rate must be 24000 (got ", sample_rate, ")");
    const int32_t* kp = chunks_per_request.data_ptr<int32_t>();
    int64_t total_chunks = 0;
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(kp[i] >= 1, "f5hip::wave_finish: request ", i, " has ", kp[i], " chunks");
        total_chunks += kp[i];
    }
    TORCH_CHECK((int64_t)chunks.size() == total_chunks, "f5hip::wave_finish: chunks needs sum(chunks_per_request) = ", total_chunks, " tensors (got ", chunks.size(), ")");
    const PointerTable tb = pointer_table("wave_finish", chunks, "chunk");
    int64_t total_out = 0, c = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t joined = 0;
        for (int32_t j = 0; j < kp[i]; j++, c++) {
            const int64_t len = tb.lens[c];
            TORCH_CHECK(len >= 1, "f5hip::wave_finish: chunk ", j, " of request ", i, " is empty");
            TORCH_CHECK(chunk_fade || kp[i] == 1 || fade == 0 || len >= 2 * fade, "f5hip::wave_finish: chunk ", j, " of request ", i, " has ", len,
                        " samples, fewer than 2 x fade = ", 2 * fade, ": its fades would overlap");
            const int64_t fin = j > 0 && (!chunk_fade || chunk_fade[c]) ? fade : 0, fout = j + 1 < kp[i] && (!chunk_fade || chunk_fade[c + 1]) ? fade : 0;
            TORCH_CHECK(len >= fin + fout, "f5hip::wave_finish: chunk ", j, " of request ", i, " has ", len, " samples, fewer than its fades (", fin,
                        " in, ", fout, " out): they would overlap");
            joined += len - fin;
        }
        total_out += (joined + 7) & ~(int64_t)7;
        TORCH_CHECK(total_out <= INT32_MAX, "f5hip::wave_finish: the outputs of the call exceed 2^31 - 1 samples");
    }
    const c10::DeviceGuard guard(chunks[0].device());   // allocations and stream on the chunks' device
    at::Tensor pcm = at::empty({total_out}, chunks[0].options().dtype(at::kShort)), lengths = at::empty({n}, chunks[0].options().dtype(at::kInt));
    const int rc = f5hip_wave_finish_joins((int32_t)n, kp, tb.ptrs.data(), tb.lens.data(), (int32_t)fade, chunk_fade, remove_silence.data_ptr<uint8_t>(),
                                           (int32_t)sample_rate, pcm.data_ptr<int16_t>(), lengths.data_ptr<int32_t>(), stream_of(chunks[0]));
    TORCH_CHECK(rc == 0, "f5hip_wave_finish: ", f5hip_last_error());
    return {pcm, lengths};
}

std::tuple<at::Tensor, at::Tensor> wave_finish(at::TensorList chunks, const at::Tensor& chunks_per_request, int64_t fade, const at::Tensor& remove_silence,
                                               int64_t sample_rate) {
    return wave_finish_impl(chunks, chunks_per_request, fade, nullptr, remove_silence, sample_rate);
}

// wave_finish with chunk_fade [sum(chunks_per_request)] uint8 host: non-zero where a chunk cross-fades into the one before it, 0 where it butts
std::tuple<at::Tensor, at::Tensor> wave_finish_joins(at::TensorList chunks, const at::Tensor& chunks_per_request, int64_t fade, const at::Tensor& chunk_fade,
                                                     const at::Tensor& remove_silence, int64_t sample_rate) {
    check_host(chunk_fade, at::kByte, "chunk_fade");
    TORCH_CHECK(chunk_fade.dim() == 1 && chunk_fade.numel() == (int64_t)chunks.size(), "f5hip::wave_finish_joins: chunk_fade needs one value per chunk (",
                chunks.size(), "), got ", chunk_fade.numel());
    return wave_finish_impl(chunks, chunks_per_request, fade, chunk_fade.data_ptr<uint8_t>(), remove_silence, sample_rate);
}

// waves: one contiguous 1-D fp32 device tensor per clip (views of ref_frontend's packed output as they are: the library reads them through a
// pointer table); variant 0 vocos, 1 bigvgan -> mel [sum T, n_mels] fp32 device, frame-major and packed in clip order
at::Tensor mel_spectrogram_ragged(at::TensorList waves, int64_t n_fft, int64_t hop_length, int64_t n_mels, int64_t sample_rate, int64_t variant) {
    const int64_t n = (int64_t)waves.size();
    TORCH_CHECK(n > 0, "f5hip::mel_spectrogram_ragged: no clips");
    TORCH_CHECK(variant == 0 || variant == 1, "f5hip::mel_spectrogram_ragged: unknown variant ", variant, " (0 vocos, 1 bigvgan)");
    TORCH_CHECK(n_fft == 1024 && hop_length >= 1 && hop_length <= n_fft && n_mels >= 1 && n_mels <= 256, "f5hip::mel_spectrogram_ragged: only n_fft = 1024, 1 <= hop_length <= n_fft, 1 <= n_mels <= 256");
    const int64_t pad = (n_fft - hop_length) / 2;
    const PointerTable tb = pointer_table("mel_spectrogram_ragged", waves, "clip");
    int64_t rows = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t len = tb.lens[i];
        TORCH_CHECK(variant ? len >= n_fft : len > n_fft / 2, "f5hip::mel_spectrogram_ragged: clip ", i, " has ", len, " samples (needs ",
                    variant ? ">= " : "> ", variant ? n_fft : n_fft / 2, ")");
        rows += variant ? (len + 2 * pad - n_fft) / hop_length + 1 : 1 + len / hop_length;
    }
    TORCH_CHECK(rows * n_mels <= INT32_MAX, "f5hip::mel_spectrogram_ragged: the output exceeds 2^31 - 1 values");
    const c10::DeviceGuard guard(waves[0].device());
    at::Tensor mel = at::empty({rows, n_mels}, waves[0].options());
    const int rc = f5hip_mel_spectrogram_ragged((int32_t)n, tb.lens.data(), tb.ptrs.data(), mel.data_ptr<float>(), (int32_t)n_fft, (int32_t)hop_length, (int32_t)n_mels,
                                                (int32_t)sample_rate, (int32_t)variant, stream_of(waves[0]));
    TORCH_CHECK(rc == 0, "f5hip_mel_spectrogram_ragged: ", f5hip_last_error());
    return mel;
}

// pcm: ONE int16 device tensor that holds every request (f5hip_wave_finish's packed PCM) or one tensor per request; in_off [n] int64 host (request
// i starts at sample in_off[i] of its tensor); max_len [n] int32 host; len_dev [n] int32 device or None; taps as ref_frontend's, for 24000 ->
// new_freq -> (out uint8 device: int16 samples little-endian, or G.711 code bytes; out_len [n] int32 device; out_off [n] int64 host, bytes)
std::tuple<at::Tensor, at::Tensor, at::Tensor> wave_encode(at::TensorList pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                           const c10::optional<at::Tensor>& len_dev, int64_t new_freq, int64_t encoding,
                                                           const c10::optional<at::Tensor>& taps) {
    const PcmRequests rq = check_pcm_requests("wave_encode", pcm, in_off, max_len, len_dev, true);
    const int64_t n = rq.n;
    const int32_t* ml = rq.ml;
    TORCH_CHECK(encoding >= 0 && encoding <= 2, "f5hip::wave_encode: unknown encoding ", encoding, " (0 pcm16, 1 mu-law, 2 A-law)");
    TORCH_CHECK(new_freq >= 1 && new_freq <= INT32_MAX, "f5hip::wave_encode: the sample rate must be positive (got ", new_freq, ")");
    const RatePair rp = rate_pair(24000, (int)new_freq);
    const int64_t of = rp.of, nf = rp.nf;
    if (new_freq != 24000) {
        TORCH_CHECK(taps.has_value(), "f5hip::wave_encode: 24000 -> ", new_freq, " Hz needs the tap table");
        check_dev_f32(*taps, "taps");
        TORCH_CHECK(taps->dim() == 2 && taps->size(0) == nf && taps->size(1) == rp.L, "f5hip::wave_encode: taps must be [nf = ", nf,
                    "][2 * width + of = ", rp.L, "] (rate_pair.h: torchaudio's defaults); got ", taps->sizes());
    }
    const PcmSources src = pcm_sources("wave_encode", pcm, rq);
    const int64_t bps = encoding == 0 ? 2 : 1;
    at::Tensor out_off = at::empty({n}, at::TensorOptions().dtype(at::kLong));
    int64_t* oo = out_off.data_ptr<int64_t>();
    int64_t total_in = 0, total_out = 0, bytes = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t n_out = (nf * ml[i] + of - 1) / of;
        total_in += ml[i]; total_out += n_out;
        TORCH_CHECK(total_in <= INT32_MAX && total_out <= INT32_MAX, "f5hip::wave_encode: the call exceeds 2^31 - 1 samples in or out");
        oo[i] = bytes;
        bytes += (n_out * bps + 15) & ~(int64_t)15;
    }
    const c10::DeviceGuard guard(rq.device);   // allocations and stream on the pcm's device
    // (a call of empty requests still has an address to give)
    at::Tensor out = at::empty({std::max<int64_t>(bytes, 16)}, pcm[0].options().dtype(at::kByte)).narrow(0, 0, bytes), out_len = at::empty({n}, pcm[0].options().dtype(at::kInt));
    const int rc = f5hip_wave_encode((int32_t)n, src.base(), src.rel.data(), ml, rq.len_dev, (int32_t)new_freq, (int32_t)encoding,
                                     new_freq != 24000 ? taps->data_ptr<float>() : (const float*)nullptr, out.data_ptr<uint8_t>(), oo,
                                     out_len.data_ptr<int32_t>(), stream_of(pcm[0]));
    TORCH_CHECK(rc == 0, "f5hip_wave_encode: ", f5hip_last_error());
    return {out, out_len, out_off};
}

// pcm, in_off, max_len, len_dev as wave_encode's, the samples at `sample_rate` already -> (out uint8 device: request i's native FLAC stream at
// byte out_off[i]; out_len [n] int32 device: its bytes; out_off [n] int64 host)
// level: null (all 0, f5hip_wave_flac) or int32 [n] on the host, each 0 or 1 (f5hip_wave_flac_levels)
static std::tuple<at::Tensor, at::Tensor, at::Tensor> wave_flac_impl(at::TensorList pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                                     const c10::optional<at::Tensor>& len_dev, int64_t sample_rate,
                                                                     const at::Tensor* level) {
    const PcmRequests rq = check_pcm_requests("wave_flac", pcm, in_off, max_len, len_dev, true);
    const int64_t n = rq.n;
    const int32_t* ml = rq.ml;
    if (level) {
        check_host(*level, at::kInt, "level");
        TORCH_CHECK(level->dim() == 1 && level->numel() == n, "f5hip::wave_flac_levels: level needs one value per request");
    }
    TORCH_CHECK(sample_rate >= 1 && sample_rate <= INT32_MAX, "f5hip::wave_flac: the sample rate must be positive (got ", sample_rate, ")");
    const PcmSources src = pcm_sources("wave_flac", pcm, rq);
    at::Tensor out_off = at::empty({n}, at::TensorOptions().dtype(at::kLong));
    int64_t* oo = out_off.data_ptr<int64_t>();
    int64_t total_in = 0, bytes = 0;
    for (int64_t i = 0; i < n; i++) {
        total_in += ml[i];
        oo[i] = bytes;
        bytes += (f5hip_wave_flac_bound(ml[i]) + 15) & ~(int64_t)15;
        TORCH_CHECK(total_in <= INT32_MAX && bytes <= INT32_MAX, "f5hip::wave_flac: the call exceeds 2^31 - 1 samples in or bytes out");
    }
    const c10::DeviceGuard guard(rq.device);   // allocations and stream on the pcm's device
    at::Tensor out = at::empty({bytes}, pcm[0].options().dtype(at::kByte)), out_len = at::empty({n}, pcm[0].options().dtype(at::kInt));
    const int rc = level ? f5hip_wave_flac_levels((int32_t)n, src.base(), src.rel.data(), ml, rq.len_dev, (int32_t)sample_rate, level->data_ptr<int32_t>(),
                                                  out.data_ptr<uint8_t>(), oo, out_len.data_ptr<int32_t>(), stream_of(pcm[0]))
                         : f5hip_wave_flac((int32_t)n, src.base(), src.rel.data(), ml, rq.len_dev, (int32_t)sample_rate, out.data_ptr<uint8_t>(), oo,
                                           out_len.data_ptr<int32_t>(), stream_of(pcm[0]));
    TORCH_CHECK(rc == 0, level ? "f5hip_wave_flac_levels: " : "f5hip_wave_flac: ", f5hip_last_error());
    return {out, out_len, out_off};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> wave_flac(at::TensorList pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                         const c10::optional<at::Tensor>& len_dev, int64_t sample_rate) {
    return wave_flac_impl(pcm, in_off, max_len, len_dev, sample_rate, nullptr);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> wave_flac_levels(at::TensorList pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                                const c10::optional<at::Tensor>& len_dev, int64_t sample_rate,
                                                                const at::Tensor& level) {
    return wave_flac_impl(pcm, in_off, max_len, len_dev, sample_rate, &level);
}

// data: the packed streams, uint8 on the device; begin, end, total, max_samples [n] int64 host; info [n, 8] int32 host (channels, bits, rate,
// min block, max block, cap, needs_host, 0) as f5hip_flac_decode's -> (out int32 device: [n, 2] status and samples per channel, then the planes:
// channel c of stream i at out_off[i] + c * cap; out_off [n] int64 host)
std::tuple<at::Tensor, at::Tensor> flac_decode(const at::Tensor& data, const at::Tensor& begin, const at::Tensor& end, const at::Tensor& info,
                                               const at::Tensor& total, const at::Tensor& max_samples) {
    check_host(begin, at::kLong, "begin"); check_host(end, at::kLong, "end"); check_host(info, at::kInt, "info");
    check_host(total, at::kLong, "total"); check_host(max_samples, at::kLong, "max_samples");
    const int64_t n = begin.numel();
    TORCH_CHECK(begin.dim() == 1 && n > 0 && n <= INT32_MAX / 2 && end.numel() == n && total.numel() == n && max_samples.numel() == n && info.dim() == 2 &&
                info.size(0) == n && info.size(1) == 8, "f5hip::flac_decode: begin, end, total, max_samples need one value per stream and info [n, 8]");
    TORCH_CHECK(data.is_cuda() && data.scalar_type() == at::kByte && data.is_contiguous() && data.dim() == 1 && data.numel() > 0,
                "f5hip::flac_decode: data must be a non-empty contiguous 1-D uint8 tensor on a HIP device");
    const int32_t* f = info.data_ptr<int32_t>();
    at::Tensor out_off = at::empty({n}, at::TensorOptions().dtype(at::kLong));
    int64_t* oo = out_off.data_ptr<int64_t>();
    int64_t words = 2 * n;
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(f[8 * i] >= 1 && f[8 * i] <= 8 && f[8 * i + 5] >= 0, "f5hip::flac_decode: stream ", i, " has ", f[8 * i], " channels and room for ", f[8 * i + 5],
                    " samples");
        oo[i] = words;
        if (!f[8 * i + 6]) words += (int64_t)f[8 * i] * f[8 * i + 5];
        TORCH_CHECK(words <= (int64_t)1 << 40, "f5hip::flac_decode: the call's streams declare more samples than one call takes");
    }
    const c10::DeviceGuard guard(data.device());
    at::Tensor out = at::empty({words}, data.options().dtype(at::kInt));
    const int rc = f5hip_flac_decode((int32_t)n, data.data_ptr<uint8_t>(), data.numel(), begin.data_ptr<int64_t>(), end.data_ptr<int64_t>(), f,
                                     total.data_ptr<int64_t>(), max_samples.data_ptr<int64_t>(), out.data_ptr<int32_t>(), oo, out.data_ptr<int32_t>(),
                                     stream_of(data));
    TORCH_CHECK(rc == 0, "f5hip_flac_decode: ", f5hip_last_error());
    return {out, out_off};
}

// frames: the clips' interleaved int16 frames packed back to back, on the device; n_in, channels [n] int32 host; clip_short [n] uint8 host ->
// (out fp32 device with room for f5hip_ref_prestep_bound samples: clip i as channels[i] planes of its output length, packed by the output
// lengths; info int32 device [n, 2]: output frames and "any sample non-zero") as f5hip_ref_prestep's
std::tuple<at::Tensor, at::Tensor> ref_prestep(const at::Tensor& frames, const at::Tensor& n_in, const at::Tensor& channels, const at::Tensor& clip_short,
                                               int64_t rate) {
    check_host(n_in, at::kInt, "n_in"); check_host(channels, at::kInt, "channels"); check_host(clip_short, at::kByte, "clip_short");
    const int64_t n = n_in.numel();
    TORCH_CHECK(n_in.dim() == 1 && n > 0 && n <= INT32_MAX / 2 && channels.numel() == n && clip_short.numel() == n,
                "f5hip::ref_prestep: n_in, channels and clip_short need one value per clip, and at least one clip");
    TORCH_CHECK(rate >= 11025 && rate <= INT32_MAX, "f5hip::ref_prestep: reference audio below 11025 Hz is not supported on this path (got ", rate, ")");
    TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kShort && frames.is_contiguous() && frames.dim() == 1,
                "f5hip::ref_prestep: frames must be a contiguous 1-D int16 tensor on a HIP device");
    const int32_t* ni = n_in.data_ptr<int32_t>();
    const int32_t* ch = channels.data_ptr<int32_t>();
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(ni[i] >= 0 && ch[i] >= 1, "f5hip::ref_prestep: clip ", i, " has ", ni[i], " frames in ", ch[i], " channels");
        total += (int64_t)ni[i] * ch[i];
        TORCH_CHECK(total <= INT32_MAX, "f5hip::ref_prestep: the clips of the call exceed 2^31 - 1 samples");
    }
    TORCH_CHECK(frames.numel() == total, "f5hip::ref_prestep: the frames need sum(n_in * channels) = ", total, " samples (got ", frames.numel(), ")");
    const int64_t bound = f5hip_ref_prestep_bound((int32_t)n, ni, ch, (int32_t)rate);
    TORCH_CHECK(bound >= 0 && bound <= INT32_MAX, "f5hip::ref_prestep: the clips of the call exceed 2^31 - 1 samples");
    const c10::DeviceGuard guard(frames.device());
    at::Tensor out = at::empty({bound}, frames.options().dtype(at::kFloat));
    at::Tensor info = at::empty({n, 2}, frames.options().dtype(at::kInt));
    const int rc = f5hip_ref_prestep((int32_t)n, ni, ch, clip_short.data_ptr<uint8_t>(), total ? frames.data_ptr<int16_t>() : (const int16_t*)nullptr, total,
                                     (int32_t)rate, out.data_ptr<float>(), info.data_ptr<int32_t>(), stream_of(frames));
    TORCH_CHECK(rc == 0, "f5hip_ref_prestep: ", f5hip_last_error());
    return {out, info};
}

// pcm: the int16 device tensor that holds every request (f5hip_wave_finish's packed PCM), normalised IN PLACE; in_off, max_len, len_dev as
// wave_encode's; gain_k [n] float64 host: K_T per request, <= 0 leaves the request alone -> stats int64 device [n, 4]: n2, S2, peak, the bits
// of g (zeros for a request that was left alone)
at::Tensor wave_loudness(at::Tensor pcm, const at::Tensor& in_off, const at::Tensor& max_len, const c10::optional<at::Tensor>& len_dev,
                         const at::Tensor& gain_k) {
    const PcmRequests rq = check_pcm_requests("wave_loudness", pcm, in_off, max_len, len_dev, false);
    const int64_t n = rq.n;
    check_host(gain_k, at::kDouble, "gain_k");
    TORCH_CHECK(gain_k.numel() == n, "f5hip::wave_loudness: gain_k needs one value per request");
    const PcmSources src = pcm_sources("wave_loudness", pcm, rq);
    const double* gk = gain_k.data_ptr<double>();
    int64_t total = 0;
    bool any = false;
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(std::isfinite(gk[i]), "f5hip::wave_loudness: the gain constant of request ", i, " is not finite");
        total += rq.ml[i];
        TORCH_CHECK(total <= INT32_MAX, "f5hip::wave_loudness: the call exceeds 2^31 - 1 samples");
        any = any || gk[i] > 0.0;
    }
    const c10::DeviceGuard guard(rq.device);
    at::Tensor stats = at::zeros({n, 4}, pcm.options().dtype(at::kLong));
    if (!any || pcm.numel() == 0) return stats;      // nothing to launch (an empty tensor has no address to give)
    const int rc = f5hip_wave_loudness((int32_t)n, src.base(), src.rel.data(), rq.ml, rq.len_dev, gk, stats.data_ptr<int64_t>(), stream_of(pcm));
    TORCH_CHECK(rc == 0, "f5hip_wave_loudness: ", f5hip_last_error());
    return stats;
}

// pcm: the int16 device tensor that holds every request (f5hip_wave_finish's packed PCM), read only; in_off, max_len, len_dev as wave_encode's;
// stretch_p, stretch_q, pitch [n] int32 host; taps: the twelve pitch tables as one fp32 device tensor (f5hip_wave_prosody_tap_offset), needed
// when a request has a pitch -> (out int16 device: request i's samples at out_off[i]; out_len [n] int32 device; out_off [n] int64 host, each
// a multiple of 8; bounds [n] int32 host: the length that max_len[i] gives)
// keep: null for wave_prosody; wave_prosody_formants' uint8 [n] host flags (a flagged request keeps its formants: no resampler, the length
// of its stretch alone)
static std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> wave_prosody_call(const at::Tensor& pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                                                   const c10::optional<at::Tensor>& len_dev, const at::Tensor& stretch_p,
                                                                                   const at::Tensor& stretch_q, const at::Tensor& pitch,
                                                                                   const at::Tensor* keep, const c10::optional<at::Tensor>& taps) {
    const PcmRequests rq = check_pcm_requests("wave_prosody", pcm, in_off, max_len, len_dev, false);
    const int64_t n = rq.n;
    const int32_t* ml = rq.ml;
    check_host(stretch_p, at::kInt, "stretch_p"); check_host(stretch_q, at::kInt, "stretch_q"); check_host(pitch, at::kInt, "pitch");
    TORCH_CHECK(stretch_p.numel() == n && stretch_q.numel() == n && pitch.numel() == n,
                "f5hip::wave_prosody: stretch_p, stretch_q and pitch need one value per request");
    const PcmSources src = pcm_sources("wave_prosody", pcm, rq);
    const int32_t* sp = stretch_p.data_ptr<int32_t>();
    const int32_t* sq = stretch_q.data_ptr<int32_t>();
    const int32_t* pt = pitch.data_ptr<int32_t>();
    const uint8_t* kp = nullptr;
    if (keep) {
        check_host(*keep, at::kByte, "keep_formants");
        TORCH_CHECK(keep->numel() == n, "f5hip::wave_prosody: keep_formants needs one value per request");
        kp = keep->data_ptr<uint8_t>();
    }
    at::Tensor out_off = at::empty({n}, at::TensorOptions().dtype(at::kLong)), bounds = at::empty({n}, at::TensorOptions().dtype(at::kInt));
    int64_t* oo = out_off.data_ptr<int64_t>();
    int32_t* bd = bounds.data_ptr<int32_t>();
    int64_t total_in = 0, total = 0;
    bool pitched = false;
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(pr_stretch_ok(sp[i], sq[i]), "f5hip::wave_prosody: request ", i, " stretches by ", sp[i], "/", sq[i],
                    ": positive terms up to 2^20 and a ratio from 1/2 to 2");
        TORCH_CHECK(pt[i] >= -kPrPitchMax && pt[i] <= kPrPitchMax, "f5hip::wave_prosody: request ", i, " has a pitch of ", pt[i], " semitones (-6 to 6)");
        int64_t m = pr_geom(ml[i], sp[i], sq[i]).m;
        if (kp && kp[i]) {
            TORCH_CHECK(pt[i] != 0, "f5hip::wave_prosody: request ", i, " keeps its formants without a pitch");
        } else if (pt[i]) {
            int p, q;
            pr_pitch_ratio(pt[i], &p, &q);
            m = (q * m + p - 1) / p;
            pitched = true;
        }
        total_in += ml[i];
        oo[i] = total;
        total += (m + 7) & ~(int64_t)7;
        TORCH_CHECK(m <= INT32_MAX && total_in <= INT32_MAX && total <= INT32_MAX, "f5hip::wave_prosody: the call exceeds 2^31 - 1 samples in or out");
        bd[i] = (int32_t)m;
    }
    if (pitched)
        TORCH_CHECK(taps.has_value() && taps->is_cuda() && taps->scalar_type() == at::kFloat && taps->is_contiguous() && taps->device() == pcm.device() &&
                    taps->numel() == f5hip_wave_prosody_tap_offset(0),
                    "f5hip::wave_prosody: a pitch needs taps, the contiguous fp32 table of ", f5hip_wave_prosody_tap_offset(0), " floats on the pcm's device");
    const c10::DeviceGuard guard(rq.device);
    at::Tensor out = at::empty({std::max<int64_t>(total, 8)}, pcm.options()).slice(0, 0, total);   // (a call of empty requests still has an address to give)
    at::Tensor out_len = at::empty({n}, pcm.options().dtype(at::kInt));
    const float* tp = pitched ? taps->data_ptr<float>() : (const float*)nullptr;
    const int rc = kp ? f5hip_wave_prosody_formants((int32_t)n, src.base(), src.rel.data(), ml, rq.len_dev, sp, sq, pt, kp, tp, out.data_ptr<int16_t>(), oo,
                                                    out_len.data_ptr<int32_t>(), stream_of(pcm))
                      : f5hip_wave_prosody((int32_t)n, src.base(), src.rel.data(), ml, rq.len_dev, sp, sq, pt, tp, out.data_ptr<int16_t>(), oo,
                                           out_len.data_ptr<int32_t>(), stream_of(pcm));
    TORCH_CHECK(rc == 0, kp ? "f5hip_wave_prosody_formants: " : "f5hip_wave_prosody: ", f5hip_last_error());
    return {out, out_len, out_off, bounds};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> wave_prosody(const at::Tensor& pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                                        const c10::optional<at::Tensor>& len_dev, const at::Tensor& stretch_p,
                                                                        const at::Tensor& stretch_q, const at::Tensor& pitch,
                                                                        const c10::optional<at::Tensor>& taps) {
    return wave_prosody_call(pcm, in_off, max_len, len_dev, stretch_p, stretch_q, pitch, nullptr, taps);
}

// wave_prosody with keep_formants [n] uint8 host: a flagged request (it must have a pitch) keeps its spectral envelope (f5hip_wave_prosody_formants)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> wave_prosody_formants(const at::Tensor& pcm, const at::Tensor& in_off, const at::Tensor& max_len,
                                                                                 const c10::optional<at::Tensor>& len_dev, const at::Tensor& stretch_p,
                                                                                 const at::Tensor& stretch_q, const at::Tensor& pitch,
                                                                                 const at::Tensor& keep_formants, const c10::optional<at::Tensor>& taps) {
    return wave_prosody_call(pcm, in_off, max_len, len_dev, stretch_p, stretch_q, pitch, &keep_formants, taps);
}

// wave: the contiguous 1-D fp32 device tensor that holds every clip (f5hip_ref_frontend's packed output), denoised IN PLACE; offset [n] int64
// host, n_samples [n] int32 host: clip i is wave[offset[i] : offset[i] + n_samples[i]]; the ranges are disjoint, whatever lies between them
// is left alone
void ref_denoise(at::Tensor wave, const at::Tensor& offset, const at::Tensor& n_samples) {
    check_host(offset, at::kLong, "offset"); check_host(n_samples, at::kInt, "n_samples");
    check_dev_f32(wave, "wave");
    const int64_t n = n_samples.numel();
    TORCH_CHECK(n_samples.dim() == 1 && n > 0 && n <= INT32_MAX && offset.numel() == n, "f5hip::ref_denoise: offset and n_samples need one value per clip, and at least one clip");
    TORCH_CHECK(wave.dim() == 1, "f5hip::ref_denoise: wave must be a contiguous 1-D fp32 tensor on a HIP device");
    const int64_t* off = offset.data_ptr<int64_t>();
    const int32_t* ns = n_samples.data_ptr<int32_t>();
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(ns[i] >= 1 && ns[i] <= kRdMaxSamples, "f5hip::ref_denoise: clip ", i, " has ", ns[i], " samples (1 .. ", kRdMaxSamples, ")");
        TORCH_CHECK(off[i] >= 0 && off[i] + ns[i] <= wave.numel(), "f5hip::ref_denoise: clip ", i, " is samples [", off[i], ", ", off[i] + ns[i], ") of a tensor of ",
                    wave.numel());
    }
    const c10::DeviceGuard guard(wave.device());
    const int rc = f5hip_ref_denoise((int32_t)n, off, ns, wave.data_ptr<float>(), stream_of(wave));
    TORCH_CHECK(rc == 0, "f5hip_ref_denoise: ", f5hip_last_error());
}

// The carriers of a watermark call, checked: a contiguous int16 device tensor [n_keys, 16384] on `device`, 1 .. 16 keys; with trace ids
// (`tagged`) [n_keys, 4, 16384], 1 .. max_keys keys: per key its own row, then its sub-keys'
const int16_t* check_carriers(const char* op, const at::Tensor& carriers, const c10::Device& device, bool tagged = false, int64_t max_keys = kWmKeysMax) {
    const bool shape = tagged ? carriers.dim() == 3 && carriers.size(1) == kWmTagRows && carriers.size(2) == kWmPeriod
                              : carriers.dim() == 2 && carriers.size(1) == kWmPeriod;
    TORCH_CHECK(carriers.is_cuda() && carriers.scalar_type() == at::kShort && carriers.is_contiguous() && shape && carriers.size(0) >= 1 &&
                carriers.size(0) <= max_keys && carriers.device() == device,
                "f5hip::", op, ": carriers must be a contiguous int16 tensor [1 .. ", max_keys, tagged ? ", 4, " : ", ", kWmPeriod, "] on the samples' device");
    return carriers.data_ptr<int16_t>();
}

// wave_mark (id null) and wave_mark_ids under their names: the request checks, then the library call
void wave_mark_call(const char* op, at::Tensor& pcm, const at::Tensor& in_off, const at::Tensor& max_len, const c10::optional<at::Tensor>& len_dev,
                    const at::Tensor& key_index, const at::Tensor* id, const c10::optional<at::Tensor>& carriers) {
    const PcmRequests rq = check_pcm_requests(op, pcm, in_off, max_len, len_dev, false);
    const int64_t n = rq.n;
    check_host(key_index, at::kInt, "key_index");
    TORCH_CHECK(key_index.numel() == n, "f5hip::", op, ": key_index needs one value per request");
    if (id) {
        check_host(*id, at::kInt, "id");
        TORCH_CHECK(id->numel() == n, "f5hip::", op, ": id needs one value per request");
    }
    const PcmSources src = pcm_sources(op, pcm, rq);
    const int32_t* ki = key_index.data_ptr<int32_t>();
    const int32_t* idp = id ? id->data_ptr<int32_t>() : nullptr;
    if (id && carriers.has_value()) check_carriers(op, *carriers, rq.device, true);   // (the other layout is refused as such, not as a key out of range)
    const int64_t n_keys = carriers.has_value() && carriers->dim() == (id ? 3 : 2) ? carriers->size(0) : 0;
    int64_t total = 0;
    bool any = false;
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(ki[i] >= -1 && ki[i] < n_keys, "f5hip::", op, ": request ", i, " names key ", ki[i], " of ", n_keys);
        if (idp) {
            TORCH_CHECK(idp[i] >= -1 && idp[i] <= kWmIdMax, "f5hip::", op, ": request ", i, " has id ", idp[i], " (-1, or 0 .. ", kWmIdMax, ")");
            TORCH_CHECK(idp[i] < 0 || ki[i] >= 0, "f5hip::", op, ": request ", i, " has an id and no key");
        }
        total += rq.ml[i];
        TORCH_CHECK(total <= INT32_MAX, "f5hip::", op, ": the call exceeds 2^31 - 1 samples");
        any = any || ki[i] >= 0;
    }
    if (!any || pcm.numel() == 0) return;            // nothing to launch (an empty tensor has no address to give)
    const int16_t* cp = check_carriers(op, *carriers, rq.device, id != nullptr);
    const c10::DeviceGuard guard(rq.device);
    if (id) {
        const int rc = f5hip_wave_mark_ids((int32_t)n, src.base(), src.rel.data(), rq.ml, rq.len_dev, ki, idp, cp, (int32_t)n_keys, stream_of(pcm));
        TORCH_CHECK(rc == 0, "f5hip_wave_mark_ids: ", f5hip_last_error());
    } else {
        const int rc = f5hip_wave_mark((int32_t)n, src.base(), src.rel.data(), rq.ml, rq.len_dev, ki, cp, (int32_t)n_keys, stream_of(pcm));
        TORCH_CHECK(rc == 0, "f5hip_wave_mark: ", f5hip_last_error());
    }
}

// pcm: the int16 device tensor that holds every request (f5hip_wave_finish's or f5hip_wave_prosody's buffer), marked IN PLACE; in_off, max_len,
// len_dev as wave_encode's; key_index [n] int32 host: the row of `carriers` per request, -1 leaves the request alone; carriers int16 device
// [n_keys, 16384], needed when a request is flagged
void wave_mark(at::Tensor pcm, const at::Tensor& in_off, const at::Tensor& max_len, const c10::optional<at::Tensor>& len_dev, const at::Tensor& key_index,
               const c10::optional<at::Tensor>& carriers) {
    wave_mark_call("wave_mark", pcm, in_off, max_len, len_dev, key_index, nullptr, carriers);
}

// wave_mark with trace ids: id [n] int32 host, -1 or 0 .. 2^30 - 1 per request; carriers int16 device [n_keys, 4, 16384]: per key its own
// carrier, then its sub-keys' (include/f5hip.h f5hip_wave_mark_ids)
void wave_mark_ids(at::Tensor pcm, const at::Tensor& in_off, const at::Tensor& max_len, const c10::optional<at::Tensor>& len_dev, const at::Tensor& key_index,
                   const at::Tensor& id, const c10::optional<at::Tensor>& carriers) {
    wave_mark_call("wave_mark_ids", pcm, in_off, max_len, len_dev, key_index, &id, carriers);
}

// watermark_detect (4 words per row) and watermark_read_ids (10, tagged carriers) under their names: the clip checks, then the library call
at::Tensor watermark_rows(const char* op, const at::Tensor& wave, const at::Tensor& offset, const at::Tensor& n_samples, const at::Tensor& carriers, bool ids) {
    check_host(offset, at::kLong, "offset"); check_host(n_samples, at::kInt, "n_samples");
    check_dev_f32(wave, "wave");
    const int64_t n = n_samples.numel();
    TORCH_CHECK(n_samples.dim() == 1 && n > 0 && n <= INT32_MAX && offset.numel() == n,
                "f5hip::", op, ": offset and n_samples need one value per clip, and at least one clip");
    TORCH_CHECK(wave.dim() == 1, "f5hip::", op, ": wave must be a contiguous 1-D fp32 tensor on a HIP device");
    const int16_t* cp = check_carriers(op, carriers, wave.device(), ids, ids ? kWdIdKeysMax : kWmKeysMax);
    const int64_t* off = offset.data_ptr<int64_t>();
    const int32_t* ns = n_samples.data_ptr<int32_t>();
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(ns[i] >= 1 && ns[i] <= kRdMaxSamples, "f5hip::", op, ": clip ", i, " has ", ns[i], " samples (1 .. ", kRdMaxSamples, ")");
        TORCH_CHECK(off[i] >= 0 && off[i] + ns[i] <= wave.numel(), "f5hip::", op, ": clip ", i, " is samples [", off[i], ", ", off[i] + ns[i],
                    ") of a tensor of ", wave.numel());
    }
    const c10::DeviceGuard guard(wave.device());
    at::Tensor rows = at::empty({n, carriers.size(0), ids ? kWdIdRowWords : 4}, wave.options());
    if (ids) {
        const int rc = f5hip_watermark_read_ids((int32_t)n, wave.data_ptr<float>(), off, ns, (int32_t)carriers.size(0), cp, rows.data_ptr<float>(), stream_of(wave));
        TORCH_CHECK(rc == 0, "f5hip_watermark_read_ids: ", f5hip_last_error());
    } else {
        const int rc = f5hip_watermark_detect((int32_t)n, wave.data_ptr<float>(), off, ns, (int32_t)carriers.size(0), cp, rows.data_ptr<float>(), stream_of(wave));
        TORCH_CHECK(rc == 0, "f5hip_watermark_detect: ", f5hip_last_error());
    }
    return rows;
}

// wave: the contiguous 1-D fp32 device tensor that holds every clip (mono, 24 kHz), read only; offset [n] int64 host, n_samples [n] int32 host:
// clip i is wave[offset[i] : offset[i] + n_samples[i]], disjoint ranges; carriers int16 device [n_keys, 16384] -> scores fp32 device
// [n, n_keys, 4]: z, offset, r at the offset, the deviation of r
at::Tensor watermark_detect(const at::Tensor& wave, const at::Tensor& offset, const at::Tensor& n_samples, const at::Tensor& carriers) {
    return watermark_rows("watermark_detect", wave, offset, n_samples, carriers, false);
}

// watermark_detect with trace ids: carriers int16 device [n_keys, 4, 16384], 1 .. 4 keys -> rows fp32 device [n, n_keys, 10]:
// watermark_detect's four, then (s_d, z_d) of the three symbols (include/f5hip.h f5hip_watermark_read_ids)
at::Tensor watermark_read_ids(const at::Tensor& wave, const at::Tensor& offset, const at::Tensor& n_samples, const at::Tensor& carriers) {
    return watermark_rows("watermark_read_ids", wave, offset, n_samples, carriers, true);
}

// wave: ONE recording, a contiguous 1-D fp32 device tensor (mono, 24 kHz, 1 .. 14 400 000 samples), read only; first_segment, n_segments [n_ranges]
// int32 host: range i is that many segments of 16384 samples from that segment; carriers int16 device [n_keys, 16384] (1 .. 16 keys) ->
// rows fp32 device [n_ranges, n_keys, 4], watermark_detect's row per range, or [n_keys, 4, 16384] (1 .. 4 keys) -> [n_ranges, n_keys, 10],
// watermark_read_ids' (include/f5hip.h f5hip_watermark_scan)
at::Tensor watermark_scan(const at::Tensor& wave, const at::Tensor& first_segment, const at::Tensor& n_segments, const at::Tensor& carriers) {
    check_host(first_segment, at::kInt, "first_segment"); check_host(n_segments, at::kInt, "n_segments");
    check_dev_f32(wave, "wave");
    const int64_t n = n_segments.numel();
    TORCH_CHECK(n_segments.dim() == 1 && n >= 1 && n <= kWsRangesMax && first_segment.numel() == n,
                "f5hip::watermark_scan: first_segment and n_segments need one value per range, 1 .. ", kWsRangesMax, " ranges");
    TORCH_CHECK(wave.dim() == 1 && wave.numel() >= 1 && wave.numel() <= kWsMaxSamples,
                "f5hip::watermark_scan: wave must be a contiguous 1-D fp32 tensor of 1 .. ", kWsMaxSamples, " samples on a HIP device (got ", wave.numel(), ")");
    const bool ids = carriers.dim() == 3;
    const int16_t* cp = check_carriers("watermark_scan", carriers, wave.device(), ids, ids ? kWdIdKeysMax : kWmKeysMax);
    const int32_t* first = first_segment.data_ptr<int32_t>();
    const int32_t* count = n_segments.data_ptr<int32_t>();
    for (int64_t i = 0; i < n; i++)
        TORCH_CHECK(ws_range_ok(wave.numel(), first[i], count[i]), "f5hip::watermark_scan: range ", i, " is ", count[i], " segments from segment ", first[i],
                    " of a recording of ", ws_segments(wave.numel()));
    const c10::DeviceGuard guard(wave.device());
    at::Tensor rows = at::empty({n, carriers.size(0), ids ? kWdIdRowWords : 4}, wave.options());
    const int rc = f5hip_watermark_scan(wave.data_ptr<float>(), wave.numel(), (int32_t)n, first, count, (int32_t)carriers.size(0), ids ? 1 : 0, cp,
                                        rows.data_ptr<float>(), stream_of(wave));
    TORCH_CHECK(rc == 0, "f5hip_watermark_scan: ", f5hip_last_error());
    return rows;
}

// raw: the contiguous 1-D fp32 device tensor that holds the raw clips (what f5hip_ref_frontend is handed), read only; raw_offset [n] int64,
// channels [n] int32, raw_len [n] int32 host: clip i is channels[i] x raw_len[i] samples at raw[raw_offset[i]]; wave, offset, n_samples as
// ref_denoise's (read only) -> rows int64 device [n, 10] (include/f5hip.h f5hip_ref_assess)
at::Tensor ref_assess(const at::Tensor& raw, const at::Tensor& raw_offset, const at::Tensor& channels, const at::Tensor& raw_len, const at::Tensor& wave,
                      const at::Tensor& offset, const at::Tensor& n_samples) {
    check_host(raw_offset, at::kLong, "raw_offset"); check_host(channels, at::kInt, "channels"); check_host(raw_len, at::kInt, "raw_len");
    check_host(offset, at::kLong, "offset"); check_host(n_samples, at::kInt, "n_samples");
    check_dev_f32(raw, "raw"); check_dev_f32(wave, "wave");
    const int64_t n = n_samples.numel();
    TORCH_CHECK(n_samples.dim() == 1 && n >= 1 && n <= kRaMaxClips && offset.numel() == n && raw_offset.numel() == n && channels.numel() == n && raw_len.numel() == n,
                "f5hip::ref_assess: the five tables need one value per clip, 1 .. ", kRaMaxClips, " clips");
    TORCH_CHECK(raw.dim() == 1 && wave.dim() == 1 && raw.device() == wave.device(), "f5hip::ref_assess: raw and wave must be contiguous 1-D fp32 tensors on one HIP device");
    const int64_t *ro = raw_offset.data_ptr<int64_t>(), *off = offset.data_ptr<int64_t>();
    const int32_t *ch = channels.data_ptr<int32_t>(), *rl = raw_len.data_ptr<int32_t>(), *ns = n_samples.data_ptr<int32_t>();
    for (int64_t i = 0; i < n; i++) {
        TORCH_CHECK(ch[i] >= 1 && ch[i] <= kRaMaxChannels, "f5hip::ref_assess: clip ", i, " has ", ch[i], " channels (1 .. ", kRaMaxChannels, ")");
        TORCH_CHECK(rl[i] >= 1 && ro[i] >= 0 && ro[i] + (int64_t)rl[i] * ch[i] <= raw.numel(), "f5hip::ref_assess: raw clip ", i, " is ", ch[i], " x ", rl[i],
                    " samples at ", ro[i], " of a tensor of ", raw.numel());
        TORCH_CHECK(ns[i] >= 1 && ns[i] <= kRdMaxSamples, "f5hip::ref_assess: clip ", i, " has ", ns[i], " samples (1 .. ", kRdMaxSamples, ")");
        TORCH_CHECK(off[i] >= 0 && off[i] + ns[i] <= wave.numel(), "f5hip::ref_assess: clip ", i, " is samples [", off[i], ", ", off[i] + ns[i], ") of a tensor of ",
                    wave.numel());
    }
    const c10::DeviceGuard guard(wave.device());
    at::Tensor rows = at::empty({n, kRaRowWords}, wave.options().dtype(at::kLong));
    const int rc = f5hip_ref_assess((int32_t)n, raw.data_ptr<float>(), ro, ch, rl, wave.data_ptr<float>(), off, ns, rows.data_ptr<int64_t>(), stream_of(wave));
    TORCH_CHECK(rc == 0, "f5hip_ref_assess: ", f5hip_last_error());
    return rows;
}

}   // namespace

TORCH_LIBRARY(f5hip, m) {
    m.def("cfm_sample(int handle, Tensor dur, Tensor? kv_len, Tensor cond, Tensor cond_mask, Tensor text, Tensor y0, Tensor t_grid, float cfg_strength) -> Tensor", &cfm_sample);
    m.def("cfm_sample_units(int handle, Tensor dur, Tensor? kv_len, Tensor cond, Tensor cond_mask, Tensor text, Tensor y0, Tensor t_grid, Tensor cfg_strength) -> Tensor", &cfm_sample_units);
    m.def("cfm_sample_grids(int handle, Tensor dur, Tensor? kv_len, Tensor cond, Tensor cond_mask, Tensor text, Tensor y0, Tensor steps, Tensor t_grids, Tensor cfg_strength) -> Tensor", &cfm_sample_grids);
    m.def("cfm_sample_span(int handle, Tensor dur, Tensor? kv_len, Tensor cond, Tensor cond_mask, Tensor text, Tensor y0, Tensor steps, Tensor t_grids, Tensor cfg_strength, Tensor last) -> Tensor", &cfm_sample_span);
    m.def("cfm_sample_methods(int handle, Tensor dur, Tensor? kv_len, Tensor cond, Tensor cond_mask, Tensor text, Tensor y0, Tensor steps, Tensor t_grids, Tensor cfg_strength, Tensor method, Tensor? last) -> Tensor", &cfm_sample_methods);
    m.def("vocos_decode(int handle, Tensor mel, int hop_length) -> Tensor", &vocos_decode);
    m.def("vocos_decode_ragged(int handle, Tensor mel, Tensor frames, int channels, int hop_length) -> Tensor", &vocos_decode_ragged);
    m.def("bigvgan_forward(int handle, Tensor mel, int total_upsample) -> Tensor", &bigvgan_forward);
    m.def("bigvgan_forward_ragged(int handle, Tensor mel, Tensor frames, int channels, int total_upsample) -> Tensor", &bigvgan_forward_ragged);
    m.def("ref_frontend(Tensor wave, Tensor n_in, Tensor channels, int orig_freq, int new_freq, Tensor? taps, float rms_floor) -> (Tensor, Tensor)", &ref_frontend);
    m.def("wave_finish(Tensor[] chunks, Tensor chunks_per_request, int fade, Tensor remove_silence, int sample_rate) -> (Tensor, Tensor)", &wave_finish);
    m.def("wave_finish_joins(Tensor[] chunks, Tensor chunks_per_request, int fade, Tensor chunk_fade, Tensor remove_silence, int sample_rate) -> (Tensor, Tensor)", &wave_finish_joins);
    m.def("mel_spectrogram_ragged(Tensor[] waves, int n_fft, int hop_length, int n_mels, int sample_rate, int variant) -> Tensor", &mel_spectrogram_ragged);
    m.def("wave_encode(Tensor[] pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, int new_freq, int encoding, Tensor? taps) -> (Tensor, Tensor, Tensor)", &wave_encode);
    m.def("wave_flac(Tensor[] pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, int sample_rate) -> (Tensor, Tensor, Tensor)", &wave_flac);
    m.def("wave_flac_levels(Tensor[] pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, int sample_rate, Tensor level) -> (Tensor, Tensor, Tensor)",
          &wave_flac_levels);
    m.def("flac_decode(Tensor data, Tensor begin, Tensor end, Tensor info, Tensor total, Tensor max_samples) -> (Tensor, Tensor)", &flac_decode);
    m.def("ref_prestep(Tensor frames, Tensor n_in, Tensor channels, Tensor clip_short, int rate) -> (Tensor, Tensor)", &ref_prestep);
    m.def("wave_loudness(Tensor(a!) pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor gain_k) -> Tensor", &wave_loudness);
    m.def("wave_prosody(Tensor pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor stretch_p, Tensor stretch_q, Tensor pitch, Tensor? taps) -> "
          "(Tensor, Tensor, Tensor, Tensor)", &wave_prosody);
    m.def("wave_prosody_formants(Tensor pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor stretch_p, Tensor stretch_q, Tensor pitch, "
          "Tensor keep_formants, Tensor? taps) -> (Tensor, Tensor, Tensor, Tensor)", &wave_prosody_formants);
    m.def("ref_denoise(Tensor(a!) wave, Tensor offset, Tensor n_samples) -> ()", &ref_denoise);
    m.def("wave_mark(Tensor(a!) pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor key_index, Tensor? carriers) -> ()", &wave_mark);
    m.def("watermark_detect(Tensor wave, Tensor offset, Tensor n_samples, Tensor carriers) -> Tensor", &watermark_detect);
    m.def("wave_mark_ids(Tensor(a!) pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor key_index, Tensor id, Tensor? carriers) -> ()", &wave_mark_ids);
    m.def("watermark_read_ids(Tensor wave, Tensor offset, Tensor n_samples, Tensor carriers) -> Tensor", &watermark_read_ids);
    m.def("watermark_scan(Tensor wave, Tensor first_segment, Tensor n_segments, Tensor carriers) -> Tensor", &watermark_scan);
    m.def("ref_assess(Tensor raw, Tensor raw_offset, Tensor channels, Tensor raw_len, Tensor wave, Tensor offset, Tensor n_samples) -> Tensor", &ref_assess);
}

// libf5hip: C ABI (include/f5hip.h) + host orchestration of the DiT / CFM path on one MI355X.
// One process per GPU; every call enqueues its kernels on the caller's HIP stream.
#include "../../include/f5hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <algorithm>
#include <vector>

#include "common.h"
#include "elementwise.h"
#include "gemm_launch.h"
#include "host_util.h"

// Time points one sampler call can evaluate: the rows of the modulation table `mod`, of the time embeddings `temb` and of the sinusoid staging
static constexpr int kMaxTimePoints = 256;
// ... and the cap of a call whose units share one grid: one 128-point block of precompute_time's GEMM chain, the limit callers plan their
// step counts against (serve.py).  The tables hold two such blocks, so a mixed-grid call has room for the union of its units' grids.
static constexpr int kMaxGridPoints = 128;
static_assert(kMaxGridPoints <= kMaxTimePoints, "a one-grid call's points are rows of the same tables");

// =================================================================================================
// DiT model
// =================================================================================================

struct TextBlock {
    float *dw_w = nullptr, *dw_b = nullptr, *ln_w = nullptr, *ln_b = nullptr, *gamma = nullptr, *beta = nullptr;
    PackedW pw1, pw2;
};

// One residual stream's transformer-block linears, indexed by block.
struct BlockWeights {
    std::vector<PackedW> qkv, out, ff1, ff2;
    void resize(int n) { qkv.resize(n); out.resize(n); ff1.resize(n); ff2.resize(n); }
};

struct f5hip_dit {
    f5hip_dit_config cfg;
    int nsplit = 2;       // operand planes of the state-touching GEMMs (1 bf16, 2 split bf16)
    // per-handle settings (the process-wide setters are only their defaults)
    int attn_invariant = -1;          // f5hip_dit_set_attention_shape_invariant: -1 = follow f5hip_set_attention_shape_invariant
    ProfState* prof = nullptr;        // f5hip_dit_set_profiling: this handle's own HIP-event spans and totals (null: the process-wide state)
    HostStage up_meta, up_time[2], up_grid;   // pinned staging of the per-call uploads (row metadata; the two planes of the sinusoid table;
                                              // f5hip_cfm_sample_grids' unit tables)
    bool blk_f16 = false; // gemm_planes == 3: transformer-block GEMMs (QKV, out, FF1, FF2) take one fp16 plane per operand
    ParamStore params;
    bool finalized = false;
    // packed weights
    PackedW time1, time2, adaln, wx, wct, conv1, conv2, proj_out;
    BlockWeights blk;                 // the audio stream (DiT, UNetT, MMDiT audio)
    BlockWeights blk_c;               // MMDiT text stream (out / ff*: all but the last, context-pre-only block)
    std::vector<PackedW> wskip;       // UNetT skip projections (later half of the layers)
    std::vector<int> mod_c, mod_x;    // offsets of the blocks' text (MMDiT) / audio modulation vectors inside one row of `mod`
    int mod_final = 0;                // offset of the final norm's (scale, shift)
    std::vector<float*> g_attn, g_ff;                     // UNetT RMSNorm gains
    float *g_out = nullptr, *zeros = nullptr;
    std::vector<TextBlock> tblk;
    float *text_emb = nullptr, *text_pos = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    float *rope_row_cos = nullptr, *rope_row_sin = nullptr;   // [rows][32]: the rotary factors of every row of the current layout (workspace; rope_rows_kernel)
    int rope_max_pos = 0;
    int arch = 0;     // 0 = DiT (F5-TTS), 1 = UNetT (E2-TTS): one extra row per sequence carries the time token, 2 = MMDiT: the text tokens of
                      // every sequence are rows of their own stream, laid out behind all audio rows (rows [M, M + Mc))
    int td_pad = 0;   // text_dim rounded up to 32 (K padding of the step-invariant input-projection operand)
    int gw = 0;       // conv_pos_embed channels per group
    int n_adaln = 0;  // floats in one row of `mod` (0 for UNetT)
    // workspace
    int cap_rows = 0, cap_frames = 0, cap_seq = 0;
    DevBuf ws;   // one arena, carved below
    float *h = nullptr, *h0 = nullptr, *ce = nullptr, *pred = nullptr, *te = nullptr, *ty = nullptr, *gx = nullptr,
          *mod = nullptr, *xstate = nullptr, *xmid = nullptr, *temb = nullptr, *rk_k2 = nullptr, *rk_k3 = nullptr;
    int ode_method = 0;   // 0 = Euler, 1 = explicit midpoint, 2 = RK4 (3/8 rule; stages k1..k3 in xmid, rk_k2, rk_k3) (f5hip_dit_set_ode_method)
    std::vector<Plane2> skipbuf;
    Plane2 hn, c1, ao, ff, xs, tn, tg, act, sinp, t1, st;
    __bf16 *qk = nullptr, *vt = nullptr;
    int *meta = nullptr;   // device int arena
    int meta_cap = 0;
    // per-call metadata (device pointers into `meta`)
    int *d_row_pos, *d_row_start, *d_row_end, *d_row_seq, *d_row_token, *d_row_frame, *d_row_condframe, *d_row_keep,
        *d_seq_row0, *d_seq_len, *d_seq_kvlen, *d_urow_c, *d_urow_u, *d_frame_is_cond;
    float* d_frame_cfg = nullptr;   // CFG strength per frame (its unit's, or the call's), in `meta` with the other arrays (MetaLayout)
    int M = 0, n_seq = 0, n_frames = 0, max_len = 0;
    int Mc = 0, Rtot = 0;   // MMDiT: text-stream rows and all rows (= row pitch of the V^T buffer); Rtot == M otherwise
    int row_c0 = 0;         // MMDiT: first row of the text stream (all audio rows of the layout; M may be a prefix of them: cfm_sample_grids)
    std::vector<int> h_seq_row0, h_seqc_row0;   // layout of the last setup_sequences: first audio / text (MMDiT) row per sequence, then the end
    // f5hip_cfm_sample_grids: d_row_tp != null -> the modulation consumers read row r's vectors from row d_row_tp[r] of `mod` (and UNetT's time
    // token from temb[d_row_tp[row0]]); forward_step is then called with ti = 0.  grid_meta: row_unit [R], row_tp [R], frame_unit [U], the unit
    // time-point table and the per-unit step sizes.
    int* d_row_tp = nullptr;
    int* grid_meta = nullptr;
    size_t grid_cap = 0;
    int *d_j_row0 = nullptr, *d_j_len = nullptr, *d_j_kvlen = nullptr, *d_j_kv_row0 = nullptr, *d_j_kv2_row0 = nullptr, *d_j_kv2_len = nullptr;   // MMDiT joint attention: 2 n_seq pseudo-sequences
    bool any_masked = false;
    std::vector<int> h_seq_len;
    // precompute_time: the time points whose tables sinp, t1, st, mod (UNetT: temb) hold -- empty: none
    std::vector<float> time_key;
};

static int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

f5hip_dit* f5hip_dit_create(const f5hip_dit_config* cfg) {
    if (!cfg) { set_error("null config"); return nullptr; }
    if (cfg->dim % 128 || cfg->dim != cfg->heads * 64 || cfg->dim % 16 || cfg->text_dim % 4 || cfg->mel_dim > 128 || cfg->mel_dim % 4 ||
        cfg->dim / 16 > 64 || cfg->gemm_planes < 1 || cfg->gemm_planes > 3 || cfg->arch < 0 || cfg->arch > 2 ||
        (cfg->arch == 1 && (cfg->conv_layers != 0 || cfg->depth % 2)) || (cfg->conv_layers > 0 && cfg->text_dim % 32) ||
        (cfg->arch == 2 && (cfg->conv_layers != 0 || cfg->text_dim != cfg->dim || cfg->depth < 1))) {
        set_error("unsupported backbone geometry (need dim %% 128 == 0, dim == 64*heads, dim/16 <= 64, mel_dim <= 128, text conv needs text_dim %% 32 == 0; UNetT: even depth, no text conv)");
        return nullptr;
    }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        set_error("no HIP device: libf5hip has no CPU fallback");
        return nullptr;
    }
    f5hip_dit* m = new f5hip_dit();
    m->cfg = *cfg;
    m->nsplit = cfg->gemm_planes == 3 ? 2 : cfg->gemm_planes;
    // both backbones: against the reference's own digests mixed mode measures 3.1e-4 rms (F5-Base, 32 NFE) and 4.9e-4 (E2-Base, N = 2340,
    // 64 NFE) of the 1e-3 bound; the U-skip projections, the final norm + proj_out and the input embedding stay split bf16
    m->blk_f16 = cfg->gemm_planes == 3;
    m->arch = cfg->arch;
    m->td_pad = cfg->arch == 2 ? 0 : ceil_to(cfg->text_dim, 32);   // MMDiT: the text never enters the input projection (mmdit.py:64-70)
    m->gw = cfg->dim / 16;
    if (cfg->arch != 1) {   // per block [MMDiT text: 6 D, or 2 D in the last (context-pre-only) block][audio: 6 D], then the final 2 D
        int off = 0;
        for (int l = 0; l < cfg->depth; l++) {
            if (cfg->arch == 2) { m->mod_c.push_back(off); off += (l == cfg->depth - 1 ? 2 : 6) * cfg->dim; }
            m->mod_x.push_back(off); off += 6 * cfg->dim;
        }
        m->mod_final = off;
        m->n_adaln = off + 2 * cfg->dim;
    }
    return m;
}

static void free_packed(PackedW& w) { dev_free(w.hi); dev_free(w.lo); dev_free(w.bias); dev_free(w.frag); w = PackedW(); }

void f5hip_dit_destroy(f5hip_dit* m) {
    if (!m) return;
    for (PackedW* w : {&m->time1, &m->time2, &m->adaln, &m->wx, &m->wct, &m->conv1, &m->conv2, &m->proj_out}) free_packed(*w);
    for (BlockWeights* b : {&m->blk, &m->blk_c})
        for (auto* v : {&b->qkv, &b->out, &b->ff1, &b->ff2}) for (auto& w : *v) free_packed(w);
    for (auto& w : m->wskip) free_packed(w);
    for (auto* v : {&m->g_attn, &m->g_ff}) for (float* g : *v) dev_free(g);
    dev_free(m->g_out); dev_free(m->zeros);
    for (auto& b : m->tblk) {
        for (float* p : {b.dw_w, b.dw_b, b.ln_w, b.ln_b, b.gamma, b.beta}) dev_free(p);
        free_packed(b.pw1); free_packed(b.pw2);
    }
    for (float* p : {m->text_emb, m->text_pos, m->rope_cos, m->rope_sin}) dev_free(p);
    dev_free(m->ws.ptr);
    dev_free(m->meta);
    delete m->prof;
    dev_free(m->grid_meta);
    m->up_meta.release(); m->up_time[0].release(); m->up_time[1].release(); m->up_grid.release();
    delete m;
}

int f5hip_dit_load_param(f5hip_dit* m, const char* name, const float* data, int64_t numel) {
    return m ? m->params.load(m->finalized, name, data, numel) : fail(-1, "load_param: bad argument");
}

#define CK(x) do { int _r = (x); if (_r) return _r; } while (0)
#define CKL(name) do { hipError_t _e = hipGetLastError(); if (_e != hipSuccess) return fail(-7, "%s launch: %s", name, hipGetErrorString(_e)); } while (0)

// One grouped Conv1d(D, D, 31, groups 16) of ConvPositionEmbedding, w [D][D / 16][31] (nn.Conv1d layout), b [D], as 16 implicit GEMMs:
// group g is output rows g * 64 .. + 64 and K = 31 taps x 64 channels, each padded with zero weights from D / 16 to 64.
static int pack_conv_pos(PackedW& out, const float* w, const float* b, int D) {
    const int gw = D / 16, K = 31 * 64;
    std::vector<float> wp((size_t)16 * 64 * K, 0.0f), bp(16 * 64, 0.0f);
    for (int g = 0; g < 16; g++)
        for (int co = 0; co < gw; co++) {
            bp[g * 64 + co] = b[g * gw + co];
            for (int ci = 0; ci < gw; ci++)
                for (int tap = 0; tap < 31; tap++)
                    wp[((size_t)(g * 64 + co)) * K + tap * 64 + ci] = w[((size_t)(g * gw + co) * gw + ci) * 31 + tap];
        }
    return pack_linear(out, wp.data(), 16 * 64, K, K, bp.data());
}

// Packs one stream's block-l linears: q | k | v concatenated into one [3 D, D] weight, the out projection `out` and the feed-forward `ff`
// (FF1 and the QKV weight also in fragment order: the W-direct gemm5 kernels).  `attn` + to_{q,k,v} + `qkv_sfx` name the q / k / v
// linears; `out` empty: a block without out projection and feed-forward (MMDiT's last, context-pre-only text block).
static int pack_block(f5hip_dit* m, BlockWeights& w, int l, const std::string& attn, const char* qkv_sfx, const std::string& out, const std::string& ff) {
    const int D = m->cfg.dim, F = m->cfg.ff_mult * D;
    const ParamStore& P = m->params;
    std::vector<float> wq((size_t)3 * D * D), bq(3 * D);
    const char* nm[3] = {"to_q", "to_k", "to_v"};
    for (int i = 0; i < 3; i++) {
        GET_PARAM(wi, P, attn + nm[i] + qkv_sfx + ".weight", (int64_t)D * D);
        GET_PARAM(bi, P, attn + nm[i] + qkv_sfx + ".bias", D);
        memcpy(&wq[(size_t)i * D * D], wi->data(), sizeof(float) * D * D);
        memcpy(&bq[(size_t)i * D], bi->data(), sizeof(float) * D);
    }
    if (pack_linear(w.qkv[l], wq.data(), 3 * D, D, D, bq.data(), 128, m->blk_f16) || pack_frag(w.qkv[l])) return -4;
    if (out.empty()) return 0;
    GET_PARAM(wo, P, out + ".weight", (int64_t)D * D); GET_PARAM(bo, P, out + ".bias", D);
    if (pack_linear(w.out[l], wo->data(), D, D, D, bo->data(), 128, m->blk_f16)) return -4;
    GET_PARAM(w1, P, ff + "ff.0.0.weight", (int64_t)F * D); GET_PARAM(b1, P, ff + "ff.0.0.bias", F);
    if (pack_linear(w.ff1[l], w1->data(), F, D, D, b1->data(), 128, m->blk_f16) || pack_frag(w.ff1[l])) return -4;
    GET_PARAM(w2, P, ff + "ff.2.weight", (int64_t)D * F); GET_PARAM(b2, P, ff + "ff.2.bias", D);
    if (pack_linear(w.ff2[l], w2->data(), D, F, F, b2->data(), 128, m->blk_f16)) return -4;
    return 0;
}

// Rotary tables (x-transformers 2.2.8 RotaryEmbedding): [4097][32] cos / sin of angle = pos * 10000^(-2i/64) in fp32.
// 4097 rows: UNetT puts the time token at position 0, so a 4096-frame sequence reaches position 4096 (unett.py:184-188)
static void rope_tables(std::vector<float>& rc, std::vector<float>& rs) {
    rc.resize((size_t)4097 * 32); rs.resize((size_t)4097 * 32);
    for (int pos = 0; pos < 4097; pos++)
        for (int i = 0; i < 32; i++) {
            float inv = 1.0f / powf(10000.0f, (float)(2 * i) / 64.0f);
            float ang = (float)pos * inv;
            rc[(size_t)pos * 32 + i] = (float)cos((double)ang);
            rs[(size_t)pos * 32 + i] = (float)sin((double)ang);
        }
}

int f5hip_dit_finalize(f5hip_dit* m) {
    if (!m) return fail(-1, "null model");
    if (m->finalized) return 0;
    const f5hip_dit_config& c = m->cfg;
    const ParamStore& P = m->params;
    const int D = c.dim, Td = c.text_dim, mel = c.mel_dim;
    const std::string T = "transformer.";
    // --- time MLP + all AdaLN linears (one [depth*6D + 2D, D] matrix: modulation depends on t only) ---
    {
        GET_PARAM(w0, P, T + "time_embed.time_mlp.0.weight", (int64_t)D * 256);
        GET_PARAM(b0, P, T + "time_embed.time_mlp.0.bias", D);
        GET_PARAM(w2, P, T + "time_embed.time_mlp.2.weight", (int64_t)D * D);
        GET_PARAM(b2, P, T + "time_embed.time_mlp.2.bias", D);
        if (pack_linear(m->time1, w0->data(), D, 256, 256, b0->data())) return -4;
        if (pack_linear(m->time2, w2->data(), D, D, D, b2->data())) return -4;
    }
    if (m->arch != 1) {   // every AdaLN linear, at its offset in a row of `mod`: DiT attn_norm; MMDiTBlock attn_norm_c (AdaLayerNormZero, or _Final in
                          // the last block) and attn_norm_x (F/model/modules.py:593-594); then norm_out
        std::vector<float> wa((size_t)m->n_adaln * D), ba(m->n_adaln);
        auto put = [&](int off, const std::string& name, int rows) {
            const std::vector<float>* w = P.get(name + "weight", (int64_t)rows * D);
            const std::vector<float>* b = w ? P.get(name + "bias", rows) : nullptr;
            if (!b) return false;
            memcpy(&wa[(size_t)off * D], w->data(), sizeof(float) * (size_t)rows * D);
            memcpy(&ba[off], b->data(), sizeof(float) * rows);
            return true;
        };
        for (int l = 0; l < c.depth; l++) {
            const std::string p = T + "transformer_blocks." + std::to_string(l) + ".";
            if (m->arch == 2 && !put(m->mod_c[l], p + "attn_norm_c.linear.", (l == c.depth - 1 ? 2 : 6) * D)) return -3;
            if (!put(m->mod_x[l], p + (m->arch == 2 ? "attn_norm_x.linear." : "attn_norm.linear."), 6 * D)) return -3;
        }
        if (!put(m->mod_final, T + "norm_out.linear.", 2 * D)) return -3;
        if (pack_linear(m->adaln, wa.data(), m->n_adaln, D, D, ba.data())) return -4;
    }
    // --- text embedding ---
    {
        GET_PARAM(e, P, T + "text_embed.text_embed.weight", (int64_t)(c.text_num_embeds + 1) * Td);
        if (upload_f32(&m->text_emb, e->data(), e->size())) return -4;
        // precompute_freqs_cis (F/model/modules.py:196-207): [cos(pos w_j) || sin(pos w_j)], fp32 angle
        std::vector<float> tab((size_t)4096 * Td);
        for (int pos = 0; pos < 4096; pos++)
            for (int j = 0; j < Td / 2; j++) {
                float w = 1.0f / powf(10000.0f, (float)(2 * j) / (float)Td);
                float ang = (float)pos * w;
                tab[(size_t)pos * Td + j] = (float)cos((double)ang);
                tab[(size_t)pos * Td + Td / 2 + j] = (float)sin((double)ang);
            }
        if (upload_f32(&m->text_pos, tab.data(), tab.size())) return -4;
        m->tblk.resize(c.conv_layers);
        for (int i = 0; i < c.conv_layers; i++) {
            std::string p = T + "text_embed.text_blocks." + std::to_string(i) + ".";
            TextBlock& b = m->tblk[i];
            GET_PARAM(dw, P, p + "dwconv.weight", (int64_t)Td * 7); GET_PARAM(db, P, p + "dwconv.bias", Td);
            GET_PARAM(lw, P, p + "norm.weight", Td); GET_PARAM(lb, P, p + "norm.bias", Td);
            GET_PARAM(w1, P, p + "pwconv1.weight", (int64_t)2 * Td * Td); GET_PARAM(b1, P, p + "pwconv1.bias", 2 * Td);
            GET_PARAM(gg, P, p + "grn.gamma", 2 * Td); GET_PARAM(gb, P, p + "grn.beta", 2 * Td);
            GET_PARAM(w2, P, p + "pwconv2.weight", (int64_t)2 * Td * Td); GET_PARAM(b2, P, p + "pwconv2.bias", Td);
            if (upload_f32(&b.dw_w, dw->data(), dw->size()) || upload_f32(&b.dw_b, db->data(), db->size()) ||
                upload_f32(&b.ln_w, lw->data(), lw->size()) || upload_f32(&b.ln_b, lb->data(), lb->size()) ||
                upload_f32(&b.gamma, gg->data(), gg->size()) || upload_f32(&b.beta, gb->data(), gb->size())) return -4;
            if (pack_linear(b.pw1, w1->data(), 2 * Td, Td, Td, b1->data())) return -4;
            if (pack_linear(b.pw2, w2->data(), Td, 2 * Td, 2 * Td, b2->data())) return -4;
        }
    }
    // --- input projection split by source: x part (changes every step) | cond + text part (step invariant) ---
    {
        const bool mm = m->arch == 2;   // MMDiT: AudioEmbedding.linear over cat(x, cond) only (mmdit.py:60-70)
        const int Kin = 2 * mel + (mm ? 0 : Td);
        GET_PARAM(w, P, T + (mm ? "audio_embed.linear.weight" : "input_embed.proj.weight"), (int64_t)D * Kin);
        GET_PARAM(b, P, T + (mm ? "audio_embed.linear.bias" : "input_embed.proj.bias"), D);
        const int Kct = 128 + m->td_pad;
        std::vector<float> wx((size_t)D * 128, 0.0f), wct((size_t)D * Kct, 0.0f);
        for (int n = 0; n < D; n++) {
            for (int k = 0; k < mel; k++) {
                wx[(size_t)n * 128 + k] = (*w)[(size_t)n * Kin + k];
                wct[(size_t)n * Kct + k] = (*w)[(size_t)n * Kin + mel + k];
            }
            for (int k = 0; k < (mm ? 0 : Td); k++) wct[(size_t)n * Kct + 128 + k] = (*w)[(size_t)n * Kin + 2 * mel + k];
        }
        if (pack_linear(m->wx, wx.data(), D, 128, 128, nullptr)) return -4;
        if (pack_linear(m->wct, wct.data(), D, Kct, Kct, b->data())) return -4;
    }
    // --- conv_pos_embed: grouped Conv1d(D, D, 31, groups 16) as 16 implicit GEMMs, each padded to 64 x (31 x 64) ---
    for (int which = 0; which < 2; which++) {
        std::string p = T + (m->arch == 2 ? "audio_embed" : "input_embed") + ".conv_pos_embed.conv1d." + std::to_string(which * 2) + ".";
        GET_PARAM(w, P, p + "weight", (int64_t)D * m->gw * 31);
        GET_PARAM(b, P, p + "bias", D);
        if (pack_conv_pos(which ? m->conv2 : m->conv1, w->data(), b->data(), D)) return -4;
    }
    // --- transformer blocks ---
    m->blk.resize(c.depth);
    if (m->arch == 2) m->blk_c.resize(c.depth);
    if (m->arch == 1) { m->wskip.resize(c.depth); m->g_attn.assign(c.depth, nullptr); m->g_ff.assign(c.depth, nullptr); }
    for (int l = 0; l < c.depth; l++) {
        // DiT: transformer_blocks.{l}.attn.* / .ff.*  (F/model/modules.py:542-556);  UNetT: layers.{l}.{0 skip_proj, 1 attn_norm, 2 attn, 3 ff_norm, 4 ff}
        const std::string p = T + (m->arch != 1 ? "transformer_blocks." : "layers.") + std::to_string(l) + ".";
        const std::string pa = p + (m->arch != 1 ? "attn." : "2."), pf = p + (m->arch == 0 ? "ff." : (m->arch == 2 ? "ff_x." : "4."));
        CK(pack_block(m, m->blk, l, pa, "", pa + "to_out.0", pf));
        // MMDiT: the text stream's own projections (Attention(context_dim=...), F/model/modules.py:365-374) and feed-forward
        if (m->arch == 2) CK(pack_block(m, m->blk_c, l, pa, "_c", l < c.depth - 1 ? pa + "to_out_c" : "", p + "ff_c."));
        if (m->arch == 1) {
            GET_PARAM(ga, P, p + "1.g", D); GET_PARAM(gf, P, p + "3.g", D);
            if (upload_f32(&m->g_attn[l], ga->data(), D) || upload_f32(&m->g_ff[l], gf->data(), D)) return -4;
            if (l >= c.depth / 2) {
                GET_PARAM(ws, P, p + "0.weight", (int64_t)D * 2 * D);
                if (pack_linear(m->wskip[l], ws->data(), D, 2 * D, 2 * D, nullptr)) return -4;
            }
        }
    }
    if (m->arch == 1) {
        GET_PARAM(go, P, T + "norm_out.g", D);
        if (upload_f32(&m->g_out, go->data(), D)) return -4;
    }
    {
        std::vector<float> z(std::max(D, 4096), 0.0f);
        if (upload_f32(&m->zeros, z.data(), z.size())) return -4;
    }
    {
        GET_PARAM(w, P, T + "proj_out.weight", (int64_t)mel * D); GET_PARAM(b, P, T + "proj_out.bias", mel);
        if (pack_linear(m->proj_out, w->data(), mel, D, D, b->data())) return -4;
    }
    {
        std::vector<float> rc, rs;
        rope_tables(rc, rs);
        if (upload_f32(&m->rope_cos, rc.data(), rc.size()) || upload_f32(&m->rope_sin, rs.data(), rs.size())) return -4;
    }
    // pack_frag only enqueues its kernels: wait for every packing kernel and check them once before the weights are used
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(-4, "finalize: weight packing: %s", hipGetErrorString(e));
    m->params.host.clear();
    m->finalized = true;
    return 0;
}

// -------------------------------------------------------------------------------------------------
// workspace
// -------------------------------------------------------------------------------------------------
// The per-call int metadata arena (f5hip_dit::meta) of a layout of R rows, S sequences and U frames: the offset of every array, in ints, and
// the total.  The host fill and the device pointers (setup_sequences) and the capacity (ensure_workspace) all read it.
struct MetaLayout {
    size_t row_pos, row_start, row_end, row_seq, row_token, row_frame, row_condframe, row_keep;   // [R]
    size_t seq_row0, seq_len, seq_kvlen;                                                          // [S]
    size_t urow_c, urow_u, frame_is_cond;                                                         // [U]
    size_t j_row0, j_len, j_kvlen, j_kv_row0, j_kv2_row0, j_kv2_len;   // MMDiT joint attention: [2 S] pseudo-sequences (empty otherwise)
    size_t frame_cfg;                                                  // [U] floats
    size_t total = 0;
    MetaLayout(size_t R, size_t S, size_t U, bool mmdit) {
        auto take = [&](size_t n) { const size_t at = total; total += n; return at; };
        for (size_t* o : {&row_pos, &row_start, &row_end, &row_seq, &row_token, &row_frame, &row_condframe, &row_keep}) *o = take(R);
        for (size_t* o : {&seq_row0, &seq_len, &seq_kvlen}) *o = take(S);
        for (size_t* o : {&urow_c, &urow_u, &frame_is_cond}) *o = take(U);
        for (size_t* o : {&j_row0, &j_len, &j_kvlen, &j_kv_row0, &j_kv2_row0, &j_kv2_len}) *o = take(mmdit ? 2 * S : 0);
        frame_cfg = take(U);
    }
};
static_assert(sizeof(float) == sizeof(int), "frame_cfg rides in the int arena");

static int ensure_workspace(f5hip_dit* m, int rows_pad, int frames, int n_seq) {
    if (rows_pad <= m->cap_rows && frames <= m->cap_frames && n_seq <= m->cap_seq) return 0;
    const f5hip_dit_config& c = m->cfg;
    const int D = c.dim, Td = c.text_dim, F = c.ff_mult * D;
    const size_t R = (size_t)std::max(rows_pad, m->cap_rows), U = (size_t)std::max(frames, m->cap_frames),
                 S = (size_t)std::max(n_seq, m->cap_seq);
    if (alloc_workspace(&m->ws.ptr, "workspace", [&](Arena& a) {
            m->h = a.f32(R * D); m->h0 = a.f32(R * D); m->ce = a.f32(R * D); m->pred = a.f32(R * 128);
            m->te = a.f32(R * Td); m->ty = a.f32(R * 2 * Td); m->gx = a.f32(S * 2 * Td);
            m->rope_row_cos = a.f32(R * 32); m->rope_row_sin = a.f32(R * 32);
            m->mod = a.f32((size_t)kMaxTimePoints * m->n_adaln + 64); m->xstate = a.f32(U * c.mel_dim); m->xmid = a.f32(U * c.mel_dim);
            m->temb = a.f32((size_t)kMaxTimePoints * D);
            m->hn = a.plane2(R * D + 256); m->c1 = a.plane2(R * D + 256); m->ao = a.plane2(R * D); m->ff = a.plane2(R * F);
            m->xs = a.plane2(R * 128); m->tn = a.plane2(R * Td); m->tg = a.plane2(R * 2 * Td); m->act = a.plane2(R * (128 + m->td_pad));
            m->sinp = a.plane2(kMaxTimePoints * 256); m->t1 = a.plane2((size_t)kMaxTimePoints * D); m->st = a.plane2((size_t)kMaxTimePoints * D);
            m->skipbuf.resize(m->arch == 1 ? c.depth / 2 : 0);
            for (auto& sb : m->skipbuf) sb = a.plane2(R * 2 * D);   // [R][2 D]: the concatenated operand [x || skip] of the U-skip Linear, built in place
            // qk: +256 rows because the last query tile of the attention (up to 256 queries) may read (never store) past the padded rows
            m->qk = a.bf16((R + 256) * 2 * D); m->vt = a.bf16((size_t)D * R);
            m->rk_k2 = a.f32(U * c.mel_dim); m->rk_k3 = a.f32(U * c.mel_dim);
        })) { m->cap_rows = 0; m->time_key.clear(); return -5; }
    m->time_key.clear();   // the time tables moved with the arena
    m->cap_rows = (int)R; m->cap_frames = (int)U; m->cap_seq = (int)S;
    const int need = (int)MetaLayout(R, S, U, m->arch == 2).total;
    if (need > m->meta_cap) {
        dev_free(m->meta);
        if (hipMalloc((void**)&m->meta, sizeof(int) * need) != hipSuccess) { m->meta = nullptr; m->meta_cap = 0; return fail(-5, "hipMalloc meta"); }
        m->meta_cap = need;
    }
    return 0;
}

// The packed row layout: every sequence starts at a multiple of 128 rows and takes ceil128(lead + len) rows.  Its `lead` leading rows (UNetT:
// the time token) belong to it (row_seq) but keep start = end = 0, an empty convolution window; its frames r0 + lead .. + len carry the
// sequence bounds [r0 + lead, r0 + lead + len).  Rows outside every sequence keep the defaults: start = end = 0, row_seq = -1.
static int seq_rows(int len, int lead) { return ceil_to(len + lead, 128); }
static void set_seq_bounds(int* row_start, int* row_end, int* row_seq, int r0, int lead, int len, int s) {
    for (int j = 0; j < lead; j++) row_seq[r0 + j] = s;
    for (int i = 0; i < len; i++) {
        const int r = r0 + lead + i;
        row_start[r] = r0 + lead; row_end[r] = r0 + lead + len; row_seq[r] = s;
    }
}

struct SeqDesc { int len, kvlen, frame0 /* first frame in caller's packed arrays */, text_row, drop_audio, drop_text, branch /* 0 cond, 1 uncond */;
                 int c_len = 0 /* MMDiT: rows of the text stream (tokens incl. filler positions, as the reference's [b, nt] text tensor has them) */; };

// Lays the sequences out (each padded to a multiple of 128 rows), builds the per-row metadata and uploads it.
// UNetT: row 0 of every sequence is the time token (F/model/backbones/unett.py:184); frames follow at rows 1..len.
// frame_cfg (n_frames floats, or null = zeros): per-frame CFG strengths, uploaded with the rest (m->d_frame_cfg).
// frame_final (n_frames flags, or null = frame_is_cond): which frames the sampler's final select overwrites with the conditioning.
static int setup_sequences(f5hip_dit* m, const std::vector<SeqDesc>& seqs, int n_frames, const int32_t* text, int nt_max,
                           const uint8_t* frame_is_cond, hipStream_t st, const float* frame_cfg = nullptr, const uint8_t* frame_final = nullptr) {
    const int extra = m->arch == 1 ? 1 : 0;
    const bool mm = m->arch == 2;
    int rows = 0, rows_x = 0;
    for (auto& s : seqs) rows += seq_rows(s.len, extra);
    rows_x = rows;
    if (mm) for (auto& s : seqs) {
        if (s.c_len <= 0 || s.c_len > 4096) return fail(-1, "MMDiT: a sequence needs 1..4096 text positions (got %d)", s.c_len);
        rows += seq_rows(s.c_len, 0);
    }
    if (ensure_workspace(m, rows, n_frames, (int)seqs.size())) return -5;
    const int R = rows, S = (int)seqs.size(), U = n_frames;
    const MetaLayout ml(R, S, U, mm);
    std::vector<int> hbuf(ml.total, 0);
    if (frame_cfg) memcpy(&hbuf[ml.frame_cfg], frame_cfg, sizeof(float) * U);
    int* const hb = hbuf.data();
    int* row_pos = hb + ml.row_pos; int* row_start = hb + ml.row_start; int* row_end = hb + ml.row_end; int* row_seq = hb + ml.row_seq;
    int* row_token = hb + ml.row_token; int* row_frame = hb + ml.row_frame; int* row_condframe = hb + ml.row_condframe; int* row_keep = hb + ml.row_keep;
    int* seq_row0 = hb + ml.seq_row0; int* seq_len = hb + ml.seq_len; int* seq_kvlen = hb + ml.seq_kvlen;
    int* urow_c = hb + ml.urow_c; int* urow_u = hb + ml.urow_u; int* fic = hb + ml.frame_is_cond;
    int r0 = 0;
    m->any_masked = false;
    m->h_seq_row0.assign(S + 1, 0); m->h_seqc_row0.assign(S + 1, rows_x);
    for (int r = 0; r < R; r++) { row_seq[r] = -1; row_token[r] = -1; row_frame[r] = -1; row_condframe[r] = -1; }
    for (int u = 0; u < U; u++) { urow_c[u] = -1; urow_u[u] = -1; fic[u] = frame_final ? frame_final[u] : frame_is_cond ? frame_is_cond[u] : 0; }
    m->max_len = 0;
    for (int s = 0; s < S; s++) {
        const SeqDesc& q = seqs[s];
        seq_row0[s] = r0; seq_len[s] = q.len + extra; seq_kvlen[s] = q.kvlen + extra;
        m->max_len = std::max(m->max_len, q.len + extra);
        if (q.kvlen < q.len) m->any_masked = true;
        if (extra) { row_pos[r0] = 0; row_keep[r0] = 1; }   // time token: start = end = 0 keeps it out of the convs
        set_seq_bounds(row_start, row_end, row_seq, r0, extra, q.len, s);
        for (int i = 0; i < q.len; i++) {
            const int r = r0 + extra + i;
            row_pos[r] = i + extra;                                   // rotary position (time token = 0)
            int tok = 0;
            if (!q.drop_text && i < nt_max) tok = text[(size_t)q.text_row * nt_max + i] + 1;   // -1 pad -> filler 0
            // nn.Embedding raises IndexError on an id outside the table; here it would be an out-of-bounds read on the GPU
            if (tok < 0 || tok > m->cfg.text_num_embeds) return fail(-1, "text token %d of sequence %d is outside the vocabulary (0..%d)", tok - 1, s, m->cfg.text_num_embeds - 1);
            row_token[r] = tok;
            row_frame[r] = q.frame0 + i;
            const bool is_c = frame_is_cond ? frame_is_cond[q.frame0 + i] != 0 : true;
            row_condframe[r] = (!q.drop_audio && is_c) ? q.frame0 + i : -1;
            row_keep[r] = i < q.kvlen ? 1 : 0;
            (q.branch ? urow_u : urow_c)[q.frame0 + i] = r;
        }
        r0 += seq_rows(q.len, extra);
        m->h_seq_row0[s + 1] = r0;
    }
    if (mm) {   // joint attention: 2 S pseudo-sequences (2 s: audio queries of sequence s, 2 s + 1: its text queries)
        int rc0 = rows_x;
        for (int s = 0; s < S; s++) {
            const SeqDesc& q = seqs[s];
            set_seq_bounds(row_start, row_end, row_seq, rc0, 0, q.c_len, s);
            for (int i = 0; i < q.c_len; i++) {
                const int r = rc0 + i;
                int tok = 0;   // filler (the reference feeds text + 1 with -1 padding -> 0; all ids 0 when the text is dropped: mmdit.py:38-40)
                if (!q.drop_text && i < nt_max) tok = text[(size_t)q.text_row * nt_max + i] + 1;
                if (tok < 0 || tok > m->cfg.text_num_embeds) return fail(-1, "text token %d of sequence %d is outside the vocabulary (0..%d)", tok - 1, s, m->cfg.text_num_embeds - 1);
                row_pos[r] = i; row_token[r] = tok; row_keep[r] = 1;
            }
            for (int qd = 0; qd < 2; qd++) {
                const int j = 2 * s + qd;
                hb[ml.j_row0 + j] = qd ? rc0 : seq_row0[s];   // query rows
                hb[ml.j_len + j] = qd ? q.c_len : q.len;
                hb[ml.j_kvlen + j] = q.kvlen;                 // first key range: the audio rows, padding masked
                hb[ml.j_kv_row0 + j] = seq_row0[s];
                hb[ml.j_kv2_row0 + j] = rc0;                  // second key range: the text rows, never masked (F/model/modules.py:508)
                hb[ml.j_kv2_len + j] = q.c_len;
            }
            m->max_len = std::max(m->max_len, q.c_len);
            rc0 += seq_rows(q.c_len, 0);
            m->h_seqc_row0[s + 1] = rc0;
        }
    }
    if (const int r_ = m->up_meta.upload(m->meta, hbuf.data(), sizeof(int) * hbuf.size(), st)) return r_;   // (pinned staging: no host sync)
    int* const d = m->meta;
    m->d_row_pos = d + ml.row_pos; m->d_row_start = d + ml.row_start; m->d_row_end = d + ml.row_end; m->d_row_seq = d + ml.row_seq;
    m->d_row_token = d + ml.row_token; m->d_row_frame = d + ml.row_frame; m->d_row_condframe = d + ml.row_condframe; m->d_row_keep = d + ml.row_keep;
    m->d_seq_row0 = d + ml.seq_row0; m->d_seq_len = d + ml.seq_len; m->d_seq_kvlen = d + ml.seq_kvlen;
    m->d_urow_c = d + ml.urow_c; m->d_urow_u = d + ml.urow_u; m->d_frame_is_cond = d + ml.frame_is_cond;
    m->d_j_row0 = d + ml.j_row0; m->d_j_len = d + ml.j_len; m->d_j_kvlen = d + ml.j_kvlen; m->d_j_kv_row0 = d + ml.j_kv_row0;
    m->d_j_kv2_row0 = d + ml.j_kv2_row0; m->d_j_kv2_len = d + ml.j_kv2_len;
    m->d_frame_cfg = reinterpret_cast<float*>(d + ml.frame_cfg);
    // rotary factors per row of this layout (one load in the QKV epilogues instead of row_pos -> table)
    hipLaunchKernelGGL(rope_rows_kernel, dim3((R * 32 + 255) / 256), dim3(256), 0, st, m->d_row_pos, m->rope_cos, m->rope_sin, R, 4097, m->rope_row_cos, m->rope_row_sin);
    if (hipGetLastError() != hipSuccess) return fail(-7, "rope_rows_kernel launch");
    m->M = rows_x; m->Mc = R - rows_x; m->Rtot = R; m->n_seq = S; m->n_frames = U; m->row_c0 = rows_x;
    return 0;
}

// -------------------------------------------------------------------------------------------------
// launch helpers
// -------------------------------------------------------------------------------------------------
static Plane2 rows_from(const Plane2& p, size_t off) { return {p.hi + off, p.lo + off}; }

static GemmArgs gemm_base(const Plane2& A, int lda, const PackedW& W, int M) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A[0] = A.hi; a.A[1] = A.lo; a.lda = lda;
    a.W[0] = W.hi; a.W[1] = W.lo; a.Wf = W.frag;
    a.M = M; a.N = W.n; a.K = W.k_pad; a.ldw = W.ld;
    a.bias = W.bias;
    return a;
}

// f5hip_get_counter: gemm5 launches with RB 11 / RB 8 / 1 x 4 consumer layout (cb 8 or 12) / gemm3 wide-tile launches / conv5 launches /
// gemm6 launches; then gemm6 by tile height (176 / 256 rows), gemm5 with cb 12, every gemm3 launch, every gemm.h launch by bn (64 / 128)
// ... and dit_rows: the summed (audio) rows M of every backbone forward; ref_frontend_launches: kernels f5hip_ref_frontend launched, and its
// resampling launches by where the tap table was read from (ref_taps_lds / ref_taps_l2); wave_finish_launches / wave_finish_requests: kernels
// f5hip_wave_finish launched and requests it finished; wave_encode_launches / wave_encode_requests: the same for f5hip_wave_encode;
// mel_ragged_launches / mel_ragged_items: launches of f5hip_mel_spectrogram_ragged and the clips they covered; wave_flac_launches /
// wave_flac_requests: kernels f5hip_wave_flac launched and requests it encoded; wave_loudness_launches / wave_loudness_requests: kernels
// f5hip_wave_loudness launched and the flagged requests it normalised; flac_decode_launches / flac_decode_streams: kernels f5hip_flac_decode
// launched and the streams it was given; ref_prestep_launches / ref_prestep_clips: the same for f5hip_ref_prestep and its clips;
// wave_prosody_launches / wave_prosody_requests: kernels f5hip_wave_prosody launched and the requests whose tempo or pitch it changed;
// ref_denoise_launches / ref_denoise_clips: kernels f5hip_ref_denoise launched and the clips it denoised; wave_mark_launches /
// wave_mark_requests: kernels f5hip_wave_mark launched and the requests it marked; wave_formant_launches / wave_formant_requests: the
// kernels f5hip_wave_prosody_formants launched beyond f5hip_wave_prosody's and the requests that kept their formants; watermark_detect_launches / watermark_detect_clips:
// kernels f5hip_watermark_detect launched and the clips it scored; ref_assess_launches / ref_assess_clips: kernels f5hip_ref_assess launched
// and the clips it measured; gemm3_thin: the gemm3 launches (counted in gemm3 too) that took the 32-row instance; time_table_builds: calls of
// precompute_time that built the tables (the others found the handle's tables built for the same time points); wave_mark_id_launches /
// wave_mark_id_requests: kernels f5hip_wave_mark_ids launched in calls where a request carried a trace id and the requests such calls marked
// (a call without an id counts on wave_mark_*); watermark_read_ids_launches / watermark_read_ids_clips: kernels f5hip_watermark_read_ids
// launched and the clips it read; watermark_scan_launches / watermark_scan_ranges: kernels f5hip_watermark_scan launched and the ranges it scored
enum { CNT_GEMM5_RB11, CNT_GEMM5_RB8, CNT_GEMM5_WIDE, CNT_GEMM3_WIDE, CNT_CONV5, CNT_GEMM6, CNT_GEMM6_R176, CNT_GEMM6_R256, CNT_GEMM5_CB12,
       CNT_GEMM3, CNT_GEMM_REG_BN64, CNT_GEMM_REG_BN128, CNT_DIT_ROWS, CNT_REF_LAUNCHES, CNT_REF_TAPS_LDS, CNT_REF_TAPS_L2, CNT_WAVE_LAUNCHES,
       CNT_WAVE_REQUESTS, CNT_WAVE_ENCODE_LAUNCHES, CNT_WAVE_ENCODE_REQUESTS, CNT_MEL_RAGGED_LAUNCHES, CNT_MEL_RAGGED_ITEMS, CNT_WAVE_FLAC_LAUNCHES,
       CNT_WAVE_FLAC_REQUESTS, CNT_WAVE_LOUDNESS_LAUNCHES, CNT_WAVE_LOUDNESS_REQUESTS, CNT_FLAC_DECODE_LAUNCHES, CNT_FLAC_DECODE_STREAMS,
       CNT_REF_PRESTEP_LAUNCHES, CNT_REF_PRESTEP_CLIPS, CNT_WAVE_PROSODY_LAUNCHES, CNT_WAVE_PROSODY_REQUESTS,
       CNT_REF_DENOISE_LAUNCHES, CNT_REF_DENOISE_CLIPS, CNT_WAVE_MARK_LAUNCHES, CNT_WAVE_MARK_REQUESTS, CNT_WAVE_FORMANT_LAUNCHES,
       CNT_WAVE_FORMANT_REQUESTS, CNT_WATERMARK_DETECT_LAUNCHES,
       CNT_WATERMARK_DETECT_CLIPS, CNT_REF_ASSESS_LAUNCHES, CNT_REF_ASSESS_CLIPS, CNT_GEMM3_THIN, CNT_TIME_TABLE_BUILDS,
       CNT_WAVE_MARK_ID_LAUNCHES, CNT_WAVE_MARK_ID_REQUESTS, CNT_WATERMARK_READ_IDS_LAUNCHES, CNT_WATERMARK_READ_IDS_CLIPS,
       CNT_WATERMARK_SCAN_LAUNCHES, CNT_WATERMARK_SCAN_RANGES, CNT_COUNT };
static long long g_counters[CNT_COUNT] = {};

// Kernel choice per GEMM (measured: profiles/r02_fillrate_microbench.txt, profiles/r01_gemm_microbench.txt):
//   fp16 one-plane operands: gemm6 for the batch-mode shapes (gemm6_choose_rows), else gemm5 (exact-fit tiles) when K % 64 == 0,
//   else gemm3; implicit-GEMM convolutions in fp16 on gemm.h;
//   one 128 x 128 tile per CU or fewer, generic epilogue, bf16 / split-bf16 operands: gemm3 (warp-specialised LDS-DMA ring);
//   everything else (implicit-GEMM convolutions, QKV in split-bf16, many-tile shapes): gemm.h, two 4-wave workgroups per CU.
// gemm3, generic epilogue: the thin 32-row instance while its grid is one round on the 256 CUs (one 8-wave workgroup per CU).  Measured per
// shape in profiles/thin_tiles_unit_bench.txt: 0.49 - 0.73 of the 128-row instance's time up to 256 thin workgroups, 1.16 - 1.72 from 352 on
// (a second round of 32-deep k-steps costs more than the idle CUs of the 128-row grid).  Both instances give a row the same bits, so the
// choice may depend on M.
static constexpr long long kThinMaxWorkgroups = 256;
static int g_thin_force = -1;   // f5hip_op_gemm's timing of both instances on one shape (F5HIP_GEMM3_THIN=0|1, unit op only); -1 on the path
static hipError_t launch_gemm3_generic_or_thin(int prec, int epi, int bn, const GemmArgs& a, int mp, int np, hipStream_t st) {
    const long long thin_wgs = (long long)((a.M + 31) / 32) * (np / 128);
    const bool thin = epi == EPI_GENERIC && bn == 128 && (g_thin_force >= 0 ? g_thin_force != 0 : thin_wgs <= kThinMaxWorkgroups);
    g_counters[CNT_GEMM3]++;
    if (!thin) return f5_launch_gemm3(prec, epi, bn, a, mp, np, st);
    g_counters[CNT_GEMM3_THIN]++;
    return f5_launch_gemm3_thin(prec, a, np, st);
}
static int run_gemm_n(int nsplit, int mp, GemmArgs& a, const PackedW& W, int epi, bool conv, int bn, hipStream_t st) {
    hipError_t e;
    const int np = W.n_pad;
    if (mp % 128 || np % bn || a.K % 32) return fail(-7, "gemm: bad padded shape %d x %d x %d", mp, np, a.K);
    prof_begin(PROF_GEMM, st);
    const long long tiles128 = (long long)(mp / 128) * (np / 128);
    if (nsplit == 3 && !conv) {   // fp16 operands, one plane each
        const Gemm5Choice c5 = gemm5_choose(a.M, np);
        // gemm6 (256 x 256 ping-pong tiles): the batch-mode shapes -- enough tiles to occupy the chip in their first round
        const bool legal6 = a.K % 64 == 0 && np % 256 == 0 && (epi != EPI_QKV || a.D % 256 == 0);
        const int rows6 = legal6 ? gemm6_choose_rows(a.M, np) : 0;
        if (rows6) {
            e = f5_launch_gemm6(epi, rows6, a, np, st);
            g_counters[CNT_GEMM6]++;
            g_counters[rows6 == 176 ? CNT_GEMM6_R176 : CNT_GEMM6_R256]++;
        } else if (a.K % 64 == 0 && c5.rb) {
            e = epi == EPI_QKV ? f5_launch_gemm5_qkv(a, c5.rb, c5.cb, np, st)
              : epi == EPI_GENERIC_ROWMUL ? f5_launch_gemm5_rowmul(a, c5.rb, c5.cb, np, st) : f5_launch_gemm5_generic(a, c5.rb, c5.cb, np, st);
            g_counters[c5.rb == 11 ? CNT_GEMM5_RB11 : CNT_GEMM5_RB8]++;
            if (c5.cb >= 8) g_counters[CNT_GEMM5_WIDE]++;
            if (c5.cb == 12) g_counters[CNT_GEMM5_CB12]++;
        } else {
            // gemm3 (round 1): 128 x 256 tile in batch mode (>= 1024 tiles of 128 x 128), 128 x 128 otherwise
            const bool wide = tiles128 >= 1024 && np % 256 == 0;
            if (wide) g_counters[CNT_GEMM3_WIDE]++;
            e = launch_gemm3_generic_or_thin(3, epi, wide ? 256 : 128, a, mp, np, st);
        }
    } else if (!conv && tiles128 <= 256 && epi != EPI_QKV) {
        e = launch_gemm3_generic_or_thin(nsplit, epi, 128, a, mp, np, st);
    } else {   // (fp16 convolutions included: BigVGAN in fp16 mode)
        g_counters[bn == 64 ? CNT_GEMM_REG_BN64 : CNT_GEMM_REG_BN128]++;
        e = f5_launch_gemm_reg(nsplit, bn, conv, epi, a, mp, np, st);
    }
    prof_end(PROF_GEMM, st);
    if (e != hipSuccess) return fail(-7, "gemm launch: %s", hipGetErrorString(e));
    return 0;
}
// One implicit-GEMM convolution over g.M rows: conv5.h (window of the tile once in LDS, taps served from it) when `conv5`, else gemm.h
// (tile width bn).  A shape conv5 does not cover falls back to gemm.h when `fallback`, else fails.
static int run_conv(int nsplit, GemmArgs& g, const PackedW& W, bool conv5, bool fallback, int bn, hipStream_t st) {
    if (conv5) {
        prof_begin(PROF_GEMM, st);
        const hipError_t e = f5_launch_conv5(nsplit, g, W.n_pad, st);
        prof_end(PROF_GEMM, st);
        if (e == hipSuccess) { g_counters[CNT_CONV5]++; return 0; }
        if (e != hipErrorInvalidValue || !fallback)
            return fail(-7, "conv5 launch: %s", e == hipErrorInvalidValue ? "does not cover this shape" : hipGetErrorString(e));
    }
    return run_gemm_n(nsplit, g.M, g, W, EPI_GENERIC, true, bn, st);
}
static int run_gemm(f5hip_dit* m, GemmArgs& a, const PackedW& W, int epi, bool conv, int bn, hipStream_t st, int m_pad = -1) {
    return run_gemm_n(W.f16 ? 3 : m->nsplit, m_pad > 0 ? m_pad : m->M, a, W, epi, conv, bn, st);
}

// LnArgs of y = LN(x) (gain_off + scale) + shift over rows x [M][ldx] of width D; every other field zero
static LnArgs ln_args(const float* x, int ldx, int M, int D, const float* scale, const float* shift, float gain_off, float eps) {
    LnArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.ldx = ldx; a.M = M; a.D = D; a.scale = scale; a.shift = shift; a.gain_off = gain_off; a.eps = eps;
    return a;
}

// Launches the ln_kernel instance of a.D's width (NV vectors of 256 floats per row); false: no instance covers it
template <bool ROW_MOD>
static bool launch_ln(const LnArgs& a, hipStream_t st) {
    dim3 grid((a.M + 3) / 4), blk(256);
    switch ((a.D + 255) / 256) {
        case 1: hipLaunchKernelGGL((ln_kernel<1, ROW_MOD>), grid, blk, 0, st, a); return true;
        case 2: hipLaunchKernelGGL((ln_kernel<2, ROW_MOD>), grid, blk, 0, st, a); return true;
        case 3: hipLaunchKernelGGL((ln_kernel<3, ROW_MOD>), grid, blk, 0, st, a); return true;
        case 4: hipLaunchKernelGGL((ln_kernel<4, ROW_MOD>), grid, blk, 0, st, a); return true;
        case 5: case 6: hipLaunchKernelGGL((ln_kernel<6, ROW_MOD>), grid, blk, 0, st, a); return true;
        default: return false;
    }
}

// row_mod: scale / shift per row (LnArgs::row_mod; f5hip_cfm_sample_grids)
static int run_ln(const LnArgs& a, hipStream_t st, bool row_mod = false) {
    prof_begin(PROF_LN, st);
    const bool launched = row_mod ? launch_ln<true>(a, st) : launch_ln<false>(a, st);
    prof_end(PROF_LN, st);
    if (!launched) return fail(-7, "ln: D=%d unsupported", a.D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-7, "ln launch: %s", hipGetErrorString(e));
    return 0;
}

// Diagnostics for tests: which GEMM path the launches since the last reset took (names in the order of the CNT_ enum), and which attn3
// instance (names in the order of tu_attn.hip's counters); name "reset" zeroes them all.
extern "C" int f5hip_get_counter(const char* name, int64_t* value) {
    static const char* names[CNT_COUNT] = {"gemm5_rb11", "gemm5_rb8", "gemm5_wide", "gemm3_wide", "conv5", "gemm6", "gemm6_r176", "gemm6_r256",
                                           "gemm5_cb12", "gemm3", "gemm_reg_bn64", "gemm_reg_bn128", "dit_rows", "ref_frontend_launches",
                                           "ref_taps_lds", "ref_taps_l2", "wave_finish_launches", "wave_finish_requests",
                                           "wave_encode_launches", "wave_encode_requests", "mel_ragged_launches", "mel_ragged_items",
                                           "wave_flac_launches", "wave_flac_requests", "wave_loudness_launches", "wave_loudness_requests",
                                           "flac_decode_launches", "flac_decode_streams", "ref_prestep_launches", "ref_prestep_clips",
                                           "wave_prosody_launches", "wave_prosody_requests", "ref_denoise_launches", "ref_denoise_clips",
                                           "wave_mark_launches", "wave_mark_requests", "wave_formant_launches", "wave_formant_requests",
                                           "watermark_detect_launches", "watermark_detect_clips",
                                           "ref_assess_launches", "ref_assess_clips", "gemm3_thin", "time_table_builds",
                                           "wave_mark_id_launches", "wave_mark_id_requests", "watermark_read_ids_launches",
                                           "watermark_read_ids_clips", "watermark_scan_launches", "watermark_scan_ranges"};
    static const char* attn_names[F5_ATTN_CNT_COUNT] = {"attn_bal8", "attn_nw8_deep", "attn_nw8", "attn_nw6_deep", "attn_nw6", "attn_nw4", "attn_seg2"};
    long long* attn = f5_attn_counters();
    if (!name) return fail(-1, "get_counter: null name");
    if (!strcmp(name, "reset")) {
        for (auto& c : g_counters) c = 0;
        for (int i = 0; i < F5_ATTN_CNT_COUNT; i++) attn[i] = 0;
        return 0;
    }
    for (int i = 0; i < CNT_COUNT; i++)
        if (!strcmp(name, names[i])) { if (value) *value = g_counters[i]; return 0; }
    for (int i = 0; i < F5_ATTN_CNT_COUNT; i++)
        if (!strcmp(name, attn_names[i])) { if (value) *value = attn[i]; return 0; }
    return fail(-1, "unknown counter %s", name);
}

// -------------------------------------------------------------------------------------------------
// step-invariant precompute: text embedding for every sequence, cond/text part of the input projection
// -------------------------------------------------------------------------------------------------
// One ConvNeXtV2 text block (F/model/modules.py:259-269) over the M rows of the layout, in place on te [M][Td]: the depthwise conv (k 7, zero
// padding at the row bounds row_start / row_end) + LayerNorm into the planes tn, pw1 + GELU (erf) into ty [M][2 Td], the GRN column norms of
// every sequence (rows seq_row0[s] .. + seq_len[s]) into gx [n_seq][2 Td], GRN into the planes tg (rows with row_seq < 0 are skipped), then
// te += pw2; out_hi (or null) also receives the block output as split-bf16 planes of pitch ldob.  Operands in `nsplit` planes.
static int run_text_block(int nsplit, const TextBlock& b, int Td, int M, int n_seq, float* te, const Plane2& tn, float* ty, const Plane2& tg,
                          float* gx, const int* row_start, const int* row_end, const int* row_seq, const int* seq_row0, const int* seq_len,
                          __bf16* out_hi, __bf16* out_lo, int ldob, hipStream_t st) {
    LnArgs ln = ln_args(te, Td, M, Td, b.ln_w, b.ln_b, 0.0f, 1e-6f);
    ln.dw_w = b.dw_w; ln.dw_b = b.dw_b; ln.row_seq_start = row_start; ln.row_seq_end = row_end;
    ln.out_hi = tn.hi; ln.out_lo = tn.lo; ln.ldo = Td;
    CK(run_ln(ln, st));
    GemmArgs g1 = gemm_base(tn, Td, b.pw1, M);
    g1.act = ACT_GELU_ERF; g1.out_f32 = ty; g1.ldo = 2 * Td;
    CK(run_gemm_n(b.pw1.f16 ? 3 : nsplit, M, g1, b.pw1, EPI_GENERIC, false, 128, st));
    prof_begin(PROF_OTHER, st);
    hipLaunchKernelGGL(grn_stats_kernel, dim3((2 * Td + 31) / 32, n_seq), dim3(256), 0, st, ty, 2 * Td, 2 * Td, seq_row0, seq_len, gx);
    CKL("grn_stats");
    hipLaunchKernelGGL(grn_apply_kernel, dim3((M + 3) / 4), dim3(256), 0, st, ty, 2 * Td, 2 * Td, M, row_seq, gx, b.gamma, b.beta, tg.hi, tg.lo,
                       2 * Td);
    CKL("grn_apply");
    prof_end(PROF_OTHER, st);
    GemmArgs g2 = gemm_base(tg, 2 * Td, b.pw2, M);
    g2.res = te; g2.ldres = Td; g2.out_f32 = te; g2.ldo = Td;
    if (out_hi) { g2.out_hi = out_hi; g2.out_lo = out_lo; g2.ldob = ldob; }
    return run_gemm_n(b.pw2.f16 ? 3 : nsplit, M, g2, b.pw2, EPI_GENERIC, false, 128, st);
}

static int precompute_text_and_ce(f5hip_dit* m, const float* cond_dev, hipStream_t st) {
    const f5hip_dit_config& c = m->cfg;
    const int D = c.dim, Td = c.text_dim, M = m->M, Kct = 128 + m->td_pad;
    prof_begin(PROF_OTHER, st);
    if (m->arch == 2) {
        // MMDiT TextEmbedding (mmdit.py:37-52): embedding + absolute position table for the rows of the text stream (rows [M, M + Mc) of
        // every per-row buffer); step invariant, copied into the stream at the start of each forward.  Padding rows stay zero.
        const int C0 = m->row_c0;
        hipLaunchKernelGGL(text_gather_kernel, dim3(m->Mc), dim3(256), 0, st, m->text_emb, m->text_pos, D, m->Mc, m->d_row_token + C0,
                           m->d_row_pos + C0, 1, m->te + (size_t)C0 * D, D, 1023);
    } else {
        hipLaunchKernelGGL(text_gather_kernel, dim3(M), dim3(256), 0, st, m->text_emb, m->text_pos, Td, M, m->d_row_token,
                           m->d_row_pos, c.conv_layers > 0 ? 1 : 0, m->te, Td, 4095);
    }
    CKL("text_gather");
    // audio-cond columns of the step-invariant operand (zero rows for dropped cond / non-cond frames / padding)
    hipLaunchKernelGGL(split_rows_kernel, dim3(M), dim3(256), 0, st, cond_dev, c.mel_dim, c.mel_dim, M, m->d_row_condframe,
                       m->act.hi, m->act.lo, Kct, 0);
    CKL("split cond");
    prof_end(PROF_OTHER, st);
    for (int i = 0; i < c.conv_layers; i++) {
        const bool last = i == c.conv_layers - 1;   // the last block also writes the text columns of the step-invariant operand
        CK(run_text_block(m->nsplit, m->tblk[i], Td, M, m->n_seq, m->te, m->tn, m->ty, m->tg, m->gx, m->d_row_start, m->d_row_end, m->d_row_seq,
                          m->d_seq_row0, m->d_seq_len, last ? m->act.hi + 128 : nullptr, last ? m->act.lo + 128 : nullptr, Kct, st));
    }
    if (c.conv_layers == 0 && m->arch != 2) {   // (MMDiT: the text is not an input of the audio projection)
        prof_begin(PROF_OTHER, st);
        hipLaunchKernelGGL(split_rows_kernel, dim3(M), dim3(256), 0, st, m->te, Td, Td, M, (const int*)nullptr, m->act.hi,
                           m->act.lo, Kct, 128);
        CKL("split text");
        prof_end(PROF_OTHER, st);
    }
    GemmArgs g = gemm_base(m->act, Kct, m->wct, M);
    g.out_f32 = m->ce; g.ldo = D;
    CK(run_gemm(m, g, m->wct, EPI_GENERIC, false, 128, st));
    return 0;
}

// time embedding + every AdaLN modulation vector for all steps at once (they depend on t only).  The GEMM chain runs once per block of 128
// time points over 128 padded rows, so a time point's vectors come out of the same kernels whichever block it sits in.
// The tables depend on the time points and the weights only, and a serving process asks for the same grid (steps, sway, solver) call after
// call: the handle keeps the list of points its tables were built for (time_key, compared by bytes), and a call with the same list leaves
// them as they are.  Nothing else writes these buffers; the key is dropped where they move (ensure_workspace) and while a build is under way,
// so a failed build is never taken for a finished one.  No path replaces a finalized handle's weights (f5hip_dit_load_param refuses after
// f5hip_dit_finalize), so there is no weight change to drop it for.  The tables of the previous call were written in stream order, which
// is the order every buffer of the handle relies on from one call to the next.
// reuse: the whole-grid sampler calls.  Not f5hip_cfm_sample_span, which is handed a moving window of every unit's grid, nor the single
// forward and the time-table unit op, the diagnostic entries whose launches the tests count call by call: those always build.
static int precompute_time(f5hip_dit* m, const float* t_host, int n_t, hipStream_t st, bool reuse = false) {
    const f5hip_dit_config& c = m->cfg;
    const int D = c.dim;
    if (n_t > kMaxTimePoints) return fail(-8, "at most %d time points per call (got %d)", kMaxTimePoints, n_t);
    if (reuse && n_t > 0 && (int)m->time_key.size() == n_t && !memcmp(m->time_key.data(), t_host, sizeof(float) * n_t)) return 0;
    m->time_key.clear();
    g_counters[CNT_TIME_TABLE_BUILDS]++;
    const int t_pad = ceil_to(n_t, 128);
    // SinusPositionEmbedding (F/model/modules.py:154-161) on the host: the table is n_t x 256
    std::vector<uint16_t> hi((size_t)t_pad * 256, 0), lo((size_t)t_pad * 256, 0);
    const float emb = logf(10000.0f) / (float)(128 - 1);
    for (int i = 0; i < n_t; i++)
        for (int k = 0; k < 128; k++) {
            const float f = expf((float)k * -emb);
            const float e = 1000.0f * t_host[i] * f;
            const float sv = (float)sin((double)e), cv = (float)cos((double)e);
            host_split_bf16(sv, hi[(size_t)i * 256 + k], lo[(size_t)i * 256 + k]);
            host_split_bf16(cv, hi[(size_t)i * 256 + 128 + k], lo[(size_t)i * 256 + 128 + k]);
        }
    CK(m->up_time[0].upload(m->sinp.hi, hi.data(), hi.size() * 2, st));
    CK(m->up_time[1].upload(m->sinp.lo, lo.data(), lo.size() * 2, st));
    for (int t0 = 0; t0 < n_t; t0 += 128) {
        const int nb = std::min(128, n_t - t0);
        GemmArgs g1 = gemm_base(rows_from(m->sinp, (size_t)t0 * 256), 256, m->time1, nb);
        g1.act = ACT_SILU; g1.out_hi = m->t1.hi + (size_t)t0 * D; g1.out_lo = m->t1.lo + (size_t)t0 * D; g1.ldob = D;
        CK(run_gemm(m, g1, m->time1, EPI_GENERIC, false, 128, st, 128));
        GemmArgs g2 = gemm_base(rows_from(m->t1, (size_t)t0 * D), D, m->time2, nb);
        if (m->arch == 1) {
            g2.out_f32 = m->temb + (size_t)t0 * D; g2.ldo = D;   // UNetT: the raw time embedding is prepended as a token (unett.py:184)
            CK(run_gemm(m, g2, m->time2, EPI_GENERIC, false, 128, st, 128));
            continue;
        }
        g2.act = ACT_SILU; g2.out_hi = m->st.hi + (size_t)t0 * D; g2.out_lo = m->st.lo + (size_t)t0 * D; g2.ldob = D;   // silu(t_emb): the only form AdaLN consumes
        CK(run_gemm(m, g2, m->time2, EPI_GENERIC, false, 128, st, 128));
        GemmArgs g3 = gemm_base(rows_from(m->st, (size_t)t0 * D), D, m->adaln, nb);
        g3.out_f32 = m->mod + (size_t)t0 * m->n_adaln; g3.ldo = m->n_adaln;
        CK(run_gemm(m, g3, m->adaln, EPI_GENERIC, false, 128, st, 128));
    }
    m->time_key.assign(t_host, t_host + n_t);
    return 0;
}

// rotary operands of a QKV launch over rows row_off ..: the per-row tables of the current layout (one load per row in the epilogue)
static void set_rope(GemmArgs& q, const f5hip_dit* m, int row_off) {
    q.row_pos = nullptr; q.rope_cos = m->rope_row_cos + (size_t)row_off * 32; q.rope_sin = m->rope_row_sin + (size_t)row_off * 32;
}

// One residual stream of the transformer blocks: rows [row0, row0 + rows) of every per-row buffer (h, hn, ao, ff, qk, V^T columns) --
// the audio rows [0, M), or MMDiT's text rows [M, M + Mc) -- and its block weights.  keep: the out projection zeroes the padded rows of
// masked sequences (row_keep; the audio stream only).
struct Stream { int row0, rows; const BlockWeights* w; bool keep; };
static Stream audio_stream(const f5hip_dit* m) { return {0, m->M, &m->blk, true}; }

// h += gate * (A W^T + b) over the stream's rows (gate null: none)
// (d_row_tp set: the gate of each row from its own modulation row -- the per-row-multiplier epilogue)
static int block_residual(f5hip_dit* m, const Stream& s, const Plane2& A, int lda, const PackedW& W, const float* gate, const int* keep, hipStream_t st) {
    const int D = m->cfg.dim;
    GemmArgs g = gemm_base(A, lda, W, s.rows);
    g.mul = gate; g.res = m->h + (size_t)s.row0 * D; g.ldres = D; g.out_f32 = m->h + (size_t)s.row0 * D; g.ldo = D; g.row_keep = keep;
    const bool per_row = gate && m->d_row_tp;
    if (per_row) { g.row_mod = m->d_row_tp + s.row0; g.mod_ld = m->n_adaln; }
    return run_gemm(m, g, W, per_row ? EPI_GENERIC_ROWMUL : EPI_GENERIC, false, 64, st, s.rows);
}

// block l's QKV projection of the stream's rows hn: rotary q | k into qk, V^T into vt (rows of the current layout)
static int block_qkv(f5hip_dit* m, const Stream& s, int l, hipStream_t st) {
    const int D = m->cfg.dim;
    const size_t r0 = s.row0;
    GemmArgs q = gemm_base(rows_from(m->hn, r0 * D), D, s.w->qkv[l], s.rows);
    q.D = D; set_rope(q, m, s.row0); q.qk = m->qk + r0 * 2 * D; q.vt = m->vt + r0; q.ldvt = m->Rtot;
    return run_gemm(m, q, s.w->qkv[l], EPI_QKV, false, 128, st, s.rows);
}

// block l's out projection of the attention output ao into the stream
static int block_out(f5hip_dit* m, const Stream& s, int l, const float* gate, hipStream_t st) {
    const int D = m->cfg.dim;
    return block_residual(m, s, rows_from(m->ao, (size_t)s.row0 * D), D, s.w->out[l], gate, s.keep && m->any_masked ? m->d_row_keep : nullptr, st);
}

// block l's feed-forward of the stream's rows hn: FF1 (GELU tanh) into ff, then FF2 into the stream
static int block_ff(f5hip_dit* m, const Stream& s, int l, const float* gate, hipStream_t st) {
    const int D = m->cfg.dim, F = m->cfg.ff_mult * D;
    const Plane2 ff = rows_from(m->ff, (size_t)s.row0 * F);
    GemmArgs f1 = gemm_base(rows_from(m->hn, (size_t)s.row0 * D), D, s.w->ff1[l], s.rows);
    f1.act = ACT_GELU_TANH; f1.out_hi = ff.hi; f1.out_lo = ff.lo; f1.ldob = F; f1.f16_out = m->blk_f16 ? 1 : 0;
    CK(run_gemm(m, f1, s.w->ff1[l], EPI_GENERIC, false, 128, st, s.rows));
    return block_residual(m, s, ff, F, s.w->ff2[l], gate, nullptr, st);
}

// AdaLayerNorm of the stream's rows of h into hn: LayerNorm(h) * (1 + scale) + shift
static int run_adaln(f5hip_dit* m, const Stream& s, const float* shift, const float* scale, bool f16, hipStream_t st) {
    const int D = m->cfg.dim;
    LnArgs ln = ln_args(m->h + (size_t)s.row0 * D, D, s.rows, D, scale, shift, 1.0f, 1e-6f);
    ln.out_hi = m->hn.hi + (size_t)s.row0 * D; ln.out_lo = m->hn.lo + (size_t)s.row0 * D; ln.ldo = D; ln.f16_out = f16 ? 1 : 0;
    if (m->d_row_tp) { ln.row_mod = m->d_row_tp + s.row0; ln.mod_ld = m->n_adaln; }   // (scale / shift per row)
    return run_ln(ln, st, m->d_row_tp != nullptr);
}

// The tail of every backbone: proj_out over the final norm's planes hn into pred [M][128]
static int run_proj_out(f5hip_dit* m, hipStream_t st) {
    GemmArgs po = gemm_base(m->hn, m->cfg.dim, m->proj_out, m->M);
    po.out_f32 = m->pred; po.ldo = 128;
    return run_gemm(m, po, m->proj_out, EPI_GENERIC, false, 128, st);
}

static int launch_attention(f5hip_dit* m, hipStream_t st) {
    const f5hip_dit_config& c = m->cfg;
    AttnArgs at; memset(&at, 0, sizeof(at));
    at.qk = m->qk; at.vt = m->vt; at.D = c.dim; at.ldvt = m->Rtot; at.seq_row0 = m->d_seq_row0; at.seq_len = m->d_seq_len;
    at.seq_kvlen = m->d_seq_kvlen; at.out_hi = m->ao.hi; at.out_lo = m->nsplit == 2 ? m->ao.lo : nullptr; at.f16_out = m->blk_f16 ? 1 : 0;
    at.shape_invariant = m->attn_invariant;
    int n_att = m->n_seq;
    if (m->arch == 2) {   // joint attention: audio and text queries of a sequence over its audio keys followed by its text keys
        at.seq_row0 = m->d_j_row0; at.seq_len = m->d_j_len; at.seq_kvlen = m->d_j_kvlen;
        at.seq_kv_row0 = m->d_j_kv_row0; at.seq_kv2_row0 = m->d_j_kv2_row0; at.seq_kv2_len = m->d_j_kv2_len;
        n_att = 2 * m->n_seq;
    }
    prof_begin(PROF_ATTN, st);
    const hipError_t e = f5_launch_attn3(at, m->max_len, c.heads, n_att, st);
    if (e != hipSuccess) { prof_end(PROF_ATTN, st); return fail(-7, "attention launch: %s", hipGetErrorString(e)); }
    prof_end(PROF_ATTN, st);
    CKL("attention");
    return 0;
}

// UNetT (E2-TTS) layers, F/model/backbones/unett.py:184-219: time token at row 0 of every sequence, pre-norm blocks
//   x = attn(RMSNorm(x)) + x;  x = ff(RMSNorm(x)) + x,  U-skips: layer l >= depth/2 first does x = W_skip [x || skip(depth-1-l)].
static int forward_unett_layers(f5hip_dit* m, int ti, int n_blocks, hipStream_t st) {
    const f5hip_dit_config& c = m->cfg;
    const int D = c.dim, M = m->M;
    const Stream x = audio_stream(m);
    prof_begin(PROF_OTHER, st);
    if (m->d_row_tp) hipLaunchKernelGGL(set_time_token_rows_kernel, dim3(m->n_seq), dim3(256), 0, st, m->h, D, m->d_seq_row0, m->temb, (const int*)m->d_row_tp);
    else hipLaunchKernelGGL(set_time_token_kernel, dim3(m->n_seq), dim3(256), 0, st, m->h, D, m->d_seq_row0, m->temb + (size_t)ti * D);
    prof_end(PROF_OTHER, st);
    CKL("set_time_token");
    const int nb = n_blocks < 0 ? c.depth : n_blocks;
    LnArgs ln = ln_args(m->h, D, M, D, nullptr, m->zeros, 0.0f, 0.0f);
    ln.rms = 1;
    ln.out_hi = m->hn.hi; ln.out_lo = m->hn.lo; ln.ldo = D;
    for (int l = 0; l < nb; l++) {
        if (l < c.depth / 2) {
            prof_begin(PROF_OTHER, st);
            // the skip is saved where its consumer wants it: columns D .. 2 D - 1 of that layer's [x || skip] operand (round 3: it used to go to a
            // [M][D] buffer and was copied behind x with hipMemcpy2DAsync at the consumer, ~55 % of the "other" kernel class at C5)
            hipLaunchKernelGGL(split_rows_kernel, dim3(M), dim3(256), 0, st, m->h, D, D, M, (const int*)nullptr, m->skipbuf[l].hi, m->skipbuf[l].lo, 2 * D, D);
            prof_end(PROF_OTHER, st);
            CKL("skip save");
        } else {
            const Plane2& sk = m->skipbuf[c.depth - 1 - l];
            prof_begin(PROF_OTHER, st);
            hipLaunchKernelGGL(split_rows_kernel, dim3(M), dim3(256), 0, st, m->h, D, D, M, (const int*)nullptr, sk.hi, sk.lo, 2 * D, 0);
            prof_end(PROF_OTHER, st);
            CKL("skip concat x");
            GemmArgs sp = gemm_base(sk, 2 * D, m->wskip[l], M);
            sp.bias = nullptr; sp.out_f32 = m->h; sp.ldo = D;
            CK(run_gemm(m, sp, m->wskip[l], EPI_GENERIC, false, 64, st));
        }
        ln.scale = m->g_attn[l];
        ln.f16_out = m->blk_f16 ? 1 : 0;   // block norms feed the fp16 block GEMMs in mixed mode; the final norm (proj_out) stays split bf16
        CK(run_ln(ln, st));
        CK(block_qkv(m, x, l, st));
        CK(launch_attention(m, st));
        CK(block_out(m, x, l, nullptr, st));
        ln.scale = m->g_ff[l];
        CK(run_ln(ln, st));
        CK(block_ff(m, x, l, nullptr, st));
    }
    if (n_blocks >= 0) return 0;
    ln.scale = m->g_out;
    ln.f16_out = 0;
    CK(run_ln(ln, st));
    return run_proj_out(m, st);
}

// One DiT evaluation at time index ti for all laid-out sequences.  xs (split bf16 of x) must be current.
// n_blocks < 0: full network, result in m->pred [M][128];  else stops after n_blocks blocks, result in m->h.
// MMDiT blocks (F/model/modules.py:614-642, JointAttnProcessor :460-536): two residual streams -- the audio rows [0, M) in m->h and the
// text rows [M, M + Mc) behind them in the same buffers -- with their own modulation, QKV, output and feed-forward weights and ONE
// joint attention per block over [audio keys ; text keys] (rotary on head 0 of each stream with its own positions).  The last block is
// context-pre-only: the text stream is only normalised and projected to q / k / v, then dropped.
static int forward_mmdit_layers(f5hip_dit* m, int ti, int n_blocks, hipStream_t st) {
    const f5hip_dit_config& c = m->cfg;
    const int D = c.dim, M = m->M, Mc = m->Mc, C0 = m->row_c0;   // (C0 == M but in a cfm_sample_grids forward over a prefix of the units)
    const float* mod = m->mod + (size_t)ti * m->n_adaln;
    const Stream x = audio_stream(m), tx{C0, Mc, &m->blk_c, false};
    // the text stream starts every forward from its step-invariant embedding
    if (hipMemcpyAsync(m->h + (size_t)C0 * D, m->te + (size_t)C0 * D, sizeof(float) * (size_t)Mc * D, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(-6, "MMDiT: text stream copy");
    const int nb = n_blocks < 0 ? c.depth : n_blocks;
    for (int l = 0; l < nb; l++) {
        const bool last = l == c.depth - 1;
        const float* mc = mod + m->mod_c[l];                       // text: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp; last block: scale, shift
        const float* mx = mod + m->mod_x[l];
        CK(last ? run_adaln(m, tx, mc + D, mc, m->blk_f16, st) : run_adaln(m, tx, mc, mc + D, m->blk_f16, st));
        CK(run_adaln(m, x, mx, mx + D, m->blk_f16, st));
        CK(block_qkv(m, x, l, st));
        CK(block_qkv(m, tx, l, st));
        CK(launch_attention(m, st));
        CK(block_out(m, x, l, mx + 2 * D, st));
        if (!last) {
            CK(block_out(m, tx, l, mc + 2 * D, st));
            CK(run_adaln(m, tx, mc + 3 * D, mc + 4 * D, m->blk_f16, st));
            CK(block_ff(m, tx, l, mc + 5 * D, st));
        }
        CK(run_adaln(m, x, mx + 3 * D, mx + 4 * D, m->blk_f16, st));
        CK(block_ff(m, x, l, mx + 5 * D, st));
    }
    if (n_blocks >= 0) return 0;
    const float* mf = mod + m->mod_final;                          // (scale, shift): F/model/modules.py:308
    CK(run_adaln(m, x, mf + D, mf, false, st));
    return run_proj_out(m, st);
}

// ConvPositionEmbedding (F/model/modules.py:171-176) over the M rows of the layout: h = Mish(GConv2(Mish(GConv1(hn)))) + h0, with hn the
// operand planes of h0 and stage 1 in the planes c1 (both [M][D], plus slack past the last row: a group narrower than 64 channels is
// read as 64).  Window rows outside [row_start, row_end) of the output row are zero.  conv5: the sliding-window kernel (conv5.h, 128-row
// tiles, one column tile per group), which takes the bounds of a tile from its first row -- the DiT and MMDiT layouts in split bf16;
// else the implicit GEMM of gemm.h (UNetT: the time-token row at the head of every sequence has an empty window of its own).
static int run_conv_pos_embed(int nsplit, bool conv5, int D, int M, const Plane2& hn, const Plane2& c1, const float* h0, float* h,
                              const PackedW& w1, const PackedW& w2, const int* row_start, const int* row_end, hipStream_t st) {
    const int gw = D / 16;
    for (int which = 0; which < 2; which++) {
        const PackedW& W = which ? w2 : w1;
        GemmArgs g = gemm_base(which ? c1 : hn, D, W, M);
        g.conv_kpt = 2; g.conv_center = 15; g.conv_group_cols = gw; g.row_seq_start = row_start; g.row_seq_end = row_end;
        g.group_w = gw; g.N = 16 * 64;
        g.act = ACT_MISH;
        if (which) { g.res = h0; g.ldres = D; g.out_f32 = h; g.ldo = D; }
        else { g.out_hi = c1.hi; g.out_lo = c1.lo; g.ldob = D; }
        CK(run_conv(W.f16 ? 3 : nsplit, g, W, conv5 && !W.f16, true, 64, st));
    }
    return 0;
}

static int forward_step(f5hip_dit* m, int ti, int n_blocks, hipStream_t st) {
    const f5hip_dit_config& c = m->cfg;
    const int D = c.dim, M = m->M;
    const float* mod = m->mod + (size_t)ti * m->n_adaln;
    g_counters[CNT_DIT_ROWS] += M;
    // input projection: x part + precomputed cond/text part
    GemmArgs gi = gemm_base(m->xs, 128, m->wx, M);
    gi.bias = nullptr; gi.res = m->ce; gi.ldres = D; gi.out_f32 = m->h0; gi.ldo = D;
    gi.out_hi = m->hn.hi; gi.out_lo = m->hn.lo; gi.ldob = D;
    CK(run_gemm(m, gi, m->wx, EPI_GENERIC, false, 128, st));
    // conv_pos_embed: Mish(GConv(Mish(GConv(h0)))) + h0   (F/model/modules.py:171-176, F/model/backbones/dit.py:86)
    CK(run_conv_pos_embed(m->nsplit, m->arch != 1 && m->nsplit == 2, D, M, m->hn, m->c1, m->h0, m->h, m->conv1, m->conv2, m->d_row_start,
                          m->d_row_end, st));

    if (m->arch == 1) return forward_unett_layers(m, ti, n_blocks, st);
    if (m->arch == 2) return forward_mmdit_layers(m, ti, n_blocks, st);
    const int nb = n_blocks < 0 ? c.depth : n_blocks;
    // Each LayerNorm is a launch of its own (fusing the norm into the epilogue of the residual GEMM in front of it measured slower -- 31.2 us
    // against 18.8 + 6.1 us for the two launches: profiles/r02_ln_fusion.txt).
    const Stream x = audio_stream(m);
    for (int l = 0; l < nb; l++) {
        const float* ml = mod + m->mod_x[l];   // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
        CK(run_adaln(m, x, ml, ml + D, m->blk_f16, st));
        CK(block_qkv(m, x, l, st));
        CK(launch_attention(m, st));
        CK(block_out(m, x, l, ml + 2 * D, st));
        CK(run_adaln(m, x, ml + 3 * D, ml + 4 * D, m->blk_f16, st));
        CK(block_ff(m, x, l, ml + 5 * D, st));
    }
    if (n_blocks >= 0) return 0;
    const float* mf = mod + m->mod_final;   // final (scale, shift): F/model/modules.py:308; split-bf16 planes for proj_out
    CK(run_adaln(m, x, mf + D, mf, false, st));
    return run_proj_out(m, st);
}

// -------------------------------------------------------------------------------------------------
// public entry points
// -------------------------------------------------------------------------------------------------
int f5hip_dit_forward(f5hip_dit* m, int32_t n_seq, const int32_t* seq_len, const int32_t* kv_len, const float* x_dev,
                      const float* cond_dev, const int32_t* text, int32_t nt_max, float time, const uint8_t* drop_audio_cond,
                      const uint8_t* drop_text, int32_t n_blocks, float* out_dev, float* h_out_dev, void* stream) {
    if (!m || !m->finalized) return fail(-1, "model not finalized");
    if (n_seq <= 0 || !seq_len || !x_dev || !cond_dev || !text) return fail(-1, "dit_forward: bad argument");
    ProfScope prof_scope(m->prof);
    hipStream_t st = (hipStream_t)stream;
    std::vector<SeqDesc> seqs(n_seq);
    int f0 = 0;
    m->h_seq_len.assign(n_seq, 0);
    for (int i = 0; i < n_seq; i++) {
        if (seq_len[i] <= 0 || seq_len[i] > 4096) return fail(-1, "seq_len[%d] = %d out of range", i, seq_len[i]);
        seqs[i] = {seq_len[i], kv_len ? kv_len[i] : seq_len[i], f0, i, drop_audio_cond ? drop_audio_cond[i] : 0, drop_text ? drop_text[i] : 0, 0};
        seqs[i].c_len = nt_max;   // MMDiT.forward embeds every position of its [b, nt] text tensor, fillers included (mmdit.py:37-52, no text mask)
        if (seqs[i].kvlen <= 0 || seqs[i].kvlen > seqs[i].len) return fail(-1, "kv_len[%d] out of range", i);
        m->h_seq_len[i] = seq_len[i];
        f0 += seq_len[i];
    }
    CK(setup_sequences(m, seqs, f0, text, nt_max, nullptr, st));
    const int M = m->M, mel = m->cfg.mel_dim, D = m->cfg.dim;
    hipLaunchKernelGGL(split_rows_kernel, dim3(M), dim3(256), 0, st, x_dev, mel, mel, M, m->d_row_frame, m->xs.hi, m->xs.lo, 128, 0);
    CKL("split x");
    CK(precompute_text_and_ce(m, cond_dev, st));
    CK(precompute_time(m, &time, 1, st));
    CK(forward_step(m, 0, n_blocks, st));
    // gather rows back to the caller's packed frame order
    if (n_blocks < 0) {
        if (!out_dev) return fail(-1, "out_dev is null");
        hipLaunchKernelGGL(gather_rows_kernel, dim3(f0), dim3(128), 0, st, m->pred, 128, mel, f0, m->d_urow_c, out_dev, mel);
    } else {
        if (!h_out_dev) return fail(-1, "h_out_dev is null");
        hipLaunchKernelGGL(gather_rows_kernel, dim3(f0), dim3(128), 0, st, m->h, D, D, f0, m->d_urow_c, h_out_dev, D);
    }
    CKL("gather rows");
    return 0;
}

int f5hip_dit_read_tap(f5hip_dit* m, const char* tap, float* dst_dev, int64_t numel, void* stream) {
    if (!m || !tap || !dst_dev) return fail(-1, "read_tap: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (!strcmp(tap, "text_embed")) {
        const int Td = m->cfg.text_dim;
        if (numel != (int64_t)m->n_frames * Td) return fail(-1, "read_tap: numel mismatch");
        hipLaunchKernelGGL(gather_rows_kernel, dim3(m->n_frames), dim3(128), 0, st, m->te, Td, Td, m->n_frames, m->d_urow_c, dst_dev, Td);
        CKL("gather tap");
        return 0;
    }
    if (!strcmp(tap, "text_rows")) {   // MMDiT: the text stream's embedding as laid out, rows [M, M + Mc) (every sequence padded to 128 rows)
        const size_t n = (size_t)m->Mc * m->cfg.text_dim;
        if (m->arch != 2 || numel != (int64_t)n) return fail(-1, "read_tap: text_rows needs an MMDiT handle and numel = text rows x text_dim");
        if (hipMemcpyAsync(dst_dev, m->te + (size_t)m->row_c0 * m->cfg.text_dim, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(-6, "read_tap: copy");
        return 0;
    }
    if (!strcmp(tap, "text_stream")) {   // MMDiT: the text residual stream behind the blocks the last forward ran, rows laid out like "text_rows"
        const size_t n = (size_t)m->Mc * m->cfg.dim;
        if (m->arch != 2 || numel != (int64_t)n) return fail(-1, "read_tap: text_stream needs an MMDiT handle and numel = text rows x dim");
        if (hipMemcpyAsync(dst_dev, m->h + (size_t)m->row_c0 * m->cfg.dim, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(-6, "read_tap: copy");
        return 0;
    }
    return fail(-1, "unknown tap %s", tap);
}

int f5hip_set_attention_shape_invariant(int32_t on) {
    f5_set_attn_shape_invariant(on);
    return 0;
}

int f5hip_dit_set_attention_shape_invariant(f5hip_dit* m, int32_t on) {
    if (!m) return fail(-1, "null model");
    m->attn_invariant = on < 0 ? -1 : (on != 0);
    return 0;
}

int f5hip_dit_set_profiling(f5hip_dit* m, int32_t enabled) {
    if (!m) return fail(-1, "null model");
    if (!m->prof) m->prof = new ProfState();
    m->prof->set(enabled != 0);
    return 0;
}

int f5hip_dit_get_profile(f5hip_dit* m, const char* kernel_class, double* total_ms, int64_t* launches) {
    if (!m || !kernel_class) return fail(-1, "dit_get_profile: bad argument");
    if (!m->prof) return fail(-1, "dit_get_profile: f5hip_dit_set_profiling was never called on this handle");
    return m->prof->get(kernel_class, total_ms, launches);
}

int f5hip_dit_set_ode_method(f5hip_dit* m, int32_t method) {
    if (!m) return fail(-1, "null model");
    if (method < 0 || method > 2) return fail(-1, "ode method %d: 0 = euler, 1 = midpoint, 2 = rk4", method);
    m->ode_method = method;
    return 0;
}

#include "cfm_sample.h"
#include "vocos.h"
#include "bigvgan.h"
#include "unit_ops.h"
#include "resample.h"
#include "wave_out.h"
#include "flac_in.h"
#include "ref_prestep.h"
#include "ref_denoise.h"
#include "wave_mark.h"
#include "ref_assess.h"
#include "wave_formant.h"
